"""Node taps and proving from device inference: dp_model_infer_trace (Context.infer_trace; k_infer_tap_pack gathers every tensor the prover
reads into one row per input) and dp_model_prove_batch_ex with DP_PROVE_DEVICE_INFER (Prover.prove_batch(..., device_infer=True)). The yardstick
of every row is dp_model_infer_host_trace, input by input; the yardstick of every proof is dp_model_prove_batch (and, where tests/golden/ holds
the stream, the committed proof). Every comparison is exact equality. The cases that need their own environment (a scratch bound of 1 MB for at
least two chunks with a partial last one, 64-bit products instead of the i8 MFMA, a row budget that forces segments) run in a child process,
tests/support/trace_child.py."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from support.trace_families import FAMILIES, IDS, NEEDS_ALL_KINDS, build, golden_proof_sha256, inputs  # noqa: E402

CHILD = os.path.join(ROOT, "tests", "support", "trace_child.py")
LN_BAD, SM_BAD = (1 << 20) + 1, (1 << 24) + 1


def _child(mode, **env):
    r = subprocess.run([sys.executable, CHILD, mode], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and f"trace child done {mode}" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return r


@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_trace_rows_equal_the_host_trace(dev, family):
    """batches of 1, 2 and 65; plain infer before and after gives the same outputs"""
    import deep_prove_amd as dpa
    mb = build(family)
    blob = mb.blob()
    all_kinds = family[0] in NEEDS_ALL_KINDS
    xs = inputs(mb, 65)
    entries, row_words = dpa.trace_layout(blob)
    want = np.stack([dpa.infer_host_trace(blob, x) for x in xs])
    want_out = np.stack([dpa.infer_host(blob, x) for x in xs[:2]])
    ctx = dpa.Context.generate(dev, blob)
    try:
        before, _ = ctx.infer(xs, all_kinds=all_kinds)
        for nb in (1, 2, 65):
            rows, view, outs, reasons, ms = ctx.infer_trace(xs[:nb], all_kinds=all_kinds)
            assert reasons is None and rows.shape == (nb, row_words) and rows.dtype == np.int64 and ms > 0
            assert (rows == want[:nb]).all(), (nb, np.argwhere(rows != want[:nb])[:5])
            assert (outs == before[:nb]).all() and (outs[:2] == want_out[:nb]).all()
            assert set(view) == {(node, role) for node, role, _, _ in entries}
            for node, role, off, n in entries:
                assert view[(node, role)].shape == (nb, n) and (view[(node, role)] == want[:nb, off:off + n]).all()
        # the checked form on good data: the same rows, no reason
        rows, _, outs, reasons, _ = ctx.infer_trace(xs, all_kinds=all_kinds, checked=True)
        assert not reasons.any() and (rows == want).all() and (outs == before).all()
        after, _ = ctx.infer(xs, all_kinds=all_kinds)
        assert (after == before).all()
        if all_kinds:  # the kind rule of dp_model_infer_ex: refused without the flag
            with pytest.raises(dpa.DeepProveError) as ei:
                ctx.infer_trace(xs[:1])
            assert ei.value.code == -1 and re.search(r"node \d+ is a \w+ layer", str(ei.value)), str(ei.value)
    finally:
        ctx.free()


@pytest.mark.parametrize("no_mfma", [False, True], ids=["i8_mfma", "no_mfma"])
def test_trace_rows_over_several_chunks(no_mfma):
    """every family under a scratch bound of 1 MB: at least two chunks, the last partial; with the i8 MFMA and with 64-bit products everywhere"""
    r = _child("rows", DP_INFER_LOG="1", DP_INFER_SCRATCH_MB="1", DP_INFER_NO_MFMA="1" if no_mfma else "0")
    ok = [ln for ln in r.stdout.split("\n") if ln.startswith("trace child rows ok")]
    assert len(ok) == len(FAMILIES), r.stdout[-1500:]
    for ln in ok:
        n, nchunks, c = (int(v) for v in re.search(r"batch (\d+) in (\d+) chunks of (\d+),", ln).groups())
        assert nchunks >= 2 and nchunks == -(-n // c) and n % c, ln
    taps = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]") and "; taps " in ln]
    plain = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]") and "; taps " not in ln]
    assert len(taps) >= 2 * len(FAMILIES) and len(plain) == 2 * len(FAMILIES)
    for ln in taps:
        m = re.search(r"in (\d+) chunks of \d+, .*; taps (\d+) entries, (\d+) words, pack_launches (\d+) pack_ms", ln)
        assert m and m.group(1) == m.group(4) and int(m.group(2)) >= 1 and int(m.group(3)) >= 4, ln
    i8 = sum(int(re.search(r"gemm_i8 (\d+)", ln).group(1)) for ln in taps)
    assert (i8 == 0) if no_mfma else (i8 > 0)


def test_checked_trace_rows():
    """one refused input of each class 1-5, in the first and in the last chunk: the host's reasons, zeros in the refused rows, the host trace elsewhere"""
    r = _child("checked", DP_INFER_LOG="1", DP_INFER_SCRATCH_MB="1")
    ok = [ln for ln in r.stdout.split("\n") if ln.startswith("trace child checked ok")]
    assert [int(re.search(r"class (\d)", ln).group(1)) for ln in ok] == [1, 2, 3, 4, 5], r.stdout[-1500:]
    for ln in ok:
        n, nchunks, c = (int(v) for v in re.search(r"batch (\d+) in (\d+) chunks of (\d+)", ln).groups())
        assert nchunks >= 2 and n % c, ln


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and x.size == y.size and (x == y).all()) for x, y in zip(a, b))


@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_proofs_from_device_inference_are_those_of_prove_batch(dev, family):
    """6 inputs, 4 in flight: word for word the proofs of prove_batch, accepted by dp_verify_batch, and — input 0 — the committed stream"""
    import deep_prove_amd as dpa
    mb = build(family)
    xs = inputs(mb, 6)
    assert (xs[0] == mb.input()).all()
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        pr = dpa.Prover(ctx)
        host, houts, _ = pr.prove_batch(xs, 4)
        got, gouts, ms = pr.prove_batch(xs, 4, device_infer=True)
        assert _same(got, host) and (gouts == houts).all() and ms > 0 and pr.last_infer_ms > 0 and ms > pr.last_infer_ms
        res, _ = dpa.verify_batch(ctx.verifier_blob(), got, xs, gouts, dev=dev)
        assert not res.any(), res
        gold = golden_proof_sha256(family)
        if gold is not None:
            assert hashlib.sha256(got[0].tobytes()).hexdigest() == gold
        again, _, _ = pr.prove_batch(xs, 4)  # (and the host path after the device path)
        assert _same(again, host)
    finally:
        ctx.free()
    assert (gold is not None) == (family[0] in ("mlp", "cnn_tiny", "attention_block", "mha_block", "gelu_mlp", "qkv_two_outputs"))


def test_proofs_in_segments():
    """DP_PROVE_TRACE_MB small enough for segments of `concurrency` inputs: 6 proofs in 2 segments, every family"""
    r = _child("prove", DP_PROVE_TRACE_MB="0.00001", DP_TIMING="1")
    ok = [ln for ln in r.stdout.split("\n") if ln.startswith("trace child prove ok")]
    assert len(ok) == len(FAMILIES) and all(ln.endswith("6 proofs in 2 segments") for ln in ok), r.stdout[-1500:]


def _scaled_until_refused(blob, x):
    import deep_prove_amd as dpa
    scale = 1
    for _ in range(40):
        scale *= 8
        try:
            dpa.infer_host(blob, x * scale)
        except dpa.DeepProveError:
            return x * scale
    raise AssertionError("the host accepts every scale")


def _poke(index, value):
    def f(blob, x):
        y = x.copy()
        y[index] = value
        return y
    return f


# no model holds a node of every refusing kind: one model per class, its batch of 6 holds refused inputs of that class at rows 1 and 4
REFUSALS = [(1, "requant", "mlp", (2, 8), dict(config=9), _scaled_until_refused),
            (2, "vocabulary", "token_mlp", (16, 50, 32), dict(config=71, max_positions=40), _poke(3, 1 << 20)),
            (3, "gelu", "gelu_only", (16,), dict(config=31), _poke(2, 1 << 14)),
            (4, "layernorm", "layernorm_mlp", (4, 8, 16), dict(config=33), _poke(9, LN_BAD)),
            (5, "softmax", "softmax_only", (2, 4), dict(config=35), _poke(5, SM_BAD))]


@pytest.mark.parametrize("cls,word,name,args,kw,make_bad", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_reasons_instead_of_a_failed_batch(dev, cls, word, name, args, kw, make_bad):
    """with `reasons` a refused input gets its class, no proof and a zero output row, the others the proofs of prove_batch on the good rows;
    without, the call fails with the host's message. prove_batch_screened(device_infer=True) returns what prove_batch_screened returns"""
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, name)(*args, **kw)
    blob = mb.blob()
    xs = inputs(mb, 6)
    for r in (1, 4):
        xs[r] = make_bad(blob, xs[r])
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.infer_host(blob, xs[r])
        assert ei.value.code == -1 and word in str(ei.value)
    good = [0, 2, 3, 5]
    ctx = dpa.Context.generate(dev, blob)
    try:
        pr = dpa.Prover(ctx)
        want, wouts, _ = pr.prove_batch(xs[good], 4)
        screened = pr.prove_batch_screened(xs, 4)
        proofs, outs, reasons, ms = pr.prove_batch_screened(xs, 4, device_infer=True)
        assert list(reasons) == [0, cls, 0, 0, cls, 0] and reasons.dtype == np.uint32 and ms > 0
        assert [p is None for p in proofs] == [False, True, False, False, True, False]
        assert _same([proofs[i] for i in good], want) and (outs[good] == wouts).all() and not outs[[1, 4]].any()
        assert _same(proofs, screened[0]) and (outs == screened[1]).all() and (reasons == screened[2]).all()
        res, _ = dpa.verify_batch(ctx.verifier_blob(), [proofs[i] for i in good], xs[good], outs[good], dev=dev)
        assert not res.any(), res
        with pytest.raises(dpa.DeepProveError) as ei:
            pr.prove_batch(xs, 4, device_infer=True)
        assert ei.value.code == -1 and word in str(ei.value), str(ei.value)
        # a batch in which every input is refused: nothing is proved
        proofs, outs, reasons, _ = pr.prove_batch_screened(xs[[1, 4]], 4, device_infer=True)
        assert proofs == [None, None] and list(reasons) == [cls, cls] and not outs.any()
        again, _, _ = pr.prove_batch(xs[good], 4, device_infer=True)  # (the model stays usable)
        assert _same(again, want)
    finally:
        ctx.free()


def test_flag_errors(dev):
    """unknown flag bits and reasons without the flag: DP_ERR_ARG; flags 0 with reasons NULL: the bytes of dp_model_prove_batch"""
    import importlib
    import deep_prove_amd as dpa
    from deep_prove_amd._lib import i64p, u64p
    lib = importlib.import_module("deep_prove_amd.infer")._load()
    mb = dpa.models.mlp(2, 8, config=9)
    xs = inputs(mb, 3)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        pr = dpa.Prover(ctx)
        want, wouts, _ = pr.prove_batch(xs, 2)

        def call(flags, reasons):
            pws, pns = (u64p * 3)(), (C.c_size_t * 3)()
            outs = np.empty((3, pr.output_len()), dtype=np.int64)
            no, ms, ims = C.c_size_t(0), C.c_double(-1), C.c_double(-1)
            rc = lib.dp_model_prove_batch_ex(ctx.h, xs.ctypes.data_as(i64p), 3, xs.shape[1], 2, flags, reasons.ctypes.data_as(C.POINTER(C.c_uint32)) if reasons is not None else None,
                                             pws, pns, outs.ctypes.data_as(i64p), outs.shape[1], C.byref(no), C.byref(ms), C.byref(ims))
            proofs = [np.ctypeslib.as_array(pws[i], shape=(pns[i],)).copy() if pws[i] else None for i in range(3)]
            for i in range(3):
                if pws[i]:
                    dpa._lib.load().dp_free(pws[i])
            return rc, proofs, outs[:, :no.value], ims.value
        for flags in (2, 3, 1 << 31):
            rc, proofs, _, _ = call(flags, None)
            assert rc == -1 and proofs == [None] * 3 and "flag" in dpa._lib.load().dp_last_error().decode(), flags
        rc, proofs, _, _ = call(0, np.zeros(3, dtype=np.uint32))
        assert rc == -1 and proofs == [None] * 3 and "DP_PROVE_DEVICE_INFER" in dpa._lib.load().dp_last_error().decode()
        rc, proofs, outs, ims = call(0, None)
        assert rc == 0 and ims == 0 and _same(proofs, want) and (outs == wouts).all()
        rc, proofs, outs, ims = call(1, None)
        assert rc == 0 and ims > 0 and _same(proofs, want) and (outs == wouts).all()
    finally:
        ctx.free()
