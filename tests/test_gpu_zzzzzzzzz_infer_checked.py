"""dp_model_infer_checked (Context.infer_checked): device inference that refuses bad data input by input — a status word per input, zeros in the
rows of refused inputs, every chunk of the batch processed — and Prover.prove_batch_screened on top of it. The yardstick of every case is
dp_model_infer_host, input by input (`_host` below): the row it returns and reason 0, or zeros and the class of the word in its DP_ERR_ARG message.
Every comparison is exact equality."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "infer_checked_child.py")
WORDS = {"requant": 1, "vocabulary": 2, "gelu": 3, "layernorm": 4, "softmax": 5}
LN_BAD, SM_BAD = (1 << 20) + 1, (1 << 24) + 1


def _host(blob, xs, nout):
    """the yardstick: (rows[n, nout], reasons[n], words[n]) of dp_model_infer_host on every input"""
    import deep_prove_amd as dpa

    def one(x):
        try:
            return dpa.infer_host(blob, x), 0, ""
        except dpa.DeepProveError as e:
            hits = [w for w in WORDS if w in str(e)]
            assert e.code == -1 and len(hits) == 1, str(e)
            return np.zeros(nout, dtype=np.int64), WORDS[hits[0]], hits[0]
    with ThreadPoolExecutor(16) as ex:
        got = list(ex.map(one, xs))
    assert all(g[0].shape == (nout,) for g in got)
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.uint32), [g[2] for g in got]


def _check(ctx, blob, xs, all_kinds=True):
    """infer_checked on xs against the yardstick; returns (outputs, reasons, the host's words)"""
    import ctypes as C
    import importlib
    import deep_prove_amd as dpa
    lib = importlib.import_module("deep_prove_amd.infer")._load()
    out, reasons, ms = ctx.infer_checked(xs, all_kinds=all_kinds)
    want, want_reasons, words = _host(blob, xs, out.shape[1])
    assert out.shape == want.shape and reasons.dtype == np.uint32 and reasons.shape == (len(xs),)
    assert (reasons == want_reasons).all(), (reasons, want_reasons)
    assert (out == want).all(), np.argwhere(out != want)[:5]
    # *nrefused, from the C call itself
    x = np.ascontiguousarray(xs, dtype=np.int64)
    o2, r2 = np.empty_like(out), np.full(len(xs), 77, dtype=np.uint32)
    no, nref = C.c_size_t(0), C.c_size_t(12345)
    rc = lib.dp_model_infer_checked(ctx.h, x.ctypes.data_as(dpa._lib.i64p), x.shape[0], x.shape[1], 1 if all_kinds else 0, o2.ctypes.data_as(dpa._lib.i64p), o2.shape[1], C.byref(no),
                                    r2.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nref), None)
    assert rc == 0 and no.value == out.shape[1] and nref.value == int(np.count_nonzero(want_reasons)) and (r2 == want_reasons).all() and (o2 == want).all()
    return out, reasons, words


def _scaled_until_refused(blob, x):
    """x times 8, 64, ... until the host refuses it (as the existing tests build such inputs)"""
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


CLASSES = [("requant", "mlp", (2, 64), dict(config=31), _scaled_until_refused, False),
           ("vocabulary", "token_mlp", (32, 300, 128), dict(config=72, max_positions=50), _poke(3, 1 << 20), False),
           (None, "gelu_mlp", (256,), dict(config=112), _scaled_until_refused, True),  # (whichever node refuses the scaled input first: the host says)
           ("gelu", "gelu_only", (16,), dict(config=31), _poke(2, 1 << 14), True),  # (within 2^20, outside the table)
           ("layernorm", "layernorm_mlp", (4, 8, 16), dict(config=33), _poke(9, LN_BAD), True),
           ("softmax", "softmax_only", (2, 4), dict(config=35), _poke(5, SM_BAD), True)]


@pytest.mark.parametrize("word,name,args,kw,make_bad,needs_all_kinds", CLASSES, ids=["requant", "token", "gelu_mlp", "gelu", "layernorm", "softmax"])
def test_each_class_alone(dev, word, name, args, kw, make_bad, needs_all_kinds):
    """a batch of 5 with refused inputs at rows 1 and 4"""
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, name)(*args, **kw)
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(5)])
    for r in (1, 4):
        xs[r] = make_bad(blob, xs[r])
    ctx = dpa.Context.generate(dev, blob)
    try:
        out, reasons, words = _check(ctx, blob, xs)
        print(name, "reasons", reasons, "host:", words)
        assert [int(r) != 0 for r in reasons] == [False, True, False, False, True]
        assert word is None or words[1] == words[4] == word
        assert words[1] == words[4]
        # the plain call refuses the whole batch, with the host's word; on the good rows alone it gives the checked call's integers
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(xs, all_kinds=True)
        assert ei.value.code == -1 and words[1] in str(ei.value), str(ei.value)
        plain, _ = ctx.infer(xs[[0, 2, 3]], all_kinds=True)
        assert (plain == out[[0, 2, 3]]).all()
        if not needs_all_kinds:  # (kinds 0-13: the same under the empty flag word)
            o0, r0, _ = ctx.infer_checked(xs)
            assert (o0 == out).all() and (r0 == reasons).all()
        out, reasons, _ = _check(ctx, blob, xs)  # (and the model stays usable)
    finally:
        ctx.free()


TL = ("transformer_layer", (16, 64, 4, 16, 128), dict(config=65))


def test_first_failure_wins_and_the_softmax_step_skips_refused_samples(dev):
    """rows 0, 4 and 8 of 9 are refused by the first LayerNorm of the transformer layer: whatever the Softmax of the Mha node and the nodes behind it
    make of those samples, the reason stays 4 and every other row is the host's. A sample only the SECOND LayerNorm refuses — behind the Softmax
    step — gets 4 as well."""
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, TL[0])(*TL[1], **TL[2])
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(9)])
    xs[[0, 4, 8], 5] = LN_BAD
    ctx = dpa.Context.generate(dev, blob)
    try:
        out, reasons, words = _check(ctx, blob, xs)
        assert [words[i] for i in (0, 4, 8)] == ["layernorm"] * 3
        assert list(reasons) == [4, 0, 0, 0, 4, 0, 0, 0, 4]
        assert len({out[i].tobytes() for i in (1, 2, 3, 5, 6, 7)}) > 1 and not out[[0, 4, 8]].any()
        n = xs.shape[1] // 3  # (three input tensors: X, X for the residual, H — the input of the second LayerNorm)
        ys = xs[1:4].copy()
        ys[1, 2 * n + 7] = LN_BAD
        _, reasons, words = _check(ctx, blob, ys)
        assert list(reasons) == [0, 4, 0] and words[1] == "layernorm"
    finally:
        ctx.free()


def test_refused_rows_in_every_chunk(tmp_path):
    """128 inputs under a scratch bound of 1 MB: the chunk size c comes from the `[dp infer]` line of an all-good checked call; then rows 0, c - 1, c,
    the whole second chunk and the last row are refused. The plain call stops at the first failing chunk; the checked call serves all of them"""
    import deep_prove_amd as dpa
    sys.path.insert(0, os.path.dirname(CHILD))
    import infer_checked_child
    import infer_tables_child
    batch = 128
    res = str(tmp_path / "checked.npz")
    r = subprocess.run([sys.executable, CHILD, str(batch), res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1", DP_INFER_SCRATCH_MB="1"))
    assert r.returncode == 0 and "infer checked child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert len(lines) == 2, r.stderr[-2000:]
    z = np.load(res)
    c, nchunks, bad = int(z["chunk"]), int(z["nchunks"]), [int(b) for b in z["bad"]]
    assert nchunks >= 3 and nchunks == -(-batch // c) and bad == infer_checked_child.bad_rows(batch, c) and set(range(c, 2 * c)) <= set(bad)
    assert lines[0].endswith("; checked, refused 0") and lines[1].endswith(f"; checked, refused {len(bad)}"), lines
    assert f"batch {batch} in {nchunks} chunks of {c}," in lines[1]
    mb = infer_tables_child.build()
    blob = mb.blob()
    xs = infer_tables_child.inputs(mb, batch)
    want, want_reasons, _ = _host(blob, xs, z["good"].shape[1])
    assert not want_reasons.any() and not z["good_reasons"].any() and (z["good"] == want).all()
    xs[bad, infer_checked_child.BAD_ELEMENT] = infer_checked_child.BAD_VALUE
    wb, wr, words = _host(blob, xs[bad], want.shape[1])
    assert (wr == 4).all() and set(words) == {"layernorm"} and not wb.any()
    want[bad] = 0
    want_reasons[bad] = 4
    assert (z["reasons"] == want_reasons).all(), (z["reasons"], want_reasons)
    assert (z["out"] == want).all(), np.argwhere(z["out"] != want)[:5]


def test_edges(dev):
    import deep_prove_amd as dpa
    # one input, good and bad; a batch in which every input is refused
    mb = dpa.models.layernorm_mlp(4, 8, 16, config=33)
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(4)])
    ctx = dpa.Context.generate(dev, blob)
    try:
        _, reasons, _ = _check(ctx, blob, xs[:1])
        assert list(reasons) == [0]
        xs[:, 9] = LN_BAD
        _, reasons, _ = _check(ctx, blob, xs[:1])
        assert list(reasons) == [4]
        out, reasons, _ = _check(ctx, blob, xs)
        assert list(reasons) == [4, 4, 4, 4] and not out.any()
    finally:
        ctx.free()
    # all-good batches of 65: no reason, the integers of the plain call
    for mb, all_kinds in ((dpa.models.mha_block(8, 16, 2, 8, config=97), True), (dpa.models.dense_128(), False)):
        xs = np.stack([mb.input(1000 + i) for i in range(65)])
        ctx = dpa.Context.generate(dev, mb.blob())
        try:
            out, reasons, ms = ctx.infer_checked(xs, all_kinds=all_kinds)
            plain, _ = ctx.infer(xs, all_kinds=all_kinds)
            assert not reasons.any() and out.shape == plain.shape and (out == plain).all() and ms > 0
            assert (out[[0, 64]] == np.stack([dpa.infer_host(mb.blob(), xs[i]) for i in (0, 64)])).all()
        finally:
            ctx.free()
    # errors of the call stay errors of the call
    mb = dpa.models.gelu_mlp(256, config=112)
    x = mb.input(1000)[None, :]
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        for call in (lambda: ctx.infer_checked(x), lambda: dpa.infer_checked(ctx, x, flags=0)):
            with pytest.raises(dpa.DeepProveError) as ei:
                call()
            assert ei.value.code == -1 and re.search(r"node \d+ is a GELU layer \(kind 17\)", str(ei.value)), str(ei.value)
        for flags in (2, 3, 1 << 31):
            with pytest.raises(dpa.DeepProveError) as ei:
                dpa.infer_checked(ctx, x, flags=flags)
            assert ei.value.code == -1 and "flag" in str(ei.value), (flags, str(ei.value))
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.infer_checked(ctx, x[:, :3], all_kinds=True)
        assert "input length" in str(ei.value)
        _check(ctx, mb.blob(), x)
    finally:
        ctx.free()


def test_screened_proving(dev):
    """prove_batch discards a batch in which the host inference of one input throws; prove_batch_screened proves the rest"""
    import deep_prove_amd as dpa
    mb = dpa.models.mha_block(4, 8, 2, 4, config=37)
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(5)])
    xs[[1, 3], 3] = LN_BAD
    ctx = dpa.Context.generate(dev, blob)
    try:
        pr = dpa.Prover(ctx)
        p0, o0 = pr.prove(xs[0])
        with pytest.raises(dpa.DeepProveError) as ei:
            pr.prove_batch(xs, 4)
        assert "layernorm" in str(ei.value)
        screened, screened_reasons, _ = _check(ctx, blob, xs)
        proofs, outs, reasons, ms = pr.prove_batch_screened(xs, 4)
        assert list(reasons) == [0, 4, 0, 4, 0] and (reasons == screened_reasons).all()
        assert [p is None for p in proofs] == [False, True, False, True, False] and ms > 0
        assert (outs == screened).all() and not outs[[1, 3]].any()
        vb = ctx.verifier_blob()
        for i in (0, 2, 4):
            dpa.verify(vb, proofs[i], xs[i], outs[i])
        p1, o1 = pr.prove(xs[0])
        assert p0.size == p1.size and (p0 == p1).all() and (o0 == o1).all() and (o0 == outs[0]).all()
        assert proofs[0].size == p0.size and (proofs[0] == p0).all()
        # nothing to prove: prove_batch is not called
        called = []
        pr.prove_batch = lambda *a: called.append(a)
        proofs, outs, reasons, ms = pr.prove_batch_screened(xs[[1, 3]], 4)
        assert proofs == [None, None] and list(reasons) == [4, 4] and not outs.any() and not called
    finally:
        ctx.free()
