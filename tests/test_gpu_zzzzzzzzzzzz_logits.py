"""Logits::Argmax (layer kind 18) on the GPU: the proof streams are byte for byte those of the host logic over the plain-loop double
(tests/golden/logits_models.json), alone and merged in a cohort; the two new kernels against numpy, word for word: k_infer_argmax (device
inference, int8 and int64 input forms; the `[dp infer]` line of a child process says which one served a call) and k_logits_cols (the diff and
one-hot columns of the proving step, through the test entry dp_test_logits_columns)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "infer_edges_child.py")  # (generic: model blobs + calls in, outputs + `[dp infer]` lines out)

from support import logits_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def proved(dev):
    """every case proved once in latency mode, 8 times in a batch with 4 in flight as ONE cohort of four members (DP_COHORT=4: the library's default
    sizing, in flight / 22 rounded up, would make four cohorts of one member, whose launches are not merged — every launch of the batch, k_logits_cols
    included, is then one kc launch with blockIdx.z = 0 .. 3), and 48 times with 48 in flight under the default sizing (cohorts of three members)"""
    import deep_prove_amd as dpa
    out = {}
    for name, (mb, x) in LC.cases().items():
        ctx = dpa.Context.generate(dev, mb.blob())
        try:
            pr = dpa.Prover(ctx)
            proof, y = pr.prove(x)
            xs = np.stack([x] * 8)
            before = os.environ.get("DP_COHORT")
            os.environ["DP_COHORT"] = "4"  # (read by the library at every batch call)
            try:
                proofs, ys, _ = pr.prove_batch(xs, 4)
            finally:
                if before is None:
                    del os.environ["DP_COHORT"]
                else:
                    os.environ["DP_COHORT"] = before
            proofs48, ys48, _ = pr.prove_batch(np.stack([x] * 48), 48)
            out[name] = dict(vb=ctx.verifier_blob().copy(), x=x, proof=proof.copy(), y=y, xs=xs, proofs=[p.copy() for p in proofs], ys=ys, numpy=mb.run(x),
                             sha48={LC.sha(p, np.uint64) for p in proofs48}, ys48=ys48, in_flight48=pr.in_flight())
        finally:
            ctx.free()
    return out


@pytest.mark.parametrize("name", LC.SMALL + LC.LARGE)
def test_stream_is_the_golden_one_alone_and_in_a_cohort(proved, name):
    g, p = LC.golden()[name], proved[name]
    assert (p["y"] == p["numpy"]).all() and LC.sha(p["y"], np.int64) == g["output"]
    assert p["proof"].size == g["stream_words"] and LC.sha(p["proof"], np.uint64) == g["stream"]
    for q, y in zip(p["proofs"], p["ys"]):
        assert (y == p["numpy"]).all() and q.size == g["stream_words"] and LC.sha(q, np.uint64) == g["stream"]
    assert p["in_flight48"] > 22 and p["sha48"] == {g["stream"]} and (p["ys48"] == p["numpy"][None, :]).all()  # (more than 22 in flight: cohorts of at least two)


@pytest.mark.parametrize("name", LC.SMALL + LC.LARGE)
def test_verifiers_accept_and_refuse_the_wrong_token(dev, proved, name):
    import deep_prove_amd as dpa
    p = proved[name]
    dpa.verify(p["vb"], p["proof"], p["x"], p["y"])
    res, _ = dpa.verify_batch(p["vb"], p["proofs"], p["xs"], p["ys"], dev=dev)  # Merkle paths authenticated on the device
    assert (res == 0).all(), res
    k = LC.cases()[name][0].layers[-1]["K"]
    wrong = p["ys"].copy()
    wrong[:, 0] = (wrong[:, 0] + 1) % k  # a token of the row that is not its argmax
    res, _ = dpa.verify_batch(p["vb"], p["proofs"], p["xs"], wrong, dev=dev)
    assert (res == -5).all(), res
    with pytest.raises(dpa.DeepProveError) as e:
        dpa.verify(p["vb"], p["proof"], p["x"], wrong[0])
    assert e.value.code == -5 and "logits: output claim evaluation check failed" in str(e.value)


# ---- k_infer_argmax

def _argmax_inputs(rows, k, batch, wide):
    """[batch][rows * k]: random rows within -128 .. 127 with, spread over the rows of the batch, ties at lanes 0 / 63 / 64 (the second wave-stride
    of a lane), an all-equal row, an all -128 row and a maximum in the last column. wide: one word of every sample is 128, so the inputs travel as
    int64 — the row that holds it has 127 | 128 side by side"""
    rng = np.random.default_rng(rows * 100003 + k * 17 + batch)
    x = rng.integers(-128, 127, size=(batch * rows, k), dtype=np.int64)  # (126 at the most: the planted maxima below stand alone)
    for r in range(batch * rows):
        kind = r % 6
        if kind == 0:
            for j in (0, 63, 64):
                if j < k:
                    x[r, j] = 127
        elif kind == 1:
            x[r] = 5
        elif kind == 2:
            x[r] = -128
        elif kind == 3:
            x[r, k - 1] = 127
        elif kind == 4 and k > 64:
            x[r, 64] = x[r, 63] = 127  # the tie is between two lanes' FIRST and SECOND element
    x = x.reshape(batch, rows * k)
    if wide:
        x[:, (rows - 1) * k] = 127
        x[:, (rows - 1) * k + 1 if k > 1 else 0] = 128
    return x


def test_device_argmax_is_numpy_and_the_host_for_both_input_forms(tmp_path):
    import deep_prove_amd as dpa
    calls, want = [], []
    for k in (2, 32, 64, 128, 4096):
        for rows in (2, 8):
            mb = dpa.models.logits_only(rows, k, config=44)
            for batch in (1, 3, 65):
                for wide in (False, True):
                    x = _argmax_inputs(rows, k, batch, wide)
                    calls.append((mb, x, 0))  # mode 0: the plain call, no DP_INFER_ALL_KINDS
                    want.append(x.reshape(batch, rows, k).argmax(axis=2))
    # the child of the inference edge tests, driven the same way
    models = []
    for mb, _, _ in calls:
        if not any(mb is m for m in models):
            models.append(mb)
    data = {"nmodels": len(models), "ncalls": len(calls)}
    for i, mb in enumerate(models):
        data["blob_%d" % i] = mb.blob()
    for c, (mb, x, mode) in enumerate(calls):  # (already grouped by model)
        data["model_%d" % c], data["x_%d" % c], data["mode_%d" % c] = [i for i, m in enumerate(models) if m is mb][0], x, mode
    src, res = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    r = subprocess.run([sys.executable, CHILD, src, res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1"))
    assert r.returncode == 0 and "infer edges child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert len(lines) == len(calls), r.stderr[-2000:]
    z = np.load(res)
    for c, (mb, x, _) in enumerate(calls):
        wide = bool((x > 127).any())
        assert str(z["error_%d" % c]) == "", str(z["error_%d" % c])
        assert re.search(r"inputs as (int8|int64),", lines[c]).group(1) == ("int64" if wide else "int8"), lines[c]
        assert int(re.search(r" argmax (\d+) ", lines[c]).group(1)) == 1, lines[c]
        got = z["out_%d" % c]
        assert got.shape == want[c].shape and (got == want[c]).all(), (mb.layers[-1], x.shape, np.argwhere(got != want[c])[:5])
        for i in range(x.shape[0]):  # ... and the host's answer, input by input
            assert (dpa.infer_host(mb.blob(), x[i]) == want[c][i]).all()


# ---- k_logits_cols

@pytest.mark.parametrize("rows,k", [(2, 2), (2, 64), (8, 128), (4, 4096)])
def test_logits_columns_kernel_word_for_word(dev, rows, k):
    import deep_prove_amd as dpa
    lib = C.CDLL(dpa.LIB_PATH)
    lib.dp_test_logits_columns.restype = C.c_int32
    lib.dp_test_logits_columns.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)] * 2
    rng = np.random.default_rng(rows * 4099 + k)
    x = rng.integers(-127, 128, size=(rows, k), dtype=np.int64)
    x[0] = -127                      # an all-equal row: the first column is chosen, every difference is zero
    x[1, k - 1] = 127; x[1, 0] = 127  # the maximum twice: the first wins
    idx, mx = x.argmax(axis=1), x.max(axis=1)
    bufs = [dpa.Mle.from_i64(dev, a.reshape(-1)) for a in (x, mx, idx)]
    d, o = C.c_void_p(), C.c_void_p()
    try:
        assert lib.dp_test_logits_columns(dev.h, bufs[0].h, bufs[1].h, bufs[2].h, C.byref(d), C.byref(o)) == 0
        diff, onehot = dpa.Mle(dev, d), dpa.Mle(dev, o)
        bufs += [diff, onehot]
        want_diff = ((mx[:, None] - x).astype(object) % P).astype(np.uint64).reshape(-1)  # (max - x) mod p: here 0 .. 254, canonical
        want_hot = np.zeros((rows, k), dtype=np.uint64)
        want_hot[np.arange(rows), idx] = 1
        assert (diff.to_numpy() == want_diff).all() and (onehot.to_numpy() == want_hot.reshape(-1)).all()
    finally:
        for b in bufs:
            b.free()


def test_logits_columns_of_negative_differences_are_canonical(dev):
    """the kernel subtracts in the field: a `max` below an entry (never the case in a proof) gives p - d, not a wrapped 64-bit word"""
    import deep_prove_amd as dpa
    lib = C.CDLL(dpa.LIB_PATH)
    lib.dp_test_logits_columns.restype = C.c_int32
    lib.dp_test_logits_columns.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)] * 2
    x = np.array([[-5, 7], [100, -100]], dtype=np.int64)
    mx, idx = np.array([-9, 0], dtype=np.int64), np.array([1, 0], dtype=np.int64)
    bufs = [dpa.Mle.from_i64(dev, a.reshape(-1)) for a in (x, mx, idx)]
    d, o = C.c_void_p(), C.c_void_p()
    try:
        assert lib.dp_test_logits_columns(dev.h, bufs[0].h, bufs[1].h, bufs[2].h, C.byref(d), C.byref(o)) == 0
        diff, onehot = dpa.Mle(dev, d), dpa.Mle(dev, o)
        bufs += [diff, onehot]
        assert [int(v) for v in diff.to_numpy()] == [(-9 + 5) % P, (-9 - 7) % P, (0 - 100) % P, 100]
        assert [int(v) for v in onehot.to_numpy()] == [0, 1, 1, 0]
    finally:
        for b in bufs:
            b.free()


# ---- next-token prediction end to end

def test_token_lm_device_inference_then_screened_batch(dev):
    import deep_prove_amd as dpa
    mb = dpa.models.token_lm(8, 16, 16, config=43)
    xs = np.stack([mb.input(1000 + i) for i in range(6)])
    want = np.stack([mb.run(x) for x in xs])
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        got, _ = ctx.infer(xs, all_kinds=True)  # (the GELU of the model needs the flag; the Logits node does not)
        assert (got == want).all()
        proofs, outs, reasons, _ = dpa.Prover(ctx).prove_batch_screened(xs, 4)
        assert (reasons == 0).all() and (outs == want).all()
        vb = ctx.verifier_blob()
        res, _ = dpa.verify_batch(vb, proofs, xs, outs, dev=dev)
        assert (res == 0).all(), res
    finally:
        ctx.free()
