"""k_infer_gemm2_i8 (csrc/infer_kernels.inc): the product of two tensors of the batch on the i8 MFMA. Every comparison is exact equality with `mb.run(x)` (numpy int64),
dp_model_infer_host is the second witness; which kernel served a call is read from the `[dp infer]` line of a child process (tests/support/infer_edges_child.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "infer_edges_child.py")
sys.path.insert(0, os.path.dirname(CHILD))
import infer_edges_child as E  # noqa: E402

QK, FINAL = ((1, 2, 0), (1, 2, 0), None), ((0, 2, 1), (1, 0, 2), (1, 0, 2))  # the axis triples of mha_qk_spec / mha_final_spec


def _child(tmp_path, calls, mode=0, **env):
    data = {"nmodels": len(calls), "ncalls": len(calls)}
    for c, (mb, xs) in enumerate(calls):
        data["blob_%d" % c], data["model_%d" % c], data["x_%d" % c], data["mode_%d" % c] = mb.blob(), c, np.ascontiguousarray(xs, dtype=np.int64), mode
    src, res = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")  # one plain call per (model, inputs) -> out, the launch counts, inputs, line
    np.savez(src, **data)
    r = subprocess.run([sys.executable, CHILD, src, res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1", **env))
    assert r.returncode == 0 and "infer edges child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines, z = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")], np.load(res)
    assert len(lines) == len(calls) and all(str(z["error_%d" % c]) == "" for c in range(len(calls))), r.stderr[-2000:]
    got = [dict(out=z["out_%d" % c], inputs=re.search(r"inputs as (int8|int64),", ln).group(1), line=ln) for c, ln in enumerate(lines)]
    return [dict(g, **{k: int(re.search(r" %s (\d+) " % k, g["line"]).group(1)) for k in ("gemm2_i8", "gemm_i8", "gemm_i64")}) for g in got]


def _product(kind, C, R, K, N):
    """one product of two model inputs, no Requant behind it. mm / mm_t: MatMul2 [R][K] x [K][N] / x [N][K]; qk: A [R][C][K], B [N][C][K];
    final: A [C][R][K], B [K][C][N], result laid out [R][C][N]; a_concat: the qk product on A [R][K][C] (A's concat axis contiguous)"""
    import deep_prove_amd as dpa
    g = dpa.models.GraphBuilder([C * R * K, C * K * N], 125)
    if kind in ("mm", "mm_t"):
        g.matmul2((-1, 0), (-1, 1), K, N, transpose_b=kind == "mm_t")
    elif kind == "a_concat":
        g.concat_matmul((-1, 0), (-1, 1), (R, K, C), (N, C, K), (2, 1, 0), (1, 2, 0))
    else:
        left, right, perm = QK if kind == "qk" else FINAL
        g.concat_matmul((-1, 0), (-1, 1), (R, C, K) if kind == "qk" else (C, R, K), (N, C, K) if kind == "qk" else (K, C, N), left, right, perm)
    return g


def _check(g, mb, xs, served, inputs="int8"):
    import deep_prove_amd as dpa
    assert (g["gemm2_i8"], g["gemm_i64"]) == ((1, 0) if served else (0, 1)) and g["gemm_i8"] == g["gemm2_i8"] and g["inputs"] == inputs, g["line"]
    want = np.stack([mb.run(x) for x in xs])
    assert g["out"].shape == want.shape and (g["out"] == want).all(), np.argwhere(g["out"] != want)[:5]
    assert all((g["out"][i] == dpa.infer_host(mb.blob(), xs[i])).all() for i in {0, len(xs) // 2, len(xs) - 1})


CASES = [("mm", 1, 2, 2, 2, 65, False), ("mm", 1, 32, 16, 64, 3, False), ("mm_t", 1, 64, 64, 32, 65, False), ("mm_t", 1, 128, 128, 2, 3, False), ("qk", 2, 64, 64, 64, 3, False),
         ("qk", 4, 2, 16, 128, 65, False), ("final", 4, 64, 64, 16, 3, False), ("final", 2, 4, 4, 2, 3, False), ("final", 1, 128, 128, 128, 1, False), ("mm", 1, 32, 64, 64, 3, True),
         ("final", 2, 32, 64, 32, 3, True)]  # (kind, C, R, K, N, batch, asymmetric): what each covers is in the docstring below


@pytest.mark.parametrize("kind,C,R,K,N,batch,asymmetric", CASES)
def test_gemm2_i8_equals_numpy_and_the_host(tmp_path, kind, C, R, K, N, batch, asymmetric):
    """mm 2x2x2 x65: rows of 2 bytes, samples of 8 (nothing is 16-aligned), one live wave. mm 32x16x64: one fragment of k, B read along n and transposed. mm_t 64x64x32 x65: both
    operands along k, one slice, a tile must not leak into the next sample. mm_t 128x128x2: two row tiles, two slices. qk: the products of an Mha node per head (C = 2, 4; N = 128: two
    column tiles). final: B [K][C][N] transposed on the way into LDS, the result permuted to [R][C][N]; 4x4x2 takes the byte path of the transposing loads. Asymmetric: A is non-zero
    only in its last k, B only in its first row (m = 0): every sum is 0, and a swapped axis or a wrong transposition pairs the two. Inputs: -128 and 127 in every sample."""
    mb = _product(kind, C, R, K, N)
    xs = E.gemm_inputs(mb, batch)
    if asymmetric:
        a, b = xs[:, :C * R * K].reshape((batch, C, R, K) if kind == "final" else (batch, R, C, K)), xs[:, C * R * K:].reshape((batch, K, C * N) if kind != "mm_t" else (batch, N, K))
        a[..., :K - 1], b[:, 1:] = 0, 0
        a[:, 0, 0, K - 1], b[:, 0, 0] = -128, 127
        assert 0 < np.count_nonzero(xs) <= batch * C * (R + N) and not mb.run(xs[0]).any()
    assert all(x.min() == -128 and x.max() == 127 for x in xs)
    _check(_child(tmp_path, [(mb, xs)])[0], mb, xs, True)


def test_accumulator_bound(tmp_path):
    """MatMul2 2 x K x 2 on -128 everywhere: K = 2^16 is the last the 32-bit accumulator holds (every sum 2^30), K = 2^17 goes to the 64-bit kernel (2^31)"""
    calls = [(mb, np.full((1, mb.input_len), -128, dtype=np.int64)) for mb in (_product("mm", 1, 2, 1 << 16, 2), _product("mm", 1, 2, 1 << 17, 2))]
    for (mb, xs), g, lk in zip(calls, _child(tmp_path, calls), (16, 17)):
        _check(g, mb, xs, lk == 16)
        assert (g["out"] == 1 << (lk + 14)).all()


def _softmax_times_v(C, R, D, a_is_softmax=True):
    """Softmax over input 0 ([C][R][R]), then the mha_final_spec product with input 1 ([R][C][D]) as V; or the probabilities as the RIGHT operand of a MatMul2 (input 1 [R][C * R])"""
    import deep_prove_amd as dpa
    g = dpa.models.GraphBuilder([C * R * R, R * C * D if a_is_softmax else R * C * R], 126)
    sm = g.softmax((-1, 0), (C, R, R), in_scale=8.0 / 127.0)
    g.concat_matmul((sm, 0), (-1, 1), (C, R, R), (R, C, D), *FINAL) if a_is_softmax else g.matmul2((-1, 1), (sm, 0), C * R, R)
    return g


@pytest.mark.parametrize("C,R,D", [(2, 4, 2), (4, 64, 16)])
def test_two_plane_probabilities(tmp_path, C, R, D):
    import deep_prove_amd as dpa
    mb = _softmax_times_v(C, R, D)
    xs = E.gemm_inputs(mb, 3, seed=1)
    probs = np.stack([dpa.models.softmax_only(C, R, config=126, in_scale=8.0 / 127.0).run(x[:C * R * R]) for x in xs])
    assert (probs == 0).any() and ((probs >= 1) & (probs <= 127)).any() and ((probs >= 128) & (probs % 128 != 0)).any() and (probs == 4096).any() and probs.max() <= 4096
    g = _child(tmp_path, [(mb, xs)], mode=E.ALL_KINDS)[0]
    _check(g, mb, xs, True)


def test_attention_models_with_and_without_the_mfma(tmp_path):
    """mha_block and transformer_block: Q K^T on int8 copies, probabilities (two planes) x V; DP_INFER_NO_MFMA=1 restores the 64-bit kernel"""
    import deep_prove_amd as dpa
    models = [dpa.models.mha_block(8, 16, 2, 8, config=97), dpa.models.transformer_block(8, 16, 2, 8, config=98)]
    calls = [(mb, np.stack([mb.input(1000 + i) for i in range(3)])) for mb in models]
    want = [np.stack([mb.run(x) for x in xs]) for mb, xs in calls]
    (tmp_path / "mfma").mkdir(), (tmp_path / "valu").mkdir()
    for a, b, w in zip(_child(tmp_path / "mfma", calls, mode=E.ALL_KINDS), _child(tmp_path / "valu", calls, mode=E.ALL_KINDS, DP_INFER_NO_MFMA="1"), want):
        assert a["gemm2_i8"] == 2 and b["gemm2_i8"] == 0 and b["gemm_i8"] == 0 and b["gemm_i64"] == a["gemm_i8"] + a["gemm_i64"], (a["line"], b["line"])
        assert (a["out"] == w).all() and (b["out"] == w).all()


def test_fallbacks_stay_on_the_64_bit_kernel(tmp_path):
    """A's concat axis contiguous; one input word of 128 (inputs as int64); a Softmax output as the right operand"""
    mb = _product("mm", 1, 32, 16, 64)
    big = np.where(np.arange(3 * mb.input_len).reshape(3, -1) == mb.input_len + 5, 128, E.gemm_inputs(mb, 3))
    calls = [(_product("a_concat", 2, 4, 4, 4), None, 0), (mb, big, 0), (_softmax_times_v(2, 4, 2, a_is_softmax=False), None, E.ALL_KINDS)]
    for i, (m, xs, mode) in enumerate(calls):
        xs = E.gemm_inputs(m, 3) if xs is None else xs
        (tmp_path / str(i)).mkdir()
        _check(_child(tmp_path / str(i), [(m, xs)], mode=mode)[0], m, xs, False, "int64" if i == 1 else "int8")
