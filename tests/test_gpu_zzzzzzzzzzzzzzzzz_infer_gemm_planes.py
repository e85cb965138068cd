"""Table-valued tensors as operands of the i8 MFMA (infer_range_plan of csrc/infer.h; k_infer_gemm_i8_pl and the int8 forms the producers write, csrc/infer_kernels.inc): a constant
product behind a GELU or an embedding sum takes the matrix units — an int8 copy within -128..127, two signed planes within -16384..16383. Exact equality with `mb.run(x)` and the host,
counts from the `[dp infer]` line of a child process: `_child` and `_exact` of test_gpu_zzzzzzzzzzzzzzzz_infer_gemm_rq.py. Dimensions are padded to powers of two: K, N are the live sizes."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(os.path.dirname(os.path.abspath(__file__)), "support")]
RQ = importlib.import_module("test_gpu_zzzzzzzzzzzzzzzz_infer_gemm_rq")
E, _child, _exact = RQ.E, RQ._child, RQ._exact
from support.decode_cases import gelu_lm, numpy_decode, prompts  # noqa: E402


def _gelu_model(in_scale):
    """gelu_mlp(16) whose last Requant is made for what its GELU gives, 128 * in_scale times the 8-bit range: that many more bits, that much smaller a multiplier (gelu_mlp's own refuses such sums)"""
    import deep_prove_amd as dpa
    mb, f = dpa.models.gelu_mlp(16, config=61, in_scale=in_scale), int(round(128 * in_scale))
    mb.layers[-1] = dict(kind=dpa.models.L_REQUANT, **dpa.models.requant_from_multiplier(2.5 / 4.0 / 127.0 / f, dpa.models.dense_output_bitsize(16) + f.bit_length() - 1))
    return mb, lambda batch: np.stack([mb.input(1000 + i) for i in range(batch)])


@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("in_scale,top", [(1.0 / 128.0, 127), (1.0 / 16.0, 16383), (1.0, 16383)], ids=["int8_copy", "planes_1_16", "planes_1"])
def test_a_product_behind_a_gelu_takes_the_matrix_units(tmp_path, in_scale, top, batch):
    """at 1 / 128 the table lies within int8 (an int8 copy, the existing kernel), at 1 / 16 and 1 within the planes. Without the range pass the second product is a k_infer_gemm_i64 launch"""
    import deep_prove_amd as dpa
    mb, inputs = _gelu_model(in_scale)
    peak = np.abs(dpa.models.gelu_apply(mb.layers[2], np.arange(-127, 128))).max()  # (what a Requant's output can reach)
    assert peak <= top and (peak > 127) == (top > 127)
    g = _child(tmp_path, [(mb, inputs(batch), E.ALL_KINDS)])[0]
    assert (g["gemm_i64"], g["gemm_i8"], g["fused"]) == (0, 2, 2), g["line"]
    _exact(g, mb, inputs(batch))


def test_no_mfma_switch_sends_the_gelu_product_back(tmp_path):
    mb, inputs = _gelu_model(1.0 / 16.0)
    g = _child(tmp_path, [(mb, inputs(5), E.ALL_KINDS)], DP_INFER_NO_MFMA="1")[0]
    assert (g["gemm_i8"], g["gemm_i64"], g["fused"]) == (0, 2, 0), g["line"]
    _exact(g, mb, inputs(5))


@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "relu"])
def test_token_lm_runs_both_products_on_the_matrix_units(tmp_path, gelu):
    import deep_prove_amd as dpa
    mb = dpa.models.token_lm(8, 32, 16, config=62, gelu=gelu)
    xs = np.stack([mb.input(1000 + i) for i in range(7)])
    g = _child(tmp_path, [(mb, xs, E.ALL_KINDS if gelu else 0)])[0]
    assert (g["gemm_i64"], g["gemm_i8"]) == (0, 2), g["line"]
    _exact(g, mb, xs)


def _sum_model(seq, k, n, table, operand, requant=False):
    """tokens -> Embeddings(table [vocab][k]) -> + operand [seq][k] -> MatMul k -> n (weights over -128..127, both in every column; a bias), optionally a Requant for |sum| <= k * 2^21"""
    import deep_prove_amd as dpa
    rng = np.random.default_rng(9000 + 100 * k + n)
    mb = dpa.models.ModelBuilder((seq,), 63)
    mb.embeddings(table.shape[0], k).add_const(1, 1, requant=False).matmul(n, bias=True, requant=False)
    kp, npad = mb.layers[2]["nrows"], mb.layers[2]["ncols"]
    t, c, w = np.zeros_like(mb.layers[0]["table"]), np.zeros((seq, kp), dtype=np.int64), np.zeros((kp, npad), dtype=np.int64)
    t[:table.shape[0], :k], c[:, :k], w[:k, :n] = table, operand, E.extreme_rows(rng, n, k).T
    mb.layers[0]["table"], mb.layers[1]["operand"], mb.layers[2]["weights"] = t, c.reshape(-1), w
    mb.layers[2]["bias"][:n] = rng.integers(-10 ** 6, 10 ** 6, size=n)
    if requant:
        mb.layers.append(dict(kind=dpa.models.L_REQUANT, **dpa.models.requant_from_multiplier(2.5 / math.sqrt(k) / 127.0 / 128.0, 22 + max(1, (kp - 1).bit_length()))))
    return mb


def _plane_tables(rng, vocab, seq, k):
    """a table within -8192..8191 and an addend within -8192..8192: the interval of the sum is exactly -16384..16383"""
    table, operand = rng.integers(-8192, 8192, size=(vocab, k), dtype=np.int64), rng.integers(-8192, 8193, size=(seq, k), dtype=np.int64)
    table[0, 0], table[1, 0], operand[0, 0], operand[1, 0] = -8192, 8191, -8192, 8192
    return table, operand


def test_plane_edges_and_the_boundary_of_the_planner(tmp_path):
    """-16384 (hi -128, lo 0), -129, -128, -1 (hi -1, lo 127), 0, 127, 128 and 16383 stand in the operand: a logical shift or an unsigned plane gives another product. One more in
    the addend — an interval up to 16384 — and the planner leaves the product on k_infer_gemm_i64"""
    seq, k, n = 8, 16, 16
    table, operand = _plane_tables(np.random.default_rng(5), 8, seq, k)
    table[2:, 1], operand[:, 1] = [-129, -128, -1, 0, 127, 128], 0  # (column 1 of the sum is the table entry)
    mb = _sum_model(seq, k, n, table, operand)
    xs = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [1, 0, 7, 6, 5, 4, 3, 2], [0, 0, 2, 2, 3, 3, 4, 4]], dtype=np.int64)
    sums = np.concatenate([(mb.layers[0]["table"][x] + mb.layers[1]["operand"].reshape(seq, -1)).reshape(-1) for x in xs])
    assert {-16384, -129, -128, -1, 0, 127, 128, 16383} <= set(sums.tolist()) and sums.min() == -16384 and sums.max() == 16383
    wide_operand = operand.copy()
    wide_operand[2, 0] = 8193  # (8191 + 8193 = 16384 is possible, whatever the tokens of the call are)
    wide = _sum_model(seq, k, n, table, wide_operand)
    a, b = _child(tmp_path, [(mb, xs, 0), (wide, xs, 0)])
    assert (a["gemm_i8"], a["gemm_i64"]) == (1, 0) and (b["gemm_i8"], b["gemm_i64"]) == (0, 1), (a["line"], b["line"])
    _exact(a, mb, xs), _exact(b, wide, xs)


# (K, N, seq) at batch 3, M = 3 seq rows. 16 x 3: one slice, the byte store (N = 4); 8 x 16: byte loads (K % 16 != 0); 130 x 80: K pads to 256 = two slices, the live part ends inside an
# MFMA step of the second, N to 128 = two column tiles; 256 x 64 at 96 rows: two row tiles, the second partial, tiles that straddle samples
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "no_fuse"])
@pytest.mark.parametrize("k,n,seq", [(16, 3, 8), (8, 16, 2), (130, 80, 8), (256, 64, 32)])
def test_two_plane_product_shapes(tmp_path, k, n, seq, fuse):
    mb = _sum_model(seq, k, n, *_plane_tables(np.random.default_rng(k + n), 16, seq, k), requant=True)
    xs = np.random.default_rng(seq).integers(0, 16, size=(3, seq), dtype=np.int64)
    xs[0, :2] = [0, 1]
    want = np.stack([mb.run(x) for x in xs])
    assert want.min() == -127 and want.max() == 127 and len(np.unique(want)) > 60
    g = _child(tmp_path, [(mb, xs, 0)], **({} if fuse else {"DP_INFER_NO_FUSE": "1"}))[0]
    assert (g["gemm_i8"], g["gemm_i64"], g["fused"], g["requant"]) == (1, 0, int(fuse), 1), g["line"]
    _exact(g, mb, xs)


def test_refusal_in_the_fused_epilogue_on_a_two_plane_input(tmp_path):
    """test_refusal_at_the_corner_of_a_partial_tile behind an embedding sum: rows (1, 2), (1, 300), (-128, 0), (-128, 1) of a [4][2] table (300: planes, no int8 copy), column 7 of the
    MatMul is (-128, 1), Requant of 14 bits. (-128, 1) gives 16385 there, one beyond 2^14, in the last live row and column; (-128, 0) gives exactly 2^14 and passes"""
    import deep_prove_amd as dpa
    mb = _sum_model(2, 2, 8, np.array([[1, 2], [1, 300], [-128, 0], [-128, 1]], dtype=np.int64), np.zeros((2, 2), dtype=np.int64))
    mb.layers[2]["weights"], mb.layers[2]["bias"] = np.array([[1] * 7 + [-128], [1] * 8], dtype=np.int64), np.zeros(8, dtype=np.int64)
    mb.layers.append(dict(kind=dpa.models.L_REQUANT, right_shift=8, fp_scale=0, fixed_point_multiplier=1, intermediate_bit_size=14))
    ok, bad = np.array([[0, 1], [1, 0], [0, 2]], dtype=np.int64), np.array([[0, 1], [1, 0], [0, 3]], dtype=np.int64)
    rows, reasons, msgs = E.host(mb.blob(), bad, 16)
    assert list(reasons) == [0, 0, 1] and not E.host(mb.blob(), ok, 16)[1].any()
    edge, chk, plain = _child(tmp_path, [(mb, ok, 0), (mb, bad, E.CHECKED), (mb, bad, 0)])
    assert edge["fused"] == chk["fused"] == plain["fused"] == 1 and edge["gemm_i64"] == 0, edge["line"]
    _exact(edge, mb, ok)
    assert list(chk["reasons"]) == [0, 0, 1] and (chk["out"] == rows).all() and (chk["out"][:2] == np.stack([mb.run(x) for x in bad[:2]])).all()
    assert all("requant: value exceeds intermediate bit size" in e for e in (plain["error"], msgs[2])) and plain["out"].size == 0, (plain["error"], msgs[2])


def test_decode_of_the_gelu_language_model_equals_numpy(dev):
    import deep_prove_amd as dpa
    mb, lens = gelu_lm(), [1, 2, 3, 5]
    ps, ctx = prompts(mb, 4), dpa.Context.generate(dev, mb.blob())
    try:
        tokens, length, stop, reasons, outs, _ = ctx.decode(ps, lens, 4, all_kinds=True)
    finally:
        ctx.free()
    for i, n in enumerate(lens):
        wt, wl, ws, wo = numpy_decode(mb, ps[i], n, 4)
        assert (tokens[i] == wt).all() and length[i] == wl and stop[i] == ws and reasons[i] == 0 and (outs[i] == wo).all(), i
