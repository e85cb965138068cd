"""k_infer_gemm2_i8_rq (csrc/infer_kernels.inc): the product of two tensors of the batch with its Requant — and the Softmax in front of it — in one launch, planned by infer_fuse_plan
(csrc/infer.h). Every comparison is exact equality with `mb.run(x)` (numpy int64), dp_model_infer_host is the second witness; `gemm2_rq` (launches of the kernel) and the other counts
are read from the `[dp infer]` line of a child process (tests/support/infer_edges_child.py)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_zzzzzzzzzzzzzzzz_infer_gemm_rq import E, ROOT, _child as _lines

pytestmark = pytest.mark.gpu
COUNTS = ("gemm2_rq", "gemm2_i8", "softmax", "requant")
FINAL = ((0, 2, 1), (1, 0, 2), (1, 0, 2))  # the axis triples of mha_final_spec
PV_GAIN = 3.0 / 4096.0  # the Requant behind probabilities x V: row 0 of a head is V's own row (probability 4096 / 4096), so three times that reaches both clamps
QK_GAIN = 7.0 / 127.0   # (over sqrt(head_dim)) the Requant behind Q K^T: behind a LayerNorm the models' own 2.5 leaves the scores within +-80


def _child(tmp_path, calls, **env):
    return [dict(g, **{k: int(re.search(r" %s (\d+) " % k, g["line"]).group(1)) for k in COUNTS}) for g in _lines(tmp_path, calls, **env)]


def _chains(mb):
    """the nodes of mb's product -> Requant chains (the Requants behind a ConcatMatMul or an Mha node); those behind probabilities get PV_GAIN, those behind Q K^T QK_GAIN"""
    import deep_prove_amd as dpa
    M, out = dpa.models, []
    for i, (l, edges) in enumerate(mb.nodes):
        src = mb.nodes[edges[0][0]] if l["kind"] == M.L_REQUANT and edges[0][0] >= 0 else None
        if src is None or src[0]["kind"] not in (M.L_CONCAT_MATMUL, M.L_MHA):
            continue
        pv = src[0]["kind"] == M.L_MHA or mb.nodes[src[1][0][0]][0]["kind"] == M.L_SOFTMAX
        if pv or src[0]["left"] == (1, 2, 0):
            mb.nodes[i] = (dict(kind=M.L_REQUANT, **M.requant_from_multiplier(PV_GAIN if pv else QK_GAIN / math.sqrt(src[0]["a_shape"][2]), l["intermediate_bit_size"])), edges)
        out.append(i)
    return out


def _at(mb, x, node):  # the tensor behind node `node` of mb on input x
    keep, mb.outputs = mb.outputs, [(node, 0)]
    y, mb.outputs = mb.run(x), keep
    return y


def _sharp(rq):
    return rq.min() == -127 and rq.max() == 127 and ((rq > -127) & (rq < 127) & (rq != 0)).any()


def _exact(g, mb, xs, counts):
    import deep_prove_amd as dpa
    want = np.stack([mb.run(x) for x in xs])
    assert tuple(g[k] for k in COUNTS) == counts, g["line"]
    assert g["error"] == "" and g["out"].shape == want.shape and (g["out"] == want).all(), (g["error"], np.argwhere(g["out"] != want)[:5], g["line"])
    assert all((g["out"][i] == dpa.infer_host(mb.blob(), xs[i])).all() for i in {0, len(xs) // 2, len(xs) - 1})


# (model, seq, heads, head_dim, batch) -> (gemm2_rq, gemm2_i8, softmax, requant). seq 8, head_dim 8: one mostly empty tile, the byte stores, scores rows of 8 words. seq 64, head_dim 32: one
# K slice, half an N tile. seq 128, head_dim 64: two row tiles, two K slices, the second wholly above the diagonal of the first row tile. head_dim 128: two N tiles, and an Mha table of
# 2^15 entries (gathered through global memory; the others are staged in LDS). heads 1 and 4 (a model's dimensions are powers of two): a tile never crosses a head. batch 1 and 5.
SHAPES = [("attention_block", 8, 1, 8, 5, (2, 2, 0, 6)), ("transformer_block", 8, 4, 8, 5, (2, 2, 1, 7)), ("transformer_block", 64, 1, 32, 1, (2, 2, 1, 7)),
          ("mha_block", 128, 1, 64, 3, (1, 2, 1, 6)), ("attention_block", 128, 4, 64, 1, (2, 2, 0, 6)), ("mha_block", 16, 4, 128, 5, (1, 2, 1, 6))]


@pytest.mark.parametrize("model,seq,heads,head_dim,batch,counts", SHAPES)
def test_fused_chains_equal_numpy_and_the_host(tmp_path, model, seq, heads, head_dim, batch, counts):
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, model)(seq, 16, heads, head_dim, config=140)
    xs = np.stack([mb.input(1000 + i) for i in range(batch)])
    assert all(_sharp(_at(mb, xs[0], node)) for node in _chains(mb))
    _exact(_child(tmp_path, [(mb, xs, E.ALL_KINDS)])[0], mb, xs, counts)


@pytest.mark.parametrize("kind,wide,counts", [("mm", False, (1, 1, 0, 1)), ("mm", True, (0, 0, 0, 1)), ("a_t", False, (1, 1, 0, 1))])
def test_model_inputs_as_operands(tmp_path, kind, wide, counts):
    """a product of two MODEL INPUTS with its Requant: the chain is fused per call, when the inputs travel as int8, and keeps the 64-bit product when one word is 128 (wide). mm: MatMul2
    [32][16] x [16][64]; a_t: ConcatMatMul on A [2][16][32] read along its rows (IG2_AT: transposed on the way into LDS), B [16][2][16], the result permuted"""
    import deep_prove_amd as dpa
    g = dpa.models.GraphBuilder([32 * 16, 16 * 64] if kind == "mm" else [2 * 16 * 32, 16 * 2 * 16], 143)
    p = g.matmul2((-1, 0), (-1, 1), 16, 64) if kind == "mm" else g.concat_matmul((-1, 0), (-1, 1), (2, 16, 32), (16, 2, 16), (0, 1, 2), FINAL[1], FINAL[2])
    g.requant((p, 0), 1.5 / math.sqrt(16) / 127.0, dpa.models.dense_output_bitsize(16))
    xs = E.gemm_inputs(g, 3)
    if wide:
        xs[1, 7] = 128
    assert _sharp(g.run(xs[0]))
    _exact(_child(tmp_path, [(g, xs, 0)])[0], g, xs, counts)


def _sm_graph(C, R, D, tail=False):
    """input 0 [C][R][R] -> Softmax; input 1 [R][C D] -> MatMul -> Requant = V; probabilities x V laid out [R][C][D] -> Requant (node 4) (-> MatMul: tail)"""
    import deep_prove_amd as dpa
    g = dpa.models.GraphBuilder([C * R * R, R * C * D], 141)
    v = g.requant((g.matmul_const((-1, 1), C * D, C * D), 0), 2.5 / math.sqrt(C * D) / 127.0, dpa.models.dense_output_bitsize(C * D))
    av = g.concat_matmul((g.softmax((-1, 0), (C, R, R), in_scale=8.0 / 127.0), 0), (v, 0), (C, R, R), (R, C, D), *FINAL)
    ar = g.requant((av, 0), PV_GAIN, 12 + 8 + max(0, (R - 1).bit_length()) + 1)
    if tail:
        g.matmul_const((ar, 0), C * D, 16)
    return g


@pytest.mark.parametrize("tail", [False, True], ids=["model_output", "reader_behind"])
def test_the_int64_form_and_the_switches(tmp_path, tail):
    """the chain's last tensor as a model output (the int64 form is written from the tile) and under an i8 product (only the int8 copy is read): by default, under DP_INFER_NO_FUSE=1
    (the launches of before) and under DP_INFER_NO_MFMA=1 (the 64-bit product): the same integers"""
    mb = _sm_graph(2, 16, 16, tail)
    xs = E.gemm_inputs(mb, 5)
    for sub, env, rq, i8 in (("a", {}, 1, 1), ("b", {"DP_INFER_NO_FUSE": "1"}, 0, 1), ("c", {"DP_INFER_NO_MFMA": "1"}, 0, 0)):
        (tmp_path / sub).mkdir()
        _exact(_child(tmp_path / sub, [(mb, xs, E.ALL_KINDS)], **env)[0], mb, xs, (rq, i8, 1, 2))


TRACE = """
import sys, numpy as np
sys.path.insert(0, %r)
import deep_prove_amd as dpa
dev, mb = dpa.Device(0), dpa.models.mha_block(8, 16, 2, 8, config=97)
xs, ctx = np.stack([mb.input(1000 + i) for i in range(3)]), dpa.Context.generate(dev, mb.blob())
rows, _, outs, _, _ = ctx.infer_trace(xs, all_kinds=True)
assert (rows == np.stack([dpa.infer_host_trace(mb.blob(), x) for x in xs])).all() and (outs == np.stack([mb.run(x) for x in xs])).all()
ctx.free(); dev.close(); print("trace ok")
""" % ROOT


def test_tap_mode_and_a_layout_the_softmax_form_does_not_admit(tmp_path):
    """the trace rows of mha_block hold every tensor of the chain, the probabilities included: `gemm2_rq 0` on that call. transformer_block whose second product reads the probabilities
    transposed (left = (0, 1, 2)): its Softmax and that product keep their launches, `gemm2_rq` counts the Q K^T chain alone"""
    import deep_prove_amd as dpa
    r = subprocess.run([sys.executable, "-c", TRACE], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1"))
    assert r.returncode == 0 and "trace ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    assert [int(re.search(r" gemm2_rq (\d+) ", ln).group(1)) for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")] == [0], r.stderr[-2000:]
    mb = dpa.models.transformer_block(16, 16, 2, 16, config=142)
    mb.nodes[9][0]["left"] = (0, 1, 2)  # (node 9: probabilities x V)
    xs = np.stack([mb.input(1000 + i) for i in range(3)])
    _exact(_child(tmp_path, [(mb, xs, E.ALL_KINDS)])[0], mb, xs, (1, 2, 1, 7))


def test_refusal_of_the_sample_in_the_middle(tmp_path):
    """batch 3: V of samples 0 and 2 is an eighth of sample 1's, and the Requant's intermediate_bit_size is lowered to the largest one sample 1's sums cross: reasons [0, 1, 0]. Then
    sample 1 instead holds a score of 2^24 + 1: the host's shift step refuses it, and the Requant refusal of the fused launch behind it leaves the class SOFTMAX"""
    mb = _sm_graph(2, 16, 16)
    xs = E.gemm_inputs(mb, 3)
    xs[0, 512:], xs[2, 512:] = xs[0, 512:] // 8, xs[2, 512:] // 8  # (512 scores in front of V's input)
    peak = [int(np.abs(_at(mb, x, 3)).max()) for x in xs]
    bits = mb.nodes[4][0]["intermediate_bit_size"] = (peak[1] - 1).bit_length() - 1
    assert max(peak[0], peak[2]) <= (1 << bits) < peak[1]
    big = np.where(np.arange(xs.size).reshape(xs.shape) == xs.shape[1] + 5, (1 << 24) + 1, xs)
    for sub, x, cls, word in (("a", xs, 1, "requant: value exceeds intermediate bit size"), ("b", big, 5, "softmax: input out of range")):
        (tmp_path / sub).mkdir()
        rows, reasons, msgs = E.host(mb.blob(), x, mb.run(xs[0]).size)
        chk, plain = _child(tmp_path / sub, [(mb, x, E.ALL_KINDS | E.CHECKED), (mb, x, E.ALL_KINDS)])
        assert chk["gemm2_rq"] == 1 and list(reasons) == list(chk["reasons"]) == [0, cls, 0] and (chk["out"] == rows).all() and not chk["out"][1].any(), chk["line"]
        assert (chk["out"][[0, 2]] == np.stack([mb.run(x[0]), mb.run(x[2])])).all() and all(word in e for e in (plain["error"], msgs[1])) and plain["out"].size == 0, (plain["error"], msgs[1])
