"""k_infer_gemm_i8_rq (csrc/infer_kernels.inc): a Dense / MatMul / QKV product, its Requant and a ReLU behind it in one launch, planned by infer_fuse_plan (csrc/infer.h). Every
comparison is exact equality with `mb.run(x)` (numpy int64), dp_model_infer_host is the second witness; `fused` (launches of the kernel) and the other counts are read from the
`[dp infer]` line of a child process (tests/support/infer_edges_child.py)."""
import math
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


def _child(tmp_path, calls, **env):
    """calls: [(model, inputs[batch][input_len], mode)] -> per call a dict: out, error, reasons, line and the counts of the line by name"""
    data = {"nmodels": len(calls), "ncalls": len(calls)}
    for c, (mb, xs, mode) in enumerate(calls):
        data["blob_%d" % c], data["model_%d" % c], data["x_%d" % c], data["mode_%d" % c] = mb.blob(), c, np.ascontiguousarray(xs, dtype=np.int64), mode
    src, res = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    r = subprocess.run([sys.executable, CHILD, src, res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1", **env))
    assert r.returncode == 0 and "infer edges child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines, z = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")], np.load(res)
    assert len(lines) == len(calls), r.stderr[-2000:]
    got = [dict(out=z["out_%d" % c], error=str(z["error_%d" % c]), reasons=z["reasons_%d" % c] if "reasons_%d" % c in z else None, line=ln) for c, ln in enumerate(lines)]
    return [dict(g, **{k: int(re.search(r" %s (\d+) " % k, g["line"]).group(1)) for k in ("fused", "gemm_i8", "gemm_i64", "requant", "relu")}) for g in got]


def _chain(kind, k, n, seq, relu):
    """E.gemm_model with a Requant (and a ReLU) behind every product; the multiplier spreads the sums over -127..127 and reaches the clamp"""
    import deep_prove_amd as dpa
    mb = E.gemm_model(kind, k, n, seq)
    mult, bits = 2.5 / math.sqrt(k) / 127.0, dpa.models.dense_output_bitsize(max(k, 2))
    if kind != "qkv":
        mb.layers.append(dict(kind=dpa.models.L_REQUANT, **dpa.models.requant_from_multiplier(mult, bits)))
        return mb.relu() if relu else mb
    outs = [mb.requant((0, i), mult, bits) for i in range(3)]
    return mb.set_outputs([(mb.relu((o, 0)) if relu else o, 0) for o in outs])


def _exact(g, mb, xs):
    import deep_prove_amd as dpa
    want = np.stack([mb.run(x) for x in xs])
    assert g["error"] == "" and g["out"].shape == want.shape and (g["out"] == want).all(), (g["error"], np.argwhere(g["out"] != want)[:5], g["line"])
    assert all((g["out"][i] == dpa.infer_host(mb.blob(), xs[i])).all() for i in {0, len(xs) // 2, len(xs) - 1})


# (kind, K, N, seq, batch). A model's dimensions are padded to powers of two >= 2, so those are the sizes the kernel can meet, and a Requant takes no tensor below 4 words: 1 x 1 at two rows (K = N = 2, one live weight); N = 2, 4, 8
# (the byte path of the int8 store, a partial 16-byte group; odd N cannot occur), 16 and 64 (vectors), 128 (a second column tile); K = 2, 8 (byte loads), 64 (half a slice),
# 128 (one), 512 (four: the prefetch wraps three times); batch x seq = 63, 64, 65 rows (the row tile is 64); seq > 1: R > 1 and tiles that straddle samples (130 and 84 rows)
SHAPES = [("matmul", 1, 1, 2, 1), ("dense", 2, 4, 1, 63), ("dense", 64, 8, 1, 64), ("dense", 128, 16, 1, 65), ("dense", 512, 64, 1, 3), ("matmul", 16, 128, 2, 65), ("matmul_t", 32, 64, 4, 21),
          ("qkv", 8, 16, 2, 65)]


@pytest.mark.parametrize("relu", [False, True], ids=["requant", "requant_relu"])
@pytest.mark.parametrize("kind,k,n,seq,batch", SHAPES)
def test_fused_chain_equals_numpy_and_the_host(tmp_path, kind, k, n, seq, batch, relu):
    mb = _chain(kind, k, n, seq, relu)
    xs = E.gemm_inputs(mb, batch)
    assert all(x.min() == -128 and x.max() == 127 for x in xs)
    g, nprod = _child(tmp_path, [(mb, xs, 0)])[0], 3 if kind == "qkv" else 1
    assert (g["fused"], g["gemm_i8"], g["gemm_i64"], g["requant"], g["relu"]) == (nprod, nprod, 0, nprod, nprod * relu), g["line"]
    _exact(g, mb, xs)


def test_the_letter_of_requant_with_and_without_fusion(tmp_path):
    """requant_model's identity Dense passes the model input on, and the inputs of requant_rounding_inputs (up to 2^18) travel as int64: such a call is not fused. So the rounding
    cases reach the fused kernel through weights: 127 on the diagonal under (635 x + 128) >> 8 for every x of -128..127 (the clamp on both sides from |x| = 52 on), and below a
    Dense whose sums are exact ties on both signs. DP_INFER_NO_FUSE=1: the launches of before, the same integers"""
    import deep_prove_amd as dpa
    mb = E.requant_model()
    mb.layers[0]["weights"] = 127 * np.eye(8, dtype=np.int64)
    mb.layers[1] = dict(kind=dpa.models.L_REQUANT, right_shift=5, fp_scale=3, fixed_point_multiplier=5, intermediate_bit_size=14)
    xs = np.arange(-128, 128, dtype=np.int64).reshape(-1, 8)
    want = np.stack([mb.run(x) for x in xs])
    assert want.min() == -127 and want.max() == 127 and len(np.unique(want)) > 100
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir(), (tmp_path / "c").mkdir()
    a, b = _child(tmp_path / "a", [(mb, xs, 0)])[0], _child(tmp_path / "b", [(mb, xs, 0)], DP_INFER_NO_FUSE="1")[0]
    assert (a["fused"], a["gemm_i8"], a["requant"]) == (1, 1, 1) and (b["fused"], b["gemm_i8"], b["requant"]) == (0, 1, 1), (a["line"], b["line"])
    _exact(a, mb, xs), _exact(b, mb, xs)
    # exact ties: Dense 2 -> 4 with rows (64, 64) and (-64, -64), twice: v = +-64 (x0 + x1) under (v + 128) >> 8, ties at v = +-128 and +-384
    tie = dpa.models.ModelBuilder(2, 124)
    tie.dense(4, 2, requant=False)
    tie.layers[0]["weights"], tie.layers[0]["bias"] = np.array([[64, 64], [-64, -64]] * 2, dtype=np.int64), np.zeros(4, dtype=np.int64)
    tie.layers.append(dict(kind=dpa.models.L_REQUANT, right_shift=8, fp_scale=0, fixed_point_multiplier=1, intermediate_bit_size=15))
    tx = np.array([[1, 1], [-1, -1], [3, 3], [-3, -3], [127, 127], [-128, -128]], dtype=np.int64)
    assert [list(tie.run(x)[:2]) for x in tx[:4]] == [[1, 0], [0, 1], [2, -1], [-1, 2]]
    g = _child(tmp_path / "c", [(tie, tx, 0)])[0]
    assert g["fused"] == 1, g["line"]
    _exact(g, tie, tx)


def test_refusal_at_the_corner_of_a_partial_tile(tmp_path):
    """MatMul [2][2] x [2][8], Requant of 14 bits, three samples = 6 rows x 8 columns of one tile. Column 7 is (-128, 1): the last row of sample 2 = (-128, 1) gives 16385 there, one
    beyond 2^14, in the last live row and column; (-128, 0) gives exactly 2^14 and passes"""
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder((2, 2), 125)
    mb.matmul(8, bias=False, requant=False)
    mb.layers[0]["weights"] = np.array([[1] * 7 + [-128], [1] * 8], dtype=np.int64)
    mb.layers.append(dict(kind=dpa.models.L_REQUANT, right_shift=8, fp_scale=0, fixed_point_multiplier=1, intermediate_bit_size=14))
    ok = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [1, 1, -128, 0]], dtype=np.int64)
    bad = np.where(np.arange(12).reshape(3, 4) == 11, 1, ok)
    rows, reasons, msgs = E.host(mb.blob(), bad, 16)
    assert list(reasons) == [0, 0, 1] and not E.host(mb.blob(), ok, 16)[1].any() and (bad[2].reshape(2, 2) @ mb.layers[0]["weights"])[1, 7] == (1 << 14) + 1
    edge, chk, plain = _child(tmp_path, [(mb, ok, 0), (mb, bad, E.CHECKED), (mb, bad, 0)])
    assert edge["fused"] == chk["fused"] == plain["fused"] == 1
    _exact(edge, mb, ok)
    assert list(chk["reasons"]) == [0, 0, 1] and (chk["out"] == rows).all() and (chk["out"][:2] == np.stack([mb.run(x) for x in bad[:2]])).all()
    assert all("requant: value exceeds intermediate bit size" in e for e in (plain["error"], msgs[2])) and plain["out"].size == 0, (plain["error"], msgs[2])


def _graph(shape):
    """MatMul 4 x 16 -> 16 (node 0) with what `shape` puts behind it; the Requants are 2.5 / 4 / 127 at the bit size of a Dense of 16"""
    import deep_prove_amd as dpa
    g = dpa.models.GraphBuilder([64, 64] if shape == "add2" else [64], 126)
    mult, bits = 2.5 / 4 / 127.0, dpa.models.dense_output_bitsize(16)
    p = g.matmul_const((-1, 0), 16, 16)
    r = g.relu((g.requant((p, 0), mult, bits), 0))
    if shape == "add2":
        g.add2((r, 0), (-1, 1), 3, 5)
    elif shape in ("fallback", "i8_product"):
        q = g.matmul_const((r, 0), 16, 16)
        if shape == "fallback":
            g.nodes[q][0]["weights"][3, 5] = 128
    return g


@pytest.mark.parametrize("shape,fused,gemm_i64", [("output", 1, 0), ("add2", 1, 0), ("fallback", 1, 1), ("i8_product", 1, 0)])
def test_elision_keeps_every_int64_form_that_is_read(tmp_path, shape, fused, gemm_i64):
    """the chain's last tensor as model output, under an Add2, under a 64-bit product (a weight of 128): its int64 form is written; under another i8 product: elided. (The library's
    graph check gives every tensor exactly one reader: a Requant or a product with two readers cannot be built, infer_fuse_plan's reader counts guard programs made otherwise.)"""
    mb = _graph(shape)
    xs = E.gemm_inputs(mb, 5)
    g = _child(tmp_path, [(mb, xs, 0)])[0]
    assert (g["fused"], g["gemm_i64"]) == (fused, gemm_i64), g["line"]
    _exact(g, mb, xs)


TAPS_AND_DECODE = """
import sys, numpy as np
sys.path[:0] = [%r, %r]
import deep_prove_amd as dpa
from support.decode_cases import relu_lm, prompts
dev, mb, lm = dpa.Device(0), dpa.models.mlp(2, 64, config=7), relu_lm()
xs, ps = np.stack([mb.input(1000 + i) for i in range(5)]), prompts(lm, 4)
ctx = dpa.Context.generate(dev, mb.blob())
rows, _, outs, _, _ = ctx.infer_trace(xs)
assert (rows == np.stack([dpa.infer_host_trace(mb.blob(), x) for x in xs])).all() and (outs == ctx.infer(xs)[0]).all()
ctx.free()
ctx = dpa.Context.generate(dev, lm.blob())
tokens, length, stop, reasons, outs, _ = ctx.decode(ps, [1, 2, 3, 5], 4)
for i, n in enumerate([1, 2, 3, 5]):
    wt, wl, ws, wr, wo = dpa.decode_host(lm.blob(), ps[i][:n], n, 4)
    assert (tokens[i] == wt).all() and length[i] == wl and stop[i] == ws and reasons[i] == wr == 0 and (outs[i] == wo).all(), i
ctx.infer(tokens)
ctx.free(); dev.close()
print("taps and decode ok")
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_tap_mode_is_not_fused_and_decode_is():
    """the trace rows of an MLP of three Dense hold every tensor: `fused 0` on the tap call, 3 on the plain call behind it; a decode of the ReLU language model equals dp_model_decode_host"""
    r = subprocess.run([sys.executable, "-c", TAPS_AND_DECODE], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1"))
    assert r.returncode == 0 and "taps and decode ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    fused = [int(re.search(r" fused (\d+) ", ln).group(1)) for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert fused == [0, 3, 2], r.stderr[-2000:]
