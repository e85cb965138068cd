"""k_infer_conv_i8_rq (csrc/infer_kernels.inc): a convolution, its Requant, a ReLU and a MaxPool behind it in one launch, planned by infer_fuse_plan (csrc/infer.h). Every comparison is exact equality with `mb.run(x)`
(numpy int64), dp_model_infer_host is the second witness; `conv_rq` (launches of the kernel) and the other counts are read from the `[dp infer]` line of a child process (tests/support/infer_edges_child.py)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_zzzzzzzzzzzzzzzz_infer_gemm_rq import E, ROOT, _child as _lines

pytestmark = pytest.mark.gpu
COUNTS = ("conv_rq", "conv", "conv_i8", "requant", "relu", "maxpool")


def _child(tmp_path, calls, **env):  # the dicts of test_gpu_..._infer_gemm_rq._child with the COUNTS of the line by name
    return [dict(g, **{k: int(re.search(r" %s (\d+) " % k, g["line"]).group(1)) for k in COUNTS}) for g in _lines(tmp_path, calls, **env)]


def _chain(shape, out_ch, kernel, relu, pool, dense=False):
    """conv + Requant (+ ReLU) (+ MaxPool) (+ Flatten and a Dense); weights uniform over -128..127 with -128 and 127 in every filter; the Requant's multiplier spreads the sums (standard deviation about
    5461 sqrt(fan_in)) to 2.5 x 43 either side of zero: both clamps, and between them both rounding directions"""
    import deep_prove_amd as dpa
    mb, per = dpa.models.ModelBuilder(shape, 127).conv(out_ch, kernel), shape[0] * kernel * kernel
    mb.layers[0]["filter"][:out_ch, :shape[0], :kernel, :kernel] = E.extreme_rows(np.random.default_rng(per + out_ch), out_ch, per).reshape(out_ch, shape[0], kernel, kernel)
    mb.layers[1] = dict(kind=dpa.models.L_REQUANT, **dpa.models.requant_from_multiplier(2.5 / math.sqrt(per) / 127.0, dpa.models.conv_output_bitsize(shape[0], kernel, kernel)))
    mb = mb.relu() if relu else mb
    mb = mb.maxpool() if pool else mb
    return mb.flatten().dense(5, requant=False) if dense else mb


def _upto(mb, x, n):  # the tensor behind layer n - 1 of mb on input x
    full, mb.layers = mb.layers, mb.layers[:n]
    y, mb.layers = mb.run(x), full
    return y


def _exact(g, mb, xs, counts):
    import deep_prove_amd as dpa
    want = np.stack([mb.run(x) for x in xs])
    assert tuple(g[k] for k in COUNTS) == counts, g["line"]
    assert g["error"] == "" and g["out"].shape == want.shape and (g["out"] == want).all(), (g["error"], np.argwhere(g["out"] != want)[:5], g["line"])
    assert all((g["out"][i] == dpa.infer_host(mb.blob(), xs[i])).all() for i in {0, len(xs) // 2, len(xs) - 1})


# (input shape, out channels, kernel, batch). (2,8,8): nn = 64 shorter than a strip, kw = 4 below the channel tile, a pooled row of 16 bytes. (2,16,16) x65: a strip must not cross a sample, 8 rows per strip.
# (4,32,32): CNN-264k's first conv, the vertical pool pair lies in two waves. (12,16,16): kw = 64, u0 = 33 inside the second channel tile, several K slices. (1,64,64): nw = 64, a strip is one pooled row.
# (1,128,128): nw = 128, the MaxPool is NOT absorbed and k_infer_maxpool runs behind the fused Requant (+ ReLU): MaxPool chains only
SHAPES = [((2, 8, 8), 3, 3, 1), ((2, 16, 16), 3, 3, 65), ((4, 32, 32), 12, 5, 3), ((12, 16, 16), 33, 5, 2), ((1, 64, 64), 2, 3, 2), ((1, 128, 128), 2, 3, 1)]
CHAINS = {"requant": (False, False), "requant_relu": (True, False), "requant_relu_maxpool": (True, True), "requant_maxpool": (False, True)}


@pytest.mark.parametrize("shape,out_ch,kernel,batch,chain", [s + (c,) for s in SHAPES for c in CHAINS if s[0][1] < 128 or CHAINS[c][1]])
def test_fused_conv_chain_equals_numpy_and_the_host(tmp_path, shape, out_ch, kernel, batch, chain):
    relu, pool = CHAINS[chain]
    mb = _chain(shape, out_ch, kernel, relu, pool)
    xs = E.gemm_inputs(mb, batch)
    rq = _upto(mb, xs[0], 2)
    assert all(x.min() == -128 and x.max() == 127 for x in xs) and all(f.min() == -128 and f.max() == 127 for f in mb.layers[0]["filter"][:out_ch])
    assert rq.min() == -127 and rq.max() == 127 and ((rq > -127) & (rq < 127) & (rq != 0)).any()
    _exact(_child(tmp_path, [(mb, xs, 0)])[0], mb, xs, (1, 1, 1, 1, int(relu), int(pool)))


@pytest.mark.parametrize("pool", [False, True], ids=["requant_relu", "requant_relu_maxpool"])
def test_the_int64_form_and_the_switches(tmp_path, pool):
    """the chain as the model's last node (its tensor is a model output: the int64 form is written from the tile) and under Flatten -> Dense (only the int8 copy is read), by default, under DP_INFER_NO_FUSE=1
    (the launches of before) and under DP_INFER_NO_MFMA=1 (k_infer_conv): the same integers"""
    calls = [(mb, E.gemm_inputs(mb, 5), 0) for mb in (_chain((2, 16, 16), 3, 3, True, pool), _chain((2, 16, 16), 3, 3, True, pool, dense=True))]
    for sub, env, rq, i8 in (("a", {}, 1, 1), ("b", {"DP_INFER_NO_FUSE": "1"}, 0, 1), ("c", {"DP_INFER_NO_MFMA": "1"}, 0, 0)):
        (tmp_path / sub).mkdir()
        for g, (mb, xs, _) in zip(_child(tmp_path / sub, calls, **env), calls):
            _exact(g, mb, xs, (rq, 1, i8, 1, 1, int(pool)))


def test_refusal_of_the_sample_in_the_middle(tmp_path):
    """batch 3: samples 0 and 2 are a quarter of the range, sample 1 the full range, and the Requant's intermediate_bit_size is lowered to the largest one sample 1's sums cross"""
    mb = _chain((2, 16, 16), 3, 3, True, True)
    xs = E.gemm_inputs(mb, 3)
    xs[0], xs[2] = xs[0] // 4, xs[2] // 4
    peak = [int(np.abs(_upto(mb, x, 1)).max()) for x in xs]
    bits = mb.layers[1]["intermediate_bit_size"] = (peak[1] - 1).bit_length() - 1
    assert max(peak[0], peak[2]) <= (1 << bits) < peak[1]
    rows, reasons, msgs = E.host(mb.blob(), xs, mb.run(xs[0]).size)
    chk, plain = _child(tmp_path, [(mb, xs, E.CHECKED), (mb, xs, 0)])
    assert chk["conv_rq"] == plain["conv_rq"] == 1 and list(reasons) == [0, 1, 0]
    assert list(chk["reasons"]) == [0, 1, 0] and (chk["out"] == rows).all() and not chk["out"][1].any() and (chk["out"][[0, 2]] == np.stack([mb.run(xs[0]), mb.run(xs[2])])).all()
    assert all("requant: value exceeds intermediate bit size" in e for e in (plain["error"], msgs[1])) and plain["out"].size == 0, (plain["error"], msgs[1])


TRACE = """
import sys, numpy as np
sys.path.insert(0, %r)
import deep_prove_amd as dpa
dev, mb = dpa.Device(0), dpa.models.cnn_tiny()
xs, ctx = np.stack([mb.input(1000 + i) for i in range(5)]), dpa.Context.generate(dev, mb.blob())
rows, _, outs, _, _ = ctx.infer_trace(xs)
assert (rows == np.stack([dpa.infer_host_trace(mb.blob(), x) for x in xs])).all() and (outs == np.stack([mb.run(x) for x in xs])).all()
ctx.free(); dev.close(); print("trace ok")
""" % ROOT


def test_shipped_cnn_models_and_tap_mode(tmp_path):
    """cnn_tiny and cnn_264k at batch 65: one launch per conv chain (1 / 2), the integers of numpy; the trace rows of cnn_tiny hold every tensor of the chain: `conv_rq 0` on that call"""
    import deep_prove_amd as dpa
    calls = [(mb, np.stack([mb.input(1000 + i) for i in range(65)]), 0) for mb in (dpa.models.cnn_tiny(), dpa.models.cnn_264k())]
    for g, (mb, xs, _), n in zip(_child(tmp_path, calls), calls, (1, 2)):
        assert (g["conv_rq"], g["conv"], g["conv_i8"], g["maxpool"]) == (n, n, n, n) and g["error"] == "" and (g["out"] == np.stack([mb.run(x) for x in xs])).all(), g["line"]
    r = subprocess.run([sys.executable, "-c", TRACE], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1"))
    assert r.returncode == 0 and "trace ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    assert [int(re.search(r" conv_rq (\d+) ", ln).group(1)) for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")] == [0], r.stderr[-2000:]
