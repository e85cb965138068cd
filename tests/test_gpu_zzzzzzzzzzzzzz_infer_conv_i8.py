"""k_infer_conv_i8 (csrc/infer_kernels.inc): a convolution of dp_model_infer on the i8 MFMA, over the packed filter image of infer_conv_pack. Every
comparison is exact equality with `mb.run(x)` (numpy, direct correlation); which kernel served a call is read from the `[dp infer]` line of a
child process (tests/support/infer_edges_child.py, driven as tests/test_gpu_zzzzzzzzzz_infer_edges.py drives it)."""
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


def _numpy(mb, xs):
    return np.stack([mb.run(x) for x in xs])


def _child(tmp_path, calls, **env):
    """calls: [(model, inputs[batch][input_len])], one plain call each -> per call a dict: out, conv, conv_i8 (launches), inputs ("int8" | "int64"), line"""
    data = {"nmodels": len(calls), "ncalls": len(calls)}
    for c, (mb, xs) in enumerate(calls):
        data["blob_%d" % c], data["model_%d" % c], data["x_%d" % c], data["mode_%d" % c] = mb.blob(), c, np.ascontiguousarray(xs, dtype=np.int64), 0
    src, res = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    r = subprocess.run([sys.executable, CHILD, src, res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1", **env))
    assert r.returncode == 0 and "infer edges child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert len(lines) == len(calls), r.stderr[-2000:]
    z = np.load(res)
    assert all(str(z["error_%d" % c]) == "" for c in range(len(calls)))
    return [dict(out=z["out_%d" % c], conv=int(re.search(r" conv (\d+) ", ln).group(1)), conv_i8=int(re.search(r" conv_i8 (\d+) ", ln).group(1)),
                 inputs=re.search(r"inputs as (int8|int64),", ln).group(1), line=ln) for c, ln in enumerate(lines)]


def _conv_model(shape, out_ch, kernel, asymmetric=False):
    """one conv without a Requant (the outputs are the exact sums); weights uniform over -128..127, -128 and 127 in every filter. asymmetric:
    filter 0 lives only in the last real row and column, filter 1 only in the first, the rest stay full"""
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder(shape, 124)
    mb.conv(out_ch, kernel, requant=False)
    kc, per = shape[0], shape[0] * kernel * kernel
    w = E.extreme_rows(np.random.default_rng(per + out_ch), out_ch, per).reshape(out_ch, kc, kernel, kernel)
    if asymmetric:
        last = kernel - 1
        w[0, :, :last, :last] = 0
        w[1, :, 1:, 1:] = 0
        w[0, 0, last, 0], w[0, 0, 0, last], w[1, 0, 0, last], w[1, 0, last, 0] = -128, 127, -128, 127
    mb.layers[0]["filter"][:out_ch, :kc, :kernel, :kernel] = w
    assert all(f.min() == -128 and f.max() == 127 for f in mb.layers[0]["filter"][:out_ch])
    return mb


# (input shape, out channels, kernel, batch, asymmetric): what each covers is in the docstring below
CONV_CASES = [((2, 8, 8), 3, 3, 1, False), ((2, 16, 16), 3, 3, 65, False), ((3, 16, 16), 5, 5, 3, False), ((4, 32, 32), 12, 5, 3, False), ((12, 16, 16), 33, 5, 2, False),
              ((2, 16, 16), 3, 3, 3, True)]


@pytest.mark.parametrize("shape,out_ch,kernel,batch,asymmetric", CONV_CASES)
def test_conv_i8_equals_numpy_and_the_host(tmp_path, shape, out_ch, kernel, batch, asymmetric):
    """(2,8,8) 3 k3 x1: rn = 4, nn = 64, a plane shorter than a strip, kw = 4 below the channel tile. (2,16,16) 3 k3 x65: a strip must not cross into
    the next sample. (3,16,16) 5 k5 x3: rn = 8, ra = 5 < rn, kx = 4 with a zero channel. (4,32,32) 12 k5 x3: CNN-264k's first conv, several strips per
    plane, live rows 28 of 32. (12,16,16) 33 k5 x2: its second, kw = 64, u0 = 33 inside the second channel tile, K = 640: several K slices.
    Asymmetric filters: a wrong ra or a row / column swap in the fragments cannot pass. Inputs uniform over the whole padded tensor, -128 and 127 in
    every sample."""
    import deep_prove_amd as dpa
    mb = _conv_model(shape, out_ch, kernel, asymmetric)
    xs = E.gemm_inputs(mb, batch)
    assert all(x.min() == -128 and x.max() == 127 for x in xs)
    g = _child(tmp_path, [(mb, xs)])[0]
    assert g["conv_i8"] == 1 and g["conv"] == 1 and g["inputs"] == "int8", g["line"]
    want = _numpy(mb, xs)
    assert g["out"].shape == want.shape and (g["out"] == want).all(), np.argwhere(g["out"] != want)[:5]
    picks = sorted({0, batch // 2, batch - 1})
    assert (g["out"][picks] == np.stack([dpa.infer_host(mb.blob(), xs[i]) for i in picks])).all()


def test_cnn_models_with_and_without_the_mfma(tmp_path):
    """cnn_tiny and cnn_264k at batch 65 in two children: conv_i8 is 1 / 2 of conv 1 / 2, 0 under DP_INFER_NO_MFMA=1, and both equal numpy"""
    import deep_prove_amd as dpa
    models = [dpa.models.cnn_tiny(), dpa.models.cnn_264k()]
    calls = [(mb, np.stack([mb.input(1000 + i) for i in range(65)])) for mb in models]
    want = [_numpy(mb, xs) for mb, xs in calls]
    for sub, env in (("mfma", {}), ("valu", {"DP_INFER_NO_MFMA": "1"})):
        (tmp_path / sub).mkdir()
        for g, w, nconv in zip(_child(tmp_path / sub, calls, **env), want, (1, 2)):
            assert g["conv_i8"] == (0 if env else nconv) and g["conv"] == nconv, g["line"]
            assert (g["out"] == w).all(), (sub, np.argwhere(g["out"] != w)[:5])


def test_conv_on_inputs_beyond_int8_stays_on_the_64_bit_kernel(tmp_path):
    """inputs x 3 000 have no int8 copy: k_infer_conv serves the conv"""
    mb = _conv_model((2, 16, 16), 3, 3)
    xs = E.gemm_inputs(mb, 3) * 3000
    g = _child(tmp_path, [(mb, xs)])[0]
    assert g["conv_i8"] == 0 and g["conv"] == 1 and g["inputs"] == "int64", g["line"]
    assert (g["out"] == _numpy(mb, xs)).all()
