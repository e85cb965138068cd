"""Convolutions of padded kernel side 1 (pointwise: infer_conv_tile<1>, both operands in K slices), 2 and 16 (infer_conv_frag<2>, <16>) on k_infer_conv_i8 / k_infer_conv_i8_rq
(csrc/infer_kernels.inc). Every comparison is exact equality with `mb.run(x)` (numpy int64), dp_model_infer_host is the second witness; the launch counts are read from the
`[dp infer]` line of a child process."""
import math

import numpy as np
import pytest
from test_gpu_zzzzzzzzzzzzzz_infer_conv_i8 import _conv_model
from test_gpu_zzzzzzzzzzzzzzzzzz_infer_conv_rq import CHAINS, E, _child, _exact, _upto

pytestmark = pytest.mark.gpu

# name: (input shape, out channels, kernel, batch). P*: pointwise. P1: kx = 4 padded to K = 32, a plane shorter than a strip, kw below the channel tile. P2: kx = 256, two K slices, u0 = 33 inside
# the second channel tile. P3: a strip must not cross a sample. P4: behind conv(4, 3) + Requant: 14 live rows and columns of 16, clear_garbage on a pointwise layer (two convs). P5: nw = 64, one
# pooled row per strip (kx = 1: a filter is ONE weight, the filters alternate between -128 and 127). S1: side 2, the smallest plane. S2: side 2, asymmetric filters (a row / column swap cannot
# pass). S3: 9 x 9 in 16 x 16, ra = 9 < rn. S4: 16 x 16, ra = rn
CASES = {"P1": ((3, 8, 8), 5, 1, 1), "P2": ((130, 8, 8), 33, 1, 2), "P3": ((2, 16, 16), 3, 1, 65), "P4": ((2, 16, 16), 5, 1, 1), "P5": ((1, 64, 64), 2, 1, 1),
         "S1": ((2, 8, 8), 3, 2, 1), "S2": ((3, 16, 16), 5, 2, 3), "S3": ((2, 32, 32), 3, 9, 2), "S4": ((1, 32, 32), 2, 16, 1)}
PLAIN = "plain"


def _model(name, chain, dense=False):
    """the conv of CASES[name] (P4: behind a 3 x 3 conv and its Requant) without a Requant (PLAIN) or with one of CHAINS behind it, as tests/test_gpu_..._infer_conv_rq._chain makes it;
    -> (model, index of the conv's layer)"""
    import deep_prove_amd as dpa
    shape, out_ch, kernel, _ = CASES[name]
    mb = dpa.models.ModelBuilder(shape, 127)
    if name == "P4":
        mb.conv(4, 3)
        mb.layers[0]["filter"][:4, :2, :3, :3] = E.extreme_rows(np.random.default_rng(3), 4, 18).reshape(4, 2, 3, 3)
    at, kc = len(mb.layers), mb.shape_og[0]
    per = kc * kernel * kernel
    mb.conv(out_ch, kernel, requant=chain != PLAIN)
    w = E.extreme_rows(np.random.default_rng(per + out_ch), out_ch, per).reshape(out_ch, kc, kernel, kernel)
    mb.layers[at]["filter"][:out_ch, :kc, :kernel, :kernel] = _conv_model(shape, out_ch, kernel, asymmetric=True).layers[0]["filter"][:out_ch, :kc, :kernel, :kernel] if name == "S2" else w
    if chain != PLAIN:
        mb.layers[at + 1] = dict(kind=dpa.models.L_REQUANT, **dpa.models.requant_from_multiplier(2.5 / math.sqrt(per) / 127.0, dpa.models.conv_output_bitsize(kc, kernel, kernel)))
        mb = mb.relu() if CHAINS[chain][0] else mb
        mb = mb.maxpool() if CHAINS[chain][1] else mb
    return (mb.flatten().dense(5, requant=False) if dense else mb), at


def _counts(name, chain, fuse=True, mfma=True):  # (conv_rq, conv, conv_i8, requant, relu, maxpool) of the `[dp infer]` line
    n, rq = 1 + (name == "P4"), (name == "P4") + (chain != PLAIN)
    return (rq * fuse * mfma, n, n * mfma, rq, int(chain != PLAIN and CHAINS[chain][0]), int(chain != PLAIN and CHAINS[chain][1]))


@pytest.mark.parametrize("name,chain", [(n, c) for n in CASES for c in (PLAIN,) + tuple(CHAINS) if n in ("P1", "S1", "S3") or c in (PLAIN, "requant_relu_maxpool")])
def test_conv_of_side_1_2_16_equals_numpy_and_the_host(tmp_path, name, chain):
    (mb, at), batch = _model(name, chain), CASES[name][3]
    xs, f = E.gemm_inputs(mb, batch), mb.layers[at]["filter"][:CASES[name][1]]
    assert all(x.min() == -128 and x.max() == 127 for x in xs) and f.min() == -128 and f.max() == 127 and (name == "P5" or all(g.min() == -128 and g.max() == 127 for g in f))
    if chain != PLAIN:
        rq = _upto(mb, xs[0], at + 2)
        assert rq.min() == -127 and rq.max() == 127 and ((rq > -127) & (rq < 127) & (rq != 0)).any()
    _exact(_child(tmp_path, [(mb, xs, 0)])[0], mb, xs, _counts(name, chain))


def test_the_int64_form_and_the_switches_on_a_pointwise_layer(tmp_path):
    """P4 with Requant + ReLU as the model's last node (the int64 form is written from the tile) and under Flatten -> Dense (only the int8 copy is read), by default, under
    DP_INFER_NO_FUSE=1 and under DP_INFER_NO_MFMA=1 (k_infer_conv): the same integers"""
    calls = [(mb, E.gemm_inputs(mb, 5), 0) for mb in (_model("P4", "requant_relu")[0], _model("P4", "requant_relu", dense=True)[0])]
    for sub, env, fuse, mfma in (("a", {}, True, True), ("b", {"DP_INFER_NO_FUSE": "1"}, False, True), ("c", {"DP_INFER_NO_MFMA": "1"}, False, False)):
        (tmp_path / sub).mkdir()
        for g, (mb, xs, _) in zip(_child(tmp_path / sub, calls, **env), calls):
            _exact(g, mb, xs, _counts("P4", "requant_relu", fuse, mfma))


def test_refusal_of_the_sample_in_the_middle_of_a_pointwise_chain(tmp_path):
    """test_refusal_of_the_sample_in_the_middle of the conv_rq tests on P3's layer: samples 0 and 2 are a quarter of the range, the Requant's intermediate_bit_size is the largest one
    sample 1's sums cross"""
    mb, _ = _model("P3", "requant_relu_maxpool")
    xs = E.gemm_inputs(mb, 3)
    xs[0], xs[2] = xs[0] // 4, xs[2] // 4
    peak = [int(np.abs(_upto(mb, x, 1)).max()) for x in xs]
    bits = mb.layers[1]["intermediate_bit_size"] = (peak[1] - 1).bit_length() - 1
    assert max(peak[0], peak[2]) <= (1 << bits) < peak[1]
    rows, reasons, msgs = E.host(mb.blob(), xs, mb.run(xs[0]).size)
    chk, plain = _child(tmp_path, [(mb, xs, E.CHECKED), (mb, xs, 0)])
    assert chk["conv_rq"] == plain["conv_rq"] == chk["conv_i8"] == 1 and list(reasons) == [0, 1, 0]
    assert list(chk["reasons"]) == [0, 1, 0] and (chk["out"] == rows).all() and not chk["out"][1].any() and (chk["out"][[0, 2]] == np.stack([mb.run(xs[0]), mb.run(xs[2])])).all()
    assert all("requant: value exceeds intermediate bit size" in e for e in (plain["error"], msgs[1])) and plain["out"].size == 0, (plain["error"], msgs[1])
