"""Many-channel convolutions on the channel-sliced k_infer_conv_i8 / k_infer_conv_i8_rq (infer_conv_tile_sl in csrc/infer_kernels.inc, infer_conv_slice in csrc/infer.h): layers whose kx spans pass
the 48 KB of LDS. Exact equality with `mb.run(x)` (numpy int64), dp_model_infer_host the second witness, the launch counts from the `[dp infer]` line of a child process."""
import numpy as np
import pytest
from test_gpu_zzzzzzzzzzzzzz_infer_conv_i8 import _conv_model
from test_gpu_zzzzzzzzzzzzzzzzzz_infer_conv_rq import CHAINS, E, _chain, _child, _exact, _upto

pytestmark = pytest.mark.gpu
# name: (input shape, out channels, kernel, batch). A: jc = 64, 8 slices, a plane shorter than a strip, a strip must not cross a sample, kw below the channel tile. B: 4 slices, u0 = 33 inside the
# second channel tile, two strips. C: side 8, ra = 5, a slice is 20 filter K slices. D9: side 16, ra = 9 < rn, jc = 32. D16: side 16, ra = rn, jc = 16 (512 bytes past the whole-span bound).
# E2: side 2, jc = 64. F: nw = 64, one pooled row per strip, 32 strips, jc = 32
CASES = {"A": ((512, 8, 8), 5, 3, 3), "B": ((256, 16, 16), 33, 3, 2), "C": ((256, 16, 16), 3, 5, 1), "D9": ((128, 32, 32), 3, 9, 1), "D16": ((64, 32, 32), 2, 16, 1),
         "E2": ((512, 8, 8), 3, 2, 1), "F": ((128, 64, 64), 2, 5, 1)}
PLAIN = "plain"


def _model(name, chain, dense=False):  # the conv of CASES[name], bare (PLAIN) or with one of CHAINS behind it; every filter holds -128 and 127
    return _conv_model(*CASES[name][:3]) if chain == PLAIN else _chain(*CASES[name][:3], *CHAINS[chain], dense=dense)


def _counts(chain, fuse=True, mfma=True):  # (conv_rq, conv, conv_i8, requant, relu, maxpool) of the `[dp infer]` line
    rq = int(chain != PLAIN)
    return (rq * fuse * mfma, 1, int(mfma), rq, int(rq and CHAINS[chain][0]), int(rq and CHAINS[chain][1]))


@pytest.mark.parametrize("name,chain", [(n, c) for n in CASES for c in (PLAIN,) + tuple(CHAINS) if n in ("A", "D16", "F") or c in (PLAIN, "requant_relu_maxpool")])
def test_wide_conv_equals_numpy_and_the_host(tmp_path, name, chain):
    mb = _model(name, chain)
    xs = E.gemm_inputs(mb, CASES[name][3])
    assert all(x.min() == -128 and x.max() == 127 for x in xs) and all(f.min() == -128 and f.max() == 127 for f in mb.layers[0]["filter"][:CASES[name][1]])
    if chain != PLAIN:
        rq = _upto(mb, xs[0], 2)
        assert rq.min() == -127 and rq.max() == 127 and ((rq > -127) & (rq < 127) & (rq != 0)).any()
    _exact(_child(tmp_path, [(mb, xs, 0)])[0], mb, xs, _counts(chain))


def test_the_int64_form_and_the_switches_on_a_sliced_conv(tmp_path):
    """B with Requant + ReLU as the model's last node (the int64 form is written from the tile) and under Flatten -> Dense (only the int8 copy is read), by default, under
    DP_INFER_NO_FUSE=1 (the sliced k_infer_conv_i8 and the separate launches) and under DP_INFER_NO_MFMA=1 (k_infer_conv): the same integers"""
    calls = [(mb, E.gemm_inputs(mb, 2), 0) for mb in (_model("B", "requant_relu"), _model("B", "requant_relu", dense=True))]
    for sub, env, fuse, mfma in (("a", {}, True, True), ("b", {"DP_INFER_NO_FUSE": "1"}, False, True), ("c", {"DP_INFER_NO_MFMA": "1"}, False, False)):
        (tmp_path / sub).mkdir()
        for g, (mb, xs, _) in zip(_child(tmp_path / sub, calls, **env), calls):
            _exact(g, mb, xs, _counts("requant_relu", fuse, mfma))


def test_refusal_of_the_sample_in_the_middle_of_a_sliced_chain(tmp_path):
    """test_refusal_of_the_sample_in_the_middle of the conv_rq tests on A's layer: samples 0 and 2 are a quarter of the range, the Requant's bit size is the largest one sample 1's sums cross"""
    mb = _model("A", "requant_relu_maxpool")
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
