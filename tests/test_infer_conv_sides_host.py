"""The packed int8 filter of convolutions of padded kernel side 1, 2 and 16 (csrc/infer.h infer_conv_pack) without a GPU, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/support/infer_conv_pack_host.cpp, the stand-alone program of tests/test_infer_conv_pack_host.py, on four single-conv models: 1 x 1 (ra = 1, k = j), 2 x 2 (ra = 2), 9 x 9 in 16 x 16
(ra = 9) and a 1 x 1 layer of 512 input channels, whose spans would not fit the LDS: the size rule of a pointwise layer does not depend on kx."""
import subprocess

import numpy as np
from test_infer_conv_pack_host import SRC


def test_filter_images_of_side_1_2_and_16(tmp_path):
    import deep_prove_amd as dpa
    args = []
    for name, shape, kernel in (("k1", (3, 32, 32), 1), ("k2", (3, 32, 32), 2), ("k9", (3, 32, 32), 9), ("k1_wide", (260, 4, 4), 1)):
        mb = dpa.models.ModelBuilder(shape, 124)
        mb.conv(5, kernel, requant=False)
        f = mb.layers[0]["filter"]
        f[:5, :shape[0], :kernel, :kernel] = np.random.default_rng(kernel).integers(-128, 128, size=(5, shape[0], kernel, kernel))
        f[4, 2, kernel - 1, kernel - 1] = -128  # (a non-zero weight in the last real row, whatever the generator drew)
        np.ascontiguousarray(mb.blob(), dtype=np.int64).tofile(str(tmp_path / name))
        args += [str(tmp_path / name), str(kernel)]
    exe = tmp_path / "infer_conv_pack_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "infer_conv_pack_host ok: 4 models" in r.stdout, r.stdout[-500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
