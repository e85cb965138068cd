"""infer_conv_pack (csrc/infer.h) on many-channel layers that get their int8 image through the slice rule (infer_conv_slice), without a GPU, under AddressSanitizer and UBSan:
tests/support/infer_conv_pack_host.cpp, the stand-alone program of tests/test_infer_conv_pack_host.py, on 3 x 3 over 512 channels, 5 x 5 over 256, 16 x 16 over 64 and 2 x 2 over 512."""
import subprocess

import numpy as np
from test_infer_conv_pack_host import SRC


def test_filter_images_of_wide_layers(tmp_path):
    import deep_prove_amd as dpa
    args = []
    for name, shape, kernel in (("a", (512, 8, 8), 3), ("c", (256, 16, 16), 5), ("d16", (64, 32, 32), 16), ("e", (512, 8, 8), 2)):
        mb = dpa.models.ModelBuilder(shape, 124).conv(3, kernel, requant=False)
        mb.layers[0]["filter"][:3, :shape[0], :kernel, :kernel] = np.random.default_rng(kernel).integers(-128, 128, size=(3, shape[0], kernel, kernel))
        mb.layers[0]["filter"][2, 2, kernel - 1, kernel - 1] = -128  # (a non-zero weight in the last real row, whatever the generator drew)
        np.ascontiguousarray(mb.blob(), dtype=np.int64).tofile(str(tmp_path / name))
        args += [str(tmp_path / name), str(kernel)]
    exe = tmp_path / "infer_conv_pack_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "infer_conv_pack_host ok: 4 models" in r.stdout, r.stdout[-500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
