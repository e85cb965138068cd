"""The packed int8 filter of a convolution (csrc/infer.h infer_conv_pack, through infer_plan) without a GPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/support/infer_conv_pack_host.cpp, a stand-alone program, compares the image with a plain loop over the
padded filter. Three single-conv models: a 5 x 5 filter in 8 x 8 (ra = 5); one whose last padded row holds one non-zero weight (ra = rn = 8);
one with a weight of 128 (no image: the op stays on the 64-bit kernel)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "infer_conv_pack_host.cpp")


def test_conv_filter_image_equals_a_plain_loop(tmp_path):
    import deep_prove_amd as dpa
    args = []
    for name, ra in (("plain", 5), ("last_row", 8), ("too_wide", 0)):
        mb = dpa.models.ModelBuilder((3, 16, 16), 124)
        mb.conv(5, 5, requant=False)
        f = mb.layers[0]["filter"]
        f[:5, :3, :5, :5] = np.random.default_rng(5).integers(-128, 128, size=(5, 3, 5, 5))
        f[4, 2, 4, 4] = -128  # (a non-zero weight in the last real row, whatever the generator drew)
        if name == "last_row":
            f[2, 1, 7, 2] = 1
        if name == "too_wide":
            f[1, 0, 2, 3] = 128
        np.ascontiguousarray(mb.blob(), dtype=np.int64).tofile(str(tmp_path / name))
        args += [str(tmp_path / name), str(ra)]
    exe = tmp_path / "infer_conv_pack_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "infer_conv_pack_host ok: 3 models" in r.stdout, r.stdout[-500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
