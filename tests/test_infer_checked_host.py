"""The host half of dp_model_infer_checked under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU: the per-sample Softmax shift
step (csrc/infer.h infer_softmax_shifts) in a stand-alone program, tests/support/infer_checked_host.cpp. A batch of 200 samples of a
softmax_only(2, 4) model holds samples with an element of +-(2^24 + 1) (refused here: DP_INFER_BAD_SOFTMAX, zero shifts), samples an earlier op
has refused, whose rows are INT64_MIN / INT64_MAX (never read: the reason stays, zero shifts) and good ones (the shifts of softmax_row_shift,
row by row). Nothing sanitized is loaded into Python: the program has its own main and reads the model blob from a file."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "infer_checked_host.cpp")


def test_per_sample_shift_step_under_sanitizers(tmp_path):
    import deep_prove_amd as dpa
    exe, blob = tmp_path / "infer_checked_host", tmp_path / "softmax_only.blob"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    np.ascontiguousarray(dpa.models.softmax_only(2, 4, config=35).blob(), dtype=np.int64).tofile(str(blob))
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "infer_checked_host ok: 200 samples of 8 rows x 4, 194 good, 3 out of range, 3 refused before" in r.stdout, r.stdout[-500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
