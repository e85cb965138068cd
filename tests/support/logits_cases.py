"""The Logits::Argmax (layer kind 18) cases shared by the CPU and the GPU tests: model blob + input per case, the CPU harness
(tests/support/logits_check.cpp over the plain-loop double) and the golden digests of tests/golden/logits_models.json."""
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "logits_models.json")


def _models():
    from deep_prove_amd import models
    return models


def logits_only_input(rows, k):
    """rows that exercise the argmax rule: all equal (index 0), the maximum twice (the first wins), the maximum in the last column and — at
    K = 256 — a row holding -128 .. 127, a spread of exactly 255, the last row of the range table"""
    m = _models()
    x = (m.quantised_tensor(40, rows * 1000 + k, rows * k) // 2).reshape(rows, k)  # within -63 .. 63: any row spreads over at most 126
    if (rows, k) == (2, 2):
        x[0] = [5, 5]
        x[1] = [-3, 9]
    elif (rows, k) == (4, 8):
        x[0] = 17
        x[1] = [3, 90, -4, 90, 0, 1, 2, 89]
        x[2] = [-60, -9, 0, 4, 8, 15, 16, 23]
    elif (rows, k) == (2, 256):
        x[0] = (np.arange(256) * 77 + 31) % 256 - 128   # a permutation of -128 .. 127
        x[1, 100] = x[1, 255] = 64                       # the maximum twice, once in the last column
    return x.reshape(-1)


def cases():
    """name -> (builder, input)"""
    m = _models()
    out = {}
    for rows, k in ((2, 2), (4, 8), (2, 256)):
        out[f"logits_only_{rows}x{k}"] = (m.logits_only(rows, k, config=41), logits_only_input(rows, k))
    mb = m.lm_head(4, 8, 16, config=42)
    out["lm_head_4x8x16"] = (mb, mb.input())
    mb = m.token_lm(8, 16, 16, config=43)
    out["token_lm_8x16x16"] = (mb, mb.input())
    return out


SMALL = ("logits_only_2x2", "logits_only_4x8")             # every word of the stream is flipped
LARGE = ("logits_only_2x256", "lm_head_4x8x16", "token_lm_8x16x16")  # the Logits step + every third word of the first 8000 others


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).astype("<" + np.dtype(dtype).str[1:]).tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _build(out, extra=()):
    src = os.path.join(ROOT, "tests", "support", "logits_check.cpp")
    csrc = os.path.join(ROOT, "deep-prove_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "support", "cpu_dev.hpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = f"{out}.tmp{os.getpid()}"  # (built beside the target and renamed over it: several workers may get here together)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", *extra, "-o", tmp, src])
        os.replace(tmp, out)
    return out


def check_bin():
    """tests/support/logits_check, built the way hostlogic_check is"""
    return _build(os.path.join(ROOT, "tests", "support", "_build", "logits_check"))


def check_bin_sanitized():
    """the same program and the host code under test once more under AddressSanitizer + UBSan: a stand-alone program, no preloaded runtime"""
    return _build(os.path.join(ROOT, "tests", "support", "_build", "logits_check_asan"), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))


def write_case(tmp, name, blob, x):
    """blob and input as the raw word files logits_check reads"""
    bp, xp = os.path.join(str(tmp), name + ".blob"), os.path.join(str(tmp), name + ".in")
    np.ascontiguousarray(blob, dtype="<i8").tofile(bp)
    np.ascontiguousarray(x, dtype="<i8").tofile(xp)
    return bp, xp


def run_check(binary, *args, timeout=600):
    return subprocess.run([binary, *map(str, args)], capture_output=True, text=True, timeout=timeout)
