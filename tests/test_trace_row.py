"""The trace row (csrc/trace_row.h; dp_model_trace_layout, dp_model_infer_host_trace, dp_model_infer_trace, dp_model_prove_batch_ex of
include/deep_prove_hip_infer.h) without a GPU: the ABI, the layout and the host trace of nine model families, and the round trip run_model ->
trace_to_row -> trace_from_row in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/support/trace_row_check.cpp).
Every comparison is exact equality."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_infer.h")
SRC = os.path.join(ROOT, "tests", "support", "trace_row_check.cpp")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]
ENTRIES = {"dp_model_trace_layout": "int32_t (*)(const int64_t*, size_t, uint64_t*, size_t, size_t*, size_t*)",
           "dp_model_infer_host_trace": "int32_t (*)(const int64_t*, size_t, const int64_t*, size_t, int64_t*, size_t*)",
           "dp_model_infer_trace": "int32_t (*)(dp_model*, const int64_t*, size_t, size_t, uint32_t, int64_t*, size_t, size_t*, int64_t*, size_t, size_t*, uint32_t*, double*)",
           "dp_model_prove_batch_ex": "int32_t (*)(dp_model*, const int64_t*, size_t, size_t, int32_t, uint32_t, uint32_t*, uint64_t**, size_t*, int64_t*, size_t, size_t*, double*, double*)"}
sys.path.insert(0, os.path.join(ROOT, "tests"))
from support.trace_families import FAMILIES, IDS, build  # noqa: E402


def refused_input(family, mb):
    """an input of the family dp_model_infer_host refuses, or None"""
    import deep_prove_amd as dpa
    x = mb.input(1000)
    if family[0] == "token_mlp":
        y = x.copy()
        y[3] = 1 << 20
        return y
    scale = 1
    for _ in range(20):
        scale *= 8
        try:
            dpa.infer_host(mb.blob(), x * scale)
        except dpa.DeepProveError:
            return x * scale
    return None


def test_library_exports_the_four_entries():
    import deep_prove_amd as dpa
    lib = ctypes.CDLL(dpa.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_header_is_strict_c11_and_a_c_program_links_against_each_entry(tmp_path):
    import deep_prove_amd as dpa
    src, out = tmp_path / "link.c", tmp_path / "link"
    body = "".join(f"  {{ {sig.replace('(*)', '(*f)')} = {name}; bad |= f == 0; }}\n" for name, sig in ENTRIES.items())
    src.write_text('#include "deep_prove_hip_infer.h"\nint main(void) {\n  int bad = DP_PROVE_DEVICE_INFER != 1u || DP_TRACE_ROLE_MHA_IN != 16u || DP_TRACE_ROLE_MHA_OUT != 17u;\n' + body + "  return bad;\n}\n")
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])
    assert subprocess.run([str(out)]).returncode == 0


def test_main_header_names_none_of_them():
    main = open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    hdr = open(HEADER).read()
    for name in list(ENTRIES) + ["DP_PROVE_DEVICE_INFER", "DP_TRACE_ROLE"]:
        assert name not in main and name in hdr, name


def test_python_and_rust_surface():
    import importlib
    import deep_prove_amd as dpa
    mod = importlib.import_module("deep_prove_amd.infer")
    for name in ENTRIES:
        assert name in mod.INFER_SIGNATURES and name not in dpa._lib.SIGNATURES, name
    assert len(mod.INFER_SIGNATURES["dp_model_infer_trace"][1]) == 13 and len(mod.INFER_SIGNATURES["dp_model_prove_batch_ex"][1]) == 14
    assert callable(dpa.trace_layout) and callable(dpa.infer_host_trace) and mod.PROVE_DEVICE_INFER == 1
    sig = inspect.signature(dpa.Context.infer_trace).parameters
    assert sig["all_kinds"].default is False and sig["checked"].default is False
    assert inspect.signature(dpa.Prover.prove_batch).parameters["device_infer"].default is False
    assert inspect.signature(dpa.Prover.prove_batch_screened).parameters["device_infer"].default is False
    infer_rs = open(os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src", "infer.rs")).read()
    for name in ENTRIES:
        assert f"pub fn {name}(" in infer_rs, name
    assert "pub const DP_PROVE_DEVICE_INFER: u32 = 1;" in infer_rs


@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_layout_and_host_trace(family):
    import deep_prove_amd as dpa
    mb = build(family)
    blob = mb.blob()
    entries, row_words = dpa.trace_layout(blob)
    assert entries and row_words > 0
    end = 0
    for node, role, off, n in entries:  # contiguous, in node order, roles of a node in the order 16, 17, 0, 1, 2
        assert off == end and n > 0 and role in (0, 1, 2, 16, 17)
        end += n
    assert end == row_words
    order = {16: 0, 17: 1, 0: 2, 1: 3, 2: 4}
    keys = [(node, order[role]) for node, role, _, _ in entries]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    x = mb.input(1000)
    row = dpa.infer_host_trace(blob, x)
    assert row.dtype == np.int64 and row.shape == (row_words,)
    view = dpa.trace_view(entries, row)
    # the model's output tensors, concatenated in their order, are dp_model_infer_host's output
    graph = hasattr(mb, "nodes")
    nnodes = len(mb.nodes) if graph else len(mb.layers)
    assert {node for node, _, _, _ in entries} == set(range(nnodes))
    outs = mb.outputs if graph and mb.outputs is not None else [(nnodes - 1, 0)]
    assert (np.concatenate([view[e] for e in outs]) == dpa.infer_host(blob, x)).all()
    # an Mha node's probabilities are the Softmax of its products
    nmha = 0
    for node, role, _, _ in entries:
        if role == 17:
            l = mb.nodes[node][0]
            S, H, _ = l["shape"]
            assert l["kind"] == dpa.models.L_MHA and (dpa.models.softmax_apply(dict(l, shape=(H, S, S)), view[(node, 16)]) == view[(node, 17)]).all()
            nmha += 1
    assert nmha == (1 if family[0] == "mha_block" else 0)
    if family[0] == "qkv_two_outputs":
        assert [(0, r) in view for r in (0, 1, 2)] == [True] * 3
    # a refused input: the code and the message of dp_model_infer_host
    bad = refused_input(family, mb)
    if family[0] in ("mlp", "token_mlp", "gelu_mlp"):
        assert bad is not None
    if bad is not None:
        with pytest.raises(dpa.DeepProveError) as e0:
            dpa.infer_host(blob, bad)
        with pytest.raises(dpa.DeepProveError) as e1:
            dpa.infer_host_trace(blob, bad)
        assert e0.value.code == e1.value.code == -1 and str(e0.value) == str(e1.value)
    # a wrong input length is the host's error too
    with pytest.raises(dpa.DeepProveError) as e0:
        dpa.infer_host(blob, x[:-1])
    with pytest.raises(dpa.DeepProveError) as e1:
        dpa.infer_host_trace(blob, x[:-1])
    assert e0.value.code == e1.value.code and str(e0.value) == str(e1.value)


def test_round_trip_under_sanitizers(tmp_path):
    """run_model -> trace_to_row -> trace_from_row gives back every field of the Trace and the same witness_host, for every family"""
    exe = tmp_path / "trace_row_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe), SRC])
    args = []
    for family in FAMILIES:
        mb = build(family)
        b, x = tmp_path / (family[0] + ".blob"), tmp_path / (family[0] + ".input")
        np.ascontiguousarray(mb.blob(), dtype=np.int64).tofile(str(b))
        np.ascontiguousarray(mb.input(1000), dtype=np.int64).tofile(str(x))
        args += [str(b), str(x)]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.count("trace_row_check ok") == len(FAMILIES), r.stdout[-2000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout
    assert " 0 conv" not in [ln for ln in out.split("\n") if "cnn_tiny" in ln][0]
    assert " 0 mha" not in [ln for ln in out.split("\n") if "mha_block" in ln][0]
    assert " 0 argmax" not in [ln for ln in out.split("\n") if "lm_head" in ln][0]
