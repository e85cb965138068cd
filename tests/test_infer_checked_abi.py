"""dp_model_infer_checked (device inference with a status per input instead of DP_ERR_ARG for the whole batch) at the ABI level, without a GPU:
the built library exports it, a strict-C11 program links against it and sees the six status constants, the main header mentions none of it, and
the Python and Rust surfaces declare it where the infer header's symbols live."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_infer.h")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]
CONSTANTS = [("DP_INFER_OK", 0), ("DP_INFER_BAD_REQUANT", 1), ("DP_INFER_BAD_TOKEN", 2), ("DP_INFER_BAD_GELU", 3), ("DP_INFER_BAD_LAYERNORM", 4), ("DP_INFER_BAD_SOFTMAX", 5)]


def test_library_exports_dp_model_infer_checked():
    import deep_prove_amd as dpa
    lib = ctypes.CDLL(dpa.LIB_PATH)
    assert hasattr(lib, "dp_model_infer_checked") and hasattr(lib, "dp_model_infer_ex") and hasattr(lib, "dp_model_infer")


def test_c_program_links_against_it_and_sees_the_constants(tmp_path):
    import deep_prove_amd as dpa
    src, out = tmp_path / "link.c", tmp_path / "link"
    src.write_text('#include "deep_prove_hip_infer.h"\n'
                   "typedef int32_t (*infer_checked_fn)(dp_model*, const int64_t*, size_t, size_t, uint32_t, int64_t*, size_t, size_t*, uint32_t*, size_t*, double*);\n"
                   "int main(void) {\n  infer_checked_fn f = dp_model_infer_checked;\n  uint32_t bad = 0;\n"
                   + "".join(f"  bad |= {name} != {value}u;\n" for name, value in CONSTANTS)
                   + "  return f == 0 || bad;\n}\n")
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])
    assert subprocess.run([str(out)]).returncode == 0


def test_headers():
    hdr = open(HEADER).read()
    assert "dp_model_infer_checked(" in hdr
    for name, value in CONSTANTS:
        assert any(ln.split()[:3] == ["#define", name, f"{value}u"] for ln in hdr.split("\n")), name
    main = open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    assert "dp_model_infer_checked" not in main and "DP_INFER_" not in main


def test_python_and_rust_surface():
    import importlib
    import inspect
    import deep_prove_amd as dpa
    mod = importlib.import_module("deep_prove_amd.infer")
    assert "dp_model_infer_checked" in mod.INFER_SIGNATURES and "dp_model_infer_checked" not in dpa._lib.SIGNATURES
    assert len(mod.INFER_SIGNATURES["dp_model_infer_checked"][1]) == 11
    assert mod.REASONS == {0: "ok", 1: "requant", 2: "token", 3: "gelu", 4: "layernorm", 5: "softmax"}
    sig = inspect.signature(mod.infer_checked).parameters
    assert sig["all_kinds"].default is False and sig["flags"].default is None
    assert inspect.signature(dpa.Context.infer_checked).parameters["all_kinds"].default is False
    assert "concurrency" in inspect.signature(dpa.Prover.prove_batch_screened).parameters
    rs = os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src")
    lib = open(os.path.join(rs, "lib.rs")).read()
    first = lib[lib.index('extern "C" {'):]
    first = first[:first.index("\n}")]
    assert "dp_model_infer_checked(" not in first
    infer_rs = open(os.path.join(rs, "infer.rs")).read()
    assert "pub fn dp_model_infer_checked(" in infer_rs
    for name, value in CONSTANTS:
        assert f"pub const {name}: u32 = {value};" in infer_rs, name
