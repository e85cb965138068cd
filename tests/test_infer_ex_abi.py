"""dp_model_infer_ex (device inference with a flag word: DP_INFER_ALL_KINDS adds LayerNorm, Softmax, Mha and GELU) at the ABI level, without a
GPU: the built library exports it, a strict-C11 program links against it, the flag is defined in the infer header — and the main header does
not mention either."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_infer.h")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]


def test_library_exports_dp_model_infer_ex():
    import deep_prove_amd as dpa
    lib = ctypes.CDLL(dpa.LIB_PATH)
    assert hasattr(lib, "dp_model_infer_ex") and hasattr(lib, "dp_model_infer")


def test_c_program_links_against_it_and_sees_the_flag(tmp_path):
    import deep_prove_amd as dpa
    src, out = tmp_path / "link.c", tmp_path / "link"
    src.write_text('#include "deep_prove_hip_infer.h"\n'
                   "typedef int32_t (*infer_ex_fn)(dp_model*, const int64_t*, size_t, size_t, uint32_t, int64_t*, size_t, size_t*, double*);\n"
                   "int main(void) { infer_ex_fn f = dp_model_infer_ex; uint32_t flags = DP_INFER_ALL_KINDS; return f == 0 || flags != 1u; }\n")
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])
    assert subprocess.run([str(out)]).returncode == 0


def test_headers():
    hdr = open(HEADER).read()
    assert "#define DP_INFER_ALL_KINDS 1u" in hdr and "dp_model_infer_ex(" in hdr
    main = open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    assert "dp_model_infer_ex" not in main and "DP_INFER_ALL_KINDS" not in main


def test_python_and_rust_surface():
    import importlib
    import inspect
    import deep_prove_amd as dpa
    mod = importlib.import_module("deep_prove_amd.infer")
    assert "dp_model_infer_ex" in mod.INFER_SIGNATURES and "dp_model_infer_ex" not in dpa._lib.SIGNATURES
    assert inspect.signature(dpa.Context.infer).parameters["all_kinds"].default is False
    assert inspect.signature(dpa.infer).parameters["all_kinds"].default is False
    rs = os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src")
    lib = open(os.path.join(rs, "lib.rs")).read()
    first = lib[lib.index('extern "C" {'):]
    first = first[:first.index("\n}")]
    assert "dp_model_infer_ex(" not in first
    assert "pub fn dp_model_infer_ex(" in open(os.path.join(rs, "infer.rs")).read()
