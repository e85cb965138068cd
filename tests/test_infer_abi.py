"""dp_model_infer (batched quantised inference on the device) at the ABI level, without a GPU: the built library exports it, its header
include/deep_prove_hip_infer.h is strict C11 and a C program links against the symbol, the Python surface exists — and the main header, whose
contents three other tests pin, does not mention it."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_infer.h")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]


def test_library_exports_dp_model_infer():
    import deep_prove_amd as dpa
    lib = ctypes.CDLL(dpa.LIB_PATH)
    assert hasattr(lib, "dp_model_infer")


def test_infer_header_is_strict_c11(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "deep_prove_hip_infer.h"\nint main(void) { return DP_OK; }\n')
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_c_program_links_against_the_entry_point(tmp_path):
    import deep_prove_amd as dpa
    src, out = tmp_path / "link.c", tmp_path / "link"
    src.write_text('#include "deep_prove_hip_infer.h"\n'
                   "typedef int32_t (*infer_fn)(dp_model*, const int64_t*, size_t, size_t, int64_t*, size_t, size_t*, double*);\n"
                   "int main(void) { infer_fn f = dp_model_infer; return f == 0; }\n")
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])


def test_python_surface():
    import deep_prove_amd as dpa
    assert callable(dpa.infer) and callable(dpa.Context.infer)
    import importlib
    mod = importlib.import_module("deep_prove_amd.infer")  # (the package attribute of that name is the function)
    assert "dp_model_infer" in mod.INFER_SIGNATURES and "dp_model_infer" not in dpa._lib.SIGNATURES


def test_main_header_does_not_declare_it():
    assert "dp_model_infer(" not in open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    assert "dp_model_infer(" in open(HEADER).read()


def test_rust_declaration_lives_outside_the_pinned_extern_block():
    rs = os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src")
    lib = open(os.path.join(rs, "lib.rs")).read()
    first = lib[lib.index('extern "C" {'):]
    first = first[:first.index("\n}")]
    assert "dp_model_infer(" not in first and "mod infer;" in lib
    assert "pub fn dp_model_infer(" in open(os.path.join(rs, "infer.rs")).read()
