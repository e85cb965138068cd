"""The peer exchange (include/deep_prove_hip_peer.h: dp_peer_create / dp_peer_connect / dp_peer_free / dp_sumcheck_prove_peer) at the ABI level, without a GPU:
the header is strict C11, a C program links the four symbols, the main header — pinned against the Rust extern block — does not mention them, the Python
surface exists, and bad arguments are refused with DP_ERR_ARG before any device is touched."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deep_prove_hip_peer.h")
C11 = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"]
NAMES = ["dp_peer_create", "dp_peer_connect", "dp_peer_free", "dp_sumcheck_prove_peer"]
DP_ERR_ARG = -1


def test_peer_header_is_strict_c11(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "deep_prove_hip_peer.h"\nint main(void) { uint8_t h[DP_PEER_HANDLE_BYTES]; h[0] = 0; return DP_OK + h[0]; }\n')
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_c_program_links_the_four_symbols(tmp_path):
    import deep_prove_amd as dpa
    src, out = tmp_path / "link.c", tmp_path / "link"
    src.write_text('#include "deep_prove_hip_peer.h"\n'
                   "typedef int32_t (*create_fn)(dp_ctx*, int32_t, int32_t, dp_peer**, uint8_t*);\n"
                   "typedef int32_t (*connect_fn)(dp_peer*, const uint8_t*);\n"
                   "typedef int32_t (*free_fn)(dp_peer*);\n"
                   "typedef int32_t (*prove_fn)(dp_ctx*, dp_peer*, uint32_t, const dp_buf* const*, int32_t, const int32_t*, const int32_t*, const uint64_t*, int32_t,\n"
                   "                            dp_transcript*, uint64_t**, size_t*, uint64_t*);\n"
                   "int main(void) { create_fn a = dp_peer_create; connect_fn b = dp_peer_connect; free_fn c = dp_peer_free; prove_fn d = dp_sumcheck_prove_peer;\n"
                   "  return (a == 0) + (b == 0) + (c == 0) + (d == 0); }\n")
    d = os.path.dirname(dpa.LIB_PATH)
    subprocess.check_call(C11 + ["-I", os.path.join(ROOT, "include"), "-O1", "-o", str(out), str(src), "-L", d, "-ldeepprove_hip", "-lpthread", "-Wl,-rpath," + d])


def test_library_exports_the_entry_points():
    import deep_prove_amd as dpa
    lib = C.CDLL(dpa.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_main_header_does_not_mention_dp_peer():
    assert "dp_peer" not in open(os.path.join(ROOT, "include", "deep_prove_hip.h")).read()
    hdr = open(HEADER).read()
    for n in NAMES:
        assert n + "(" in hdr
    assert "#define DP_PEER_HANDLE_BYTES 128" in hdr


def test_rust_declarations_live_outside_the_pinned_extern_block():
    rs = os.path.join(ROOT, "rust", "deep-prove-hip-sys", "src")
    lib = open(os.path.join(rs, "lib.rs")).read()
    first = lib[lib.index('extern "C" {'):]
    first = first[:first.index("\n}")]
    assert "dp_peer" not in first and "mod peer;" in lib
    peer = open(os.path.join(rs, "peer.rs")).read()
    for n in NAMES:
        assert "pub fn " + n + "(" in peer


def test_python_surface():
    import deep_prove_amd as dpa
    sh = dpa.sharded
    assert callable(sh.PeerGroup) and callable(sh.prove_sharded_peer)
    for attr in ("connect", "close"):
        assert callable(getattr(sh.PeerGroup, attr))
    assert set(sh.PEER_SIGNATURES) == set(NAMES) and not set(NAMES) & set(dpa._lib.SIGNATURES)
    assert sh.PEER_HANDLE_BYTES == 128


def _lib():
    import deep_prove_amd as dpa
    return dpa.sharded._peer_lib()


@pytest.mark.parametrize("rank,world,ctx_null,what", [(0, 2, True, "null context"), (0, 3, False, "power of two"), (0, 32, False, "power of two"), (0, 0, False, "power of two"),
                                                      (2, 2, False, "rank outside"), (4, 4, False, "rank outside"), (-1, 2, False, "rank outside")])
def test_create_refuses_bad_arguments_without_a_device(rank, world, ctx_null, what):
    """(the world and the rank are checked before the context is looked at: a word that only has to be non-null stands for it there)"""
    lib = _lib()
    out, handle = C.c_void_p(), (C.c_uint8 * 128)()
    fake = C.c_uint64(0)
    ctx = None if ctx_null else C.cast(C.pointer(fake), C.c_void_p)
    assert lib.dp_peer_create(ctx, rank, world, C.byref(out), handle) == DP_ERR_ARG
    assert what in lib.dp_last_error().decode()
    assert not out.value and bytes(handle) == bytes(128)


def test_null_pointers_are_refused_without_a_device():
    lib = _lib()
    out, handle = C.c_void_p(), (C.c_uint8 * 128)()
    assert lib.dp_peer_create(None, 0, 1, None, handle) == DP_ERR_ARG
    assert lib.dp_peer_create(None, 0, 1, C.byref(out), None) == DP_ERR_ARG
    assert lib.dp_peer_connect(None, handle) == DP_ERR_ARG and "null group / handles" in lib.dp_last_error().decode()
    fake = C.c_uint64(0)
    assert lib.dp_peer_connect(C.cast(C.pointer(fake), C.c_void_p), None) == DP_ERR_ARG  # null handles: refused before the group is looked at
    assert lib.dp_sumcheck_prove_peer(None, None, 4, None, 1, None, None, None, 1, None, None, None, None) == DP_ERR_ARG
    assert lib.dp_peer_free(None) == 0  # (as free(NULL))
