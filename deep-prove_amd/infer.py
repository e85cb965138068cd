"""Batched quantised inference on the device: ctypes binding of include/deep_prove_hip_infer.h (dp_model_infer, dp_model_infer_ex, dp_model_infer_checked). The entry points have a header and a
binding table of its own: `_lib.SIGNATURES` lists exactly the symbols of include/deep_prove_hip.h."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, i64p, vp

# name -> (restype, argtypes): every symbol declared in include/deep_prove_hip_infer.h
INFER_SIGNATURES = {
    "dp_model_infer": (C.c_int32, [vp, i64p, C.c_size_t, C.c_size_t, i64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]),
    "dp_model_infer_ex": (C.c_int32, [vp, i64p, C.c_size_t, C.c_size_t, C.c_uint32, i64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]),
    "dp_model_infer_checked": (C.c_int32, [vp, i64p, C.c_size_t, C.c_size_t, C.c_uint32, i64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.POINTER(C.c_double)]),
}
ALL_KINDS = 1  # DP_INFER_ALL_KINDS
# DP_INFER_OK, DP_INFER_BAD_*: the status of one input of dp_model_infer_checked
REASONS = {0: "ok", 1: "requant", 2: "token", 3: "gelu", 4: "layernorm", 5: "softmax"}

_bound = None


def _load():
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (res, args) in INFER_SIGNATURES.items():
            if os.environ.get("DP_LIB_VARIANT") and not hasattr(lib, name):
                continue  # (a diagnostic library built from older sources, measured beside this one: it has the entry points of its day)
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return _bound


def _prepare(ctx, inputs_i64, all_kinds, flags):
    """(lib, inputs [n][ninput] contiguous int64, outputs [n][output length] to be written, flag word)"""
    lib = _load()
    x = np.ascontiguousarray(inputs_i64, dtype=np.int64)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    n, _ = x.shape  # (two dimensions)
    cap = C.c_size_t(0)
    check(lib.dp_model_output_len(ctx.h, C.byref(cap)))
    if flags is None:
        flags = ALL_KINDS if all_kinds else 0
    return lib, x, np.empty((n, cap.value), dtype=np.int64), flags


def infer(ctx, inputs_i64, all_kinds=False, flags=None):
    """Model::run for every row of inputs_i64[n, ninput] on the context's GPU; returns (outputs[n, nout], wall_ms). The integers are those of
    infer_host, row by row. Models with LayerNorm / Softmax / Mha / GELU nodes raise DeepProveError (DP_ERR_ARG) unless all_kinds is set
    (dp_model_infer_ex with DP_INFER_ALL_KINDS: the Softmax row shifts are computed on the host). flags: the raw flag word, instead of all_kinds."""
    lib, x, outs, flags = _prepare(ctx, inputs_i64, all_kinds, flags)
    no = C.c_size_t(0)
    ms = C.c_double()
    check(lib.dp_model_infer_ex(ctx.h, x.ctypes.data_as(i64p), x.shape[0], x.shape[1], flags, outs.ctypes.data_as(i64p), outs.shape[1], C.byref(no), C.byref(ms)))
    return outs[:, :no.value].copy(), ms.value


def infer_checked(ctx, inputs_i64, all_kinds=False, flags=None):
    """dp_model_infer_checked: infer() with a status per input; returns (outputs[n, nout], reasons[n] uint32, wall_ms). reasons[i] == 0: row i is
    that of infer_host. Otherwise infer_host refuses input i with DP_ERR_ARG, reasons[i] is the class of the first node that does (REASONS) and
    row i is zeros. Errors of the model or the call (a refused kind, unknown flag bits, shapes) raise DeepProveError as infer() does."""
    lib, x, outs, flags = _prepare(ctx, inputs_i64, all_kinds, flags)
    reasons = np.zeros(x.shape[0], dtype=np.uint32)
    no, nref = C.c_size_t(0), C.c_size_t(0)
    ms = C.c_double()
    check(lib.dp_model_infer_checked(ctx.h, x.ctypes.data_as(i64p), x.shape[0], x.shape[1], flags, outs.ctypes.data_as(i64p), outs.shape[1], C.byref(no),
                                     reasons.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nref), C.byref(ms)))
    assert nref.value == int(np.count_nonzero(reasons))
    return outs[:, :no.value].copy(), reasons, ms.value
