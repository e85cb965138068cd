"""Batched quantised inference on the device: ctypes binding of include/deep_prove_hip_infer.h (dp_model_infer, dp_model_infer_ex, dp_model_infer_checked; the trace row: dp_model_trace_layout, dp_model_infer_host_trace, dp_model_infer_trace;
dp_model_prove_batch_ex is bound here and called by api.Prover). The entry points have a header and a
binding table of its own: `_lib.SIGNATURES` lists exactly the symbols of include/deep_prove_hip.h.
Decoding (include/deep_prove_hip_decode.h: dp_model_decode, dp_model_decode_host, dp_verify_decode) is bound here too, from DECODE_SIGNATURES."""
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
    "dp_model_trace_layout": (C.c_int32, [i64p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "dp_model_infer_host_trace": (C.c_int32, [i64p, C.c_size_t, i64p, C.c_size_t, i64p, C.POINTER(C.c_size_t)]),
    "dp_model_infer_trace": (C.c_int32, [vp, i64p, C.c_size_t, C.c_size_t, C.c_uint32, i64p, C.c_size_t, C.POINTER(C.c_size_t), i64p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "dp_model_prove_batch_ex": (C.c_int32, [vp, i64p, C.c_size_t, C.c_size_t, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t),
                                            i64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}
# name -> (restype, argtypes): every symbol declared in include/deep_prove_hip_decode.h
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
DECODE_SIGNATURES = {
    "dp_model_decode": (C.c_int32, [vp, i64p, u32p, C.c_size_t, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, i64p, u32p, u32p, u32p, i64p, C.POINTER(C.c_double)]),
    "dp_model_decode_host": (C.c_int32, [i64p, C.c_size_t, i64p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, i64p, u32p, u32p, u32p, i64p]),
    "dp_verify_decode": (C.c_int32, [u64p, C.c_size_t, u64p, C.c_size_t, i64p, C.c_size_t, i64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32]),
}
ALL_KINDS = 1  # DP_INFER_ALL_KINDS
STOP_EOS, STOP_WINDOW, STOP_MAX_NEW, STOP_REFUSED = 1, 2, 3, 4  # DP_DECODE_STOP_*
STOPS = {1: "eos", 2: "window", 3: "max_new", 4: "refused"}
PROVE_DEVICE_INFER = 1  # DP_PROVE_DEVICE_INFER
ROLE_MHA_IN, ROLE_MHA_OUT = 16, 17  # DP_TRACE_ROLE_MHA_IN / _OUT: the two inner tensors of an Mha node in a trace row
# DP_INFER_OK, DP_INFER_BAD_*: the status of one input of dp_model_infer_checked
REASONS = {0: "ok", 1: "requant", 2: "token", 3: "gelu", 4: "layernorm", 5: "softmax"}

_bound = None


def _load():
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (res, args) in list(INFER_SIGNATURES.items()) + list(DECODE_SIGNATURES.items()):
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


def trace_layout(model_blob):
    """dp_model_trace_layout: (entries, row_words) of a model blob — entries = [(node, role, offset, len)] in the order of a trace row: per node
    the two inner tensors of an Mha node (roles 16, 17), then its output slots (roles 0, 1, 2). Host only."""
    lib = _load()
    b = np.ascontiguousarray(model_blob, dtype=np.int64)
    ne, rw = C.c_size_t(0), C.c_size_t(0)
    check(lib.dp_model_trace_layout(b.ctypes.data_as(i64p), b.size, None, 0, C.byref(ne), C.byref(rw)))
    ent = np.zeros((ne.value, 4), dtype=np.uint64)
    check(lib.dp_model_trace_layout(b.ctypes.data_as(i64p), b.size, ent.ctypes.data_as(C.POINTER(C.c_uint64)), ne.value, C.byref(ne), C.byref(rw)))
    return [tuple(int(v) for v in e) for e in ent], int(rw.value)


def trace_view(entries, rows):
    """{(node, role): rows[..., offset : offset + len]} — views into a trace row, or into the rows of a batch"""
    return {(node, role): rows[..., off:off + n] for node, role, off, n in entries}


def infer_host_trace(model_blob, input_i64):
    """dp_model_infer_host_trace: the trace row of one input on the host (run_model, flattened by trace_layout); the errors of infer_host"""
    lib = _load()
    b = np.ascontiguousarray(model_blob, dtype=np.int64)
    x = np.ascontiguousarray(input_i64, dtype=np.int64)
    ne, rw = C.c_size_t(0), C.c_size_t(0)
    check(lib.dp_model_trace_layout(b.ctypes.data_as(i64p), b.size, None, 0, C.byref(ne), C.byref(rw)))
    row = np.empty(max(rw.value, 1), dtype=np.int64)
    n = C.c_size_t(row.size)
    check(lib.dp_model_infer_host_trace(b.ctypes.data_as(i64p), b.size, x.ctypes.data_as(i64p), x.size, row.ctypes.data_as(i64p), C.byref(n)))
    return row[:n.value].copy()


def infer_trace(ctx, inputs_i64, all_kinds=False, checked=False, flags=None):
    """dp_model_infer_trace: infer() (or, checked, infer_checked()) that also returns the trace row of every input, gathered on the device. Returns
    (rows[n, row_words], view, outputs[n, nout], reasons[n] or None, wall_ms); view = {(node, role): rows[:, offset : offset + len]}. Row i holds
    the integers of infer_host_trace for input i; checked: zeros where reasons[i] != 0."""
    lib, x, outs, flags = _prepare(ctx, inputs_i64, all_kinds, flags)
    entries, rw = trace_layout(ctx.model_blob)
    rows = np.empty((x.shape[0], max(rw, 1)), dtype=np.int64)
    reasons = np.zeros(x.shape[0], dtype=np.uint32) if checked else None
    no, got = C.c_size_t(0), C.c_size_t(0)
    ms = C.c_double()
    check(lib.dp_model_infer_trace(ctx.h, x.ctypes.data_as(i64p), x.shape[0], x.shape[1], flags, rows.ctypes.data_as(i64p), rows.shape[1], C.byref(got),
                                   outs.ctypes.data_as(i64p), outs.shape[1], C.byref(no), reasons.ctypes.data_as(C.POINTER(C.c_uint32)) if checked else None, C.byref(ms)))
    assert got.value == rw
    rows = rows[:, :rw].copy()
    return rows, trace_view(entries, rows), outs[:, :no.value].copy(), reasons, ms.value


def _prompt_block(prompts, prompt_lens, seq=None):
    """(prompts as [n][seq] contiguous int64 — a list of token lists of different lengths is padded with zeros, which are never read —, lengths[n] uint32)"""
    if isinstance(prompts, np.ndarray) or all(len(p) == len(prompts[0]) for p in prompts):
        x = np.ascontiguousarray(prompts, dtype=np.int64)
        if x.ndim == 1:
            x = x.reshape(1, -1)
    else:
        x = np.zeros((len(prompts), max(len(p) for p in prompts)), dtype=np.int64)
        for i, p in enumerate(prompts):
            x[i, :len(p)] = p
    if seq is not None and x.shape[1] != seq:
        w = np.zeros((x.shape[0], seq), dtype=np.int64)
        w[:, :min(seq, x.shape[1])] = x[:, :seq]
        x = w
    lens = np.ascontiguousarray(np.broadcast_to(np.asarray(prompt_lens, dtype=np.uint32), (x.shape[0],)))
    return x, lens


def decode(ctx, prompts, prompt_lens, max_new, eos=None, pad=0, all_kinds=False):
    """dp_model_decode: greedy decoding of every prompt on the context's GPU, the whole loop on the device. prompts[n, <= seq] (row i read up to
    prompt_lens[i]); eos None: no end-of-sequence token. Returns (tokens[n, seq], lengths[n], stops[n], reasons[n], outputs[n, seq], wall_ms):
    tokens[i] = the prompt, what was generated (the end-of-sequence token is not appended) and `pad` behind it; stops[i] in STOPS; outputs[i] =
    the model's output on tokens[i]. A prompt the inference refuses has stops[i] == STOP_REFUSED, its class in reasons[i] (REASONS) and zeros
    for its outputs. The integers are those of decode_host, prompt by prompt."""
    lib = _load()
    seq = C.c_size_t(0)
    check(lib.dp_model_output_len(ctx.h, C.byref(seq)))
    x, lens = _prompt_block(prompts, prompt_lens, seq.value)
    n = x.shape[0]
    tokens, outs = np.zeros((n, seq.value), dtype=np.int64), np.zeros((n, seq.value), dtype=np.int64)
    length, stop, reasons = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    ms = C.c_double()
    check(lib.dp_model_decode(ctx.h, x.ctypes.data_as(i64p), lens.ctypes.data_as(u32p), n, max_new, -1 if eos is None else eos, pad, ALL_KINDS if all_kinds else 0,
                              tokens.ctypes.data_as(i64p), length.ctypes.data_as(u32p), stop.ctypes.data_as(u32p), reasons.ctypes.data_as(u32p), outs.ctypes.data_as(i64p), C.byref(ms)))
    return tokens, length, stop, reasons, outs, ms.value


def decode_host(model_blob, prompt, prompt_len=None, max_new=0, eos=None, pad=0):
    """dp_model_decode_host: the decode loop for ONE prompt on the host (the yardstick of decode; no device involved). prompt_len None: the
    whole of `prompt`. Returns (tokens[seq], length, stop, reason, output[seq])."""
    lib = _load()
    b = np.ascontiguousarray(model_blob, dtype=np.int64)
    x = np.ascontiguousarray(prompt, dtype=np.int64).reshape(-1)
    plen = x.size if prompt_len is None else int(prompt_len)
    if plen > x.size:  # (the library refuses a prompt_len beyond the window; it must not read past the prompt before it does)
        x = np.concatenate([x, np.zeros(plen - x.size, dtype=np.int64)])
    seq = int(b[0]) if b.size and 0 < int(b[0]) < (1 << 32) else 1  # (word 0 of a blob: the input length, which is the window of a decodable model — the library writes that many words, after it has accepted the blob)
    tokens, out = np.zeros(seq, dtype=np.int64), np.zeros(seq, dtype=np.int64)
    length, stop, reason = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(lib.dp_model_decode_host(b.ctypes.data_as(i64p), b.size, x.ctypes.data_as(i64p), plen, max_new, -1 if eos is None else eos, pad,
                                   tokens.ctypes.data_as(i64p), C.byref(length), C.byref(stop), C.byref(reason), out.ctypes.data_as(i64p)))
    return tokens, int(length.value), int(stop.value), int(reason.value), out


def verify_decode(verifier_blob, proof_words, tokens, output, prompt_len, length, stop, eos=None, pad=0, max_new=0):
    """dp_verify_decode: accept `proof_words` as a completion — tokens[:length] is what decoding tokens[:prompt_len] gives under (eos, pad,
    max_new), it stopped for the reason `stop`, and the proof shows that `output` is the model's output on `tokens`. Host only. Raises
    DeepProveError(DP_ERR_VERIFY) with the condition that fails; the relation is checked before the proof is read."""
    lib = _load()
    vb = np.ascontiguousarray(verifier_blob, dtype=np.uint64)
    pw = np.ascontiguousarray(proof_words, dtype=np.uint64)
    t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
    y = np.ascontiguousarray(output, dtype=np.int64).reshape(-1)
    if y.size != t.size:
        raise ValueError("verify_decode: tokens and output must both hold seq words")
    check(lib.dp_verify_decode(vb.ctypes.data_as(u64p), vb.size, pw.ctypes.data_as(u64p), pw.size, t.ctypes.data_as(i64p), t.size, y.ctypes.data_as(i64p),
                               int(prompt_len), int(length), int(stop), -1 if eos is None else eos, pad, max_new))
