//! Raw FFI to the second public header, `include/deep_prove_hip_infer.h`: `Model::run` for a batch of inputs on the model's GPU.
//! The integers are those of `dp_model_infer_host`, input by input; LayerNorm / Softmax / Mha / GELU models are refused with `DP_ERR_ARG`
//! unless `dp_model_infer_ex` is given `DP_INFER_ALL_KINDS` (the Softmax row shifts are then computed on the host, one round trip per Softmax and chunk).
use crate::dp_model;

/// flag of `dp_model_infer_ex`: also LayerNorm, Softmax, Mha, GELU (kinds 14-17)
pub const DP_INFER_ALL_KINDS: u32 = 1;
/// status of one input of `dp_model_infer_checked`: inferred, or the class of the first node at which the host refuses it
pub const DP_INFER_OK: u32 = 0;
pub const DP_INFER_BAD_REQUANT: u32 = 1;
pub const DP_INFER_BAD_TOKEN: u32 = 2;
pub const DP_INFER_BAD_GELU: u32 = 3;
pub const DP_INFER_BAD_LAYERNORM: u32 = 4;
pub const DP_INFER_BAD_SOFTMAX: u32 = 5;
/// roles of the two inner tensors of an Mha node in a trace row (the roles 0, 1, 2 are a node's output slots)
pub const DP_TRACE_ROLE_MHA_IN: u64 = 16;
pub const DP_TRACE_ROLE_MHA_OUT: u64 = 17;
/// flag of `dp_model_prove_batch_ex`: infer on the device, with taps, instead of on the host
pub const DP_PROVE_DEVICE_INFER: u32 = 1;

extern "C" {
    /// `outputs`: `ninputs * noutput_cap` words; `*noutput` = words per output; `wall_ms` may be null.
    pub fn dp_model_infer(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64) -> i32;
    /// `dp_model_infer` with a flag word (0: exactly `dp_model_infer`); unknown bits: `DP_ERR_ARG`.
    pub fn dp_model_infer_ex(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, flags: u32, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64) -> i32;
    /// `dp_model_infer_ex` with a status per input: `reasons` holds `ninputs` words (`DP_INFER_OK` or `DP_INFER_BAD_*`; the rows of refused inputs
    /// are zeros), `nrefused` and `wall_ms` may be null. Bad data never fails the call; errors of the model or the call do, as in `dp_model_infer_ex`.
    pub fn dp_model_infer_checked(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, flags: u32, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, reasons: *mut u32, nrefused: *mut usize, wall_ms: *mut f64) -> i32;
    /// The layout of a trace row of a model blob (host only): four words per entry — node, role, offset, len — in node order; `entries` may be
    /// null with `cap_entries` 0 to count. `*nentries` and `*row_words` are always set.
    pub fn dp_model_trace_layout(model_blob: *const i64, nwords: usize, entries: *mut u64, cap_entries: usize, nentries: *mut usize, row_words: *mut usize) -> i32;
    /// `dp_model_infer_host` that returns the whole trace row (host only). In: `*row_words` = capacity of `row`; out: the words of a row.
    pub fn dp_model_infer_host_trace(model_blob: *const i64, nwords: usize, input: *const i64, ninput: usize, row: *mut i64, row_words: *mut usize) -> i32;
    /// `dp_model_infer_ex` (`reasons` null) or `dp_model_infer_checked` that also returns the trace row of every input: `rows` holds
    /// `ninputs * row_cap` words, `*row_words` = words per row; the row of an input refused in checked mode is zeros.
    pub fn dp_model_infer_trace(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, flags: u32, rows: *mut i64, row_cap: usize, row_words: *mut usize, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, reasons: *mut u32, wall_ms: *mut f64) -> i32;
    /// `dp_model_prove_batch` with a flag word (0 and `reasons` null: exactly that call). `DP_PROVE_DEVICE_INFER`: the inputs are inferred on the
    /// device, with taps, segment by segment (`DP_PROVE_TRACE_MB`); with `reasons` (`nproofs` words) a refused input gets its class, a null proof
    /// and a zero output row instead of failing the batch. `wall_ms`, `infer_ms` may be null.
    pub fn dp_model_prove_batch_ex(m: *mut dp_model, inputs: *const i64, nproofs: usize, ninput: usize, concurrency: i32, flags: u32, reasons: *mut u32, proof_words: *mut *mut u64, proof_nwords: *mut usize, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64, infer_ms: *mut f64) -> i32;
}
