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

extern "C" {
    /// `outputs`: `ninputs * noutput_cap` words; `*noutput` = words per output; `wall_ms` may be null.
    pub fn dp_model_infer(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64) -> i32;
    /// `dp_model_infer` with a flag word (0: exactly `dp_model_infer`); unknown bits: `DP_ERR_ARG`.
    pub fn dp_model_infer_ex(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, flags: u32, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64) -> i32;
    /// `dp_model_infer_ex` with a status per input: `reasons` holds `ninputs` words (`DP_INFER_OK` or `DP_INFER_BAD_*`; the rows of refused inputs
    /// are zeros), `nrefused` and `wall_ms` may be null. Bad data never fails the call; errors of the model or the call do, as in `dp_model_infer_ex`.
    pub fn dp_model_infer_checked(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, flags: u32, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, reasons: *mut u32, nrefused: *mut usize, wall_ms: *mut f64) -> i32;
}
