//! Raw FFI to the second public header, `include/deep_prove_hip_infer.h`: `Model::run` for a batch of inputs on the model's GPU.
//! The integers are those of `dp_model_infer_host`, input by input; LayerNorm / Softmax / Mha / GELU models are refused with `DP_ERR_ARG`.
use crate::dp_model;

extern "C" {
    /// `outputs`: `ninputs * noutput_cap` words; `*noutput` = words per output; `wall_ms` may be null.
    pub fn dp_model_infer(m: *mut dp_model, inputs: *const i64, ninputs: usize, ninput: usize, outputs: *mut i64, noutput_cap: usize, noutput: *mut usize, wall_ms: *mut f64) -> i32;
}
