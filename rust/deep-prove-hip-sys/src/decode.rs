//! Raw FFI to `include/deep_prove_hip_decode.h`: greedy decoding of a batch of prompts on the model's GPU (`dp_model_decode`), its host
//! yardstick (`dp_model_decode_host`) and the verifier that accepts a proof as a completion of its prompt (`dp_verify_decode`).
//! A model is decodable when node 0 is an Embeddings layer on its single input of `seq` tokens, its only output is a Logits node with
//! `seq` rows, and it holds no Softmax; the header states the step and the stop reasons.
use crate::dp_model;

/// why a prompt stopped
pub const DP_DECODE_STOP_EOS: u32 = 1;
pub const DP_DECODE_STOP_WINDOW: u32 = 2;
pub const DP_DECODE_STOP_MAX_NEW: u32 = 3;
pub const DP_DECODE_STOP_REFUSED: u32 = 4;

extern "C" {
    /// `prompts`: `nprompts * seq` words, row `i` read up to `prompt_len[i]`; `tokens`, `outputs` (may be null): `nprompts * seq` words;
    /// `length`, `stop`, `reasons`: `nprompts` words. `eos < 0`: no end-of-sequence token. `flags`: `DP_INFER_ALL_KINDS` as in `dp_model_infer_ex`.
    /// Refused data never fails the call (`stop[i] = DP_DECODE_STOP_REFUSED`, `reasons[i] = DP_INFER_BAD_*`); `wall_ms` may be null.
    pub fn dp_model_decode(m: *mut dp_model, prompts: *const i64, prompt_len: *const u32, nprompts: usize, max_new: u32, eos: i64, pad: i64, flags: u32, tokens: *mut i64, length: *mut u32, stop: *mut u32, reasons: *mut u32, outputs: *mut i64, wall_ms: *mut f64) -> i32;
    /// The same loop on the host for one prompt of a model blob: `prompt` holds `prompt_len` words, `tokens` and `output` (may be null) `seq` words.
    pub fn dp_model_decode_host(model_blob: *const i64, nwords: usize, prompt: *const i64, prompt_len: u32, max_new: u32, eos: i64, pad: i64, tokens: *mut i64, length: *mut u32, stop: *mut u32, reason: *mut u32, output: *mut i64) -> i32;
    /// `dp_verify` that also checks that `tokens` is the completion of its first `prompt_len` tokens under (`eos`, `pad`, `max_new`) and that it
    /// stopped for the reason `stop`; host only, every failure is `DP_ERR_VERIFY`.
    pub fn dp_verify_decode(verifier_blob: *const u64, nwords: usize, proof: *const u64, nproof: usize, tokens: *const i64, seq: usize, output: *const i64, prompt_len: u32, length: u32, stop: u32, eos: i64, pad: i64, max_new: u32) -> i32;
}
