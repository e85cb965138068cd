/* deep_prove_hip_decode.h — greedy decoding on the device, and proofs that are completions of their prompts. Types, status codes and conventions
 * are those of deep_prove_hip.h; the inference it drives is that of deep_prove_hip_infer.h (included below). No status code is added here.
 *
 * A model is DECODABLE when it has exactly one input tensor of `seq` words, read by an Embeddings node that is node 0; its only output is a
 * Logits node with rows == seq that chooses among K <= vocabulary tokens; and it holds no Softmax (Softmax or Mha node: the row shifts would need
 * a host step in every decode step). Anything else is refused with DP_ERR_ARG and a message that names the condition.
 *
 * The state of one prompt is (tokens[seq], length, stop). Start: tokens = the prompt followed by `pad`, length = prompt_len, with
 * 1 <= prompt_len <= seq and 0 <= pad < vocabulary. eos < 0: there is no end-of-sequence token. One step:
 *   1. length == seq                     -> stop = DP_DECODE_STOP_WINDOW
 *   2. length == prompt_len + max_new    -> stop = DP_DECODE_STOP_MAX_NEW
 *   3. otherwise infer the whole window `tokens` (nothing is cached) and take t = output[length - 1]
 *   4. t == eos                          -> stop = DP_DECODE_STOP_EOS; the end-of-sequence token is NOT appended
 *   5. otherwise tokens[length] = t, length += 1.
 * Only generated tokens are compared with eos: a prompt token equal to eos stops nothing. A prompt whose inference is refused (the data classes of
 * dp_model_infer_checked) gets stop = DP_DECODE_STOP_REFUSED, the class in `reasons`, and the tokens and the length it had reached.
 * outputs[i] is the model's output on the FINAL tokens[i], from a pass of its own after the last step: it is what a proof of the input tokens[i]
 * carries. A prompt refused in that pass is REFUSED as well; the output row of a refused prompt is zeros.
 */
#ifndef DEEP_PROVE_HIP_DECODE_H
#define DEEP_PROVE_HIP_DECODE_H
#include "deep_prove_hip_infer.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DP_DECODE_STOP_EOS     1u   /* the model chose the end-of-sequence token (not appended) */
#define DP_DECODE_STOP_WINDOW  2u   /* length == seq */
#define DP_DECODE_STOP_MAX_NEW 3u   /* length == prompt_len + max_new */
#define DP_DECODE_STOP_REFUSED 4u   /* an inference of the prompt was refused: reasons[i] = DP_INFER_BAD_* */

/* Decode `nprompts` prompts on the model's GPU. prompts: nprompts x seq words, row i read up to prompt_len[i]. flags: DP_INFER_ALL_KINDS as in
 * dp_model_infer_ex (a GELU model needs it). tokens: nprompts x seq; length, stop, reasons: nprompts words; outputs (nullable): nprompts x seq;
 * wall_ms nullable. The whole loop runs on the device: per chunk of the batch (DP_INFER_SCRATCH_MB) the prompts go up once, the steps are
 * enqueued without a host synchronisation inside a step, the stop words are polled every few steps so that a chunk ends when all its prompts
 * have stopped, and one download brings everything back. Integers are those of dp_model_decode_host, prompt by prompt.
 * Errors of the call — a model that is not decodable, pad outside the vocabulary, a prompt_len outside 1..seq, a kind that needs the flag,
 * unknown flag bits — are DP_ERR_ARG before any device work. Refused data never fails the call. Not to be called while a prove call of the same
 * model runs. DP_TIMING=1: one line `[dp decode] prompts N chunks C steps S launches L polls P final_ms X` on stderr. */
int32_t dp_model_decode(dp_model* m, const int64_t* prompts, const uint32_t* prompt_len, size_t nprompts, uint32_t max_new, int64_t eos, int64_t pad,
                        uint32_t flags, int64_t* tokens, uint32_t* length, uint32_t* stop, uint32_t* reasons, int64_t* outputs /* nullable */,
                        double* wall_ms /* nullable */);

/* The yardstick: the same loop over dp_model_infer_host's inference for ONE prompt of a model blob; host only, no device involved. prompt:
 * prompt_len words; tokens: seq words; output (nullable): seq words. The eligibility checks and messages of dp_model_decode. */
int32_t dp_model_decode_host(const int64_t* model_blob, size_t nwords, const int64_t* prompt, uint32_t prompt_len, uint32_t max_new, int64_t eos,
                             int64_t pad, int64_t* tokens, uint32_t* length, uint32_t* stop, uint32_t* reason, int64_t* output /* nullable */);

/* Accept a proof as a completion: `tokens` (seq words) is what decoding the first prompt_len of them gives under (eos, pad, max_new), it ended for
 * the reason `stop`, and the proof shows that `output` is the model's output on `tokens`. Host only. The relation is checked first, in this order,
 * then dp_verify(verifier_blob, proof, tokens, output); every failure is DP_ERR_VERIFY with a message that names the condition and the first
 * offending position:
 *   1. 1 <= prompt_len <= length <= seq
 *   2. output[t] == tokens[t + 1] for prompt_len - 1 <= t <= length - 2   (every appended token is the one the model chose)
 *   3. none of those output[t] equals eos
 *   4. tokens[t] == pad for t >= length
 *   5. the stop reason: EOS needs length < seq, length < prompt_len + max_new and output[length - 1] == eos; WINDOW needs length == seq;
 *      MAX_NEW needs length == prompt_len + max_new and length < seq; REFUSED (or any other word) is never verifiable. */
int32_t dp_verify_decode(const uint64_t* verifier_blob, size_t nwords, const uint64_t* proof, size_t nproof, const int64_t* tokens, size_t seq,
                         const int64_t* output, uint32_t prompt_len, uint32_t length, uint32_t stop, int64_t eos, int64_t pad, uint32_t max_new);

#ifdef __cplusplus
}
#endif
#endif
