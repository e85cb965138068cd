/* deep_prove_hip_infer.h — batched quantised inference on the device, the second public header of libdeepprove_hip.so.
 *
 * Types, status codes and conventions are those of deep_prove_hip.h (included below): int32 status, nothing throws or aborts across
 * the ABI, dp_last_error() carries the message. No status code is added here.
 *
 * Layer coverage of dp_model_infer (and of dp_model_infer_ex without flags): Dense, Requant, ReLU, Conv, MaxPool, Flatten, MatMul (constant
 * matrix, bias, TransposeB), Add with a static operand, Embeddings, Positional::Learned, MatMul / Add of two inputs, ConcatMatMul and QKV
 * (layer kinds 0-13), in chain blobs and graph blobs with several input and output tensors. A model that holds a LayerNorm, Softmax, Mha or
 * GELU node (kinds 14-17) is refused with DP_ERR_ARG before any device work — the message names the node and the kind.
 *
 * dp_model_infer_ex with DP_INFER_ALL_KINDS covers every kind the prover accepts. The tables of the four kinds (GELU, inverse square root,
 * Softmax exponential) are made in f32 with the host's libm: they belong to the model, so the host builds them once with the functions the
 * prover uses and uploads them, and LayerNorm, GELU and the table part of Softmax are integer work on the device. The shift of a Softmax row
 * is minus the logarithm of a sum of exponentials in f32, which a device libm does not reproduce bit for bit: it is computed ON THE HOST, by
 * the function dp_model_infer_host calls. At every Softmax (one per Softmax or Mha node) and chunk of the batch the device hands the Softmax
 * input to the host, the host computes one shift per row on up to min(DP_HOST_THREADS, 16) threads and the device goes on: one round trip
 * each, counted in the `[dp infer]` line.
 *
 * Errors in the data are the host's: a Requant input beyond 2^intermediate_bit_size, an Embeddings token outside the vocabulary and, under
 * DP_INFER_ALL_KINDS, a GELU input beyond 2^20 or outside its table ("gelu: ..."), a LayerNorm input beyond 2^20 or a row whose variance leaves
 * the inverse-square-root table ("layernorm: ..."), a Softmax input beyond 2^24 ("softmax: ...") make the whole call return DP_ERR_ARG (as
 * dp_model_infer_host does for that input); the model stays usable. The call ends at the first chunk of the batch that holds such an input, with
 * the message the host has for it, and writes none of that chunk's rows. The device marks refused inputs one by one (below) and the host
 * reads the marks before it computes any shift, so no row that follows bad data reaches expf. Flag bits other than DP_INFER_ALL_KINDS: DP_ERR_ARG.
 *
 * dp_model_infer_checked hands the same marks to the caller and refuses such data input by input instead: the call returns DP_OK, every chunk of
 * the batch is processed, and
 * reasons[i] says whether input i was inferred (DP_INFER_OK: its row holds the integers of dp_model_infer_host) or which kind of node refused
 * it first, in node order (DP_INFER_BAD_*: dp_model_infer_host returns DP_ERR_ARG for that input with the message of that class; its row is
 * zeros). On the device every sample of a chunk has a status word that only the first refusal writes; a refused sample's values travel on
 * through the later kernels, which stay inside their tables and buffers on any data, and the host's Softmax shift step skips refused samples
 * (zero shifts: nothing of theirs reaches expf) and range-checks the others one by one. What is wrong with the model or the call — bad
 * pointers, a wrong input length, an output buffer too small, unknown flag bits, a kind refused under the flag word given — stays an error of
 * the call, with the codes and messages of dp_model_infer_ex. A batch can so be screened before it is proved (Python:
 * Prover.prove_batch_screened): dp_model_prove_batch discards every proof of a batch in which the host inference of one input throws.
 *
 * Knobs (environment): DP_INFER_SCRATCH_MB (activation scratch of one chunk of the batch, default 1024), DP_INFER_NO_MFMA=1 (64-bit
 * products everywhere), DP_INFER_LOG=1 (one `[dp infer]` line per call on stderr: launches per kernel, chunks, wall time; gelu / layernorm / softmax launches,
 * shift_trips = round trips of the Softmax shift step and shift_ms = the milliseconds spent in them; a checked call appends
 * `; checked, refused N`), DP_PROVE_TRACE_MB (host memory for the trace rows of one segment of dp_model_prove_batch_ex, default 4096).
 */
#ifndef DEEP_PROVE_HIP_INFER_H
#define DEEP_PROVE_HIP_INFER_H
#include "deep_prove_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Model::run for `ninputs` independent inputs (concatenated, `ninput` words each) on the model's GPU.
 * outputs: ninputs x noutput_cap words; *noutput = words per output; wall_ms nullable (upload to download).
 * Integers are exactly those of dp_model_infer_host, input by input. Not to be called while a prove call of the same model runs. */
int32_t dp_model_infer(dp_model* m, const int64_t* inputs, size_t ninputs, size_t ninput,
                       int64_t* outputs, size_t noutput_cap, size_t* noutput, double* wall_ms);

#define DP_INFER_ALL_KINDS 1u   /* also LayerNorm, Softmax, Mha, GELU (kinds 14-17) */
/* dp_model_infer with a flag word: 0 = exactly dp_model_infer (the same refusal included); DP_INFER_ALL_KINDS as described above. The flattened
 * model is kept per flag word. */
int32_t dp_model_infer_ex(dp_model* m, const int64_t* inputs, size_t ninputs, size_t ninput, uint32_t flags,
                          int64_t* outputs, size_t noutput_cap, size_t* noutput, double* wall_ms);

/* The status of one input of dp_model_infer_checked: inferred, or the class of the first node (in node order) at which the host refuses it. */
#define DP_INFER_OK            0u
#define DP_INFER_BAD_REQUANT   1u   /* host: "requant: ..." */
#define DP_INFER_BAD_TOKEN     2u   /* host: "embeddings: token outside the vocabulary" */
#define DP_INFER_BAD_GELU      3u   /* host: "gelu: ..." */
#define DP_INFER_BAD_LAYERNORM 4u   /* either "layernorm: ..." message */
#define DP_INFER_BAD_SOFTMAX   5u   /* host: "softmax: ..." */
/* dp_model_infer_ex (the same flags, the same flattened model and device constants) with a status per input instead of DP_ERR_ARG for the whole
 * batch. reasons: ninputs words; row i of outputs is zero-filled when reasons[i] != DP_INFER_OK; *nrefused (nullable) = the number of such rows. */
int32_t dp_model_infer_checked(dp_model* m, const int64_t* inputs, size_t ninputs, size_t ninput, uint32_t flags,
                               int64_t* outputs, size_t noutput_cap, size_t* noutput,
                               uint32_t* reasons /* ninputs */, size_t* nrefused /* nullable */, double* wall_ms /* nullable */);

/* ---- The trace row: every tensor the prover reads of one inference, as one row of int64 words.
 * A row is described by entries (node, role, offset, len), in node order. Within a node: for an Mha node role DP_TRACE_ROLE_MHA_IN (the products
 * Q K^T its Softmax reads) and then DP_TRACE_ROLE_MHA_OUT (the probabilities); then roles 0, 1, 2 for the node's output slots (QKV has three).
 * Offsets are contiguous: the first is 0, each entry starts where the one before ends, the last ends at row_words. A Flatten node's output is
 * entered like any other (a copy of its input). Not in the row: the model inputs (the caller has them) and derived data (the FFT tables of a
 * Conv node, the row maxima of a Logits node). */
#define DP_TRACE_ROLE_MHA_IN  16u
#define DP_TRACE_ROLE_MHA_OUT 17u
/* The layout of a model blob (as dp_model_infer_host takes it); host only. entries: 4 words per entry (node, role, offset, len), cap_entries =
 * the entries it has room for (entries may be NULL with cap_entries 0: the call then only counts). *nentries and *row_words are always set;
 * more entries than cap_entries: DP_ERR_ARG. */
int32_t dp_model_trace_layout(const int64_t* model_blob, size_t nwords, uint64_t* entries, size_t cap_entries, size_t* nentries, size_t* row_words);
/* dp_model_infer_host that returns the whole trace row instead of the outputs; host only, the yardstick of dp_model_infer_trace. In: *row_words =
 * the capacity of `row`; out: the words of a row. The errors and messages of dp_model_infer_host. */
int32_t dp_model_infer_host_trace(const int64_t* model_blob, size_t nwords, const int64_t* input, size_t ninput, int64_t* row, size_t* row_words);
/* dp_model_infer_ex (reasons NULL) or dp_model_infer_checked (reasons: ninputs words) that also returns the trace row of every input: rows =
 * ninputs x row_cap words, *row_words = the words of a row (row_cap too small: DP_ERR_ARG). Row i holds the integers of
 * dp_model_infer_host_trace for input i; in checked mode the row of a refused input is zeros, as its output row is. The rows are gathered on the
 * device (one launch per chunk of the batch) and come down in one copy per chunk beside the outputs; they enter the accounting of
 * DP_INFER_SCRATCH_MB, and the `[dp infer]` line gets `; taps T entries, W words, pack_launches L pack_ms X` (in front of `; checked, ...`).
 * Flag and kind rules, errors and messages: those of the two calls it extends. */
int32_t dp_model_infer_trace(dp_model* m, const int64_t* inputs, size_t ninputs, size_t ninput, uint32_t flags,
                             int64_t* rows, size_t row_cap, size_t* row_words,
                             int64_t* outputs, size_t noutput_cap, size_t* noutput,
                             uint32_t* reasons /* nullable: checked mode */, double* wall_ms /* nullable */);

/* ---- Proving from the device inference.
 * dp_model_prove_batch with a flag word. flags == 0 and reasons == NULL: exactly dp_model_prove_batch (every input is inferred on the host, by
 * the thread that proves it or a helper). DP_PROVE_DEVICE_INFER: the inputs are inferred on the model's GPU with taps and all kinds
 * (dp_model_infer_trace) before any proof of theirs starts, and the host work in front of a proof shrinks to rebuilding the trace from its row and
 * the host half of the witness generation (the Softmax shifts, the witness columns and the FFT tables of a Conv node stay host work). The proofs
 * are word for word those of dp_model_prove_batch.
 * The rows live in host memory: at most DP_PROVE_TRACE_MB (environment, default 4096) of them at a time. The batch is cut into segments of at most
 * max(concurrency, budget / bytes of a row) inputs; each segment is inferred and then proved, the proofs in flight ramp up and drain once per segment.
 * reasons (nproofs words, needs DP_PROVE_DEVICE_INFER): an input the inference refuses does not fail the batch — reasons[i] is its class
 * (DP_INFER_BAD_*), proof_words[i] is NULL with 0 words and its output row is zeros; every other input is proved. reasons == NULL: such an input
 * ends the call with DP_ERR_ARG and the host's message, and every proof of the batch is discarded, as in dp_model_prove_batch.
 * wall_ms (nullable): inference + proving; infer_ms (nullable): the device inference alone (0 without the flag). Unknown flag bits, or reasons
 * without the flag: DP_ERR_ARG. */
#define DP_PROVE_DEVICE_INFER 1u
int32_t dp_model_prove_batch_ex(dp_model* m, const int64_t* inputs, size_t nproofs, size_t ninput, int32_t concurrency, uint32_t flags,
                                uint32_t* reasons /* nullable */, uint64_t** proof_words, size_t* proof_nwords,
                                int64_t* outputs, size_t noutput_cap, size_t* noutput, double* wall_ms /* nullable */, double* infer_ms /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
