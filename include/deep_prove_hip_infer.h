/* deep_prove_hip_infer.h — batched quantised inference on the device, the second public header of libdeepprove_hip.so.
 *
 * Types, status codes and conventions are those of deep_prove_hip.h (included below): int32 status, nothing throws or aborts across
 * the ABI, dp_last_error() carries the message. No status code is added here.
 *
 * Layer coverage: Dense, Requant, ReLU, Conv, MaxPool, Flatten, MatMul (constant matrix, bias, TransposeB), Add with a static operand,
 * Embeddings, Positional::Learned, MatMul / Add of two inputs, ConcatMatMul and QKV (layer kinds 0-13), in chain blobs and graph blobs with
 * several input and output tensors. A model that holds a LayerNorm, Softmax, Mha or GELU node (kinds 14-17) is refused with DP_ERR_ARG before
 * any device work — the message names the node and the kind: their tables are made in floating point and Softmax shifts its rows by logf,
 * which a device libm does not reproduce bit for bit. They are a follow-up; dp_model_infer_host covers them meanwhile.
 *
 * Errors in the data are the host's: a Requant input beyond 2^intermediate_bit_size or an Embeddings token outside the vocabulary makes the
 * whole call return DP_ERR_ARG (as dp_model_infer_host does for that input); the model stays usable.
 *
 * Knobs (environment): DP_INFER_SCRATCH_MB (activation scratch of one chunk of the batch, default 1024), DP_INFER_NO_MFMA=1 (64-bit
 * products everywhere), DP_INFER_LOG=1 (one `[dp infer]` line per call on stderr: launches per kernel, chunks, wall time).
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

#ifdef __cplusplus
}
#endif
#endif
