/* deep_prove_hip_peer.h — the sharded sumcheck between PROCESSES, the third public header of libdeepprove_hip.so.
 *
 * Types, status codes and conventions are those of deep_prove_hip.h (included below): int32 status, nothing throws or aborts across
 * the ABI, dp_last_error() carries the message. No status code is added here.
 *
 * W ranks — one process per device on a multi-GPU host, or several contexts of one process — prove ONE sumcheck together as
 * dp_sumcheck_prove_sharded does, but the ranks' round shares travel through peer-mapped mailboxes instead of RCCL: every rank owns a
 * mailbox in device memory, exports it (hipIpcGetMemHandle), maps every peer's (hipIpcOpenMemHandle), and per round ONE kernel posts the
 * rank's shares into every peer's mailbox, polls its own until every peer's shares have arrived, adds them mod p and publishes the total
 * to the host. Messages are self-checking (a tag binds the group's exchange number to the payload), so nothing depends on the order in
 * which stores land. Once connected the ranks need no other channel: the words the prover exchanges outside the rounds travel the same way.
 *
 * Life cycle of a rank:
 *   dp_peer_create(ctx, rank, world, &p, handle)   the mailbox, and its 128-byte description
 *   ... the ranks exchange their handles by any means (files, pipes, a launcher) ...
 *   dp_peer_connect(p, handles)                    all `world` handles in rank order, this rank's own included
 *   dp_sumcheck_prove_peer(ctx, p, ...)            any number of proofs; every rank makes the same calls in the same order
 *   ... the ranks synchronise: nobody frees while a peer may still post to it ...
 *   dp_peer_free(p)
 *
 * A rank's kernel WAITS for its peers' kernels (bounded: DP_POLL_TIMEOUT_S, default 20 s; then the call fails with DP_ERR_HIP). Ranks
 * that share one device must therefore run on different hardware queues: a context opens one stream, and the library asks for 24
 * hardware queues (GPU_MAX_HW_QUEUES) when it is loaded, so up to 16 ranks on a device have a queue each.
 * After ANY error of dp_sumcheck_prove_peer the group is poisoned — its exchange counter may be out of step with the peers' — and every
 * later call on it returns DP_ERR_HIP; free it and connect a new one.
 * A rank that waits for a peer that never comes (a crashed process) fails after the timeout, it does not hang.
 */
#ifndef DEEP_PROVE_HIP_PEER_H
#define DEEP_PROVE_HIP_PEER_H
#include "deep_prove_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_peer dp_peer;
#define DP_PEER_HANDLE_BYTES 128

/* Allocates this rank's mailbox on ctx's device and writes its exportable description to `handle`.
 * world: a power of two, 1 .. 16; 0 <= rank < world. */
int32_t dp_peer_create(dp_ctx* ctx, int32_t rank, int32_t world, dp_peer** out, uint8_t handle[DP_PEER_HANDLE_BYTES]);

/* handles: world x DP_PEER_HANDLE_BYTES in rank order (this rank's own included). A handle that is not one (magic, version), that was
 * made for another world size or slot capacity, or that stands at the place of another rank: DP_ERR_ARG, before any device work. A handle
 * made by this process is used through its address; every other one is opened with hipIpcOpenMemHandle. */
int32_t dp_peer_connect(dp_peer* p, const uint8_t* handles);

/* Closes the mappings of the peers' mailboxes, then frees this rank's own. A rank must not free while a peer may still post to it:
 * the ranks synchronise before they free. */
int32_t dp_peer_free(dp_peer* p);

/* dp_sumcheck_prove_sharded with the shares exchanged through the peers' mailboxes; same arguments otherwise: `tables` are THIS rank's
 * slices (2^(num_vars - log2 world) entries each), the proof and the final evaluations are those of the whole sumcheck, identical on
 * every rank and bit-identical to dp_sumcheck_prove on the whole tables. */
int32_t dp_sumcheck_prove_peer(dp_ctx* ctx, dp_peer* peer, uint32_t num_vars, const dp_buf* const* tables, int32_t ntables,
                               const int32_t* term_degree, const int32_t* term_tables, const uint64_t* term_coeffs, int32_t nterms,
                               dp_transcript* t, uint64_t** proof_words, size_t* proof_nwords, uint64_t* finals);

#ifdef __cplusplus
}
#endif
#endif
