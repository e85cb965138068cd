//! Raw FFI to the third public header, `include/deep_prove_hip_peer.h`: one sumcheck proved by W ranks (processes, one per device, or contexts
//! of one process) whose round shares travel through peer-mapped mailboxes in device memory. Every rank creates its group, the ranks exchange
//! the 128-byte handles by any means, connect, and make the same `dp_sumcheck_prove_peer` calls; they synchronise before they free.
use crate::{dp_buf, dp_ctx, dp_transcript};

/// opaque: this rank's mailbox and the mappings of its peers'
#[repr(C)]
pub struct dp_peer { _private: [u8; 0] }
pub const DP_PEER_HANDLE_BYTES: usize = 128;

extern "C" {
    /// `world`: a power of two, 1 to 16; `handle`: `DP_PEER_HANDLE_BYTES` bytes, written.
    pub fn dp_peer_create(ctx: *mut dp_ctx, rank: i32, world: i32, out: *mut *mut dp_peer, handle: *mut u8) -> i32;
    /// `handles`: `world * DP_PEER_HANDLE_BYTES` bytes in rank order, this rank's own included.
    pub fn dp_peer_connect(p: *mut dp_peer, handles: *const u8) -> i32;
    /// Not while a peer may still post to this rank.
    pub fn dp_peer_free(p: *mut dp_peer) -> i32;
    /// `dp_sumcheck_prove_sharded` with the shares exchanged through the peers' mailboxes.
    pub fn dp_sumcheck_prove_peer(ctx: *mut dp_ctx, peer: *mut dp_peer, num_vars: u32, tables: *const *const dp_buf, ntables: i32, term_degree: *const i32, term_tables: *const i32, term_coeffs: *const u64, nterms: i32, t: *mut dp_transcript, proof_words: *mut *mut u64, proof_nwords: *mut usize, finals: *mut u64) -> i32;
}
