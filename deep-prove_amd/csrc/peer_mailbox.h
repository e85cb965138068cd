// The mailbox protocol of the peer exchange (sharded sumcheck, csrc/sharded.h): W ranks — processes, one per device, or contexts of one
// process — all-gather a short message by WRITING it into every peer's mailbox and POLLING their own. No collective library, no host
// hop: a rank's mailbox is device memory that every peer has mapped (hipIpcOpenMemHandle), the post is a burst of relaxed system-scope
// stores, the gather a poll with relaxed system-scope loads (k_peer_exchange_publish, kernels.inc). This header is the protocol alone —
// layout, tag, post, read — as plain inline functions over a word type W and two accessors, so that the kernel (W = u64, hip atomics)
// and the host-side protocol check (W = std::atomic<uint64_t>, tests/support/peer_mailbox_check.cpp) run the same code.
//
// Layout. A rank's mailbox is 2 parities x world slots x (PEER_SLOT_WORDS payload words + 1 tag word). Slot (parity, sender) is written
// by `sender` only, parity = exchange number & 1.
//
// Tag. tag = mix(exchange number) + sum_i (i + 1) * word_i + nwords: the position-weighted checksum of the publish kernels (sc_publish)
// under a mixing function of the pub_mix family. A reader accepts a payload only if the tag it reads equals the tag it recomputes from
// the words it read; otherwise it polls again. Nothing relies on the order in which the stores land or on an acquire: a torn read (tag of
// one exchange, words of another) or a stale one (the slot's previous contents) fails the comparison and is simply re-read — the
// protocol of wait_flag / chal_poll.
//
// The exchange number is the GROUP's counter, identical on every rank: 1 at connect, + 1 per exchange (it is not a context's publish
// sequence number, which differs between ranks).
//
// Why two parities suffice. Rank A posts exchange e + 1 only after its kernel of exchange e has ended, i.e. after A has seen every
// peer's post of e. A peer B posts e only after ITS kernel of e - 1 has ended, i.e. after B has read every slot of parity (e - 1) & 1
// of its mailbox. The slot A's post of e + 1 overwrites in B's mailbox — parity (e + 1) & 1 = (e - 1) & 1 — has therefore been fully
// consumed. And what B may still find in a slot it polls for e is A's post of e - 2 (or zeros): its tag carries mix(e - 2) and fails.
// A rank can thus run at most one exchange ahead of a peer, which is what two parities hold.
#pragma once
#include "gl64.h"

namespace dp {

constexpr int PEER_SLOT_WORDS = 2048;                    // payload capacity of a slot: the sharded round message (nwords / 2 <= 1024 extension values)
constexpr int PEER_SLOT_STRIDE = PEER_SLOT_WORDS + 1;    // + the tag word
constexpr int PEER_MAX_WORLD = 16;
enum { PEER_MODE_SUM = 0, PEER_MODE_GATHER = 1 };        // what k_peer_exchange_publish hands the host: the mod-p sum of the shares / the shares in rank order

DP_HD size_t peer_mailbox_words(int world) { return (size_t)2 * (size_t)world * PEER_SLOT_STRIDE; }
// word offset of slot (exchange & 1, sender) in a mailbox of `world` ranks
DP_HD size_t peer_slot(unsigned long long exchange, int sender, int world) { return ((size_t)(exchange & 1) * (size_t)world + (size_t)sender) * PEER_SLOT_STRIDE; }
DP_HD u64 peer_mix(unsigned long long exchange) { return exchange * 0x9E3779B97F4A7C15ull + 0x7F4A7C159E3779B9ull; }
DP_HD u64 peer_tag(unsigned long long exchange, u64 checksum, size_t nwords) { return peer_mix(exchange) + checksum + (u64)nwords; }

// Lane `lane` of `nlanes` stores its share (words lane, lane + nlanes, ...) of a payload into a slot; returns its share of the checksum.
// St: void(W*, u64), a relaxed store.
template <class W, class St>
DP_HD u64 peer_post_words(St st, W* slot, const u64* words, size_t nwords, size_t lane, size_t nlanes) {
  u64 cs = 0;
  for (size_t i = lane; i < nwords; i += nlanes) { const u64 v = words[i]; st(slot + i, v); cs += (u64)(i + 1) * v; }
  return cs;
}
// ... and reads it: the words go to `out`, the return value is the lane's share of the checksum of WHAT WAS READ. Ld: u64(const W*), a relaxed load.
template <class W, class Ld>
DP_HD u64 peer_read_words(Ld ld, const W* slot, u64* out, size_t nwords, size_t lane, size_t nlanes) {
  u64 cs = 0;
  for (size_t i = lane; i < nwords; i += nlanes) { const u64 v = ld(slot + i); out[i] = v; cs += (u64)(i + 1) * v; }
  return cs;
}
// mode SUM: acc += words, word by word mod p (an extension value is two words, added componentwise)
DP_HD void peer_sum_into(u64* acc, const u64* words, size_t nwords, size_t lane, size_t nlanes) {
  for (size_t i = lane; i < nwords; i += nlanes) acc[i] = gl_add(acc[i], words[i]);
}

// The whole post of one rank, by one thread: payload, then tag, into slot (exchange & 1, rank) of `box`.
template <class W, class St>
DP_HD void peer_post(St st, W* box, unsigned long long exchange, int rank, int world, const u64* words, size_t nwords) {
  W* slot = box + peer_slot(exchange, rank, world);
  const u64 cs = peer_post_words(st, slot, words, nwords, 0, 1);
  st(slot + PEER_SLOT_WORDS, peer_tag(exchange, cs, nwords));
}
// One poll of slot (exchange & 1, sender) of `box`, by one thread: true — `out` holds sender's payload of `exchange`; false — not there (yet), poll again.
template <class W, class Ld>
DP_HD bool peer_try_read(Ld ld, const W* box, unsigned long long exchange, int sender, int world, u64* out, size_t nwords) {
  const W* slot = box + peer_slot(exchange, sender, world);
  const u64 cs = peer_read_words(ld, slot, out, nwords, 0, 1);
  return ld(slot + PEER_SLOT_WORDS) == peer_tag(exchange, cs, nwords);
}

}  // namespace dp
