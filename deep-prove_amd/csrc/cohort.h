// Launch groups: the host side of merged cohort launches, free of HIP (hip_dev.hip supplies the stream, the fire functions and the
// ring's memory; tests/support/launch_group_check.cpp drives the same code from plain threads).
//
// A cohort is a set of proofs of the SAME model proved in lock step by one host thread (each proof a fiber, fiber.h). Proofs of one
// model issue the same sequence of launches with the same shapes — only pointers and challenges differ — so launch number i of every
// member is merged into ONE kc<Body> launch with gridDim.z = members. A LAUNCH GROUP is what the cohorts that share a hardware queue
// have in common: the stream, the argument-pack ring, the queue of launches being assembled and the fire path. With one cohort per
// group (enough hardware queues for every cohort) a group is exactly the cohort of earlier rounds; with several, launch number i of
// ALL their members is one launch, assembled by several host threads: the one-workgroup tails, whose duration is a member's dependent
// chain whatever the member count, are then paid once per group step instead of once per cohort step on a queue the cohorts share.
//
// A member never blocks at a launch: it drops its argument pack and goes on to its next wait (where it yields to the next member of
// its thread); whoever completes a launch's set of packs fires it, still holding the group's lock, so the stream's order is the launch
// sequence. The lock is held for a memcpy and at most a kernel launch: never across a device wait, a fiber yield or a sleep.
#pragma once
#include "dev.h"
#include <atomic>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <utility>

namespace dp {

struct LaunchGroup {
  struct Pending {
    void (*fire)(const Pending&, void* stream);  // also the identity of the kernel (one instantiation per Body)
    const char* name;
    unsigned gx, gy, bx; size_t lds, pack_bytes;
    char* packs; const char* packs_dev;
    int count, expected;
    size_t ring_begin, ring_end;
  };
  // the ring's memory: host memory the device can read (`dev_view` = the device's address of it)
  struct RingHooks { char* (*alloc)(size_t bytes, const char** dev_view); void (*release)(char* ring); };

  std::mutex mu;             // guards everything below
  void* stream = nullptr;    // (a hipStream_t; the owner creates and destroys it)
  int members = 0;           // proofs currently in the group, all cohorts together
  int nominal = 0;           // members when the batch started (every member joins before the first launch): what launch shapes may depend on — `members` shrinks while a batch drains
  int ncohorts = 1;          // cohorts dealt to this group for the current batch: the grid caps of a merged launch scale with it
  char* ring = nullptr; const char* ring_dev = nullptr;
  size_t ring_cap = 0, ring_off = 0;
  RingHooks hooks{nullptr, nullptr};
  std::deque<Pending> q; size_t q_base = 0;            // q[i] = launch number q_base + i of the common sequence, not yet fired
  std::deque<std::pair<size_t, size_t>> inflight;      // (launch number, ring_begin) of fired launches not known to have run
  size_t executed = 0;                                 // every launch number < executed has run to completion
  size_t nfired = 0, npacks = 0;
  std::atomic<size_t> fire_epoch{0};                   // fires so far (read without the lock by the cohorts' DP_TIMING accounting)

  LaunchGroup(void* stream_, size_t ring_bytes, RingHooks h) : stream(stream_), hooks(h) { ring_alloc_(ring_bytes); }
  ~LaunchGroup() { if (ring) hooks.release(ring); }
  LaunchGroup(const LaunchGroup&) = delete;
  LaunchGroup& operator=(const LaunchGroup&) = delete;

  // the cohorts of the next batch: `n` of them, `ring_bytes` of ring in all (the sum of what they would have had on their own). Only between batches.
  void configure(int n, size_t ring_bytes) {
    std::lock_guard<std::mutex> lk(mu);
    if (members || !q.empty() || !inflight.empty()) throw DpError(DP_ERR_SHAPE, "a launch group is regrouped only between batches");
    ncohorts = n > 0 ? n : 1;
    if (ring_bytes > ring_cap) { hooks.release(ring); ring = nullptr; ring_alloc_(ring_bytes); ring_off = 0; }
  }
  // member `li`-th launch of its sequence: add its pack to launch number `li`, fire every launch whose set is complete.
  // Returns the number of launches this call fired.
  size_t submit(size_t li, void (*fire)(const Pending&, void*), const char* name, unsigned gx, unsigned gy, unsigned bx, size_t lds, const void* pack, size_t pack_bytes) {
    std::lock_guard<std::mutex> lk(mu);
    if (li < q_base) throw DpError(DP_ERR_SHAPE, std::string("cohort out of step: a member reached launch ") + name + " after it was fired (the proofs of a cohort must issue identical launch sequences)");
    size_t k = li - q_base;
    if (k > q.size()) throw DpError(DP_ERR_SHAPE, "cohort out of step: launch sequence gap");
    if (k == q.size()) {
      Pending p; p.fire = fire; p.name = name; p.gx = gx; p.gy = gy; p.bx = bx; p.lds = lds; p.pack_bytes = pack_bytes; p.count = 0; p.expected = members;
      p.ring_begin = ring_take_(pack_bytes * (size_t)members); p.ring_end = ring_off;
      p.packs = ring + p.ring_begin % ring_cap; p.packs_dev = ring_dev + p.ring_begin % ring_cap;
      q.push_back(p);
    }
    Pending& p = q[k];
    if (p.fire != fire || p.gx != gx || p.gy != gy || p.bx != bx || p.lds != lds || p.pack_bytes != pack_bytes)
      throw DpError(DP_ERR_SHAPE, std::string("cohort out of step: launch ") + name + " of one member meets " + p.name + " of another (the proofs of a cohort must issue identical launch sequences)");
    if (p.count >= p.expected) throw DpError(DP_ERR_SHAPE, "cohort out of step: too many packs for one launch");
    memcpy(p.packs + (size_t)p.count * pack_bytes, pack, pack_bytes);
    p.count++; npacks++;
    return flush_();
  }
  // a member has seen the result of its launch number `li` (or of a later round of it): everything before it has run
  void note_executed(size_t li) { std::lock_guard<std::mutex> lk(mu); if (li > executed) executed = li; }
  // a proof joins (before the first launch of a batch); returns the launch number its sequence starts at
  size_t join() {
    std::lock_guard<std::mutex> lk(mu);
    if (!q.empty()) throw DpError(DP_ERR_SHAPE, "a proof cannot join a cohort in the middle of a step");
    members++; nominal = members;
    return q_base;
  }
  // a member leaves (its proofs are done, or it failed) having issued `li` launches: later launches no longer wait for it
  size_t leave(size_t li) {
    std::lock_guard<std::mutex> lk(mu);
    members--;
    for (size_t k = li > q_base ? li - q_base : 0; k < q.size(); k++) q[k].expected--;
    return flush_();
  }
  // drain = drain_begin, a wait for the stream OUTSIDE the lock, drain_end: every launch fired before drain_begin has then run
  size_t drain_begin() { std::lock_guard<std::mutex> lk(mu); return q_base; }
  void drain_end(size_t mark) {
    std::lock_guard<std::mutex> lk(mu);
    if (mark > executed) executed = mark;
    while (!inflight.empty() && inflight.front().first < executed) inflight.pop_front();
  }
  void take_stats(size_t* fired, size_t* packs) { std::lock_guard<std::mutex> lk(mu); *fired = nfired; *packs = npacks; nfired = npacks = 0; }

 private:
  void ring_alloc_(size_t bytes) { ring_cap = bytes; ring = hooks.alloc(bytes, &ring_dev); if (!ring) throw DpError(DP_ERR_OOM, "cohort argument ring: no host memory"); }
  // ring space for `bytes` (virtual offsets grow monotonically; physical = virtual mod capacity, regions never straddle
  // the end), never overlapping a region a launch may still read: those of unfired launches and of fired launches not yet
  // known to have run
  size_t ring_take_(size_t bytes) {
    bytes = (bytes + 63) & ~size_t(63);
    while (!inflight.empty() && inflight.front().first < executed) inflight.pop_front();
    size_t head = ring_off;
    if (head % ring_cap + bytes > ring_cap) head += ring_cap - head % ring_cap;
    size_t tail = !inflight.empty() ? inflight.front().second : !q.empty() ? q.front().ring_begin : head;
    if (bytes > ring_cap || head + bytes - tail > ring_cap) throw DpError(DP_ERR_OOM, "cohort argument ring exhausted (DP_COHORT_RING_BYTES)");
    ring_off = head + bytes;
    return head;
  }
  size_t flush_() {
    size_t n = 0;
    while (!q.empty() && q.front().count >= q.front().expected) {
      Pending& p = q.front();
      if (p.count > 0) {
        std::atomic_thread_fence(std::memory_order_release);
        p.fire(p, stream);
        inflight.push_back({q_base, p.ring_begin});
        nfired++; n++;
        fire_epoch.fetch_add(1, std::memory_order_release);
      }
      q.pop_front(); q_base++;
    }
    return n;
  }
};

}  // namespace dp
