// The placement policy of dp_model_prove_batch (capi.cpp prove_batch_body) as pure arithmetic: how large a worker's arena is, how many proofs fit in flight,
// how they are grouped into cohorts, which cohorts share a launch group, and how many host threads drive them. Nothing of HIP and nothing of the device
// interface: tests/support/batch_plan_check.cpp calls it on a CPU, with the environment of a box it does not have (4 hardware queues, a 16-CPU quota).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace dp {

// DP_TIMING, read per call (the tests change it between calls of one process)
inline bool timing_on() { const char* e = getenv("DP_TIMING"); return e && atoi(e); }
// DP_HOST_THREADS as default_host_threads takes it: 0 = not set, else at least 1
inline int env_host_threads() { const char* e = getenv("DP_HOST_THREADS"); return e ? std::max(1, atoi(e)) : 0; }
// Host threads of a call: what the caller or DP_HOST_THREADS asks for (`asked` > 0), else the CPUs the process may really use (cgroup quota, fiber.h
// host_cpu_budget), leaving two for the HIP runtime's own threads. Every entry point puts its own cap on top.
inline size_t default_host_threads(int asked, double cpu_budget) { return asked > 0 ? (size_t)asked : (size_t)std::max(1.0, cpu_budget - 2.0); }

// The knobs of one call of prove_batch_body, parsed. Read once per call and never kept in a static: the GPU tests change these variables between calls.
struct BatchEnv {
  bool has_arena = false; size_t arena_bytes = 0;  // DP_WORKER_ARENA_BYTES
  double hbm_fraction = 0.9;                       // DP_HBM_FRACTION, clamped to [0.01, 0.95]
  int cohort = -1;                                 // DP_COHORT (-1: not set; 0: no cohorts)
  size_t launch_groups = 0;                        // DP_LAUNCH_GROUPS (0: not set; else >= 1)
  int hw_queues = 0;                               // GPU_MAX_HW_QUEUES (0: not set)
  int host_threads = 0;                            // DP_HOST_THREADS (0: not set; else >= 1)
  bool host_sponge = false; int sponge_threads = 6;  // DP_HOST_SPONGE, DP_SPONGE_THREADS
  size_t prep_threads = 2, prep_ahead = 0;         // DP_PREP_THREADS (0 = off), DP_PREP_AHEAD (0: not set = the proofs in flight)
  double stagger_ms = 0.0;                         // DP_COHORT_STAGGER_MS
  bool timing = false;                             // DP_TIMING
  static BatchEnv read() {
    BatchEnv v;
    if (const char* e = getenv("DP_WORKER_ARENA_BYTES")) { v.has_arena = true; v.arena_bytes = strtoull(e, nullptr, 10); }
    if (const char* e = getenv("DP_HBM_FRACTION")) v.hbm_fraction = std::min(0.95, std::max(0.01, atof(e)));
    if (const char* e = getenv("DP_COHORT")) v.cohort = std::max(0, atoi(e));
    if (const char* e = getenv("DP_LAUNCH_GROUPS")) v.launch_groups = (size_t)std::max(1, atoi(e));
    if (const char* e = getenv("GPU_MAX_HW_QUEUES")) v.hw_queues = std::max(0, atoi(e));
    v.host_threads = env_host_threads();
    if (const char* e = getenv("DP_HOST_SPONGE")) v.host_sponge = atoi(e) != 0;
    if (const char* e = getenv("DP_SPONGE_THREADS")) v.sponge_threads = std::max(1, atoi(e));
    if (const char* e = getenv("DP_PREP_THREADS")) v.prep_threads = (size_t)std::max(0, atoi(e));
    if (const char* e = getenv("DP_PREP_AHEAD")) v.prep_ahead = (size_t)std::max(1, atoi(e));
    if (const char* e = getenv("DP_COHORT_STAGGER_MS")) v.stagger_ms = std::max(0.0, atof(e));
    v.timing = timing_on();
    return v;
  }
};

// Arena of a worker: DP_WORKER_ARENA_BYTES, else 1.25 x the largest footprint a proof of this model has had (one proof
// alone runs in latency mode, whose multi-workgroup sumchecks keep every fold level: an upper bound of what a proof in
// flight needs) + 64 MB (at least 256 MB), else — nothing proved yet — 1.5 GB. The number of proofs in flight is cut to what fits in
// 90 % of the free HBM instead of failing: `concurrency` is a cap, not a demand.
// (round 6: 1.125 x the footprint + 16 MB in steps of 16 MB — 336 MB for Dense-4M where 1.25 x + 64 MB in steps of 64 gave 448: a proof's footprint does not depend on
// its input, the margin only has to cover what latency mode and throughput mode allocate differently, and throughput mode allocates LESS; ~700 proofs fit in flight
// instead of ~540, and the rate still grows with them: 1 066 / 1 116 proofs/s at 448 / 660, tools/r06/call23.sh)
inline size_t worker_arena_bytes(const BatchEnv& env, size_t prove_peak) {
  const size_t MB64 = size_t(64) << 20, MB16 = size_t(16) << 20;
  if (env.has_arena) return env.arena_bytes;
  return prove_peak ? std::max(4 * MB64, ((prove_peak + prove_peak / 8 + MB16 + MB16 - 1) / MB16) * MB16) : (size_t(3) << 29);
}
// What one worker takes of the HBM: its arena + its staging and small buffers (the twiddle / coset tables are the context's, shared)
inline size_t worker_hbm_bytes(size_t arena) { return arena + (size_t(24) << 20); }
// The proofs in flight that fit: the workers there are, the context, and as many more workers as fit in DP_HBM_FRACTION (default 0.9) of the FREE HBM — the
// share this process sizes its workers against: less when several processes share one GPU (bench.py with DP_FORCE_DEVICE: both ranks read the same free figure
// at the same moment)
inline size_t in_flight_cap(size_t workers_now, size_t free_bytes, size_t arena, const BatchEnv& env) {
  return workers_now + 1 + (size_t)((double)free_bytes * env.hbm_fraction / (double)worker_hbm_bytes(arena));
}

struct BatchPlan {
  size_t nw = 0;                         // proofs in flight (after the cap and after worker creation)
  size_t csize = 0, nco = 0, ngroups = 0;  // members per cohort (at most), cohorts, launch groups
  size_t nth = 1;                        // host threads that prove
  size_t nprep = 0, prep_ahead = 0;      // helper threads that prepare inputs ahead, and how far beyond the input handed out last
  double stagger_ms = 0.0;               // cohort c starts c * stagger_ms late (0: off)
  // cohorts c < ngroups lead a group: cohorts c, c + ngroups, c + 2 ngroups, ... launch through it
  size_t lead(size_t c) const { return (nco - c + ngroups - 1) / ngroups; }
  size_t leader_of(size_t c) const { return c % ngroups; }
  size_t cohort_of(size_t wi) const { return wi % nco; }
  size_t thread_of(size_t wi) const { return (nco ? wi % nco : wi) % nth; }
};

inline BatchPlan plan_batch(const BatchEnv& env, size_t nw, size_t nproofs, double cpu_budget, long idle_sleep_ns) {
  BatchPlan p;
  p.nw = nw;
  // Cohorts (hip_dev.hip struct Cohort, cohort.h): the proofs in flight are grouped into cohorts of DP_COHORT members (default: in flight / 22, rounded up)
  // that prove in lock step — launch number i of all members of a cohort is ONE kernel launch — with one host thread per cohort.
  // DP_COHORT=0: every proof on its own stream (the round-1 scheme).
  // Default: as many cohorts as hardware queues serve without time slicing (22 of the 24), each as small as that allows — a merged
  // launch ends with its slowest member, so small cohorts stall less (batch of 8: 121 ms with cohorts of 1, 165 ms with one cohort
  // of 8; batch of 64: 262 ms with cohorts of 3, 302 ms with 12; 256 in flight: cohorts of 12; profiles/r02_batch_cohort_sweep.txt)
  p.csize = env.cohort >= 0 ? (size_t)env.cohort : std::max<size_t>(1, (nw + 22 - 1) / 22);
  p.nco = (p.csize >= 1 && nw > 1) ? (nw + p.csize - 1) / p.csize : 0;
  // Launch groups (cohort.h): the cohorts are dealt round robin to DP_LAUNCH_GROUPS groups — default: the hardware queues of the process (GPU_MAX_HW_QUEUES, which
  // the library's constructor guarantees is present) when there are fewer of them than cohorts, otherwise one group per cohort, i.e. every cohort launches on
  // its own as it always has. The cohorts of a group share one stream, one argument ring (the sum of theirs) and every launch: streams that share a hardware
  // queue run their kernels one after the other, and a one-workgroup tail lasts as long as a member's dependent chain however many members it has — five or
  // six cohorts on one queue pay it five or six times in a row, a group once. Host work stays where it was: one thread per cohort (cohorts of 176 on four
  // threads are host-bound, NOTES_NEXT_ROUND.md). DP_STREAM_SHARE (cohorts taking turns on one stream, measured -3 % / -11 %,
  // profiles/r05_stream_share_ab.txt) went with this: a group is the same sharing with the launches merged.
  p.ngroups = p.nco;
  if (env.launch_groups) p.ngroups = env.launch_groups;
  else if (env.hw_queues >= 1 && (size_t)env.hw_queues < p.nco) p.ngroups = (size_t)env.hw_queues;
  p.ngroups = std::min(p.ngroups, p.nco);
  // `nw` proofs in flight on `nth` host threads: every worker is a fiber; a thread switches to its next fiber whenever the
  // current one waits for the device (fiber.h). All members of a cohort live on one thread (what several cohorts share is their launch group's, behind its lock);
  // cohorts (or, without cohorts, workers) are dealt round robin to the threads. The thread count follows the CPUs the
  // process may really use (cgroup quota), leaving two for the HIP runtime's own threads.
  p.nth = default_host_threads(env.host_threads, cpu_budget);
  // the sponge servers (csrc/sponge_host.h) spin too: they come out of the same CPU budget
  if (!env.host_threads && env.host_sponge) p.nth = (size_t)std::max(2.0, cpu_budget - 2.0 - (double)env.sponge_threads);
  // with sleeping idle threads (fiber.h, DP_IDLE_SLEEP_US) a cohort's thread costs what its members' host work costs (~0.3 cores), not a whole core of polling:
  // one thread per cohort as long as that is at most twice the CPU budget (22 cohorts on a 16-CPU quota: 6.3 cores busy)
  if (!env.host_threads && p.nco && nw > 1 && idle_sleep_ns > 0 && (double)p.nco <= 2.0 * cpu_budget) p.nth = std::max(p.nth, p.nco);
  p.nth = std::min(p.nth, p.nco ? p.nco : nw);
  // The host work a proof starts with — inference and the host half of the witness generation (zkml.h witness_host: lookup columns, table multiplicities;
  // 0.6 ms for Dense-4M, ~10 ms for the transformer layer) — is made AHEAD of the proofs by DP_PREP_THREADS helper threads (default 2, 0 = off): the members of
  // a cohort start a proof together on ONE host thread, and until the last of them has submitted its first launch the cohort's stream is idle.
  // (The first nw proofs start at once, their workers prepare them themselves: a batch of no more than nw proofs has no helpers.)
  p.nprep = (nw > 1 && nproofs > nw) ? env.prep_threads : 0;
  p.prep_ahead = env.prep_ahead ? env.prep_ahead : nw;  // inputs prepared beyond the one handed out last
  // DP_COHORT_STAGGER_MS = d (diagnostic, default 0): cohort c starts c * d milliseconds late. The cohorts of a batch otherwise run IN PHASE — identical launch sequences
  // from a common start: every queue in one-workgroup tails, then every queue in the streaming kernels, then every queue hashing (profiles/r06_timeline_704.txt). A
  // staggered start persists (profiles/r06_timeline_704_staggered.txt) and changes the rate by nothing, in every combination tried (profiles/r06_plateau_sweeps.txt,
  // call 16 / 20 / 21 / 24): a tail that starts beside other cohorts' hash layers waits milliseconds for room.
  p.stagger_ms = (p.nco && nproofs > nw) ? env.stagger_ms : 0.0;
  return p;
}

}  // namespace dp
