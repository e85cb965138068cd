// The placement policy of dp_model_prove_batch (deep-prove_amd/csrc/batch_plan.h) without a GPU: prints what the header decides for ONE case —
//   batch_plan_check NW NPROOFS CPU_BUDGET IDLE_SLEEP_NS PROVE_PEAK_BYTES FREE_HBM_BYTES WORKERS_NOW
// with the knobs in the environment, as the library reads them — one "key value" line each; tests/test_batch_plan_host.py compares them with figures worked
// out by hand. The two invariants every plan has to keep are checked here as well (exit status 1).
#include "../../deep-prove_amd/csrc/batch_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  if (argc != 8) { fprintf(stderr, "usage: batch_plan_check NW NPROOFS CPU_BUDGET IDLE_SLEEP_NS PROVE_PEAK_BYTES FREE_HBM_BYTES WORKERS_NOW\n"); return 2; }
  const size_t nw = strtoull(argv[1], nullptr, 10), nproofs = strtoull(argv[2], nullptr, 10);
  const double budget = atof(argv[3]);
  const long idle_ns = atol(argv[4]);
  const size_t peak = strtoull(argv[5], nullptr, 10), free_b = strtoull(argv[6], nullptr, 10), workers_now = strtoull(argv[7], nullptr, 10);
  const dp::BatchEnv env = dp::BatchEnv::read();
  const size_t arena = dp::worker_arena_bytes(env, peak);
  const dp::BatchPlan p = dp::plan_batch(env, nw, nproofs, budget, idle_ns);
  printf("arena %zu\nhbm_fraction %.4f\nin_flight_cap %zu\ntiming %d\n", arena, env.hbm_fraction, dp::in_flight_cap(workers_now, free_b, arena, env), dp::timing_on() ? 1 : 0);
  printf("nw %zu\ncsize %zu\nnco %zu\nngroups %zu\nnth %zu\nnprep %zu\nprep_ahead %zu\nstagger_ms %.3f\n", p.nw, p.csize, p.nco, p.ngroups, p.nth, p.nprep, p.prep_ahead, p.stagger_ms);
  printf("leads");
  for (size_t c = 0; c < p.ngroups; c++) printf(" %zu", p.lead(c));
  printf("\nfollower_leaders");  // of cohorts ngroups .. nco - 1
  for (size_t c = p.ngroups; c < p.nco; c++) printf(" %zu", p.leader_of(c));
  printf("\ncohort_of");
  for (size_t wi = 0; wi < nw && p.nco; wi++) printf(" %zu", p.cohort_of(wi));
  printf("\nthread_of");
  for (size_t wi = 0; wi < nw; wi++) printf(" %zu", p.thread_of(wi));
  printf("\ndefault_host_threads %zu %zu %zu\n", dp::default_host_threads(0, budget), dp::default_host_threads(5, budget), dp::default_host_threads(-1, budget));
  int bad = 0;
  size_t sum = 0;
  for (size_t c = 0; c < p.ngroups; c++) sum += p.lead(c);
  if (sum != p.nco) { fprintf(stderr, "FAIL: the lead sizes sum to %zu, there are %zu cohorts\n", sum, p.nco); bad = 1; }
  for (size_t wi = 0; wi < nw && p.nco; wi++) {
    const size_t c = p.cohort_of(wi), leader = c < p.ngroups ? c : p.leader_of(c);
    if (c >= p.nco || leader >= p.ngroups) { fprintf(stderr, "FAIL: worker %zu: cohort %zu, group leader %zu of %zu groups\n", wi, c, leader, p.ngroups); bad = 1; }
  }
  for (size_t wi = 0; wi < nw; wi++) if (p.thread_of(wi) >= p.nth) { fprintf(stderr, "FAIL: worker %zu on thread %zu of %zu\n", wi, p.thread_of(wi), p.nth); bad = 1; }
  printf("invariants ok=%d\n", !bad);
  return bad;
}
