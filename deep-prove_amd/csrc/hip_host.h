// The free functions hip_dev.hip defines for capi.cpp: contexts and workers, cohorts and their launch groups, and what the C API reads of a HipDev beyond the
// Dev interface. No HIP types: capi.cpp includes it beside dev.h, hip_dev.hip includes it so that definition and declaration cannot drift apart.
// (The device inference has its own: infer.h hip_infer_*.)
#pragma once
#include "dev.h"
#include <cstddef>
#include <string>

namespace dp {

struct Cohort;  // hip_dev.hip (its launch group: cohort.h)

Dev* make_hip_dev(int device);
Dev* make_hip_worker(int device, size_t arena_bytes);

Cohort* hip_cohort_new();
void hip_cohort_lead(Cohort* c, size_t n);
void hip_cohort_follow(Cohort* c, Cohort* leader);
void hip_cohort_free(Cohort* c);
void hip_cohort_drain(Cohort* c);
void hip_cohort_stats(Cohort* c, size_t* fired, size_t* packs);
void hip_dev_cohort_attach(Dev* d, Cohort* c);
void hip_dev_cohort_detach(Dev* d);

void hip_dev_set_latency_mode(Dev* d, bool on);
void hip_dev_pcs_share(Dev* worker, Dev* owner);
void hip_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
size_t hip_dev_arena_peak(Dev* d);
void hip_dev_arena_peak_reset(Dev* d);
double hip_dev_probe_compress_rate(Dev* d, size_t nodes, int reps);
void hip_dev_peer_all_gather(Dev* d, const Dev::PeerMailboxes* pm, const u64* send, size_t nwords, u64* out);

void hip_dev_profile_enable(Dev* d, bool on);
std::string hip_dev_profile_report(Dev* d);
void hip_dump_wg_times();
void hip_dev_dump_host_stats(Dev* d);
void hip_dev_dump_sc_debug(Dev* d);

}  // namespace dp
