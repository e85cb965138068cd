"""The placement policy of dp_model_prove_batch (deep-prove_amd/csrc/batch_plan.h) without a GPU: worker arena, in-flight cap, cohort size and count, launch
groups (who leads how many, who follows whom), host threads, helper threads. tests/support/batch_plan_check.cpp prints what the header decides for one case,
with the knobs in the CHILD's environment only; every expected figure below was worked out by hand from the rules, none by calling the
header. The 4-queue branch — which a box with 24 hardware queues never takes — is one of the cases. For every case the program also checks that the lead
sizes sum to the number of cohorts and that every worker's cohort launches through a group that exists. And: batch_plan.h and prep_ahead.h include nothing
of HIP and nothing of the device interface."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep-prove_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "support", "batch_plan_check.cpp")
KNOBS = ["DP_WORKER_ARENA_BYTES", "DP_HBM_FRACTION", "DP_COHORT", "DP_LAUNCH_GROUPS", "GPU_MAX_HW_QUEUES", "DP_HOST_THREADS", "DP_HOST_SPONGE", "DP_SPONGE_THREADS",
         "DP_PREP_THREADS", "DP_PREP_AHEAD", "DP_COHORT_STAGGER_MS", "DP_TIMING"]
MiB = 1 << 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", out, SRC])
    return out


def plan(exe, env, nw, nproofs=None, budget=16, idle_ns=20000, peak=0, free=0, workers_now=0):
    child = {k: v for k, v in os.environ.items() if k not in KNOBS}
    child.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([exe] + [str(x) for x in (nw, 3 * nw if nproofs is None else nproofs, budget, idle_ns, peak, free, workers_now)],
                       capture_output=True, text=True, env=child, timeout=60)
    assert r.returncode == 0 and "invariants ok=1" in r.stdout, r.stdout + r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        key, _, rest = ln.partition(" ")
        out[key] = rest
    for k in ("leads", "follower_leaders", "cohort_of", "thread_of"):
        out[k] = [int(x) for x in out[k].split()]
    for k in ("arena", "in_flight_cap", "nw", "csize", "nco", "ngroups", "nth", "nprep", "prep_ahead"):
        out[k] = int(out[k])
    return out


def test_704_in_flight_on_24_queues_every_cohort_launches_on_its_own(exe):
    # ceil(704 / 22) = 32 members, ceil(704 / 32) = 22 cohorts; 24 queues are not fewer than 22 cohorts: one group per cohort
    p = plan(exe, {"GPU_MAX_HW_QUEUES": 24}, 704)
    assert (p["csize"], p["nco"], p["ngroups"]) == (32, 22, 22)
    assert p["leads"] == [1] * 22 and p["follower_leaders"] == []
    assert p["cohort_of"] == [wi % 22 for wi in range(704)]
    # budget 16 leaves 14 threads; 22 cohorts <= 2 x 16 and the idle sleep is on: one thread per cohort
    assert p["nth"] == 22 and p["thread_of"] == [wi % 22 for wi in range(704)]
    assert (p["nprep"], p["prep_ahead"], p["stagger_ms"]) == (2, 704, "0.000")


def test_704_in_flight_on_4_queues_four_groups_lead_6_6_5_5(exe):
    p = plan(exe, {"GPU_MAX_HW_QUEUES": 4}, 704)
    assert (p["csize"], p["nco"], p["ngroups"]) == (32, 22, 4)
    assert p["leads"] == [6, 6, 5, 5]  # cohorts 0 4 8 12 16 20 / 1 5 9 13 17 21 / 2 6 10 14 18 / 3 7 11 15 19
    assert p["follower_leaders"] == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1]  # cohorts 4 .. 21: c % 4
    assert p["nth"] == 22  # (host work stays where it was: one thread per cohort)


def test_448_in_flight(exe):
    p = plan(exe, {}, 448)  # ceil(448 / 22) = 21 (20 x 22 = 440 < 448), ceil(448 / 21) = 22 (21 x 21 = 441 < 448)
    assert (p["csize"], p["nco"], p["ngroups"]) == (21, 22, 22)


def test_19_in_flight_cohorts_of_3_and_the_launch_group_knob(exe):
    p = plan(exe, {"DP_COHORT": 3}, 19)
    assert (p["csize"], p["nco"], p["ngroups"], p["leads"]) == (3, 7, 7, [1] * 7)
    assert p["nth"] == 7  # 14 threads of the budget, at most one per cohort
    p = plan(exe, {"DP_COHORT": 3, "DP_LAUNCH_GROUPS": 2}, 19)
    assert (p["nco"], p["ngroups"], p["leads"], p["follower_leaders"]) == (7, 2, [4, 3], [0, 1, 0, 1, 0])
    p = plan(exe, {"DP_COHORT": 3, "DP_LAUNCH_GROUPS": 99}, 19)
    assert (p["nco"], p["ngroups"], p["leads"]) == (7, 7, [1] * 7)
    p = plan(exe, {"DP_COHORT": 3, "DP_LAUNCH_GROUPS": 0}, 19)  # (clamped to 1)
    assert (p["ngroups"], p["leads"], p["follower_leaders"]) == (1, [7], [0] * 6)
    p = plan(exe, {"DP_COHORT": 3, "DP_LAUNCH_GROUPS": 2, "GPU_MAX_HW_QUEUES": 4}, 19)  # (the knob wins over the queues)
    assert p["ngroups"] == 2


def test_19_in_flight_nothing_set_cohorts_of_one(exe):
    p = plan(exe, {}, 19)
    assert (p["csize"], p["nco"], p["ngroups"], p["nth"]) == (1, 19, 19, 19)


def test_no_cohorts(exe):
    p = plan(exe, {"DP_COHORT": 0}, 20)
    assert (p["csize"], p["nco"], p["ngroups"], p["leads"], p["cohort_of"]) == (0, 0, 0, [], [])
    assert p["nth"] == 14 and p["thread_of"] == [wi % 14 for wi in range(20)]
    p = plan(exe, {"DP_COHORT": -5}, 20)  # (clamped to 0)
    assert (p["csize"], p["nco"]) == (0, 0)


def test_one_proof_in_flight_has_no_cohorts_and_no_helpers(exe):
    p = plan(exe, {}, 1, nproofs=5)
    assert (p["csize"], p["nco"], p["ngroups"], p["nth"], p["nprep"], p["thread_of"]) == (1, 0, 0, 1, 0, [0])


def test_host_threads(exe):
    assert plan(exe, {}, 704, budget=16, idle_ns=20000)["nth"] == 22  # one per cohort: 22 <= 32
    assert plan(exe, {}, 704, budget=16, idle_ns=0)["nth"] == 14      # polling threads: the budget less two
    p = plan(exe, {"DP_COHORT": 1}, 40, budget=16)                    # 40 cohorts > 2 x 16
    assert (p["nco"], p["nth"]) == (40, 14)
    p = plan(exe, {"DP_HOST_THREADS": 3}, 704)
    assert p["nth"] == 3 and p["thread_of"] == [(wi % 22) % 3 for wi in range(704)]
    assert plan(exe, {"DP_HOST_THREADS": 0}, 704)["nth"] == 1         # (clamped to 1: set, not "unset")
    assert plan(exe, {"DP_HOST_THREADS": 64}, 704)["nth"] == 22       # never more than cohorts
    assert plan(exe, {}, 704, budget=2.5, idle_ns=0)["nth"] == 1      # max(1, 0.5)
    # the sponge servers come out of the same budget: 16 - 2 - 6 = 8, 16 - 2 - 10 = 4, at least 2; an explicit thread count wins
    assert plan(exe, {"DP_HOST_SPONGE": 1}, 704, idle_ns=0)["nth"] == 8
    assert plan(exe, {"DP_HOST_SPONGE": 1, "DP_SPONGE_THREADS": 10}, 704, idle_ns=0)["nth"] == 4
    assert plan(exe, {"DP_HOST_SPONGE": 1, "DP_SPONGE_THREADS": 40}, 704, idle_ns=0)["nth"] == 2
    assert plan(exe, {"DP_HOST_SPONGE": 1, "DP_HOST_THREADS": 5}, 704, idle_ns=0)["nth"] == 5
    assert plan(exe, {"DP_HOST_SPONGE": 0}, 704, idle_ns=0)["nth"] == 14
    # what dp_async_create and dp_verify_batch share with the batch: asked > 0 wins, else the budget less two
    assert plan(exe, {}, 2)["default_host_threads"] == "14 5 14"


def test_helper_threads_and_stagger(exe):
    assert plan(exe, {"DP_PREP_THREADS": 0}, 8)["nprep"] == 0
    assert plan(exe, {"DP_PREP_THREADS": 5}, 8)["nprep"] == 5
    assert plan(exe, {}, 8, nproofs=8)["nprep"] == 0  # every proof starts at once: nothing to prepare ahead
    assert plan(exe, {"DP_PREP_AHEAD": 5}, 8)["prep_ahead"] == 5
    assert plan(exe, {"DP_PREP_AHEAD": 0}, 8)["prep_ahead"] == 1
    assert plan(exe, {"DP_COHORT_STAGGER_MS": 1.5}, 8)["stagger_ms"] == "1.500"
    assert plan(exe, {"DP_COHORT_STAGGER_MS": 1.5}, 8, nproofs=8)["stagger_ms"] == "0.000"
    assert plan(exe, {"DP_COHORT_STAGGER_MS": 1.5, "DP_COHORT": 0}, 8)["stagger_ms"] == "0.000"
    assert plan(exe, {"DP_COHORT_STAGGER_MS": -3}, 8)["stagger_ms"] == "0.000"
    assert plan(exe, {"DP_TIMING": 2}, 8)["timing"] == "1" and plan(exe, {"DP_TIMING": 0}, 8)["timing"] == "0" and plan(exe, {}, 8)["timing"] == "0"


def test_worker_arena(exe):
    assert plan(exe, {}, 2, peak=0)["arena"] == 1536 * MiB                 # nothing proved yet: 3 << 29
    assert plan(exe, {}, 2, peak=300 * MiB)["arena"] == 368 * MiB          # 300 + 37.5 + 16 = 353.5 -> 23 steps of 16
    assert plan(exe, {}, 2, peak=10 * MiB)["arena"] == 256 * MiB           # 27.25 -> 32, at least 256
    assert plan(exe, {}, 2, peak=256 * MiB)["arena"] == 304 * MiB          # 256 + 32 + 16 = 304 exactly: no step added
    assert plan(exe, {"DP_WORKER_ARENA_BYTES": 123456789}, 2, peak=300 * MiB)["arena"] == 123456789


def test_in_flight_cap(exe):
    # a worker takes its arena + 24 MiB: 976 + 24 = 1000 MiB; 100 500 MiB free
    arena = {"DP_WORKER_ARENA_BYTES": 976 * MiB}
    free = 100500 * MiB
    p = plan(exe, arena, 2, free=free)
    assert p["hbm_fraction"] == "0.9000" and p["in_flight_cap"] == 1 + 90      # floor(90.45)
    assert plan(exe, arena, 2, free=free, workers_now=3)["in_flight_cap"] == 4 + 90
    p = plan(exe, dict(arena, DP_HBM_FRACTION=2), 2, free=free)
    assert p["hbm_fraction"] == "0.9500" and p["in_flight_cap"] == 1 + 95      # floor(95.475)
    p = plan(exe, dict(arena, DP_HBM_FRACTION=0.001), 2, free=free)
    assert p["hbm_fraction"] == "0.0100" and p["in_flight_cap"] == 1 + 1       # floor(1.005)
    assert plan(exe, dict(arena, DP_HBM_FRACTION=0.5), 2, free=free)["in_flight_cap"] == 1 + 50
    assert plan(exe, arena, 2, free=0)["in_flight_cap"] == 1


def test_headers_are_free_of_hip_and_of_the_device_interface():
    for name in ("batch_plan.h", "prep_ahead.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert "hip_runtime" not in src and "hipStream" not in src and "hipError" not in src, name
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
        assert includes and all("/" not in h and not h.endswith(".h") and not h.startswith("hip") for h in includes), (name, includes)  # standard headers only
