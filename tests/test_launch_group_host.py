"""The launch group of merged cohort launches (deep-prove_amd/csrc/cohort.h) without a GPU: tests/support/launch_group_check.cpp drives the header's own code from
four threads (cohorts) of three members over 300 launches with random yields, members leaving at different launch numbers and one failing early — every launch
fired exactly once and in order, count = the members present, every pack intact in its slot, no ring region reused while its launch is unfired or in flight,
and the program ends (its own watchdog exits non-zero). The same stand-alone program once plain and once under ThreadSanitizer (when the compiler has its runtime)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "launch_group_check.cpp")
CXX = ["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(CXX + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "launch group ok=1" in r.stdout, r.stdout + r.stderr
    assert "launches 300 " in r.stdout and "failures 0" in r.stdout, r.stdout
    assert "FAIL" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr, r.stderr


def _has_tsan(tmp_path):
    probe = tmp_path / "tsan_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=thread", "-o", str(tmp_path / "tsan_probe"), str(probe)], capture_output=True).returncode == 0


def test_header_is_free_of_hip_and_states_the_lock_rule():
    src = open(os.path.join(ROOT, "deep-prove_amd", "csrc", "cohort.h")).read()
    assert "hip_runtime" not in src and "hipStream" not in src.replace("a hipStream_t", "")
    assert "never across a device wait, a fiber yield or a sleep" in src


def test_group_fires_every_launch_once_in_order_with_the_members_present(tmp_path):
    _build_and_run(tmp_path, "launch_group_check", ["-O2"])


def test_group_under_thread_sanitizer(tmp_path):
    flags = ["-O1", "-g"] + (["-fsanitize=thread"] if _has_tsan(tmp_path) else [])  # (no runtime: the plain program once more)
    _build_and_run(tmp_path, "launch_group_check_tsan", flags)
