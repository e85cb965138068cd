"""The prepare-ahead hand-over of dp_model_prove_batch (deep-prove_amd/csrc/prep_ahead.h) without a GPU: tests/support/prep_ahead_check.cpp drives the header's own
code from four consumer threads and two helper threads over 2 000 items, with a make() that yields at random and throws for a fixed subset when a helper calls
it and for a smaller subset whoever calls it — every item taken exactly once, a helper's failure repeated by the consumer (and succeeding), a failure for
everybody surfacing the consumer's own exception, helpers never further ahead than allowed, stop() ending helpers that wait, and the program ends (its own
watchdog exits non-zero). The same stand-alone program once plain and once under ThreadSanitizer (when the compiler has its runtime)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "prep_ahead_check.cpp")
CXX = ["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(CXX + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "prep ahead ok=1" in r.stdout, r.stdout + r.stderr
    assert "items 2000 " in r.stdout and "own errors 21 " in r.stdout and "failures 0" in r.stdout, r.stdout  # (i % 97 == 5 below 2 000: 21 items)
    assert "FAIL" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr, r.stderr


def _has_tsan(tmp_path):
    probe = tmp_path / "tsan_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=thread", "-o", str(tmp_path / "tsan_probe"), str(probe)], capture_output=True).returncode == 0


def test_every_item_is_taken_once_and_failures_are_the_consumers_own(tmp_path):
    _build_and_run(tmp_path, "prep_ahead_check", ["-O2"])


def test_hand_over_under_thread_sanitizer(tmp_path):
    flags = ["-O1", "-g"] + (["-fsanitize=thread"] if _has_tsan(tmp_path) else [])  # (no runtime: the plain program once more)
    _build_and_run(tmp_path, "prep_ahead_check_tsan", flags)
