"""The mailbox protocol of the peer exchange (deep-prove_amd/csrc/peer_mailbox.h) without a GPU: tests/support/peer_mailbox_check.cpp runs the header's own post /
read functions over std::atomic mailboxes with W = 1, 2, 4, 8 threads as ranks — 200 exchanges, message lengths 1 to 2048 words, both modes, random delays — and
checks that stale and torn slots are refused. The same stand-alone program once plain, once under ThreadSanitizer, once under Address- and UB-Sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "peer_mailbox_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "peer mailbox ok=1" in r.stdout, r.stdout + r.stderr
    assert "exchanges 200 per world" in r.stdout and "failures 0" in r.stdout, r.stdout
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r.stdout


def test_header_states_layout_and_the_two_parity_argument():
    src = open(os.path.join(ROOT, "deep-prove_amd", "csrc", "peer_mailbox.h")).read()
    assert "PEER_SLOT_WORDS = 2048" in src and "Why two parities suffice" in src


def test_every_rank_gathers_what_was_posted_and_bad_slots_are_refused(tmp_path):
    _build_and_run(tmp_path, "peer_mailbox_check", ["-O2"])


@pytest.mark.parametrize("name,flags", [("tsan", ["-fsanitize=thread"]), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_protocol_program_under_host_sanitizers(tmp_path, name, flags):
    _build_and_run(tmp_path, "peer_mailbox_check_" + name, ["-O1", "-g"] + flags)
