"""The host build of tests/support/field_probe.hip (g++ -DDP_PROBE_HOST) on the input file of tests/support/field_cases.py: the portable forms that the
host, the CPU SIMT emulator and every -DDP_NO_GFX950_ASM library compile — p2f::mul / red128 / mul_add_w / w_reduce (poseidon2_fast.h), p2l_ref_fma3 /
p2l_ref_join3 (kernels.inc), the canonical wrappers of gl64.h, a3_add_prod7 / a3_reduce / ExAcc (gl64_lazy.h) and the one-lane Poseidon2 — against Python
integers, on any-u64 edge values, the inputs that send the gfx950 forms down their rare paths, and random data. The same cases, reference and file
parsing serve tests/test_gpu_field_forms.py, which runs the two device builds."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from support import field_cases as fc  # noqa: E402


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    import __graft_entry__ as entry
    exe = entry.build_field_probe()[2]
    d = tmp_path_factory.mktemp("field_probe_host")
    plan = fc.write_input(str(d / "input.bin"))
    r = subprocess.run([exe, str(d / "input.bin"), str(d)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "variant: host" in r.stdout, r.stdout + r.stderr
    return plan, {s: fc.read_words(str(d / f"{s}.bin")) for s in "abcde"}


def test_raw_forms_on_any_u64(host_run):
    """section a: every value is the reference mod p; under `if (lane & 1)` the other records keep the sentinel"""
    plan, out = host_run
    pos = 0
    for blk in plan["form"]:
        got = out["a"][pos:pos + blk.n * fc.A_OUT].reshape(blk.n, fc.A_OUT)
        pos += blk.n * fc.A_OUT
        want, _ = fc.form_expected(blk)
        act = fc.form_active(blk)
        assert (got[~act] == np.uint64(fc.SENTINEL)).all()
        bad = np.argwhere((got[act].astype(object) % fc.P) != want[act])
        assert len(bad) == 0, f"{len(bad)} mismatches, first (record, column) {bad[0]}: record {blk.recs[act][bad[0][0]]}"
    assert pos == len(out["a"]) and len(out["b"]) == 0 and len(out["d"]) == 0


def test_wrappers_are_bit_exact_canonical(host_run):
    """section c: gl_mul .. ex_inv on canonical operands, the lz:: products and ExAcc on any representative, mul_add_w"""
    plan, out = host_run
    pos = 0
    for blk in plan["wrap"]:
        want = fc.wrapper_expected(blk)
        got = out["c"][pos:pos + want.size].reshape(want.shape)
        pos += want.size
        bad = np.argwhere(got.astype(object) != want)
        assert len(bad) == 0, f"block tag {blk.tag}: {len(bad)} mismatches, first (record, word) {bad[0]}"
    assert pos == len(out["c"])


def test_one_lane_poseidon2(host_run):
    """section e, one-lane route: p2f::permute and p2f::compress give the independent big-int permutation / digest, canonical"""
    plan, out = host_run
    blk = plan["perm"][-1]
    assert blk.tag == fc.TAG_PERM1 and len(out["e"]) == blk.n * fc.PERM1_OUT
    got = out["e"].reshape(blk.n, fc.PERM1_OUT).astype(object)
    exp = fc.perm_expected()
    for row, i in zip(got, blk.meta["idx"]):
        assert list(row[:8]) == exp[i][0] and list(row[8:]) == exp[i][1], f"state {i}"
