"""The hand-written gfx950 instruction sequences of deep-prove_amd/csrc/gl64_gfx950.h, and everything the kernels build from them, checked as FUNCTIONS on
the GPU: gx::mul / fma / mul_small, the deferred-borrow forms mul_f / fma3_f / join3_f with their flag words, the canonical and lazy wrappers, the DPP
blocks lin_full / lin_sum8 and the lane-parallel Poseidon2 — on any-u64 edge values, on the input families that take each correction branch (random data
takes them once in 2^64), placed in the waves every way a wave-uniform branch with a per-lane correction can go wrong, and under a partial EXEC mask.

tests/support/field_probe.hip runs the forms and writes files; the cases and the reference (Python integers) are tests/support/field_cases.py. The fixture
runs the asm build of the probe once, then the -DDP_NO_GFX950_ASM build once, each in its own process; if the first fails the second is not started and
every test fails from the recorded output. The tests only parse files.

`if (flag | pend)` of p2l_permute is covered in two halves: the flag words by the section-b tests (the forms set exactly the bits of the lanes that borrowed),
the second pass by permute_impl<true> on the section-e states. No Poseidon2 input that sets a flag inside a permutation is known."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from support import field_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = np.uint64(fc.SENTINEL)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    import __graft_entry__ as entry
    exes = entry.build_field_probe()
    d = tmp_path_factory.mktemp("field_probe")
    plan = fc.write_input(str(d / "input.bin"))
    runs = {}
    for name, exe in (("asm", exes[0]), ("noasm", exes[1])):
        od = d / name
        od.mkdir()
        try:
            r = subprocess.run([exe, str(d / "input.bin"), str(od)], capture_output=True, text=True, timeout=120)
            rc, log = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            rc, log = "timeout", f"{e.stdout or ''}{e.stderr or ''}"
        if rc != 0:
            runs[name] = (f"the {name} probe ended with {rc}: {log}", None)
            break  # nothing more is started on the GPU
        runs[name] = (log, {s: fc.read_words(str(od / f"{s}.bin")) for s in "abcde"})
    return plan, runs


def _out(probes, name):
    plan, runs = probes
    assert name in runs, "not run: " + runs["asm"][0]
    log, out = runs[name]
    assert out is not None, log
    assert ("variant: gfx950 asm" if name == "asm" else "variant: portable device forms") in log, log
    return plan, out


def _form_a(plan, out):
    """[(block, (n, 10) values)]"""
    pos, res = 0, []
    for blk in plan["form"]:
        res.append((blk, out["a"][pos:pos + blk.n * fc.A_OUT].reshape(blk.n, fc.A_OUT)))
        pos += blk.n * fc.A_OUT
    assert pos == len(out["a"])
    return res


def _form_b(plan, out):
    """[(block, (n, 3) values, per-lane bit of the wave's flag word, of its pend word)]"""
    pos, res = 0, []
    for blk in plan["form"]:
        waves = (blk.n + 63) // 64
        vals = out["b"][pos:pos + blk.n * fc.B_OUT].reshape(blk.n, fc.B_OUT)
        words = out["b"][pos + blk.n * fc.B_OUT:pos + blk.n * fc.B_OUT + 2 * waves].reshape(waves, 2)
        pos += blk.n * fc.B_OUT + 2 * waves
        assert not (words == SENT).any(), "a wave did not store its flag words"
        i = np.arange(blk.n)
        bits = (words[i >> 6] >> (i & 63).astype(np.uint64)[:, None]) & np.uint64(1)
        res.append((blk, vals, bits[:, 0].astype(bool), bits[:, 1].astype(bool)))
    assert pos == len(out["b"])
    return res


@pytest.mark.parametrize("name", ["asm", "noasm"])
def test_raw_forms_on_any_u64(probes, name):
    """section a: gx::mul, gx::fma, gx::mul_small (k = 0, 1, 7, 2^31, 2^32 - 1) and the FIX = true forms mul_f / fma3_f / join3_f are the reference mod p on the
    edge grid, the documented bound corners of fma3_f / join3_f, every rare family in every wave placement, and random any-u64 / canonical data; the lanes
    outside `if (lane & 1)` keep the sentinel. (noasm: the portable forms of the same calls.)"""
    plan, out = _out(probes, name)
    for blk, got in _form_a(plan, out):
        want, _ = fc.form_expected(blk)
        act = fc.form_active(blk)
        assert (got[~act] == SENT).all(), "an inactive lane stored"
        bad = np.argwhere((got[act].astype(object) % fc.P) != want[act])
        cols = sorted({int(c) for c in bad[:, 1]}) if len(bad) else []
        assert len(bad) == 0, (f"{len(bad)} mismatches in columns {cols} (0 mul, 1 fma, 2-6 mul_small, 7 mul_f, 8 fma3_f, 9 join3_f); first: record "
                               f"{[hex(int(v)) for v in blk.recs[act][bad[0][0]]]} kind {np.array(blk.meta['kinds'], dtype=object)[act][bad[0][0]]!r} got {hex(int(got[act][tuple(bad[0])]))}")


def test_deferred_flags_name_exactly_the_lanes_that_borrowed(probes):
    """section b: flag = pend = 0; mul_f<false>; fma3_f<false>; join3_f<false>. Per lane and block exactly one of: the value is the reference mod p, or it is
    off by 2^64 = 2^32 - 1 (mod p) and the lane's bit is set in the word the header assigns to the block — `flag` for the first two, `pend` for the third.
    Every lane of a rare family has its bit, no canonical random case has any, the lanes outside `if (lane & 1)` keep the sentinel and set no bit."""
    plan, out = _out(probes, "asm")
    seen = {k: 0 for k in fc.KINDS[1:]}
    for blk, vals, flag, pend in _form_b(plan, out):
        _, want = fc.form_expected(blk)
        act = fc.form_active(blk)
        assert (vals[~act] == SENT).all(), "an inactive lane stored"
        assert not flag[~act].any() and not pend[~act].any(), "a bit is set for a lane that did not run"
        diff = (vals[act].astype(object) - want[act]) % fc.P  # 0: exact; eps: a borrow of 2^64 not taken back; p - eps: a carry of 2^64 not added
        assert ((diff[:, :2] == 0) | (diff[:, :2] == fc.EPS)).all() and ((diff[:, 2] == 0) | (diff[:, 2] == fc.P - fc.EPS)).all(), "a value is neither the reference nor off by 2^64"
        wrong = diff != 0
        lanes = np.flatnonzero(act)
        bad = np.flatnonzero((wrong[:, 0] | wrong[:, 1]) != flag[act])
        assert len(bad) == 0, f"`flag` differs from the lanes whose first or second block borrowed at records {lanes[bad][:8]} of a launch of {blk.n} (masked: {blk.mode})"
        bad = np.flatnonzero(wrong[:, 2] != pend[act])
        assert len(bad) == 0, f"`pend` differs from the lanes whose third block carried at records {lanes[bad][:8]} of a launch of {blk.n} (masked: {blk.mode})"
        kinds = np.array(blk.meta["kinds"], dtype=object)
        for k in fc.KINDS[1:]:
            sel = act & (kinds == k)
            seen[k] += int(sel.sum())
            assert (pend if k == "join3" else flag)[sel].all(), f"a lane of the rare family {k!r} is not flagged"
        if blk.meta["canonical_random"]:
            assert not flag.any() and not pend.any(), "a canonical random case set a deferred bit"
    assert all(v > 500 for v in seen.values()), seen


def test_portable_forms_set_no_flag(probes):
    """section b of the -DDP_NO_GFX950_ASM build: exact values, the flag words stay 0"""
    plan, out = _out(probes, "noasm")
    for blk, vals, flag, pend in _form_b(plan, out):
        _, want = fc.form_expected(blk)
        act = fc.form_active(blk)
        assert (vals[~act] == SENT).all() and not flag.any() and not pend.any()
        assert ((vals[act].astype(object) % fc.P) == want[act]).all()


@pytest.mark.parametrize("name", ["asm", "noasm"])
def test_wrappers_are_bit_exact_canonical(probes, name):
    """section c: gl_mul, gl_sqr, gl_mul7, ex_mul, ex_mul_base, ex_lerp, ex_lerp_base, ex_inv on canonical operands; lz::ex_mul / ex_fma / ex_fma_base + ex_canon and
    ExAcc (1, 2, 3, 4096 additions, 2^64 - 1 among them) on any representative; p2f::mul_add_w with a row sum of eight any-representative words"""
    plan, out = _out(probes, name)
    pos = 0
    for blk in plan["wrap"]:
        want = fc.wrapper_expected(blk)
        got = out["c"][pos:pos + want.size].reshape(want.shape)
        pos += want.size
        bad = np.argwhere(got.astype(object) != want)
        assert len(bad) == 0, f"block tag {blk.tag}: {len(bad)} mismatches, first (record, word) {bad[0]}: got {hex(int(got[tuple(bad[0])]))} want {hex(int(want[tuple(bad[0])]))}"
    assert pos == len(out["c"])


@pytest.mark.parametrize("name", ["asm", "noasm"])
def test_linear_blocks_give_exact_limbs(probes, name):
    """section d: p2l_lin_full(x, rc) = limbs of circ(2 M4, M4) x + rc and p2l_lin_sum8(x) = the 8-lane sum, limb by limb, on maximal limbs (eight words 2^64 - 1),
    single-hot groups and eight different groups per wave"""
    plan, out = _out(probes, name)
    blk = plan["lin"][0]
    want = fc.lin_expected(blk)
    got = out["d"].reshape(blk.n, fc.LIN_OUT).astype(object)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} limbs differ (columns 0-2 lin_full, 3-5 lin_sum8), first (lane, column) {bad[0]}"


@pytest.mark.parametrize("name", ["asm", "noasm"])
def test_every_permutation_route_gives_the_reference(probes, name):
    """section e: p2l_permute_impl<false>, <true>, p2l_permute, p2l_compress and the one-lane p2f::permute / compress on the same states, 1, 3, 8 and 9 groups per
    64-lane block: the independent big-int permutation / digest, canonical; the first pass sets no flag on these states (a flag that is wrongly set would
    double every one-wave permutation and change no result)"""
    plan, out = _out(probes, name)
    exp = fc.perm_expected()
    pos, covered, sizes = 0, set(), set()
    for blk in plan["perm"]:
        w = fc.PERM_OUT if blk.tag == fc.TAG_PERM else fc.PERM1_OUT
        got = out["e"][pos:pos + blk.n * w].reshape(blk.n, w).astype(object)
        pos += blk.n * w
        for row, i in zip(got, blk.meta["idx"]):
            perm, digest = exp[i]
            if blk.tag == fc.TAG_PERM:
                assert list(row[0:8]) == perm, f"permute_impl<false>, state {i}, {blk.n} groups"
                assert list(row[8:16]) == perm, f"permute_impl<true>, state {i}, {blk.n} groups"
                assert list(row[16:24]) == perm, f"p2l_permute, state {i}, {blk.n} groups"
                assert list(row[24:28]) == digest, f"p2l_compress, state {i}, {blk.n} groups"
                assert not any(row[28:44]), f"a deferred flag is set after the first pass, state {i}, {blk.n} groups"
                covered.add(i); sizes.add(blk.n)
            else:
                assert list(row[0:8]) == perm and list(row[8:12]) == digest, f"one-lane p2f route, state {i}"
    assert pos == len(out["e"]) and covered == set(range(len(exp))) and sizes == set(fc.PERM_GROUPS)


def test_the_two_device_builds_agree(probes):
    """the -DDP_NO_GFX950_ASM probe's outputs, canonicalised, are the asm probe's (section b: wherever the asm form did not defer a borrow)"""
    plan, asm = _out(probes, "asm")
    _, por = _out(probes, "noasm")
    for s in "acde":
        assert len(asm[s]) == len(por[s])
        assert ((asm[s].astype(object) % fc.P) == (por[s].astype(object) % fc.P)).all(), f"section {s}"
    for (blk, va, flag, pend), (_, vp, _, _) in zip(_form_b(plan, asm), _form_b(plan, por)):
        act = fc.form_active(blk)
        keep = np.stack([act & ~flag, act & ~flag, act & ~pend], axis=1)
        assert ((va[keep].astype(object) % fc.P) == (vp[keep].astype(object) % fc.P)).all()
