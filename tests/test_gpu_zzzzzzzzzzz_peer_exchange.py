"""The sharded sumcheck with the ranks' shares exchanged through peer-mapped mailboxes (include/deep_prove_hip_peer.h, k_peer_exchange_publish): ranks as
threads of one process and ranks as processes, on one GPU. The oracle is the yardstick of every case: proof words, final evaluations and the next challenge of
every rank's transcript."""
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "peer_child.py")
JOIN_S = 90.0  # a rank that waits for a peer gives up after 20 s on the device, 30 s on the host: no thread outlives this


def _mixed_case(nv, world):
    """the tables and terms of test_in_library_sharded_loop_on_several_contexts: base, extension, base; three terms"""
    rng = np.random.default_rng(4100 + 16 * nv + world)
    exts = [False, True, False]
    tabs = [rng.integers(0, P, size=(2 if e else 1) << nv, dtype=np.uint64) for e in exts]
    terms = [((1, 0), [0, 1, 2]), ((5, 7), [1, 2]), ((9, 0), [0])]
    return tabs, exts, terms


def _oracle(oracle, nv, tabs, exts, terms):
    ot = oracle.transcript(b"test")
    proof, finals = oracle.sumcheck_prove(nv, tabs, exts, terms, ot)
    return proof, finals, ot.read_challenge()


class Ranks:
    """`world` contexts on GPU 0, a connected PeerGroup each; prove() runs one Python thread per rank (ctypes releases the GIL)"""

    def __init__(self, dpa, world):
        self.dpa, self.world = dpa, world
        self.devs = [dpa.Device(0) for _ in range(world)]
        self.groups = [dpa.sharded.PeerGroup(d, g, world) for g, d in enumerate(self.devs)]
        handles = [g.handle for g in self.groups]
        for g in self.groups:
            g.connect(handles)

    def prove(self, jobs):
        """jobs: [(nv, tabs, exts, terms)], proved one after the other on the same groups. Returns [rank][job] = (proof, finals, next challenge)."""
        dpa, world = self.dpa, self.world
        rows = []
        for nv, tabs, exts, terms in jobs:
            chunk = (1 << nv) // world
            rows.append([[(dpa.Mle.from_ext(d, t[2 * g * chunk:2 * (g + 1) * chunk]) if e else dpa.Mle.from_base(d, t[g * chunk:(g + 1) * chunk])) for t, e in zip(tabs, exts)]
                         for g, d in enumerate(self.devs)])
        out, errs = [[None] * len(jobs) for _ in range(world)], [None] * world

        def rank(g):
            try:
                for j, (nv, _, _, terms) in enumerate(jobs):
                    t = dpa.Transcript(b"test")
                    proof, finals = dpa.sharded.prove_sharded_peer(self.devs[g], self.groups[g], nv, rows[j][g], terms, t)
                    out[g][j] = (proof, finals, t.read_challenge())
            except Exception as e:  # noqa: BLE001 (reported by the test's thread)
                errs[g] = e

        th = [threading.Thread(target=rank, args=(g,), daemon=True) for g in range(world)]
        deadline = time.monotonic() + JOIN_S
        for t in th:
            t.start()
        for t in th:
            t.join(max(0.0, deadline - time.monotonic()))
        assert not any(t.is_alive() for t in th), "a rank did not come back"
        for job in rows:  # (everyone is back: nobody posts any more)
            for row in job:
                for m in row:
                    m.free()
        assert errs == [None] * world, errs
        return out

    def close(self):
        for g in self.groups:
            g.close()
        for d in self.devs:
            d.close()


@pytest.fixture
def ranks():
    import deep_prove_amd as dpa
    made = []

    def make(world):
        made.append(Ranks(dpa, world))
        return made[-1]
    yield make
    for r in made:
        r.close()


def _check(oracle, world, jobs, out):
    for j, (nv, tabs, exts, terms) in enumerate(jobs):
        oproof, ofinals, onext = _oracle(oracle, nv, tabs, exts, terms)
        for g in range(world):
            proof, finals, nxt = out[g][j]
            assert proof.size == oproof.size and (proof == oproof).all(), f"rank {g}, proof {j}: the proof differs from the oracle's"
            assert (finals == ofinals).all() and nxt == onext, f"rank {g}, proof {j}"


@pytest.mark.parametrize("world,nv", [(w, n) for w, k in ((1, 0), (2, 1), (4, 2)) for n in (k + 1, k + 2, k + 3, 12)])
def test_ranks_as_threads_of_one_process(oracle, ranks, world, nv):
    """nv = k + 1: one local round, one parity; k + 2: both parities; k + 3: the first overwrite of a slot; 12: many. Every local round is one
    k_peer_exchange_publish launch (mode SUM); with more than one rank two more (mode GATHER) carry the ranks' agreement word and stage 2's final values.
    k_shares_sum_publish, the kernel behind the other two exchanges, does not run."""
    k = world.bit_length() - 1
    r = ranks(world)
    for d in r.devs:
        d.profile(True)
    jobs = [(nv,) + _mixed_case(nv, world)]
    out = r.prove(jobs)
    reports = [{e["kernel"]: e["launches"] for e in d.profile_report()} for d in r.devs]
    for d in r.devs:
        d.profile(False)
    _check(oracle, world, jobs, out)
    for rep in reports:
        assert rep.get("k_peer_exchange_publish") == (nv - k) + (2 if world > 1 else 0), rep
        assert "k_shares_sum_publish" not in rep, rep


def test_long_messages_take_the_strided_path(oracle, ranks):
    """130 terms of degree 1 over two tables: 260 extension values per round, 520 words — more than the 256 threads of the workgroup, so the whole workgroup
    reads every sender's slot in strides (and the round runs as three launches of at most MAX_TERMS = 48 terms whose shares travel in ONE exchange)"""
    world, nv = 2, 6
    rng = np.random.default_rng(77)
    tabs = [rng.integers(0, P, size=1 << nv, dtype=np.uint64) for _ in range(2)]
    co = rng.integers(1, P, size=(130, 2), dtype=np.uint64)
    terms = [((int(co[j, 0]), int(co[j, 1])), [j % 2]) for j in range(130)]
    jobs = [(nv, tabs, [False, False], terms)]
    r = ranks(world)
    for d in r.devs:
        d.profile(True)
    out = r.prove(jobs)
    reports = [{e["kernel"]: e["launches"] for e in d.profile_report()} for d in r.devs]
    _check(oracle, world, jobs, out)
    for rep in reports:
        assert rep.get("k_peer_exchange_publish") == (nv - 1) + 2, rep  # one exchange per local round, whatever the number of terms


def test_two_proofs_back_to_back_on_the_same_groups(oracle, ranks):
    """nv = 5 then nv = 6 with two ranks, then nv = 5 again: 6, 7 and 6 exchanges (the local rounds, the agreement word, stage 2's final values). The group's
    counter carries over, the slots still hold the previous proof's messages, and the third proof begins on the other parity than the first"""
    world = 2
    jobs = [(nv,) + _mixed_case(nv, world) for nv in (5, 6)]
    r = ranks(world)
    _check(oracle, world, jobs, r.prove(jobs))
    _check(oracle, world, jobs[:1], r.prove(jobs[:1]))  # after 6 + 7 = 13 exchanges


def _run_children(tmp_path, world, nv):
    d = str(tmp_path)
    procs = [subprocess.Popen([sys.executable, CHILD, d, str(g), str(world), str(nv)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for g in range(world)]
    deadline = time.monotonic() + 180.0
    try:
        pending = list(range(world))
        while pending:
            for g in list(pending):
                rc = procs[g].poll()
                if rc is not None:
                    pending.remove(g)
                    assert rc == 0, f"rank {g} failed ({rc}):\n{procs[g].stdout.read()[-3000:]}"
            assert time.monotonic() < deadline, "the ranks ran over 180 s"
            if pending:
                try:
                    procs[pending[0]].wait(timeout=0.05)
                except subprocess.TimeoutExpired:
                    pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
            p.stdout.close()
    res = []
    for g in range(world):
        nxt = json.load(open(os.path.join(d, f"next_{g}.json")))
        res.append((np.load(os.path.join(d, f"proof_{g}.npy")), np.load(os.path.join(d, f"finals_{g}.npy")), tuple(nxt["next_challenge"])))
    for g in range(1, world):
        assert res[g][0].size == res[0][0].size and (res[g][0] == res[0][0]).all() and (res[g][1] == res[0][1]).all() and res[g][2] == res[0][2], f"rank {g} and rank 0 differ"
    return res


@pytest.mark.parametrize("world,nv", [(2, 10), (4, 12)])
def test_ranks_as_processes(oracle, tmp_path, world, nv):
    """every rank a fresh process with its own HIP runtime: the mailboxes are mapped with hipIpcOpenMemHandle, the handles travel through files"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
    import peer_child
    tabs = [peer_child.full_table(nv, j) for j in range(peer_child.NTABLES)]
    oproof, ofinals, onext = _oracle(oracle, nv, tabs, [False] * 3, [((1, 0), [0, 1, 2])])
    for proof, finals, nxt in _run_children(tmp_path, world, nv):
        assert proof.size == oproof.size and (proof == oproof).all() and (finals == ofinals).all() and nxt == tuple(onext)


def test_ranks_as_processes_at_2pow22_equal_the_golden(tmp_path):
    """two processes, 2^21 entries of every table each, against tests/golden/sumcheck24.json (the checks of test_gpu_sharded._check_against_golden)"""
    import deep_prove_amd as dpa
    nv = 22
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "sumcheck24.json")))
    gold = g["cases"][str(nv)]
    assert g["k"] == 3
    for proof, finals, nxt in _run_children(tmp_path, 2, nv):
        assert proof.size == gold["proof_words"]
        assert hashlib.sha256(proof.tobytes()).hexdigest() == gold["sha256"], "2^22 sumcheck between two processes: proof stream differs from the oracle's"
        assert [int(v) for v in finals] == gold["finals"]
        assert list(nxt) == gold["next_challenge"]
    # the host verifier accepts it: claimed sum = p_0(0) + p_0(1) of the first round message, sub-claim = product of the finals
    off = 1 + 2 * nv + 1 + 1
    e0, e1 = (int(proof[off]), int(proof[off + 1])), (int(proof[off + 2]), int(proof[off + 3]))
    claimed = ((e0[0] + e1[0]) % P, (e0[1] + e1[1]) % P)
    _, expected = dpa.verify_sumcheck(claimed, proof, nv, 3, dpa.Transcript(b"test"))
    prod = (1, 0)
    for i in range(3):
        b = (int(finals[2 * i]), int(finals[2 * i + 1]))
        prod = ((prod[0] * b[0] + 7 * prod[1] * b[1]) % P, (prod[0] * b[1] + prod[1] * b[0]) % P)
    assert prod == tuple(expected), "final evaluations do not multiply to the verifier's sub-claim"


def test_connect_refuses_bad_handles_and_the_context_stays_usable(dev, oracle):
    import deep_prove_amd as dpa
    from deep_prove_amd._lib import DeepProveError
    a, b = dpa.sharded.PeerGroup(dev, 0, 2), dpa.sharded.PeerGroup(dev, 1, 2)
    four = dpa.sharded.PeerGroup(dev, 1, 4)
    try:
        corrupt = bytes([a.handle[0] ^ 0x40]) + a.handle[1:]
        for what, handles in (("rank order", [b.handle, a.handle]), ("another world size", [a.handle, four.handle]), ("not a mailbox handle", [corrupt, b.handle])):
            with pytest.raises(DeepProveError) as e:
                a.connect(handles)
            assert e.value.code == -1 and what in str(e.value), (what, str(e.value))  # DP_ERR_ARG
        a.connect([a.handle, b.handle])  # nothing of the refused calls stuck: the right handles still connect
    finally:
        for g in (a, b, four):
            g.close()
    nv = 8
    rng = np.random.default_rng(5)
    tabs = [rng.integers(0, P, size=1 << nv, dtype=np.uint64) for _ in range(2)]
    ms = [dpa.Mle.from_base(dev, t) for t in tabs]
    try:
        vp = dpa.VirtualPolynomial(nv)
        vp.add_mle_list(ms, (3, 1))
        proof, finals = dpa.prove_parallel(dev, vp, dpa.Transcript(b"test"))
    finally:
        for m in ms:
            m.free()
    oproof, ofinals, _ = _oracle(oracle, nv, tabs, [False, False], [((3, 1), [0, 1])])
    assert (proof == oproof).all() and (finals == ofinals).all()
