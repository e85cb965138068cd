"""The rounds of the batch opening publish from the LAST workgroup of their streaming kernel (kernels.inc k_classic_fused_pub, k_bf_fold_msg, k_bf_msg with a
ticket; hip_dev.hip classic_round / bf_round / round_ticket_now), members of a cohort included; DP_CLASSIC_TICKET=0 keeps the separate reduction launches
(k_classic_fused + k_classic_reduce, k_fold + k_bf_msg + k_reduce_publish). Both forms must give the same proof bytes — the oracle's, and the latency-mode proof's
in throughput mode — and the form that ran must be the one asked for. The switch is read once, so every variant runs in a child process of its own
(this file run as a script); one child per variant serves all the cases below."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXSIZE = 1 << 18
# (nv, extension field) of the opened polynomials. A batch opening takes no polynomial of fewer than 8 variables (7 and fewer are trivial commitments, opened on
# their own), so the pairs of 2^5, 2 and 1 entries are reached by FOLDING: every pair is folded in every round, and in latency mode (and with profiling) all rounds
# are streamed ones — an nv = 8 pair is 2^5 entries long after round 3, goes from two entries to one in round 8 (the h == 1 fold) and stays at one entry after
# that, while the nv = 18 pair next to it in the same launch still has 2^10. nv = 15: the first factored size (classic_eq_split); nv = 18: 128 workgroups in round 0 and 64 in round 1 (the last
# workgroup's lanes stride twice over them) beside one-workgroup pairs; 19 pairs: the last workgroup's four waves stride five times over the pairs.
PCS_CASES = {
    "mixed": [(18, False), (15, False), (9, False), (8, False), (12, True)],
    "many_pairs": [(15, False), (8, False)] + [(8 + i % 4, i % 2 == 1) for i in range(17)],
    "small_only": [(9, False), (8, True)],
}
MODES = ("latency", "throughput", "profiled")
NEW = ("k_classic_fused_pub", "k_bf_fold_msg")


def _child_pcs():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deep_prove_amd as dpa
    with_oracle = os.environ.get("TICKET_TEST_ORACLE") == "1"
    if with_oracle:
        from support import oracle_lib
        oracle = oracle_lib.load()
    dev = dpa.Device(0)
    pcs = dpa.Basefold(dev, MAXSIZE)
    out, kernels = {"cases": {}}, set()
    for name, shape in PCS_CASES.items():
        rng = np.random.default_rng(9100 + len(shape))
        raws = [rng.integers(0, P, size=(2 if e else 1) << nv, dtype=np.uint64) for nv, e in shape]
        mles = [dpa.Mle.from_ext(dev, w) if e else dpa.Mle.from_base(dev, w) for w, (nv, e) in zip(raws, shape)]
        comms = [pcs.commit(m) for m in mles]
        points = [[(int(a), int(b)) for a, b in rng.integers(0, P, size=(nv, 2), dtype=np.uint64)] for nv, _ in shape]
        evals = [m.evaluate(p) for m, p in zip(mles, points)]
        rec = {}
        # latency mode; the context in throughput mode (device-side Fiat-Shamir); latency mode with launch profiling, which names the kernels that ran and
        # keeps the one-workgroup tails out: every round down to two entries is then a streamed one
        for mode in MODES:
            dev.set_throughput_mode(mode == "throughput")
            dev.profile(mode == "profiled")
            t = dpa.Transcript(b"test")
            proof = pcs.batch_open(comms, points, evals, t)
            dpa.Basefold.batch_verify(MAXSIZE, [c.root for c in comms], [nv for nv, _ in shape], [not e for _, e in shape], points, evals, proof, dpa.Transcript(b"test"))
            rec[mode] = {"sha256": hashlib.sha256(proof.tobytes()).hexdigest(), "words": int(proof.size), "challenge": [int(v) for v in t.read_challenge()]}
        kernels |= {r["kernel"] for r in dev.profile_report()}
        dev.profile(False)
        if with_oracle:
            ot = oracle.transcript(b"test")
            exp = oracle.pcs_batch_open(MAXSIZE, raws, [e for _, e in shape], points, evals, ot)
            rec["oracle"] = {"sha256": hashlib.sha256(exp.tobytes()).hexdigest(), "words": int(exp.size), "challenge": [int(v) for v in ot.read_challenge()]}
        out["cases"][name] = rec
        for m in mles:
            m.free()
    out["kernels"] = sorted(kernels)
    dev.close()
    print("RESULT " + json.dumps(out), flush=True)


def _child_batch():
    sys.path.insert(0, ROOT)
    import deep_prove_amd as dpa
    dev = dpa.Device(0)
    mb = dpa.models.mlp(3, 256, config=5)
    ctx = dpa.Context.generate(dev, mb.blob())
    pr = dpa.Prover(ctx)
    conc = 11  # DP_COHORT=8: one full cohort and one of three
    xs = np.stack([mb.input(8800 + i) for i in range(conc)])
    seq = [pr.prove(x) for x in xs]
    h = hashlib.sha256()
    for rep in range(3):  # back to back: every member's ticket has to be back at zero when its next proof starts
        proofs, outs, _ = pr.prove_batch(xs, conc)
        assert pr.in_flight() == conc
        for i in range(conc):
            assert (outs[i] == seq[i][1]).all(), f"batch {rep}: output {i}"
            assert proofs[i].size == seq[i][0].size and (proofs[i] == seq[i][0]).all(), f"batch {rep}: proof {i} differs from its latency-mode proof"
            dpa.verify(ctx.verifier_blob(), proofs[i], xs[i], outs[i])
            h.update(proofs[i].tobytes())
    ctx.free()
    dev.close()
    print("RESULT " + json.dumps({"sha256": h.hexdigest(), "proofs": 3 * conc}), flush=True)


def _run(what, ticket, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, DP_CLASSIC_TICKET=ticket, **env))
    assert r.returncode == 0, f"{what} DP_CLASSIC_TICKET={ticket}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0][len("RESULT "):]), r.stderr


@pytest.fixture(scope="module")
def pcs_runs():
    return {"1": _run("pcs", "1", TICKET_TEST_ORACLE="1")[0], "0": _run("pcs", "0")[0]}


@pytest.fixture(scope="module")
def batch_runs():
    return {k: _run("batch", k, DP_COHORT="8", DP_TIMING="2") for k in ("1", "0")}


@pytest.mark.parametrize("case", sorted(PCS_CASES))
def test_batch_opening_same_bytes_with_and_without_the_ticket(pcs_runs, case):
    """dp_pcs_batch_open, latency and throughput mode of the context: the oracle's stream and transcript state with the ticket, the same without"""
    new, old = pcs_runs["1"]["cases"][case], pcs_runs["0"]["cases"][case]
    for mode in MODES:
        assert new[mode] == new["oracle"], f"{case}, {mode}: the proof differs from the oracle's"
        assert old[mode] == new[mode], f"{case}, {mode}: DP_CLASSIC_TICKET=0 gives other bytes"


def test_batch_opening_runs_the_form_asked_for(pcs_runs):
    new, old = pcs_runs["1"]["kernels"], pcs_runs["0"]["kernels"]
    assert all(k in new for k in NEW) and "k_classic_reduce" not in new, new
    assert all(k in old for k in ("k_classic_fused", "k_classic_reduce", "k_fold", "k_reduce_publish")) and not any(k in old for k in NEW), old


def test_cohort_members_publish_from_their_own_last_workgroup(batch_runs):
    """Prover.prove_batch, 11 in flight in cohorts of 8 + 3, three batches back to back in one process: every proof equals its latency-mode proof and
    verifies (asserted in the child), the same bytes come out with the fallback, and the merged launches are the ones asked for"""
    (new, new_err), (old, old_err) = batch_runs["1"], batch_runs["0"]
    assert new["proofs"] == old["proofs"] == 33 and new["sha256"] == old["sha256"]
    launched = lambda err: {ln.split()[-1] for ln in err.splitlines() if ln.startswith("[dp launches]")}
    assert all(k in launched(new_err) for k in NEW) and "k_classic_reduce" not in launched(new_err), sorted(launched(new_err))
    assert "k_classic_reduce" in launched(old_err) and not any(k in launched(old_err) for k in NEW), sorted(launched(old_err))


if __name__ == "__main__":
    {"pcs": _child_pcs, "batch": _child_batch}[sys.argv[1]]()
