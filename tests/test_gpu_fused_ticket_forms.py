"""The streamed rounds of one large product (kernels.inc k_sc_fused) end in the last-workgroup epilogue (sc_block_sums_finish: the block sums written through, a
ticket, the last workgroup adds them up and publishes); DP_FUSED_TICKET=0 keeps the separate k_reduce_publish launch per round (hip_dev.hip sc_round /
round_ticket_now / round_sums). Both forms must give the oracle's proof, and the form that ran must be the one asked for. The switch is read once, so each value
runs in a child process of its own (this file run as a script); one child per value serves all the cases below.

Shapes: nv = 19 is the smallest polynomial whose first round is streamed (2^19 entries are above the multi-workgroup range: k_sc_terms, then k_sc_fused from round 1
on, whose 512-workgroup grid makes the last workgroup's lanes stride eight times over the block sums); nv = 20 with coefficient one are the claimed-sum forms, the
base-table one through the two-round grid (k_sc_terms2 / k_sc_fused2, which DP_FUSED_TICKET leaves alone) with k_sc_fused on extension tables after it.
Every case runs in latency mode and once more with per-kernel profiling, which supplies the launch counts. Profiling does not change what sc_round launches
(only the batch opening's and the layers' one-launch tails look at it), so the counts are those of the latency-mode proof as well — and the one-workgroup
persistent kernel (k_sc_persist_lds in every profile report of these cases) still takes over once the tables fit in LDS, in both modes: k_sc_fused does NOT run
down to a one-workgroup grid here, and the edge "the first ticket is also the last" is not covered by this file."""
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
# (nv, [is_ext per table], (coefficient, [table idx])): K = 1, 2, 3 on base and on extension tables, the claim known (coefficient one: SKIP1) or not; the base
# cases continue on extension tables from their second streamed round on
CASES = {
    "k3_base_claim": (19, [False, False, False], ((1, 0), [0, 1, 2])),
    "k3_base": (19, [False, False, False], ((1, 1), [2, 0, 1])),
    "k2_base_claim": (19, [False, False], ((1, 0), [1, 0])),
    "k2_ext": (19, [True, True], ((3, 5), [0, 1])),
    "k1_base": (19, [False], ((6, 2), [0])),
    "k1_ext_claim": (19, [True], ((1, 0), [0])),
    "k2_base_claim_grid2": (20, [False, False], ((1, 0), [1, 0])),
    "k3_ext_claim": (20, [True, True, True], ((1, 0), [0, 1, 2])),
}
MODES = ("latency", "profiled")
REPEATED = "k3_base_claim"


def _child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deep_prove_amd as dpa
    with_oracle = os.environ.get("TICKET_TEST_ORACLE") == "1"
    if with_oracle:
        from support import oracle_lib
        oracle = oracle_lib.load()
    dev = dpa.Device(0)

    def record(proof, finals, t):
        return {"sha256": hashlib.sha256(proof.tobytes()).hexdigest(), "words": int(proof.size), "finals": [int(v) for v in np.asarray(finals).ravel()],
                "challenge": [int(v) for v in t.read_challenge()]}

    out = {}
    for seed, (name, (nv, exts, term)) in enumerate(CASES.items()):
        rng = np.random.default_rng(7300 + seed)
        raw = [rng.integers(0, P, size=(2 if e else 1) << nv, dtype=np.uint64) for e in exts]
        mles = [dpa.Mle.from_ext(dev, w) if e else dpa.Mle.from_base(dev, w) for w, e in zip(raw, exts)]
        vp = dpa.VirtualPolynomial(nv)
        vp.tables = list(mles)
        vp.terms = [term]
        rec = {}
        for mode in MODES + (("again",) * 3 if name == REPEATED else ()):  # back to back in one process: the ticket has to be back at zero every time
            dev.profile(mode == "profiled")
            t = dpa.Transcript(b"test")
            proof, finals = dpa.prove_parallel(dev, vp, t)
            rec.setdefault(mode, []).append(record(proof, finals, t))
            if mode == "profiled":
                rec["launches"] = {r["kernel"]: r["launches"] for r in dev.profile_report()}
                dev.profile(False)
        if with_oracle:
            ot = oracle.transcript(b"test")
            oproof, ofinals = oracle.sumcheck_prove(nv, raw, exts, [term], ot)
            rec["oracle"] = record(oproof, ofinals, ot)
        out[name] = rec
        for m in mles:
            m.free()
    dev.close()
    print("RESULT " + json.dumps(out), flush=True)


def _run(ticket, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, DP_FUSED_TICKET=ticket, **env))
    assert r.returncode == 0, f"DP_FUSED_TICKET={ticket}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0][len("RESULT "):])


@pytest.fixture(scope="module")
def runs():
    return {"1": _run("1", TICKET_TEST_ORACLE="1"), "0": _run("0")}


def _count(launches, kernel):
    """launches of every instantiation of `kernel` (k_sc_fused<3, true, false> .. — not k_sc_fused2<..>)"""
    return sum(n for k, n in launches.items() if k == kernel or k.startswith(kernel + "<"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_streamed_rounds_same_bytes_with_and_without_the_ticket(runs, case):
    """proof words, final evaluations and the closing challenge: the oracle's with the ticket, in latency mode and profiled, and the same without it"""
    new, old = runs["1"][case], runs["0"][case]
    for mode in MODES:
        assert len(new[mode]) == len(old[mode]) == 1
        assert new[mode][0] == new["oracle"], f"{case}, {mode}: the proof differs from the oracle's"
        assert old[mode][0] == new[mode][0], f"{case}, {mode}: DP_FUSED_TICKET=0 gives other bytes"


@pytest.mark.parametrize("case", sorted(CASES))
def test_streamed_rounds_run_the_form_asked_for(runs, case):
    """without the ticket every k_sc_fused launch is followed by a k_reduce_publish launch of its own, with it by none (the launch counts of the profiled proof; the
    latency-mode proof launches the same kernels, see above)"""
    new, old = runs["1"][case]["launches"], runs["0"][case]["launches"]
    print(case, "ticket:", new, "fallback:", old)
    fused = _count(old, "k_sc_fused")
    assert fused >= 2 and _count(new, "k_sc_fused") == fused, (new, old)
    assert _count(old, "k_reduce_publish") - _count(new, "k_reduce_publish") == fused, (new, old)
    grid2 = case.endswith("grid2")
    assert (_count(new, "k_sc_terms2") == _count(old, "k_sc_terms2") == 1 and _count(new, "k_sc_fused2") == _count(old, "k_sc_fused2") == 1) if grid2 \
        else not any(k.startswith(("k_sc_terms2", "k_sc_fused2")) for k in list(new) + list(old)), (new, old)


def test_ticket_is_back_at_zero_for_the_next_proof(runs):
    """one nv = 19 case three more times back to back in the ticket child, other proofs before and after: a ticket left above zero would let an earlier workgroup
    publish a partial sum, or nobody publish, and the proof would differ or the host's wait run out"""
    rec = runs["1"][REPEATED]
    assert len(rec["again"]) == 3 and all(r == rec["oracle"] for r in rec["again"] + rec["latency"] + rec["profiled"])


if __name__ == "__main__":
    _child()
