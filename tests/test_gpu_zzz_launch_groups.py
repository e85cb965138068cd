"""Launch groups (csrc/cohort.h, dp_model_prove_batch): cohorts that share a hardware queue merge their launches — launch number i of ALL their members is one
kernel, assembled by the cohorts' host threads. Ragged groups, one group for everything, the identity grouping, members leaving at different times (a batch
longer than the number in flight), a convolution graph: every proof must equal the proof `Prover.prove` gives for the same input, and verify.
(File name sorts last: these run after the cohort suite.)"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check(pr, vb, xs, seq, conc):
    import deep_prove_amd as dpa
    proofs, outs, _ = pr.prove_batch(xs, conc)
    assert len(proofs) == len(xs)
    for i in range(len(xs)):
        assert (outs[i] == seq[i][1]).all()
        assert proofs[i].size == seq[i][0].size and (proofs[i] == seq[i][0]).all(), f"proof {i} differs from the sequential proof"
    for i in (0, len(xs) - 1):
        dpa.verify(vb, proofs[i], xs[i], outs[i])


@pytest.fixture(scope="module")
def mlp_case(dev):
    """the model, 27 inputs and their sequential proofs: made once, shared by the cases, left unchanged"""
    import deep_prove_amd as dpa
    mb = dpa.models.mlp(2, 64, config=43)
    ctx = dpa.Context.generate(dev, mb.blob())
    pr = dpa.Prover(ctx)
    xs = np.stack([mb.input(5000 + i) for i in range(27)])
    seq = [pr.prove(x) for x in xs]
    yield pr, ctx.verifier_blob(), xs, seq
    ctx.free()


_LINE = re.compile(r"\[dp timing\] (\d+) cohorts of <= (\d+) proofs in (\d+) launch groups: (\d+) merged launches for (\d+) proof launches")


def _timing_lines(capfd):
    return [tuple(int(v) for v in m.groups()) for m in _LINE.finditer(capfd.readouterr().err)]


@pytest.mark.parametrize("groups", ["2", "1", "7"])
def test_launch_groups_match_sequential_mlp(mlp_case, groups, monkeypatch, capfd):
    """27 proofs, 19 in flight, cohorts of 3: 7 cohorts (6 x 3 + 1) in 2 groups (4 and 3 cohorts: 12 and 7 members), in 1 group (every cohort in one launch)
    and in 7 (the identity: every cohort launches on its own, as with enough hardware queues). 27 over 19 makes members leave at different times.
    Then 19 proofs, all in flight — every member proves exactly one, so the launch counts are exact: a proof issues L launches, a group fires L merged launches,
    G groups fire G x L; with 7 groups that is the 7 x L of seven cohorts launching on their own."""
    pr, vb, xs, seq = mlp_case
    monkeypatch.setenv("DP_COHORT", "3")
    monkeypatch.setenv("DP_LAUNCH_GROUPS", groups)
    monkeypatch.setenv("DP_TIMING", "1")
    capfd.readouterr()
    _check(pr, vb, xs, seq, 19)
    assert pr.in_flight() == 19
    lines = _timing_lines(capfd)
    assert len(lines) == 1 and lines[0][:3] == (7, 3, int(groups)), lines
    _check(pr, vb, xs[:19], seq[:19], 19)
    (nco, csize, ngroups, fired, packs), = _timing_lines(capfd)
    print(f"groups={groups}: {fired} merged launches for {packs} proof launches")
    assert packs % 19 == 0
    per_proof = packs // 19
    assert (nco, ngroups) == (7, int(groups)) and fired == int(groups) * per_proof


def test_identity_grouping_launches_what_ungrouped_cohorts_launch(mlp_case, monkeypatch, capfd):
    """DP_LAUNCH_GROUPS unset: the group count follows the hardware queues of the process — one group per cohort when there are enough, in which case the
    merged-launch count must be the one DP_LAUNCH_GROUPS=7 gives (cohorts x launches of a proof); with fewer queues, that many groups' worth"""
    import os
    pr, vb, xs, seq = mlp_case
    monkeypatch.setenv("DP_COHORT", "3")
    monkeypatch.delenv("DP_LAUNCH_GROUPS", raising=False)
    monkeypatch.setenv("DP_TIMING", "1")
    capfd.readouterr()
    _check(pr, vb, xs[:19], seq[:19], 19)
    (nco, csize, ngroups, fired, packs), = _timing_lines(capfd)
    nq = int(os.environ.get("GPU_MAX_HW_QUEUES", "24"))  # (not preset: the library asked for 24 when it was loaded)
    print(f"{nq} hardware queues: {ngroups} groups, {fired} merged launches for {packs} proof launches")
    assert nco == 7 and ngroups == min(nq, 7) and fired == ngroups * (packs // 19)


def test_launch_groups_match_sequential_cnn(dev, monkeypatch):
    """conv / maxpool graph, 11 proofs in cohorts of 2 (5 x 2 + 1) in two groups of 3 cohorts"""
    import deep_prove_amd as dpa
    monkeypatch.setenv("DP_COHORT", "2")
    monkeypatch.setenv("DP_LAUNCH_GROUPS", "2")
    mb = dpa.models.cnn_tiny()
    ctx = dpa.Context.generate(dev, mb.blob())
    pr = dpa.Prover(ctx)
    xs = np.stack([mb.input(6000 + i) for i in range(11)])
    seq = [pr.prove(x) for x in xs]
    _check(pr, ctx.verifier_blob(), xs, seq, 11)
    ctx.free()
