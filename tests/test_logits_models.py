"""Logits::Argmax (layer kind 18) as a model: the numpy inference of deep_prove_amd.models against dp_model_infer_host, what the model setup
refuses, mutated kind-18 blobs (through the entry point tests/support/fuzz_blob.py drives: dpa.infer_host), and the wire format of a Logits proof."""
import os
import subprocess
import sys

import numpy as np
import pytest

from support import logits_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_inference_is_the_hosts_over_random_rows_with_ties():
    import deep_prove_amd as dpa
    rng = np.random.default_rng(18)
    for rows, k in ((2, 2), (4, 8), (8, 64), (2, 256)):
        mb = dpa.models.logits_only(rows, k, config=45)
        for it in range(12):
            x = rng.integers(-4, 5, size=(rows, k)) if it % 2 else rng.integers(-127, 128, size=(rows, k))  # (a narrow range: many ties)
            if it % 3 == 0:
                x[rng.integers(rows)] = int(rng.integers(-128, 128))  # a row of equal values
            got = dpa.infer_host(mb.blob(), x.reshape(-1))
            assert (got == mb.run(x.reshape(-1))).all() and (got == x.argmax(axis=1)).all()
    # the plain inference answers whatever a row spreads over (only proving refuses a spread beyond the range table)
    x = np.array([[-(1 << 40), 1 << 40], [7, 7]], dtype=np.int64)
    assert list(dpa.infer_host(dpa.models.logits_only(2, 2, config=45).blob(), x.reshape(-1))) == [1, 0]
    for mb in (dpa.models.lm_head(4, 8, 16, config=46), dpa.models.token_lm(8, 16, 16, config=47), dpa.models.token_lm(8, 16, 16, config=48, gelu=False, max_positions=16)):
        for i in range(4):
            x = mb.input(1000 + i)
            y = dpa.infer_host(mb.blob(), x)
            assert y.shape == (mb.shape_pad[0],) and (y == mb.run(x)).all() and y.min() >= 0 and y.max() < mb.layers[-1]["K"]


def test_graph_form_and_what_the_setup_refuses():
    """valid in chain and graph form; refused (DP_ERR_ARG = -1, naming node and kind) unless the node's output is the model's ONLY output tensor,
    read by nothing, and its input has rows * K entries"""
    import deep_prove_amd as dpa
    M = dpa.models
    x = LC.logits_only_input(4, 8)
    g = M.GraphBuilder([32], config=49)
    g.logits((-1, 0), 4, 8)
    assert (dpa.infer_host(g.blob(), x) == x.reshape(4, 8).argmax(axis=1)).all() and (g.run(x) == x.reshape(4, 8).argmax(axis=1)).all()

    def refused(blob, inp, word):
        with pytest.raises(dpa.DeepProveError) as e:
            dpa.infer_host(blob, inp)
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    g = M.GraphBuilder([32], config=49)  # a node reads the tokens
    lg = g.logits((-1, 0), 4, 8)
    g.relu((lg, 0))
    refused(g.blob(), x, "node 0 (kind 18, logits)")
    g = M.GraphBuilder([32, 32], config=49)  # a second output tensor
    lg = g.logits((-1, 0), 4, 8)
    rl = g.relu((-1, 1))
    g.set_outputs([(lg, 0), (rl, 0)])
    refused(g.blob(), np.concatenate([x, x]), "node 0 (kind 18, logits)")
    g = M.GraphBuilder([32], config=49)  # rows * K is not the input's length
    g.logits((-1, 0), 4, 4)
    refused(g.blob(), x, "node 0 (kind 18, logits)")
    for r_, k_ in ((3, 8), (4, 6), (1, 32), (32, 1), (0, 8), (-4, 8), (4, 1 << 40)):  # not powers of two >= 2 within bounds
        refused(np.array([32, 1, 18, r_, k_], dtype=np.int64), x, "logits")
    refused(np.array([32, 1, 18, 4], dtype=np.int64), x, "truncated")


def test_mutated_logits_blobs_never_crash():
    """the mutations of tests/support/fuzz_blob.py on kind-18 blobs through the call it drives (dpa.infer_host; that script has its own fixed list of
    models and no function to hand it others), in a child process (a crash would be its exit status): every outcome is a DeepProveError (DP_ERR_ARG or
    DP_ERR_SHAPE) or an answer, and the answer to a mutated one-node blob is compared with numpy"""
    code = r"""
import sys, os
sys.path.insert(0, sys.argv[1])
import numpy as np
import deep_prove_amd as dpa
rng = np.random.default_rng(7)
bases = [dpa.models.logits_only(4, 8, config=50), dpa.models.lm_head(4, 8, 16, config=51), dpa.models.token_lm(4, 8, 8, config=52, gelu=False)]
g = dpa.models.GraphBuilder([32], config=53); g.logits((-1, 0), 4, 8); bases.append(g)
ok = err = same = 0
for it in range(1600):
    mb = bases[it % len(bases)]
    b = mb.blob().copy(); x = mb.input()
    for _ in range(int(rng.integers(1, 4))):
        tail = rng.random() < 0.5  # the Logits parameters are the last words of these blobs
        pos = int(rng.integers(max(0, b.size - 6), b.size)) if tail else int(rng.integers(0, max(1, min(b.size, 64))))
        mode = rng.integers(0, 5)
        if mode == 0: b[pos] = int(rng.integers(-5, 70))
        elif mode == 1: b[pos] = int(rng.integers(-2**62, 2**62))
        elif mode == 2: b[pos] ^= 1 << int(rng.integers(0, 63))
        elif mode == 3: b = b[:int(rng.integers(1, max(2, b.size)))]
        else: b[pos] = [0, -1, 2**31, 2**32, 2**40, 2**63 - 1][int(rng.integers(0, 6))]
        if b.size == 0: break
    try:
        y = dpa.infer_host(b, x); ok += 1
        if b.size == 5 and b[2] == 18:  # a mutated logits_only blob the library accepts is still [input_len, 1, 18, rows, K]: its answer is numpy's
            assert b[3] * b[4] == x.size and (y == x.reshape(int(b[3]), int(b[4])).argmax(axis=1)).all(), (b, y); same += 1
    except dpa.DeepProveError as e:
        assert e.code in (-1, -4), (e.code, str(e)); err += 1
print("fuzz done: accepted", ok, "compared", same, "rejected", err)
"""
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout + r.stderr[-2000:]
    rejected, compared = int(r.stdout.split("rejected")[1]), int(r.stdout.split("compared")[1].split()[0])
    assert rejected > 400 and compared >= 1, r.stdout


def test_wire_format_round_trip_of_a_logits_proof(tmp_path):
    """LayerProof::Logits with the reference's field names in declaration order (logits.rs:62-76), both ways"""
    import deep_prove_amd as dpa
    mb, x = LC.cases()["logits_only_4x8"]
    sp = str(tmp_path / "stream")
    r = LC.run_check(LC.check_bin(), "run", *LC.write_case(tmp_path, "w", mb.blob(), x), sp, str(tmp_path / "out"))
    assert r.returncode == 0, r.stdout + r.stderr
    words = np.fromfile(sp, dtype="<u8")
    tree = dpa.wire.parse_stream(words)
    (node, kind, lp), = tree["steps"]
    assert (node, kind) == (0, 18)
    assert list(lp) == ["logup_proof", "max_eval", "max_commitment", "sumcheck_proof", "max_mat_eval", "hadamard_proof", "input_eval"]
    model = dpa.wire.to_serde_model(tree)
    assert list(model["steps"][0]) == ["Logits"] and list(model["steps"][0]["Logits"]) == list(lp)
    back = dpa.wire.from_rmp(dpa.wire.to_rmp(words))
    assert dpa.wire.stream_equal_modulo_skipped(words, back)
    # what the wire format drops are the base-field trivial openings (`#[serde(skip)]`), nothing of the Logits step: the step's words come back as they went
    step = lambda w: dpa.wire.parse_stream(w)["steps"][0][2]
    kept = dpa.wire.strip_skipped(words)
    assert step(kept) == lp and step(back) == lp
