"""Decoding on the device (include/deep_prove_hip_decode.h; k_infer_next_token and hip_infer_decode of csrc/infer_kernels.inc): Context.decode
against dp_model_decode_host prompt by prompt — tokens, lengths, stops and outputs, exact equality — for both decodable families, batches on
either side of the wave of the one-thread-per-sample kernel, mixed prompt lengths and mixed stops; refused prompts; several chunks and the polling
of the stop words (child processes, tests/support/decode_child.py); Prover.decode_and_prove and verify_decode."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from support.decode_cases import EOS, FAMILIES, IDS, MAX_NEW, REFUSED, SEQ, VOCAB, WINDOW, gelu_lm, prompts  # noqa: E402

CHILD = os.path.join(ROOT, "tests", "support", "decode_child.py")
PLENS = (1, 2, 8, 2, 7, 2, 3, 2)  # prompt i has PLENS[i % 8] tokens: 1 and seq among them


def _child(mode, **env):
    r = subprocess.run([sys.executable, CHILD, mode], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and f"decode child done {mode}" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return r


def _decode_line(r):
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp decode]")]
    assert len(lines) == 1, r.stderr[-3000:]
    m = re.fullmatch(r"\[dp decode\] prompts (\d+) chunks (\d+) steps (\d+) launches (\d+) polls (\d+) final_ms [0-9.]+", lines[0])
    assert m, lines[0]
    return dict(zip(("prompts", "chunks", "steps", "launches", "polls"), (int(v) for v in m.groups())))


def _host(blob, xs, lens, max_new, eos, pad, cache):
    """decode_host for every prompt: (tokens, lengths, stops, reasons, outputs)"""
    import deep_prove_amd as dpa
    rows = []
    for x, n in zip(xs, lens):
        key = (bytes(x[:n]), max_new, eos, pad)
        if key not in cache:
            cache[key] = dpa.decode_host(blob, x[:n], int(n), max_new, eos=eos, pad=pad)
        rows.append(cache[key])
    return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]), np.stack([r[4] for r in rows]))


@pytest.mark.parametrize("name,make,all_kinds", FAMILIES, ids=IDS)
def test_device_decode_equals_the_host_decode(dev, name, make, all_kinds):
    """batches of 1, 63, 64 and 65; prompt lengths 1 .. seq in one batch; eos none, 9 (every prompt stops early) and 12 (mixed stops); pad 0 and 3"""
    import deep_prove_amd as dpa
    mb = make()
    blob = mb.blob()
    xs = prompts(mb, 65)
    lens = np.array([PLENS[i % 8] for i in range(65)], dtype=np.uint32)
    cache, stops = {}, set()
    ctx = dpa.Context.generate(dev, blob)
    try:
        before, _ = ctx.infer(xs[:3], all_kinds=all_kinds)
        for nb in (1, 63, 64, 65):
            for max_new, eos, pad in ((6, None, 0), (6, 9, 0), (6, 12, 3), (1, 12, 0), (0, None, 0)):
                want = _host(blob, xs[:nb], lens[:nb], max_new, eos, pad, cache)
                tokens, length, stop, reasons, outs, ms = ctx.decode(xs[:nb], lens[:nb], max_new, eos=eos, pad=pad, all_kinds=all_kinds)
                assert tokens.shape == outs.shape == (nb, SEQ) and tokens.dtype == outs.dtype == np.int64 and length.dtype == stop.dtype == reasons.dtype == np.uint32 and ms > 0
                where = (name, nb, max_new, eos, pad)
                assert (tokens == want[0]).all(), (where, np.argwhere(tokens != want[0])[:5])
                assert (length == want[1]).all() and (stop == want[2]).all() and not reasons.any() and not want[3].any(), where
                assert (outs == want[4]).all(), (where, np.argwhere(outs != want[4])[:5])
                if nb == 65 and eos == 12 and max_new == 6:
                    assert len(set(stop.tolist())) >= 2, stop  # (mixed stops in one batch)
                stops |= set(stop.tolist())
        assert stops == {EOS, WINDOW, MAX_NEW}
        # a list of prompts of different lengths, one length for all, and plain inference afterwards: the model stays as it was
        tokens, length, stop, _, outs, _ = ctx.decode([list(xs[0][:2]), list(xs[1][:3])], 2, 6, all_kinds=all_kinds)
        want = _host(blob, xs[:2], [2, 2], 6, None, 0, cache)
        assert (tokens == want[0]).all() and (length == want[1]).all() and (stop == want[2]).all() and (outs == want[4]).all()
        after, _ = ctx.infer(xs[:3], all_kinds=all_kinds)
        assert (after == before).all()
        if all_kinds:  # the kind rule of dp_model_infer_ex: refused without the flag, before any device work
            with pytest.raises(dpa.DeepProveError) as ei:
                ctx.decode(xs[:1], 2, 6)
            assert ei.value.code == -1 and re.search(r"node \d+ is a GELU layer", str(ei.value)), str(ei.value)
        for kw, message in ((dict(pad=VOCAB), "pad 16 lies outside the vocabulary"), (dict(prompt_lens=[2, 0]), "prompt_len 0 of prompt 1"), (dict(prompt_lens=[9, 2]), "prompt_len 9 of prompt 0")):
            args = dict(prompt_lens=2, max_new=6, all_kinds=all_kinds)
            args.update(kw)
            with pytest.raises(dpa.DeepProveError) as ei:
                ctx.decode(xs[:2], **args)
            assert ei.value.code == -1 and "dp_model_decode: " in str(ei.value) and message in str(ei.value), str(ei.value)
    finally:
        ctx.free()


def test_models_that_are_not_decodable_are_refused(dev):
    import deep_prove_amd as dpa
    for mb, message in ((dpa.models.lm_head(8, 16, 16, config=3), "node 0 must be an Embeddings layer"), (dpa.models.token_mlp(8, 16, 16, config=3), "the only output of the model must be a Logits node")):
        ctx = dpa.Context.generate(dev, mb.blob())
        try:
            with pytest.raises(dpa.DeepProveError) as ei:
                ctx.decode(np.zeros((2, mb.input_len), dtype=np.int64), 1, 2)
            assert ei.value.code == -1 and message in str(ei.value), str(ei.value)
        finally:
            ctx.free()


def test_a_refused_prompt_leaves_its_neighbours_alone(dev):
    """one wave of 64 prompts: prompt 5 holds a token outside the vocabulary (REFUSED, DP_INFER_BAD_TOKEN, its tokens as they stood), prompt 37 holds
    one at the full window (no step is run for it: the final pass refuses it); prompt 6 holds one BEHIND its prompt_len, which is never read"""
    import deep_prove_amd as dpa
    mb = gelu_lm()
    blob = mb.blob()
    xs = prompts(mb, 64)
    lens = np.array([PLENS[i % 8] for i in range(64)], dtype=np.uint32)
    lens[5], lens[37] = 3, SEQ
    xs[5, 0] = VOCAB
    xs[37, 6] = 1 << 40
    xs[6, lens[6]:] = VOCAB + 7
    good = [i for i in range(64) if i not in (5, 37)]
    want = _host(blob, xs, lens, 6, 12, 0, {})
    assert list(np.flatnonzero(want[2] == REFUSED)) == [5, 37] and list(want[3][[5, 37]]) == [2, 2] and want[1][5] == 3 and want[1][37] == SEQ
    ctx = dpa.Context.generate(dev, blob)
    try:
        tokens, length, stop, reasons, outs, _ = ctx.decode(xs, lens, 6, eos=12, all_kinds=True)
        assert list(np.flatnonzero(stop == REFUSED)) == [5, 37] and list(np.flatnonzero(reasons)) == [5, 37] and list(reasons[[5, 37]]) == [2, 2]
        assert list(tokens[5]) == [VOCAB] + list(xs[5, 1:3]) + [0] * 5 and length[5] == 3 and list(tokens[37]) == list(xs[37]) and length[37] == SEQ and not outs[[5, 37]].any()
        for got, w in zip((tokens, length, stop, reasons, outs), want):
            assert (got == w).all()
        assert (tokens[good] == want[0][good]).all() and (outs[good] == want[4][good]).all() and len(set(stop[good].tolist())) >= 2
    finally:
        ctx.free()


def test_decode_over_several_chunks():
    """a scratch bound of 1 MB: at least three chunks, the last partial, in one call"""
    r = _child("chunks", DP_INFER_SCRATCH_MB="1", DP_TIMING="1")
    n, per_chunk = (int(v) for v in re.search(r"decode child chunks ok: prompts (\d+) per_chunk (\d+)", r.stdout).groups())
    line = _decode_line(r)
    assert line["prompts"] == n and line["chunks"] == -(-n // per_chunk) >= 3 and n % per_chunk, (line, n, per_chunk)
    assert line["steps"] >= line["chunks"] and line["launches"] > line["steps"]


def test_the_stop_words_are_polled_less_often_than_steps_are_run():
    """seven steps (prompts of one token fill a window of eight): no host synchronisation inside a step, one poll every few steps"""
    line = _decode_line(_child("polls", DP_TIMING="1"))
    assert line["prompts"] == 5 and line["chunks"] == 1 and line["steps"] >= 7 and 1 <= line["polls"] < line["steps"], line


def test_decode_and_prove(dev):
    """six prompts: every proof is word for word Prover.prove(tokens[i]); verify_decode accepts it with its stop reason and refuses it with
    another prompt's tokens (the proof check answers), a changed generated token, a length one too small and WINDOW claimed for an EOS stop"""
    import deep_prove_amd as dpa
    mb = gelu_lm()
    xs = prompts(mb, 6)
    lens = np.array([2, 2, 2, 2, SEQ, 7], dtype=np.uint32)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        pr = dpa.Prover(ctx)
        tokens, length, stop, reasons, outs, proofs = pr.decode_and_prove(xs, lens, 6, eos=9, concurrency=4, all_kinds=True)
        assert not reasons.any() and list(stop[:5]) == [EOS] * 4 + [WINDOW] and list(length[:5]) == [5] * 4 + [SEQ] and stop[5] in (EOS, WINDOW)
        vb = ctx.verifier_blob()
        for i in range(6):
            want, wout = pr.prove(tokens[i])
            assert proofs[i].size == want.size and (proofs[i] == want).all() and (outs[i] == wout).all(), i
            dpa.verify_decode(vb, proofs[i], tokens[i], outs[i], lens[i], length[i], stop[i], eos=9, pad=0, max_new=6)
        assert (tokens[0] != tokens[2]).any()
        with pytest.raises(dpa.DeepProveError) as ei:  # the relation holds for prompt 2's tokens and outputs: the proof does not fit them
            dpa.verify_decode(vb, proofs[0], tokens[2], outs[2], 2, length[2], stop[2], eos=9, max_new=6)
        assert ei.value.code == -5 and "dp_verify_decode" not in str(ei.value), str(ei.value)
        bad = tokens[0].copy()
        bad[3] = (bad[3] + 1) % VOCAB
        for args, message in (((bad, outs[0], 2, 5, EOS), "token 3 is not the one the model chose at position 2"),
                              ((tokens[0], outs[0], 2, 4, EOS), "token 4 behind the completion is not the pad token"),
                              ((tokens[0], outs[0], 2, 5, WINDOW), "stop WINDOW claimed at length 5 of 8"),
                              ((tokens[0], outs[0], 2, 5, MAX_NEW), "stop MAX_NEW claimed at length 5")):
            with pytest.raises(dpa.DeepProveError) as ei:
                dpa.verify_decode(vb, proofs[0], *args, eos=9, max_new=6)
            assert ei.value.code == -5 and "dp_verify_decode: " + message in str(ei.value), str(ei.value)
    finally:
        ctx.free()
