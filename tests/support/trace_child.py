"""Child process of tests/test_gpu_zzzzzzzzzzzzz_trace.py: DP_INFER_SCRATCH_MB, DP_INFER_NO_MFMA, DP_INFER_LOG and DP_PROVE_TRACE_MB are read
from the environment the parent gives, some of them once per process. Every comparison is exact equality against dp_model_infer_host_trace /
dp_model_infer_host (through the Python wrappers); a mismatch is an AssertionError and a non-zero exit status.
usage: trace_child.py rows     every family of trace_families.py: a batch large enough for at least two chunks with a partial last one under the
                               scratch bound given; rows against the host trace, plain infer before and after
       trace_child.py checked  one model per refusal class: a refused input in the first and in the last chunk
       trace_child.py prove    every family: 6 proofs from device inference in segments against those of prove_batch"""
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from support import trace_families as T  # noqa: E402

WORDS = {"requant": 1, "vocabulary": 2, "gelu": 3, "layernorm": 4, "softmax": 5}
LN_BAD, SM_BAD = (1 << 20) + 1, (1 << 24) + 1
POOL = 5


def captured(call):
    """call() with the library's stderr through a file; returns (result, what it wrote) and prints it again"""
    log = tempfile.TemporaryFile()
    sys.stderr.flush()
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        res = call()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    log.seek(0)
    text = log.read().decode()
    sys.stderr.write(text)
    return res, text


def chunked_batch(ctx, pool, all_kinds, checked):
    """(n, chunks, chunk size): a batch size at which an infer_trace call of inputs pool[i % len(pool)] takes at least two chunks, the last partial"""
    n = 64
    while n < 200000:
        x = pool[np.arange(n) % len(pool)]
        _, text = captured(lambda: ctx.infer_trace(x, all_kinds=all_kinds, checked=checked))
        m = re.search(r"batch (\d+) in (\d+) chunks of (\d+),", text)
        assert m and int(m.group(1)) == n and "; taps " in text, text
        nchunks, c = int(m.group(2)), int(m.group(3))
        if nchunks >= 2 and n % c:
            return n, nchunks, c
        n = n + 1 if nchunks >= 2 else 4 * n + 1
    raise AssertionError("no batch size gives two chunks")


def host_rows(dpa, blob, xs, row_words, nout):
    """the yardstick, input by input: (rows, outputs, reasons) — zeros and the class of the word in the message where the host refuses"""
    rows, outs, reasons = np.zeros((len(xs), row_words), dtype=np.int64), np.zeros((len(xs), nout), dtype=np.int64), np.zeros(len(xs), dtype=np.uint32)
    for i, x in enumerate(xs):
        try:
            rows[i] = dpa.infer_host_trace(blob, x)
            outs[i] = dpa.infer_host(blob, x)
        except dpa.DeepProveError as e:
            hits = [w for w in WORDS if w in str(e)]
            assert e.code == -1 and len(hits) == 1, str(e)
            reasons[i] = WORDS[hits[0]]
    return rows, outs, reasons


def mode_rows(dpa, dev):
    for family in T.FAMILIES:
        mb = T.build(family)
        blob = mb.blob()
        all_kinds = family[0] in T.NEEDS_ALL_KINDS
        pool = T.inputs(mb, POOL)
        ctx = dpa.Context.generate(dev, blob)
        before, _ = ctx.infer(pool[:3], all_kinds=all_kinds)
        n, nchunks, c = chunked_batch(ctx, pool, all_kinds, False)
        idx = np.arange(n) % POOL
        rows, view, outs, reasons, ms = ctx.infer_trace(pool[idx], all_kinds=all_kinds)
        entries, row_words = dpa.trace_layout(blob)
        want_rows, want_outs, want_reasons = host_rows(dpa, blob, pool, row_words, outs.shape[1])
        assert reasons is None and not want_reasons.any() and rows.shape == (n, row_words)
        assert (rows == want_rows[idx]).all(), np.argwhere(rows != want_rows[idx])[:5]
        assert (outs == want_outs[idx]).all()
        assert all((view[(node, role)] == want_rows[idx][:, off:off + ln]).all() for node, role, off, ln in entries)
        after, _ = ctx.infer(pool[:3], all_kinds=all_kinds)
        assert (before == after).all() and (before == want_outs[:3]).all()
        ctx.free()
        print(f"trace child rows ok: {family[0]} batch {n} in {nchunks} chunks of {c}, {len(entries)} entries, {row_words} words")


def poke(index, value):
    def f(dpa, blob, x):
        y = x.copy()
        y[index] = value
        return y
    return f


def scaled_until_refused(dpa, blob, x):
    scale = 1
    for _ in range(40):
        scale *= 8
        try:
            dpa.infer_host(blob, x * scale)
        except dpa.DeepProveError:
            return x * scale
    raise AssertionError("the host accepts every scale")


# (class, model, arguments, keywords, what makes an input of that class)
CLASSES = [(1, "mlp", (2, 64), dict(config=31), scaled_until_refused),
           (2, "token_mlp", (16, 50, 32), dict(config=71, max_positions=40), poke(3, 1 << 20)),
           (3, "gelu_only", (16,), dict(config=31), poke(2, 1 << 14)),
           (4, "layernorm_mlp", (4, 8, 16), dict(config=33), poke(9, LN_BAD)),
           (5, "softmax_only", (2, 4), dict(config=35), poke(5, SM_BAD))]


def mode_checked(dpa, dev):
    for cls, name, args, kw, make_bad in CLASSES:
        mb = getattr(dpa.models, name)(*args, **kw)
        blob = mb.blob()
        pool = T.inputs(mb, POOL)
        ctx = dpa.Context.generate(dev, blob)
        n, nchunks, c = chunked_batch(ctx, pool, True, True)
        idx = np.arange(n) % POOL
        xs = pool[idx]
        bad = [1, n - 1]  # (the first and the last chunk)
        assert bad[0] < c and bad[1] >= (nchunks - 1) * c
        bad_x = make_bad(dpa, blob, pool[1])
        xs[bad] = bad_x
        (rows, view, outs, reasons, ms), text = captured(lambda: ctx.infer_trace(xs, all_kinds=True, checked=True))
        assert text.rstrip().endswith(f"; checked, refused {len(bad)}") and "; taps " in text, text
        entries, row_words = dpa.trace_layout(blob)
        want_rows, want_outs, want_reasons = host_rows(dpa, blob, np.concatenate([pool, bad_x[None, :]]), row_words, outs.shape[1])
        assert list(want_reasons) == [0] * POOL + [cls], (name, want_reasons)
        pick = idx.copy()
        pick[bad] = POOL
        assert (reasons == want_reasons[pick]).all(), (name, np.flatnonzero(reasons != want_reasons[pick])[:5])
        assert not rows[bad].any() and not outs[bad].any()
        assert (rows == want_rows[pick]).all() and (outs == want_outs[pick]).all()
        # the plain trace call refuses the batch with the host's message, and the model stays usable
        try:
            ctx.infer_trace(xs, all_kinds=True)
            raise AssertionError("the plain trace call accepted a refused input")
        except dpa.DeepProveError as e:
            assert e.code == -1 and [w for w in WORDS if w in str(e)] == [w for w, k in WORDS.items() if k == cls], str(e)
        good, _, _, _, _ = ctx.infer_trace(pool, all_kinds=True)
        assert (good == want_rows[:POOL]).all()
        ctx.free()
        print(f"trace child checked ok: class {cls} {name} batch {n} in {nchunks} chunks of {c}")


def mode_prove(dpa, dev):
    for family in T.FAMILIES:
        mb = T.build(family)
        xs = T.inputs(mb, 6)
        ctx = dpa.Context.generate(dev, mb.blob())
        pr = dpa.Prover(ctx)
        host, houts, _ = pr.prove_batch(xs, 4)
        (got, gouts, ms), text = captured(lambda: pr.prove_batch(xs, 4, device_infer=True))
        m = re.search(r"prove_batch_ex: 6 proofs in (\d+) segments of <= (\d+),", text)
        assert m and int(m.group(1)) >= 2 and int(m.group(2)) == 4, text[-2000:]
        assert (gouts == houts).all() and len(got) == 6
        for a, b in zip(got, host):
            assert a.size == b.size and (a == b).all()
        res, _ = dpa.verify_batch(ctx.verifier_blob(), got, xs, gouts, dev=dev)
        assert not res.any(), res
        ctx.free()
        print(f"trace child prove ok: {family[0]} 6 proofs in {m.group(1)} segments")


if __name__ == "__main__":
    import deep_prove_amd as dpa
    dev = dpa.Device(0)
    {"rows": mode_rows, "checked": mode_checked, "prove": mode_prove}[sys.argv[1]](dpa, dev)
    dev.close()
    print("trace child done", sys.argv[1])
