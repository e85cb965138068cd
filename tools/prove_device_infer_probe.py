"""Probe (torch-free) of dp_model_prove_batch_ex with DP_PROVE_DEVICE_INFER against dp_model_prove_batch on the same inputs.
1. Host preparation per proof (DP_TIMING, DP_PREP_THREADS=0 so that the proving thread makes it itself and the figure is no wait for a helper; a
   batch of 16, 8 in flight): the median of the `host phases of one proof: inference + witness columns` figures, with run_model and from the taps.
2. The batch rate, A and B alternating batch by batch in one process over <batches> pairs (A = host inference, B = the flag; NOTES: figures of
   different calls are not comparable): wall_ms of the call (B: inference + proving) and proofs/s, medians and ranges; the device inference of a
   batch (infer_ms); from the `[dp infer]` lines of the B calls the size of the tap image and the GB/s k_infer_tap_pack moves at 16 bytes per word.
The proofs of the first pair are compared word for word.
transformer_layer: golden case 14's model (64 x 256, 4 heads of 64, ffn 1 024, config 66).
usage: python tools/prove_device_infer_probe.py dense_4m|cnn_264k|transformer_layer <batch> <concurrency> <batches>"""
import os, re, subprocess, sys, tempfile, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
os.environ["DP_INFER_LOG"] = "1"  # (read once per process, at the first inference)
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa

wl, batch, conc, nbatches = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
mb = dpa.models.transformer_layer(64, 256, 4, 64, 1024, config=66) if wl == "transformer_layer" else getattr(dpa.models, wl)()
blob = mb.blob()
xs = np.stack([mb.input(3000 + i) for i in range(batch)])
entries, row_words = dpa.trace_layout(blob)
dev = dpa.Device(0)
ctx = dpa.Context.generate(dev, blob)
pr = dpa.Prover(ctx)


def med(v):
    return sorted(v)[len(v) // 2]


def captured(call):
    log = tempfile.TemporaryFile()
    sys.stderr.flush(); saved = os.dup(2); os.dup2(log.fileno(), 2)
    try:
        res = call()
    finally:
        os.dup2(saved, 2); os.close(saved)
    log.seek(0)
    return res, log.read().decode()


# warm-up: one proof alone first (its footprint sizes the workers' arenas, as in bench.py: without it far fewer proofs fit in flight); workers, cohorts
# and arenas are made by the first batch; the first inference plans the model and uploads its constants
pr.prove(xs[0])
a, aout, _ = pr.prove_batch(xs, conc)
b, bout, _ = pr.prove_batch(xs, conc, device_infer=True)
same = len(a) == len(b) and all(p.size == q.size and bool((p == q).all()) for p, q in zip(a, b)) and bool((aout == bout).all())
del a, b
# 1. host preparation per proof
os.environ["DP_TIMING"] = "1"; os.environ["DP_PREP_THREADS"] = "0"
small = xs[:min(batch, 16)]
prep = {}
for name, flag in (("run_model", False), ("taps", True)):
    _, text = captured(lambda: pr.prove_batch(small, min(conc, 8), device_infer=flag))
    v = [float(t) for t in re.findall(r"host phases of one proof: inference \+ witness columns \(or the wait for the helper that made them\) ([0-9.]+) ms", text)]
    prep[name] = v
del os.environ["DP_TIMING"], os.environ["DP_PREP_THREADS"]
# 2. the batch rate, alternating
wall = {False: [], True: []}; clock = {False: [], True: []}; infer_ms, lines = [], []
for _ in range(nbatches):
    for flag in (False, True):
        t0 = time.perf_counter()
        (proofs, _, ms), text = captured(lambda: pr.prove_batch(xs, conc, device_infer=flag))
        clock[flag].append(1000 * (time.perf_counter() - t0)); wall[flag].append(ms)
        del proofs
        if flag:
            infer_ms.append(pr.last_infer_ms)
            lines += [ln for ln in text.split("\n") if ln.startswith("[dp infer]") and "; taps " in ln]
packs = [(int(n), int(w), int(k), float(p)) for n, w, k, p in re.findall(r"batch (\d+) in \d+ chunks.*; taps \d+ entries, (\d+) words, pack_launches (\d+) pack_ms ([0-9.]+)", "\n".join(lines))]
gbs = [n * w * 16 / (p * 1e6) for n, w, k, p in packs if p > 0]
sha = subprocess.run([sys.executable, os.path.join(_root, "tools", "srchash.py")], capture_output=True, text=True).stdout.strip()
print(lines[-1] if lines else "(no [dp infer] line)", flush=True)
print(f"{wl} batch {batch}, {pr.in_flight()} in flight of {conc} asked (csrc {sha}), {nbatches} pairs alternating; proofs identical: {same}")
for name in ("run_model", "taps"):
    v = prep[name]
    print(f"  host preparation per proof, {name}: median {med(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}, {len(v)} proofs of worker 0, batch {len(small)})" if v else f"  host preparation per proof, {name}: no figure")
print(f"  trace row {row_words} words in {len(entries)} entries = {row_words * 8 / 1e6:.3f} MB per input, tap image of the batch {batch * row_words * 8 / 1e6:.1f} MB")
if gbs:
    print(f"  k_infer_tap_pack: median {med([p for _, _, _, p in packs]):.3f} ms per call ({packs[-1][2]} launches) = {med(gbs):.0f} GB/s at 16 bytes per word (min {min(gbs):.0f}, max {max(gbs):.0f})")
print(f"  device inference of the batch (infer_ms): median {med(infer_ms):.2f} ms (min {min(infer_ms):.2f}, max {max(infer_ms):.2f}) = {med(infer_ms) / batch:.3f} ms per input")
for flag, name in ((False, "A host inference (dp_model_prove_batch)"), (True, "B DP_PROVE_DEVICE_INFER")):
    w = wall[flag]
    print(f"  {name}: wall_ms median {med(w):.1f} (min {min(w):.1f}, max {max(w):.1f}) = {batch / med(w) * 1000:.1f} proofs/s; Python call median {med(clock[flag]):.1f} ms")
print(f"  B against A: {100 * (med(wall[False]) / med(wall[True]) - 1):+.1f} % proofs/s (medians)", flush=True)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
