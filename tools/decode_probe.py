"""Probe (torch-free) of Context.decode: greedy decoding of a batch of prompts with the whole loop on the device, against the two ways a caller
had before — one Context.infer call per token (a host round trip and a fresh upload each; the tokens are appended on the host) — and against
decode_host prompt by prompt (a sample of the batch; the figure is per prompt). Model: token_lm(64, 1024, 256), a window of 64 tokens, a
vocabulary of 1 024; 256 prompts of 8 tokens, up to 56 new tokens each, no end-of-sequence token (every prompt fills its window: the most steps).
The three ways alternate within each repeat, after a warm-up of each; times are host clocks around calls that end in a device synchronise.
The completions of the three ways are compared. It is a record, not a pass mark: the figures go to profiles/decode_device.txt.
usage: python tools/decode_probe.py [repeats] [output file]"""
import os, re, subprocess, sys, tempfile, time
os.environ["DP_TIMING"] = "1"  # (read once per process: the `[dp decode]` line of every decode call)
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(_root, "profiles", "decode_device.txt")
SEQ, VOCAB, WIDTH, NPROMPTS, PLEN, HOST_SAMPLE = 64, 1024, 256, 256, 8, 8
mb = dpa.models.token_lm(SEQ, VOCAB, WIDTH, config=43)
blob = mb.blob()
xs = np.stack([mb.input(3000 + i) for i in range(NPROMPTS)])
max_new = SEQ - PLEN
dev = dpa.Device(0)
ctx = dpa.Context.generate(dev, blob)


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


def device_decode():
    return ctx.decode(xs, PLEN, max_new, all_kinds=True)[0]


def infer_loop():
    """what a caller could do before: the window of every prompt goes up and its output comes down once per token"""
    tokens = np.zeros((NPROMPTS, SEQ), dtype=np.int64)
    tokens[:, :PLEN] = xs[:, :PLEN]
    for length in range(PLEN, SEQ):
        out, _ = ctx.infer(tokens, all_kinds=True)
        tokens[:, length] = out[:, length - 1]
    return tokens


def host_decode():
    return np.stack([dpa.decode_host(blob, xs[i][:PLEN], PLEN, max_new)[0] for i in range(HOST_SAMPLE)])


ways = (("Context.decode (device loop)", device_decode, NPROMPTS), ("Context.infer per token", infer_loop, NPROMPTS), ("decode_host", host_decode, HOST_SAMPLE))
results = [w[1]() for w in ways]  # warm-up: plans the model, uploads its constants, loads the code objects
same = bool((results[0] == results[1]).all() and (results[0][:HOST_SAMPLE] == results[2]).all())
times = {name: [] for name, _, _ in ways}
line = ""
for _ in range(repeats):
    for name, call, _ in ways:
        t0 = time.perf_counter()
        _, text = captured(call)
        times[name].append(1000 * (time.perf_counter() - t0))
        found = [ln for ln in text.split("\n") if ln.startswith("[dp decode]")]
        line = found[-1] if found else line
sha = subprocess.run([sys.executable, os.path.join(_root, "tools", "srchash.py")], capture_output=True, text=True).stdout.strip()
rows = [f"decode_probe: token_lm({SEQ}, {VOCAB}, {WIDTH}), {NPROMPTS} prompts of {PLEN} tokens, {max_new} new tokens each (csrc {sha}), {repeats} repeats alternating; completions identical: {same}", "  " + line]
for name, _, n in ways:
    v = times[name]
    rows.append(f"  {name}: median {med(v):.1f} ms for {n} prompts (min {min(v):.1f}, max {max(v):.1f}) = {med(v) / n:.3f} ms per prompt, {n * max_new / med(v) * 1000:.0f} tokens/s")
d, i, h = (med(times[w[0]]) / w[2] for w in ways)
rows.append(f"  per prompt, Context.decode against the per-token infer loop: {i / d:.2f} x; against decode_host: {h / d:.2f} x (medians)")
text = "\n".join(rows) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write(text)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
