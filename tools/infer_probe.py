"""Probe (torch-free) of dp_model_infer: the median wall_ms of <repeats> device calls on a batch (after two warm-up calls: the first one plans the
model and uploads the int8 weights), next to the wall time of the same inputs through dp_model_infer_host, one call per input spread over 16
threads — what a caller without the device entry point does on the CPUs a GPU box allows. Outputs of the two paths are compared.
--all-kinds: dp_model_infer_ex with DP_INFER_ALL_KINDS (LayerNorm / Softmax / Mha / GELU models); the `[dp infer]` lines of the timed calls are
read back (the library's stderr is redirected to a file) for the share of the wall time spent in the Softmax shift round trips.
transformer_layer / transformer_layer_gelu: golden case 14's model (64 x 256, 4 heads of 64, ffn 1 024, config 66), without / with GELU.
--checked: dp_model_infer_checked (a status per input) timed beside the plain call on the same inputs, the two alternating call by call; its
outputs must be the plain call's and no input may be refused.
usage: python tools/infer_probe.py dense_4m|cnn_264k|transformer_layer[_gelu]|<model of deep_prove_amd.models> <batch> <repeats> [--all-kinds] [--checked]"""
import os, re, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa
all_kinds = "--all-kinds" in sys.argv
checked = "--checked" in sys.argv
argv = [a for a in sys.argv if a not in ("--all-kinds", "--checked")]
wl = argv[1]; batch = int(argv[2]); reps = int(argv[3]) if len(argv) > 3 else 5
if all_kinds:  # (read once per process, at the first call)
    os.environ["DP_INFER_LOG"] = "1"
mb = dpa.models.transformer_layer(64, 256, 4, 64, 1024, config=66, gelu=wl.endswith("_gelu")) if wl.startswith("transformer_layer") else getattr(dpa.models, wl)()
blob = mb.blob()
xs = np.stack([mb.input(3000 + i) for i in range(batch)])
dev = dpa.Device(0)
ctx = dpa.Context.generate(dev, blob)
for _ in range(2):
    ctx.infer(xs, all_kinds=all_kinds)
    if checked:
        ctx.infer_checked(xs, all_kinds=all_kinds)
lib_ms, call_ms, chk_ms = [], [], []
log = tempfile.TemporaryFile() if all_kinds else None
if log:  # the [dp infer] lines of the timed calls: fd 2 goes to a file meanwhile
    sys.stderr.flush(); saved = os.dup(2); os.dup2(log.fileno(), 2)
for _ in range(reps):
    t0 = time.perf_counter(); out, ms = ctx.infer(xs, all_kinds=all_kinds); call_ms.append(1000 * (time.perf_counter() - t0)); lib_ms.append(ms)
    if checked:
        cout, reasons, ms = ctx.infer_checked(xs, all_kinds=all_kinds); chk_ms.append(ms)
shift = ""
if log:
    os.dup2(saved, 2); os.close(saved); log.seek(0)
    lines = [ln for ln in log.read().decode().split("\n") if ln.startswith("[dp infer]") and "; checked" not in ln]
    trips = [(int(a), float(b), float(c)) for a, b, c in re.findall(r"shift_trips (\d+) shift_ms ([0-9.]+);.* ([0-9.]+) ms", "\n".join(lines))]
    if trips:
        t = sorted(trips, key=lambda v: v[2])[len(trips) // 2]
        shift = f"; shift round trips {t[0]} per call, {t[1]:.2f} ms of {t[2]:.2f} ms = {100 * t[1] / t[2]:.0f} % of the wall time (the call of median wall time)"
    print(lines[-1], flush=True)
with ThreadPoolExecutor(16) as ex:
    t0 = time.perf_counter(); host = np.stack(list(ex.map(lambda x: dpa.infer_host(blob, x), xs))); host_ms = 1000 * (time.perf_counter() - t0)
same = bool((host == out).all())
chk = ""
if checked:
    same = same and bool((cout == out).all()) and not reasons.any()
    cm = sorted(chk_ms)[len(chk_ms) // 2]
    chk = f"; dp_model_infer_checked wall_ms median {cm:.2f} (min {min(chk_ms):.2f}, max {max(chk_ms):.2f}) = {100 * (cm / sorted(lib_ms)[len(lib_ms) // 2] - 1):+.1f} % against the plain call, alternating; refused {int(np.count_nonzero(reasons))}"
sha = subprocess.run([sys.executable, os.path.join(_root, "tools", "srchash.py")], capture_output=True, text=True).stdout.strip()
med = sorted(lib_ms)[len(lib_ms) // 2]
print(f"{wl} batch {batch} (csrc {sha}): {'dp_model_infer_ex(DP_INFER_ALL_KINDS)' if all_kinds else 'dp_model_infer'} wall_ms median {med:.2f} (min {min(lib_ms):.2f}, max {max(lib_ms):.2f}; Python call median {sorted(call_ms)[len(call_ms) // 2]:.2f}) = "
      f"{batch / med * 1000:.0f} inputs/s; dp_model_infer_host x {batch} over 16 threads {host_ms:.0f} ms = {batch / host_ms * 1000:.0f} inputs/s; device / host speed-up {host_ms / med:.1f}x; outputs identical: {same}{shift}{chk}", flush=True)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
