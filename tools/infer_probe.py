"""Probe (torch-free) of dp_model_infer: the median wall_ms of <repeats> device calls on a batch (after two warm-up calls: the first one plans the
model and uploads the int8 weights), next to the wall time of the same inputs through dp_model_infer_host, one call per input spread over 16
threads — what a caller without the device entry point does on the CPUs a GPU box allows. Outputs of the two paths are compared.
usage: python tools/infer_probe.py dense_4m|cnn_264k|<model of deep_prove_amd.models> <batch> <repeats>"""
import os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa
wl = sys.argv[1]; batch = int(sys.argv[2]); reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
mb = getattr(dpa.models, wl)()
blob = mb.blob()
xs = np.stack([mb.input(3000 + i) for i in range(batch)])
dev = dpa.Device(0)
ctx = dpa.Context.generate(dev, blob)
for _ in range(2):
    ctx.infer(xs)
lib_ms, call_ms = [], []
for _ in range(reps):
    t0 = time.perf_counter(); out, ms = ctx.infer(xs); call_ms.append(1000 * (time.perf_counter() - t0)); lib_ms.append(ms)
with ThreadPoolExecutor(16) as ex:
    t0 = time.perf_counter(); host = np.stack(list(ex.map(lambda x: dpa.infer_host(blob, x), xs))); host_ms = 1000 * (time.perf_counter() - t0)
same = bool((host == out).all())
sha = subprocess.run([sys.executable, os.path.join(_root, "tools", "srchash.py")], capture_output=True, text=True).stdout.strip()
med = sorted(lib_ms)[len(lib_ms) // 2]
print(f"{wl} batch {batch} (csrc {sha}): dp_model_infer wall_ms median {med:.2f} (min {min(lib_ms):.2f}, max {max(lib_ms):.2f}; Python call median {sorted(call_ms)[len(call_ms) // 2]:.2f}) = "
      f"{batch / med * 1000:.0f} inputs/s; dp_model_infer_host x {batch} over 16 threads {host_ms:.0f} ms = {batch / host_ms * 1000:.0f} inputs/s; device / host speed-up {host_ms / med:.1f}x; outputs identical: {same}", flush=True)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
