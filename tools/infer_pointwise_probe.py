"""Probe (torch-free) of dp_model_infer on a CNN whose weight sits in pointwise layers, built inline: input (64, 32, 32), conv(64, 1) -> ReLU -> conv(128, 1) -> ReLU -> MaxPool ->
conv(32, 3) -> ReLU -> MaxPool -> Flatten -> Dense(10), a Requant behind every conv. The median wall_ms of <repeats> device calls after two warm-up calls, the `[dp infer]` line of the
last call, and the outputs of the first, middle and last input against dp_model_infer_host. The widest pointwise layer is conv(128, 1): 128 x 64 x 1024 multiply-adds per input.
usage: python tools/infer_pointwise_probe.py <batch> <repeats>   (DP_LIB_VARIANT=<tag>: another build of the library)"""
import os, subprocess, sys
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
os.environ["DP_INFER_LOG"] = "1"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa
batch, reps = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 7
mb = dpa.models.ModelBuilder((64, 32, 32), 131).conv(64, 1).relu().conv(128, 1).relu().maxpool().conv(32, 3).relu().maxpool().flatten().dense(10, requant=False)
blob = mb.blob()
xs = np.random.default_rng(7).integers(-128, 128, size=(batch, mb.input_len), dtype=np.int64)
dev = dpa.Device(0)
ctx = dpa.Context.generate(dev, blob)
for _ in range(2):
    ctx.infer(xs)
ms = sorted(ctx.infer(xs)[1] for _ in range(reps))
out = ctx.infer(xs)[0]
same = all(bool((dpa.infer_host(blob, xs[i]) == out[i]).all()) for i in (0, batch // 2, batch - 1))
sha = subprocess.run([sys.executable, os.path.join(_root, "tools", "srchash.py")], capture_output=True, text=True).stdout.strip()
print(f"pointwise CNN batch {batch} (csrc {sha}, library {os.environ.get('DP_LIB_VARIANT') or 'this'}): dp_model_infer wall_ms median {ms[len(ms) // 2]:.2f} (min {ms[0]:.2f}, max {ms[-1]:.2f}) = "
      f"{batch / ms[len(ms) // 2] * 1000:.0f} inputs/s; outputs of 3 inputs identical to dp_model_infer_host: {same}", flush=True)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
