"""Probe (torch-free) of dp_model_infer on ONE many-channel conv chain, built inline: conv(kx -> kx, 3 x 3) -> Requant -> ReLU on an input of (kx, nw, nw) — 256 channels at nw = 16 or
512 at nw = 8, the layers whose kx spans pass the LDS of the whole-span k_infer_conv_i8 (csrc/infer.h infer_conv_pack). The median wall_ms of <repeats> device calls after two warm-up
calls, the `[dp infer]` line of the last call, the multiply-adds of a call, and the outputs of the first, middle and last input against dp_model_infer_host.
usage: python tools/infer_conv_wide_probe.py <kx: 256 | 512> <batch> <repeats>   (DP_LIB_VARIANT=<tag>: another build of the library)"""
import os, subprocess, sys
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
os.environ["DP_INFER_LOG"] = "1"
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import numpy as np
import deep_prove_amd as dpa
kx, batch, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 7
nw = {256: 16, 512: 8}[kx]
mb = dpa.models.ModelBuilder((kx, nw, nw), 131).conv(kx, 3).relu()
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
macs = batch * kx * kx * 12 * nw * nw  # what the kernel multiplies: K = kx * ra * rn = kx * 3 * 4 per output of the padded plane
print(f"conv({kx} -> {kx}, 3 x 3) + Requant + ReLU at nw {nw}, batch {batch} (csrc {sha}, library {os.environ.get('DP_LIB_VARIANT') or 'this'}): dp_model_infer wall_ms median "
      f"{ms[len(ms) // 2]:.2f} (min {ms[0]:.2f}, max {ms[-1]:.2f}); {macs / 1e9:.2f} G multiply-adds of the padded K per call; outputs of 3 inputs identical to dp_model_infer_host: {same}", flush=True)
ctx.free()
dev.close()
sys.exit(0 if same else 1)
