"""Child process of tests/test_gpu_zzzzzzzz_infer_tables.py: DP_INFER_LOG / DP_INFER_NO_MFMA are read once per process, so the path the
transformer layer takes under DP_INFER_ALL_KINDS is observed here.
usage: infer_tables_child.py <batch> <out.npy>   (the `[dp infer]` line goes to stderr)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def build():
    import deep_prove_amd as dpa
    return dpa.models.transformer_layer(16, 64, 4, 16, 128, config=65)


def inputs(mb, batch):
    return np.stack([mb.input(1000 + i) for i in range(batch)])


if __name__ == "__main__":
    import deep_prove_amd as dpa
    mb = build()
    x = inputs(mb, int(sys.argv[1]))
    dev = dpa.Device(0)
    ctx = dpa.Context.generate(dev, mb.blob())
    out, ms = ctx.infer(x, all_kinds=True)
    np.save(sys.argv[2], out)
    ctx.free()
    dev.close()
    print("infer child ok", out.shape, ms)
