"""Child process of tests/test_gpu_zzzzzzz_infer.py: DP_INFER_LOG / DP_INFER_NO_MFMA are read once per process, so the path a model takes is
observed here. usage: infer_child.py <model> <batch> <out.npy>   (the `[dp infer]` line goes to stderr)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def build(name):
    import deep_prove_amd as dpa
    if name == "large_inputs":  # the model of test_host_inference.py::test_large_inputs_take_the_64_bit_path
        mb = dpa.models.ModelBuilder((8, 4), 5)
        mb.matmul(16, requant=False).matmul(8, bias=False, requant=False)
        return mb, 3000
    return getattr(dpa.models, name)(), 1


def inputs(mb, scale, batch):
    return np.stack([mb.input(1000 + i) * scale for i in range(batch)])


if __name__ == "__main__":
    import deep_prove_amd as dpa
    mb, scale = build(sys.argv[1])
    x = inputs(mb, scale, int(sys.argv[2]))
    dev = dpa.Device(0)
    ctx = dpa.Context.generate(dev, mb.blob())
    out, ms = ctx.infer(x)
    np.save(sys.argv[3], out)
    ctx.free()
    dev.close()
    print("infer child ok", out.shape, ms)
