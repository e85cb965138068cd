"""The decode cases that need an environment of their own (tests/test_gpu_zzzzzzzzzzzzzz_decode.py runs them in a child process):
  chunks   DP_INFER_SCRATCH_MB=1: enough prompts for at least three chunks with a partial last one — the count follows from the bytes one sample
           takes in the chunk's scratch, worked out here from the model's layers — decoded in one call and compared with decode_host prompt by prompt
  polls    DP_TIMING=1: a decode of seven steps; the parent reads the `[dp decode]` line
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deep_prove_amd as dpa  # noqa: E402
from support.decode_cases import SEQ, WINDOW, prompts, relu_lm  # noqa: E402


def bytes_per_sample(mb):
    """what one sample takes in the scratch of a chunk during decode: every tensor of the flattened model as int64, an int8 copy beside the
    tensors known to lie within -128..127 (what a Requant writes, and what a ReLU makes of it), the int64 token block and the output block"""
    m = dpa.models
    entries, _ = dpa.trace_layout(mb.blob())
    lens = {node: n for node, role, _, n in entries if role == 0}
    total, q = mb.input_len * 8, False
    for node, l in enumerate(mb.layers):
        q = l["kind"] == m.L_REQUANT or (l["kind"] == m.L_RELU and q)
        total += lens[node] * (9 if q else 8)
    return total + mb.input_len * 8 + lens[len(mb.layers) - 1] * 8


def main(mode):
    mb = relu_lm()
    blob = mb.blob()
    dev = dpa.Device(0)
    ctx = dpa.Context.generate(dev, blob)
    try:
        if mode == "chunks":
            per_chunk = (int(os.environ["DP_INFER_SCRATCH_MB"]) << 20) // bytes_per_sample(mb)
            n = 2 * per_chunk + per_chunk // 3 + 1
            xs = prompts(mb, n)
            lens = np.array([(1, 2, 8, 2, 7, 3)[i % 6] for i in range(n)], dtype=np.uint32)
            tokens, length, stop, reasons, outs, _ = ctx.decode(xs, lens, 6, eos=12, pad=1)
            assert not reasons.any()
            for i in range(n):
                wt, wl, ws, wr, wo = dpa.decode_host(blob, xs[i][:lens[i]], int(lens[i]), 6, eos=12, pad=1)
                assert (tokens[i] == wt).all() and length[i] == wl and stop[i] == ws and wr == 0 and (outs[i] == wo).all(), i
            assert len(set(stop.tolist())) >= 2
            print(f"decode child chunks ok: prompts {n} per_chunk {per_chunk}")
        elif mode == "polls":
            xs = prompts(mb, 5)
            tokens, length, stop, _, _, _ = ctx.decode(xs, 1, 7)
            assert (length == SEQ).all() and (stop == WINDOW).all()
    finally:
        ctx.free()
        dev.close()
    print(f"decode child done {mode}")


if __name__ == "__main__":
    main(sys.argv[1])
