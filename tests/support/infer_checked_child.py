"""Child process of tests/test_gpu_zzzzzzzzz_infer_checked.py: DP_INFER_LOG / DP_INFER_SCRATCH_MB are read once per process, so the chunks of
a checked call are observed here. Two calls of dp_model_infer_checked on the transformer layer of infer_tables_child.py, batch <batch>: an all-good
one, whose `[dp infer]` line gives the chunk size c, then one in which the rows 0, c - 1, c, every row of the second chunk and the last row carry
an element the first LayerNorm refuses. The library's stderr goes through a file meanwhile and is printed again afterwards.
usage: infer_checked_child.py <batch> <out.npz>   (out: good, good_reasons, out, reasons, bad, chunk, nchunks)"""
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_tables_child  # noqa: E402  (puts the repository root on sys.path)

BAD_ELEMENT, BAD_VALUE = 5, (1 << 20) + 1  # (an element of the first input tensor: what the first LayerNorm normalises)


def bad_rows(batch, c):
    return sorted(set([0, c - 1, c, batch - 1] + list(range(c, min(2 * c, batch)))))


if __name__ == "__main__":
    import deep_prove_amd as dpa
    batch = int(sys.argv[1])
    mb = infer_tables_child.build()
    x = infer_tables_child.inputs(mb, batch)
    dev = dpa.Device(0)
    ctx = dpa.Context.generate(dev, mb.blob())
    log = tempfile.TemporaryFile()
    sys.stderr.flush()
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        good, good_reasons, _ = ctx.infer_checked(x, all_kinds=True)
    finally:
        os.dup2(saved, 2)
    log.seek(0)
    first = log.read().decode()
    sys.stderr.write(first)
    m = re.search(r"batch (\d+) in (\d+) chunks of (\d+),", first)
    assert m and int(m.group(1)) == batch, first
    nchunks, c = int(m.group(2)), int(m.group(3))
    bad = bad_rows(batch, c)
    xb = x.copy()
    xb[bad, BAD_ELEMENT] = BAD_VALUE
    out, reasons, ms = ctx.infer_checked(xb, all_kinds=True)
    np.savez(sys.argv[2], good=good, good_reasons=good_reasons, out=out, reasons=reasons, bad=np.array(bad), chunk=c, nchunks=nchunks)
    ctx.free()
    dev.close()
    os.close(saved)
    print("infer checked child ok", out.shape, ms)
