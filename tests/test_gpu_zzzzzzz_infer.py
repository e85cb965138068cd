"""dp_model_infer: Model::run for a batch of inputs on the device (include/deep_prove_hip_infer.h; csrc/infer.h, csrc/infer_kernels.inc).
Expected values always come from `mb.run(x)`, the numpy inference of deep_prove_amd/models.py, which shares no code with the library;
dp_model_infer_host is the second witness. Every comparison is exact equality: the i8 MFMA path, the 64-bit path and the host compute the
same integers. Random quantised weights are asymmetric, so a row / column or operand swap in the MFMA fragments cannot pass."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "infer_child.py")

MODELS = [("mlp", (2, 64), dict(config=31)), ("dense_4m", (), {}), ("cnn_tiny", (), {}), ("cnn_264k", (), {}),
          ("seq_mlp", (16, 64), dict(config=63, transpose_last=True, positional=True)), ("seq_1m", (), {}),
          ("token_mlp", (32, 300, 128), dict(config=72, max_positions=50)), ("attention_block", (16, 64, 4, 16), dict(config=64)),
          ("matmul_pair", (8, 16, 8), dict(config=81)), ("matmul_pair", (8, 16, 8), dict(config=82, transpose_b=True)),
          ("qkv_two_outputs", (8, 16, 8), dict(config=83))]


def _host_all(blob, xs):
    """dp_model_infer_host for every row (ctypes releases the GIL: 16 threads, what a caller has today)"""
    import deep_prove_amd as dpa
    with ThreadPoolExecutor(16) as ex:
        return np.stack(list(ex.map(lambda x: dpa.infer_host(blob, x), xs)))


def _spread(n, k=64):
    return sorted(set([0, n - 1] + [int(i) for i in np.linspace(0, n - 1, k)]))


@pytest.mark.parametrize("name,args,kw", MODELS, ids=[m[0] + ("_t" if m[2].get("transpose_b") else "") for m in MODELS])
def test_device_inference_equals_numpy_and_host(dev, monkeypatch, name, args, kw):
    """batches of 1, 3 and 65 against numpy and the host, input by input; a large batch (4 224 for Dense-4M, 512 otherwise) against the host on
    every output and against numpy on 64 of them, with the scratch bound set so low that chunk boundaries fall inside the batch"""
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, name)(*args, **kw)
    blob = mb.blob()
    large = 4224 if name == "dense_4m" else 512
    xs = np.stack([mb.input(1000 + i) for i in range(large)])
    ctx = dpa.Context.generate(dev, blob)
    try:
        for batch in (1, 3, 65):
            out, ms = ctx.infer(xs[:batch])
            want = np.stack([mb.run(x) for x in xs[:batch]])
            assert out.shape == want.shape and (out == want).all(), (name, batch, np.argwhere(out != want)[:5])
            assert (out == _host_all(blob, xs[:batch])).all() and ms > 0
        host = _host_all(blob, xs)
        picks = _spread(large)
        want = np.stack([mb.run(xs[i]) for i in picks])
        # per-sample activation scratch: Dense-4M ~110 KB (64 MB: chunks of ~580), the small models a few KB (1 MB: chunks well below 512)
        for mbytes in (["64"] if name == "dense_4m" else ["1"]) + [None]:
            if mbytes is None:
                monkeypatch.delenv("DP_INFER_SCRATCH_MB", raising=False)
            else:
                monkeypatch.setenv("DP_INFER_SCRATCH_MB", mbytes)
            out, _ = ctx.infer(xs)
            assert out.shape == host.shape and (out == host).all(), (name, mbytes, np.argwhere(out != host)[:5])
            assert (out[picks] == want).all()
    finally:
        ctx.free()


def _child(model, batch, tmp_path, tag, **env):
    e = dict(os.environ, DP_INFER_LOG="1", **env)
    out = str(tmp_path / f"{tag}.npy")
    r = subprocess.run([sys.executable, CHILD, model, str(batch), out], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0 and "infer child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert len(lines) == 1, r.stderr[-2000:]
    counts = {k: int(v) for k, v in re.findall(r"(gemm_i8|gemm_i64|conv|requant|relu) (\d+)", lines[0])}
    return np.load(out), counts


def test_dense_4m_takes_the_mfma_path_and_the_64_bit_path_agrees(tmp_path):
    import deep_prove_amd as dpa
    a, ca = _child("dense_4m", 65, tmp_path, "mfma")
    b, cb = _child("dense_4m", 65, tmp_path, "valu", DP_INFER_NO_MFMA="1")
    assert ca["gemm_i8"] == 6 and ca["gemm_i64"] == 0, ca
    assert cb["gemm_i8"] == 0 and cb["gemm_i64"] == 6, cb
    mb = dpa.models.dense_4m()
    want = np.stack([mb.run(mb.input(1000 + i)) for i in range(65)])
    assert (a == want).all() and (b == want).all()


def test_large_inputs_take_the_64_bit_kernels(tmp_path):
    """the model of test_host_inference.py::test_large_inputs_take_the_64_bit_path (inputs x 3 000, no Requant in front of the second MatMul)"""
    sys.path.insert(0, os.path.dirname(CHILD))
    import infer_child
    out, c = _child("large_inputs", 5, tmp_path, "large")
    assert c["gemm_i64"] == 2 and c["gemm_i8"] == 0, c
    mb, scale = infer_child.build("large_inputs")
    xs = infer_child.inputs(mb, scale, 5)
    assert np.abs(xs).max() > 32767
    assert (out == np.stack([mb.run(x) for x in xs])).all()


def test_requant_range_error_is_the_hosts_and_the_model_stays_usable(dev):
    import deep_prove_amd as dpa
    mb = dpa.models.dense_4m()
    blob = mb.blob()
    good = np.stack([mb.input(1000 + i) for i in range(3)])
    bad, scale = None, 1
    for _ in range(40):  # scale an input until the first Requant's bit-size check trips on the host
        scale *= 8
        x = good[1] * scale
        try:
            dpa.infer_host(blob, x)
        except dpa.DeepProveError as e:
            assert e.code == -1 and "requant" in str(e)
            bad = x
            break
    assert bad is not None
    ctx = dpa.Context.generate(dev, blob)
    try:
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(np.stack([good[0], bad, good[2]]))
        assert ei.value.code == -1 and "requant" in str(ei.value)
        out, _ = ctx.infer(good)
        assert (out == np.stack([mb.run(x) for x in good])).all()
        with pytest.raises(dpa.DeepProveError) as ei:  # wrong input length: DP_ERR_SHAPE, as the prove calls
            ctx.infer(good[:, :2])
        assert ei.value.code == -4
    finally:
        ctx.free()


def test_token_outside_the_vocabulary_is_refused(dev):
    import deep_prove_amd as dpa
    mb = dpa.models.token_mlp(32, 300, 128, config=72, max_positions=50)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        x = np.stack([mb.input(1000), mb.input(1001)])
        x[1, 3] = 1 << 20
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(x)
        assert ei.value.code == -1 and "vocabulary" in str(ei.value)
        with pytest.raises(dpa.DeepProveError):
            dpa.infer_host(mb.blob(), x[1])
        x[1, 3] = 0
        out, _ = ctx.infer(x)
        assert (out == np.stack([mb.run(v) for v in x])).all()
    finally:
        ctx.free()


@pytest.mark.parametrize("name,args,kw,kind", [("gelu_mlp", (256,), dict(config=112), "GELU"), ("transformer_layer", (16, 64, 4, 16, 128), dict(config=65), "LayerNorm")])
def test_float_table_kinds_are_refused(dev, name, args, kw, kind):
    import deep_prove_amd as dpa
    mb = getattr(dpa.models, name)(*args, **kw)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(mb.input()[None, :])
        assert ei.value.code == -1 and re.search(r"node \d+ is a (LayerNorm|Softmax|Mha|GELU) layer \(kind 1[4-7]\)", str(ei.value)) and kind in str(ei.value), str(ei.value)
    finally:
        ctx.free()


def test_proofs_do_not_move(dev):
    """the proof words of an input before any infer call and after one are identical; the proof's output is infer's output"""
    import deep_prove_amd as dpa
    mb = dpa.models.mlp(2, 64, config=31)
    x = mb.input(1000)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        pr = dpa.Prover(ctx)
        p0, o0 = pr.prove(x)
        out, _ = ctx.infer(np.stack([x, mb.input(1001)]))
        p1, o1 = pr.prove(x)
        assert p0.size == p1.size and (p0 == p1).all() and (o0 == o1).all()
        assert (out[0] == o0).all()
        dpa.verify(ctx.verifier_blob(), p1, x, out[0])
    finally:
        ctx.free()


def test_in_flight_of_a_batch_does_not_depend_on_infer(dev):
    import deep_prove_amd as dpa
    mb = dpa.models.dense_4m()
    xs = np.stack([mb.input(1000 + i) for i in range(24)])
    seen = []
    for infer_first in (False, True):
        ctx = dpa.Context.generate(dev, mb.blob())
        try:
            if infer_first:
                ctx.infer(xs)
            pr = dpa.Prover(ctx)
            _, outs, _ = pr.prove_batch(xs, concurrency=24)
            seen.append(pr.in_flight())
            assert (outs[0] == mb.run(xs[0])).all()
        finally:
            ctx.free()
    assert seen[0] == seen[1] and seen[0] > 0, seen
