"""dp_model_infer_host — the yardstick of every device inference test — at the edge values and shapes tests/test_gpu_zzzzzzzzzz_infer_edges.py
runs on the device: every accepted input gives the integers of the numpy inference (`mb.run`, which shares no code with the library), every
refused one raises DP_ERR_ARG with the word of its class. The cases are built by tests/support/infer_edges_child.py, shared with the GPU file.
INT64_MIN is part of them: |v| computed as `v < 0 ? -v : v` overflows there (undefined behaviour). The Requant's bit-size check then let the value
through and returned 0; the scans that decide on the int16 shortcut of Dense / MatMul / QKV saw a magnitude of 0 for it, and whether the value was
then multiplied or dropped (cast to an int16 0) depended on how the compiler had treated the overflow: a g++ build of zkml.h dropped it. The
magnitudes are unsigned now (abs_u64)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "support"))
import infer_edges_child as E  # noqa: E402

I64_MIN = E.I64_MIN


def _run_all(mb, xs):
    return np.stack([mb.run(x) for x in xs])


def _host_all(mb, xs):
    import deep_prove_amd as dpa
    blob = mb.blob()
    return np.stack([dpa.infer_host(blob, x) for x in xs])


@pytest.mark.parametrize("name", list(E.EDGES))
def test_last_accepted_and_first_refused_value(name):
    """Requant, GELU (two scales), LayerNorm (rows of 128, of 200 padded to 256, of 2), Softmax (rows of 4, with zero tables, of 64) and
    Embeddings at the last value each accepts and the first it refuses, on both signs"""
    import deep_prove_amd as dpa
    e = E.EDGES[name]()
    blob = e.mb.blob()
    for i, x in enumerate(e.good):
        assert (dpa.infer_host(blob, x) == e.mb.run(x)).all(), (name, i)
    for i, (x, word, fragment) in enumerate(e.bad):
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.infer_host(blob, x)
        assert ei.value.code == -1 and word in str(ei.value) and fragment in str(ei.value), (name, i, str(ei.value))


def test_requant_refuses_int64_min():
    """|INT64_MIN| is 2^63: beyond every intermediate bit size"""
    import deep_prove_amd as dpa
    mb = E.requant_model()
    x = mb.input(1000)
    x[5] = I64_MIN
    with pytest.raises(dpa.DeepProveError) as ei:
        dpa.infer_host(mb.blob(), x)
    assert ei.value.code == -1 and "requant" in str(ei.value)


@pytest.mark.parametrize("kind", ["dense", "matmul", "matmul_t", "qkv"])
def test_int64_min_next_to_small_values_is_multiplied_not_dropped(kind):
    """an INT64_MIN among inputs of -128..127 must not take the int16 shortcut: the sums are numpy's wrapped products (INT64_MIN times an odd
    weight is INT64_MIN, times an even one 0 — the column it meets holds both)"""
    mb = E.gemm_model(kind, 8, 16, seq=2)
    w = mb.layers[0]["weights"] if kind != "qkv" else mb.nodes[0][0]["weights"]
    col = 3  # (the input feature the value sits in)
    if kind == "qkv":
        w[:, col, 0], w[:, col, 1] = 127, -128
    elif kind == "matmul":
        w[col, 0], w[col, 1] = 127, -128
    else:  # [n][k]
        w[0, col], w[1, col] = 127, -128
    xs = E.gemm_inputs(mb, 3)
    xs[1, col] = I64_MIN
    want = _run_all(mb, xs)
    assert (np.abs(want[1]) > (1 << 62)).any() and (np.abs(want[1]) < (1 << 31)).any()  # (wrapped through the odd weight, gone through the even one)
    assert (_host_all(mb, xs) == want).all()


@pytest.mark.parametrize("kind,k,n,seq,batch", E.GEMM_CASES, ids=["%s_k%d_n%d_s%d_b%d" % c for c in E.GEMM_CASES])
def test_products_over_the_full_int8_range(kind, k, n, seq, batch):
    """weights and inputs over -128..127 with both extremes in every row (quantised_tensor never makes a -128)"""
    mb = E.gemm_model(kind, k, n, seq=seq, bias=(k, n) != (16, 16))
    xs = E.gemm_inputs(mb, min(batch, 5))
    assert xs.min() == -128 and xs.max() == 127
    assert (_host_all(mb, xs) == _run_all(mb, xs)).all()


def test_padded_dimensions_of_one_are_refused():
    """why K = 1 and N = 1 are run as matrices padded to 2: a Dense of one padded row or column is no valid model"""
    import deep_prove_amd as dpa
    for rows, cols in ((1, 2), (2, 1)):
        mb = dpa.models.ModelBuilder(cols, 120)
        mb.layers.append(dict(kind=dpa.models.L_DENSE, nrows=rows, ncols=cols, weights=np.full((rows, cols), -128, dtype=np.int64), bias=np.zeros(rows, dtype=np.int64)))
        with pytest.raises(dpa.DeepProveError) as ei:
            dpa.infer_host(mb.blob(), np.full(cols, -128, dtype=np.int64))
        assert ei.value.code == -4 and "dense" in str(ei.value)


@pytest.mark.parametrize("log_k", [16, 17])
def test_sums_of_two_to_the_30_and_31(log_k):
    mb = E.accumulator_model(log_k)
    xs = np.full((3, 1 << log_k), -128, dtype=np.int64)
    want = _run_all(mb, xs)
    assert (want == 1 << (log_k + 14)).all()
    assert (_host_all(mb, xs) == want).all()


def test_inputs_at_the_int8_boundary():
    mb = E.gemm_model("dense", 8, 8)
    for a, b in ((127, -128), (128, 0), (-129, 0)):
        xs = E.gemm_inputs(mb, 3)
        xs[1, 2], xs[1, 5] = a, b
        assert (_host_all(mb, xs) == _run_all(mb, xs)).all()


def test_maxpool_on_negative_data():
    mb = E.maxpool_model()
    xs = np.stack([mb.input(1000 + i) for i in range(3)])
    xs = np.concatenate([xs, -np.abs(xs) - 1])
    assert xs.min() == -128
    assert (_host_all(mb, xs) == _run_all(mb, xs)).all()


def test_products_wrap_around_64_bits():
    """inputs x 2^52 through two products without a Requant: the sums wrap, as numpy's int64 does; an INT64_MIN among them too"""
    mb = E.large_inputs_model()
    xs = np.stack([mb.input(1000 + i) for i in range(3)]) << 52
    xs[2, 5] = I64_MIN
    want = _run_all(mb, xs)
    l = mb.layers[0]
    exact = xs[0].reshape(-1, l["nrows"]).astype(object) @ l["weights"].astype(object) + l["bias"].astype(object)  # (Python integers)
    assert max(abs(int(v)) for v in exact.reshape(-1)) >= 1 << 63  # (the sums of the first product already leave 64 bits)
    assert (_host_all(mb, xs) == want).all()
