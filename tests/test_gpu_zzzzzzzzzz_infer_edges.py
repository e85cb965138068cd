"""The kernels of dp_model_infer / dp_model_infer_ex / dp_model_infer_checked (csrc/infer_kernels.inc) at the values and shapes where they can be
wrong: -128 on both sides of the i8 MFMA, the accumulator bound, the int8 / int64 upload choice at 127 | 128 and -128 | -129, LayerNorm rows
longer than a wave, every range check at the last value it accepts and the first it refuses, MaxPool on negative data, 64-bit wrap-around, and
the per-sample refusals of checked mode where a wave spans samples. Expected values of accepted inputs are always `mb.run(x)` (numpy), with
dp_model_infer_host as the second witness; for refused inputs dp_model_infer_host is the yardstick (E.host). Every comparison is exact equality.
Cases whose point is WHICH kernel ran go through tests/support/infer_edges_child.py with DP_INFER_LOG=1 and assert its `[dp infer]` lines.
tests/test_host_inference_edges.py pins the yardstick itself at the same cases."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "support", "infer_edges_child.py")
sys.path.insert(0, os.path.dirname(CHILD))
import infer_edges_child as E  # noqa: E402


def _numpy(mb, xs):
    return np.stack([mb.run(x) for x in xs])


def _child(tmp_path, calls, **env):
    """calls: [(model, inputs[batch][input_len], mode)] -> per call a dict: out, error, reasons, counts (launches by name), inputs ("int8" | "int64").
    env: further environment variables of the child"""
    models = []
    for mb, _, _ in calls:
        if not any(mb is m for m in models):
            models.append(mb)
    index = lambda mb: [i for i, m in enumerate(models) if m is mb][0]
    order = sorted(range(len(calls)), key=lambda c: index(calls[c][0]))  # (stable: the calls of a model keep their order)
    data = {"nmodels": len(models), "ncalls": len(calls)}
    for i, mb in enumerate(models):
        data["blob_%d" % i] = mb.blob()
    for pos, c in enumerate(order):
        data["model_%d" % pos], data["x_%d" % pos], data["mode_%d" % pos] = index(calls[c][0]), np.ascontiguousarray(calls[c][1], dtype=np.int64), calls[c][2]
    src, res = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    r = subprocess.run([sys.executable, CHILD, src, res], capture_output=True, text=True, timeout=600, env=dict(os.environ, DP_INFER_LOG="1", **env))
    assert r.returncode == 0 and "infer edges child ok" in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("[dp infer]")]
    assert len(lines) == len(calls), r.stderr[-2000:]
    z = np.load(res)
    got = [None] * len(calls)
    for pos, c in enumerate(order):
        counts = {k: int(v) for k, v in re.findall(r"(gemm_i8|gemm_i64|requant|maxpool|conv) (\d+)", lines[pos])}
        got[c] = dict(out=z["out_%d" % pos], error=str(z["error_%d" % pos]), reasons=z["reasons_%d" % pos] if "reasons_%d" % pos in z else None, counts=counts,
                      inputs=re.search(r"inputs as (int8|int64),", lines[pos]).group(1), line=lines[pos])
    return got


# ---- (a) k_infer_gemm_i8: shapes and extremes

def test_gemm_i8_shapes_with_both_extremes(tmp_path):
    """One product per model, no Requant behind it (the outputs are the exact sums; a Requant would clamp an error away), weights and inputs uniform
    over -128..127 with -128 and 127 in every weight row and every sample. The subset of K x N x batch, E.GEMM_CASES:
      Dense K 1, 2, 8 (the byte packing of infer_ld16, negative bytes), 16, 32 (less than a K slice), 64, 128 (one and two slices); N 1, 2, 16 (only wave
      column 0 has live columns), 32, 64, 128 (two tiles); batches 1, 63, 64, 65, 129 (M on either side of the 64-row tile, up to three tiles) —
      (K, N, batch) = (1, 1, 1) (2, 2, 63) (8, 16, 64) (16, 32, 65) (32, 64, 129) (64, 128, 65) (128, 128, 129) (128, 1, 63) (8, 128, 1);
      MatMul seq 2 (64 x 32, batch 65) and seq 8 (16 x 16, no bias, batch 63): the rows of a tile belong to different samples; MatMul with
      transpose_b (32 x 64, batch 64); a QKV node (8 x 16, seq 2, batch 65): the three b_is_nk = false copies.
    K = 1 / N = 1 are unpadded sizes: the library refuses padded dimensions below 2 (test_host_inference_edges.py::
    test_padded_dimensions_of_one_are_refused), so those matrices are zero padded to 2 and the kernel sees one live column / row of two.
    Every call must have run k_infer_gemm_i8 on int8 inputs: a sweep that fell back to the 64-bit kernel would prove nothing."""
    import deep_prove_amd as dpa
    models = [E.gemm_model(kind, k, n, seq=seq, bias=(k, n) != (16, 16)) for kind, k, n, seq, _ in E.GEMM_CASES]
    inputs = [E.gemm_inputs(mb, case[4]) for mb, case in zip(models, E.GEMM_CASES)]
    got = _child(tmp_path, [(mb, xs, 0) for mb, xs in zip(models, inputs)])
    for case, mb, xs, g in zip(E.GEMM_CASES, models, inputs, got):
        assert xs.min() == -128 and xs.max() == 127
        assert g["counts"]["gemm_i8"] == (3 if case[0] == "qkv" else 1) and g["counts"]["gemm_i64"] == 0 and g["inputs"] == "int8", (case, g["line"])
        want = _numpy(mb, xs)
        assert g["error"] == "" and g["out"].shape == want.shape and (g["out"] == want).all(), (case, np.argwhere(g["out"] != want)[:5])
        picks = sorted({0, len(xs) // 2, len(xs) - 1})
        assert (g["out"][picks] == np.stack([dpa.infer_host(mb.blob(), xs[i]) for i in picks])).all(), case


# ---- (b) the accumulator bound

def test_accumulator_bound(tmp_path):
    """Dense with K = 2^16, every weight and input -128: every sum is 2^30 and the i8 kernel serves it. K = 2^17: every sum is 2^31 — K * 128 * 128
    is no longer below 2^31 and the planner must send the product to the 64-bit kernel. Output width 2, batch 3"""
    calls = [(E.accumulator_model(lk), np.full((3, 1 << lk), -128, dtype=np.int64), 0) for lk in (16, 17)]
    got = _child(tmp_path, calls)
    for lk, (mb, xs, _), g, kernel in zip((16, 17), calls, got, ("gemm_i8", "gemm_i64")):
        assert g["counts"][kernel] == 1 and g["counts"]["gemm_i8"] + g["counts"]["gemm_i64"] == 1 and g["inputs"] == "int8", (lk, g["line"])
        assert g["error"] == "" and g["out"].shape == (3, 2) and (g["out"] == 1 << (lk + 14)).all(), (lk, g["out"])
        assert (g["out"] == _numpy(mb, xs)).all()


# ---- (c) the int8 / int64 upload choice

def test_inputs_at_the_int8_boundary(tmp_path):
    """Dense 8 -> 8 over the full weight range, no Requant, batch 3. Sample 1 holds a 127 and a -128: int8 upload, i8 kernel. A 128 or a -129
    in sample 1: int64 upload, 64-bit kernel (an off-by-one in the scan would turn 128 into -128 on the way)"""
    mb = E.gemm_model("dense", 8, 8)
    calls = []
    for a, b in ((127, -128), (128, 0), (-129, 0)):
        xs = np.clip(E.gemm_inputs(mb, 3), -127, 126)
        xs[1, 2], xs[1, 5] = a, b
        calls.append((mb, xs, 0))
    got = _child(tmp_path, calls)
    for (_, xs, _), g, (inputs, kernel) in zip(calls, got, (("int8", "gemm_i8"), ("int64", "gemm_i64"), ("int64", "gemm_i64"))):
        assert g["inputs"] == inputs and g["counts"][kernel] == 1 and g["counts"]["gemm_i8"] + g["counts"]["gemm_i64"] == 1, g["line"]
        assert g["error"] == "" and (g["out"] == _numpy(mb, xs)).all(), xs[1]
        assert (g["out"] == E.host(mb.blob(), xs, g["out"].shape[1])[0]).all()


# ---- (i) MaxPool on negative data

def test_maxpool_on_negative_data(tmp_path):
    """conv -> Requant -> MaxPool -> Flatten -> Dense without a ReLU: the MaxPool sees signed values and its int8 copy feeds the i8 kernel"""
    mb = E.maxpool_model()
    xs = np.stack([mb.input(1000 + i) for i in range(3)])
    xs = np.concatenate([xs, -np.abs(xs) - 1])
    got = _child(tmp_path, [(mb, xs, 0)])[0]
    assert got["counts"]["gemm_i8"] == 1 and got["counts"]["gemm_i64"] == 0 and got["counts"]["maxpool"] == 1 and got["inputs"] == "int8", got["line"]
    want = _numpy(mb, xs)
    assert got["error"] == "" and (got["out"] == want).all(), np.argwhere(got["out"] != want)[:5]
    assert (got["out"] == E.host(mb.blob(), xs, want.shape[1])[0]).all()
    pooled = np.stack([_run_to(mb, x, 3) for x in xs])  # (conv, Requant, MaxPool)
    assert pooled.min() < 0 < pooled.max()  # (the MaxPool's output does hold negative values)


def _run_to(mb, x, nlayers):
    """the numpy inference of the first `nlayers` layers"""
    import deep_prove_amd as dpa
    head = dpa.models.ModelBuilder(mb.input_shape_og, mb.config)
    head.layers = mb.layers[:nlayers]
    return head.run(x)


# ---- (d) - (h) every range check at its threshold, plain and checked

def _plain_and_checked(ctx, e):
    """e.good against numpy and the host in both modes; every refused input between two good ones: the plain call raises the host's message, the
    checked call gives the host's reason, a zero row and the neighbours' integers"""
    import deep_prove_amd as dpa
    blob = e.mb.blob()
    want = _numpy(e.mb, e.good)
    out, ms = ctx.infer(e.good, all_kinds=e.all_kinds)
    assert out.shape == want.shape and (out == want).all(), (e.name, np.argwhere(out != want)[:5])
    hrows, hreasons, _ = E.host(blob, e.good, want.shape[1])
    assert not hreasons.any() and (out == hrows).all() and ms > 0
    out, reasons, _ = ctx.infer_checked(e.good, all_kinds=e.all_kinds)
    assert not reasons.any() and (out == want).all(), (e.name, reasons)
    for i, (x, word, fragment) in enumerate(e.bad):
        xs = np.stack([e.good[0], x, e.good[1]])
        hrows, hreasons, msgs = E.host(blob, xs, want.shape[1])
        assert list(hreasons) == [0, E.WORDS[word], 0] and fragment in msgs[1], (e.name, i, msgs)
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(xs, all_kinds=e.all_kinds)
        assert ei.value.code == -1 and word in str(ei.value) and fragment in str(ei.value), (e.name, i, str(ei.value))
        out, reasons, _ = ctx.infer_checked(xs, all_kinds=e.all_kinds)
        assert (reasons == hreasons).all(), (e.name, i, reasons)
        assert (out == hrows).all() and not out[1].any() and (out[[0, 2]] == want[:2]).all(), (e.name, i)
    # all of them in one checked batch, good inputs in between
    xs = np.stack([v for j, (x, _, _) in enumerate(e.bad) for v in (x, e.good[j % len(e.good)])])
    hrows, hreasons, _ = E.host(blob, xs, want.shape[1])
    out, reasons, _ = ctx.infer_checked(xs, all_kinds=e.all_kinds)
    assert (reasons == hreasons).all() and (out == hrows).all(), (e.name, reasons, hreasons)
    assert list(reasons != 0) == [True, False] * len(e.bad)


@pytest.mark.parametrize("name", list(E.EDGES))
def test_last_accepted_and_first_refused_value(dev, name):
    """(the cases of E.EDGES, docstrings there)
    requant: Dense 8 -> 8 with the identity matrix, intermediate_bit_size 18: +-2^18 accepted, +-(2^18 + 1), INT64_MAX and INT64_MIN refused; multiples
      of (1 << sh) // (2 m) + 1 on both signs: the rounding of negative halves, up to the clamp at +-127.
    gelu, gelu_1.4: gelu_only(16) at the multipliers 32 and 45: the first and last input whose scaled value has a table row (-128 | 127 for 32) accepted, one
      beyond refused; the edge is computed as models.gelu_apply does.
    layernorm_128 / _200 / _2: layernorm_mlp(4, f, 16), rows of 128, of 200 padded to 256 (dim_size < fd), of 2. A constant row (100, and -2^20: the two
      products of the variance wrap around 64 bits and still cancel), a zero row, rows alternating +-a for the largest a whose table input stays below
      2^14 (f = 128: also +-200, table input 10 156) accepted; a + 1 (f = 128: also +-400) and a single +-2^20 refused with "leaves its table", a
      single +-(2^20 + 1) with "input out of range".
    softmax_4 / _4_zero_tables / _64: softmax_only(2, n) (in_scale 8 / 127: with zero tables): single elements of +-2^24, a sample of 2^24 everywhere, samples
      alternating +-2^24 accepted; +-(2^24 + 1) refused, under the causal mask too.
    token: token_mlp(4, 5, 8), the vocabulary padded to 8: token 7 accepted, 8, -1 and INT64_MIN refused."""
    import deep_prove_amd as dpa
    e = E.EDGES[name]()
    ctx = dpa.Context.generate(dev, e.mb.blob())
    try:
        _plain_and_checked(ctx, e)
    finally:
        ctx.free()


@pytest.mark.parametrize("features", [128, 200, 2])
def test_layernorm_rows_on_either_side_of_a_wave(dev, features):
    """layernorm_mlp(4, features, 16) on ordinary inputs, batches of 1, 3 and 65: rows of 128 and 256 words make a second (and fourth) trip through
    the lane loops of k_infer_layernorm, rows of 2 leave 62 lanes idle; 200 of 256 features are live (dim_size < fd)"""
    import deep_prove_amd as dpa
    mb = dpa.models.layernorm_mlp(4, features, 16, config=33)
    assert mb.layers[0]["dim"] == dpa.models.next_pow2(features) and mb.layers[0]["dim_size"] == features
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(65)])
    want = _numpy(mb, xs)
    assert len({w.tobytes() for w in want}) > 1
    assert (E.host(blob, xs, want.shape[1])[0] == want).all()
    ctx = dpa.Context.generate(dev, blob)
    try:
        for batch in (1, 3, 65):
            out, _ = ctx.infer(xs[:batch], all_kinds=True)
            assert out.shape == want[:batch].shape and (out == want[:batch]).all(), (features, batch, np.argwhere(out != want[:batch])[:5])
        out, reasons, _ = ctx.infer_checked(xs, all_kinds=True)
        assert not reasons.any() and (out == want).all()
    finally:
        ctx.free()


# ---- (j) wrap-around

def test_products_wrap_around_64_bits(dev):
    """the large_inputs model (two products, no Requant) on inputs x 2^52, an INT64_MIN among them: numpy's int64 wrap-around"""
    import deep_prove_amd as dpa
    mb = E.large_inputs_model()
    xs = np.stack([mb.input(1000 + i) for i in range(3)]) << 52
    xs[2, 5] = E.I64_MIN
    want = _numpy(mb, xs)
    l = mb.layers[0]
    exact = xs[0].reshape(-1, l["nrows"]).astype(object) @ l["weights"].astype(object) + l["bias"].astype(object)
    assert max(abs(int(v)) for v in exact.reshape(-1)) >= 1 << 63  # (the sums of the first product already leave 64 bits)
    ctx = dpa.Context.generate(dev, mb.blob())
    try:
        out, _ = ctx.infer(xs)
        assert (out == want).all(), np.argwhere(out != want)[:5]
        assert (out == E.host(mb.blob(), xs, want.shape[1])[0]).all()
    finally:
        ctx.free()


# ---- (k) infer_flag where a wave spans samples (checked mode)

def _checked_equals_host(ctx, blob, xs, all_kinds, refused):
    out, reasons, _ = ctx.infer_checked(xs, all_kinds=all_kinds)
    hrows, hreasons, _ = E.host(blob, xs, out.shape[1])
    assert [i for i, r in enumerate(hreasons) if r] == refused, hreasons  # (the pattern is what it is meant to be)
    assert (reasons == hreasons).all(), (reasons, hreasons)
    assert (out == hrows).all(), np.argwhere(out != hrows)[:5]


def _flag_case(kernel):
    """(edge, words per sample on the device, input index behind its last / its first word, a value the kernel refuses)"""
    if kernel == "gelu":
        g = E.gelu_edge()
        return g, 16, 15, 0, E.gelu_edges(g.mb.layers[0])[1] + 1
    if kernel == "requant":
        return E.requant_edge(), 8, 7, 0, (1 << 18) + 1
    if kernel == "token":
        return E.token_edge(), 4 * 8, 3, 0, 8
    return E.softmax_edge(4), 2 * 4 * 4, 31, 0, (1 << 24) + 1


@pytest.mark.parametrize("kernel", ["gelu", "requant", "token", "softmax"])
def test_refusals_where_a_wave_spans_samples(dev, kernel):
    """fewer than 64 words per sample, batch 8, so a wave of an element-wise kernel holds several samples. Three calls: samples 2 and 3 bad at their
    last and their first word only (adjacent bad lanes of two samples: one atomic per run would miss sample 3 without the `i % per == 0` clause);
    every word of samples 4 to 7 bad; only the last word of the last sample bad. (Embeddings: a token is 8 words — the last / first token. Softmax: the
    host's shift step has refused such a sample before k_infer_softmax sees it, so this case holds the step and the kernel to the same answer)"""
    import deep_prove_amd as dpa
    e, per, last, first, bad = _flag_case(kernel)
    assert per < 64
    blob = e.mb.blob()
    base = np.stack([e.mb.input(1000 + i) for i in range(8)])
    ctx = dpa.Context.generate(dev, blob)
    try:
        xs = base.copy()
        xs[2, last], xs[3, first] = bad, bad
        _checked_equals_host(ctx, blob, xs, e.all_kinds, [2, 3])
        xs = base.copy()
        xs[4:8, :] = bad
        _checked_equals_host(ctx, blob, xs, e.all_kinds, [4, 5, 6, 7])
        xs = base.copy()
        xs[7, last] = bad
        _checked_equals_host(ctx, blob, xs, e.all_kinds, [7])
    finally:
        ctx.free()


def test_a_bad_run_across_a_wave_boundary_inside_a_sample(dev):
    """128 words per sample (gelu_only(128)), batch 8: elements 60 to 70 of sample 3 are bad — the run crosses from one wave into the next"""
    import deep_prove_amd as dpa
    mb = dpa.models.gelu_only(128, config=31)
    bad = E.gelu_edges(mb.layers[0])[1] + 1
    blob = mb.blob()
    xs = np.stack([mb.input(1000 + i) for i in range(8)])
    xs[3, 60:71] = bad
    ctx = dpa.Context.generate(dev, blob)
    try:
        _checked_equals_host(ctx, blob, xs, True, [3])
        xs[5, 127], xs[6, 0] = bad, bad  # (and a run that ends a wave and a sample together)
        _checked_equals_host(ctx, blob, xs, True, [3, 5, 6])
    finally:
        ctx.free()


# ---- (l) what a plain call makes of the status words

@pytest.mark.parametrize("table_first", [True, False])
def test_both_layernorm_messages_in_one_chunk(dev, table_first):
    """layernorm_mlp(4, 2, 16), batch 4: inputs 1 and 2 are the layernorm_2 edge's first row that "leaves its table" and its single 2^20 + 1 row, in
    both orders, between two good inputs. The plain call names "input out of range" either way (the host's two LayerNorm messages keep their
    order, whichever sample comes first); the checked call knows one class for both"""
    import deep_prove_amd as dpa
    e = E.layernorm_edge(2)
    table = [x for x, _, fragment in e.bad if fragment == "leaves its table"][0]
    rng = [x for x, _, fragment in e.bad if fragment == "input out of range"][0]
    assert np.abs(rng).max() == (1 << 20) + 1
    xs = np.stack([e.good[0], table, rng, e.good[1]] if table_first else [e.good[0], rng, table, e.good[1]])
    blob = e.mb.blob()
    want = _numpy(e.mb, xs[[0, 3]])
    hrows, hreasons, msgs = E.host(blob, xs, want.shape[1])
    assert list(hreasons) == [0, 4, 4, 0] and sorted(("leaves its table" in m, "input out of range" in m) for m in msgs[1:3]) == [(False, True), (True, False)], msgs
    ctx = dpa.Context.generate(dev, blob)
    try:
        with pytest.raises(dpa.DeepProveError) as ei:
            ctx.infer(xs, all_kinds=True)
        assert ei.value.code == -1 and "layernorm: input out of range" in str(ei.value) and "table" not in str(ei.value), str(ei.value)
        out, reasons, _ = ctx.infer_checked(xs, all_kinds=True)
        assert list(reasons) == [0, 4, 4, 0] and (reasons == hreasons).all(), reasons
        assert not out[[1, 2]].any() and (out[[0, 3]] == want).all() and (out == hrows).all()
    finally:
        ctx.free()


def test_plain_call_refused_in_a_later_chunk(tmp_path):
    """gelu_only(128), batch 700 under a scratch bound of 1 MB (three chunks at least): one refused value in the last input. The plain call raises
    the GELU's message — after the chunks before it went through —, the same batch without the value gives numpy's rows, the checked call refuses
    exactly that input"""
    import deep_prove_amd as dpa
    mb = dpa.models.gelu_only(128, config=31)
    good = np.stack([mb.input(1000 + i) for i in range(700)])
    bad = good.copy()
    bad[699, 77] = E.gelu_edges(mb.layers[0])[1] + 1
    plain, refused, checked = _child(tmp_path, [(mb, good, E.ALL_KINDS), (mb, bad, E.ALL_KINDS), (mb, bad, E.ALL_KINDS | E.CHECKED)], DP_INFER_SCRATCH_MB="1")
    for g in (plain, refused, checked):
        m = re.search(r"batch 700 in (\d+) chunks of (\d+),", g["line"])
        assert m and int(m.group(1)) >= 3 and int(m.group(1)) == -(-700 // int(m.group(2))), g["line"]  # (the bad input sits in the last chunk, and the plain call got there)
    want = _numpy(mb, good)
    assert plain["error"] == "" and (plain["out"] == want).all()
    assert "gelu: input out of range" in refused["error"] and refused["out"].size == 0, refused["error"]
    hrows, hreasons, _ = E.host(mb.blob(), bad[696:], want.shape[1])
    assert list(hreasons) == [0, 0, 0, 3]
    assert checked["error"] == "" and list(checked["reasons"]) == [0] * 699 + [3] and not checked["out"][699].any() and (checked["out"][:699] == want[:699]).all()
    assert (checked["out"][696:] == hrows).all()
