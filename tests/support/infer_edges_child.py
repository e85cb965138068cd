"""Child process of tests/test_gpu_zzzzzzzzzz_infer_edges.py, and the case builders that file shares with tests/test_host_inference_edges.py.
DP_INFER_LOG is read once per process, so which kernel served a call (gemm_i8 / gemm_i64, inputs as int8 / int64) is observed here: the child
runs a list of calls and the library prints one `[dp infer]` line per call to stderr, refused calls included.
usage: infer_edges_child.py <cases.npz> <out.npz>
  cases.npz: nmodels, ncalls, blob_<m>; per call c: model_<c> (non-decreasing), x_<c> [batch][input_len], mode_<c> (bit 0: all kinds, bit 1: checked)
  out.npz:   per call c: out_<c> (empty when the plain call was refused), error_<c> (its message, "" otherwise), reasons_<c> (checked calls)"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
WORDS = {"requant": 1, "vocabulary": 2, "gelu": 3, "layernorm": 4, "softmax": 5}  # the word of a class in the host's message -> DP_INFER_BAD_*
ALL_KINDS, CHECKED = 1, 2


def host(blob, xs, nout):
    """the yardstick: (rows[n, nout], reasons[n], messages[n]) of dp_model_infer_host on every input; a refused input has a zero row"""
    import deep_prove_amd as dpa

    def one(x):
        try:
            return dpa.infer_host(blob, x), 0, ""
        except dpa.DeepProveError as e:
            hits = [w for w in WORDS if w in str(e)]
            assert e.code == -1 and len(hits) == 1, str(e)
            return np.zeros(nout, dtype=np.int64), WORDS[hits[0]], str(e)
    with ThreadPoolExecutor(16) as ex:
        got = list(ex.map(one, xs))
    assert all(g[0].shape == (nout,) for g in got)
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.uint32), [g[2] for g in got]


# ---- (a) one product without a Requant behind it: the outputs are the exact sums

def extreme_rows(rng, n, k):
    """[n][k] uniform over -128..127 with -128 and 127 in every row (k == 1: the rows alternate between the two)"""
    w = rng.integers(-128, 128, size=(n, k), dtype=np.int64)
    for r in range(n):
        if k == 1:
            w[r, 0] = -128 if r % 2 == 0 else 127
        else:
            a, b = rng.choice(k, size=2, replace=False)
            w[r, a], w[r, b] = -128, 127
    return w


def gemm_model(kind, k, n, seq=1, bias=True, seed=0):
    """kind: dense | matmul | matmul_t (transpose_b) | qkv. k / n = 1 is the UNPADDED size: the library refuses padded dimensions below 2
    (validate_model), so such a matrix is zero padded to 2 as Tensor::pad_next_power_of_two does, and the kernel sees K (N) = 2 with one live
    column (row)"""
    import deep_prove_amd as dpa
    rng = np.random.default_rng(1000 * k + n + seed)
    kp, npad = max(k, 2), max(n, 2)

    def wt():  # [n][k], padded
        w = np.zeros((npad, kp), dtype=np.int64)
        w[:n, :k] = extreme_rows(rng, n, k)
        return w
    if kind == "dense":
        mb = dpa.models.ModelBuilder(kp, 120)
        mb.dense(npad, kp, requant=False)
        mb.layers[0]["weights"] = wt()
    elif kind in ("matmul", "matmul_t"):
        mb = dpa.models.ModelBuilder((seq, kp), 120)
        mb.matmul(npad, bias=bias, requant=False, transpose_b=kind == "matmul_t")
        mb.layers[0]["weights"] = wt() if kind == "matmul_t" else np.ascontiguousarray(wt().T)
    else:
        mb = dpa.models.GraphBuilder([seq * kp], 120)
        q = mb.qkv((-1, 0), kp, npad)
        mb.set_outputs([(q, 0), (q, 1), (q, 2)])
        mb.nodes[0][0]["weights"] = np.stack([np.ascontiguousarray(wt().T) for _ in range(3)])
    return mb


def gemm_inputs(mb, batch, seed=0):
    """[batch][input_len] uniform over -128..127, -128 and 127 in every sample"""
    return extreme_rows(np.random.default_rng(77 + seed + batch), batch, mb.input_len)


# the subset of K x N x batch (and the four other node forms) the tests run: every listed value appears at least once
GEMM_CASES = [("dense", 1, 1, 1, 1), ("dense", 2, 2, 1, 63), ("dense", 8, 16, 1, 64), ("dense", 16, 32, 1, 65), ("dense", 32, 64, 1, 129), ("dense", 64, 128, 1, 65),
              ("dense", 128, 128, 1, 129), ("dense", 128, 1, 1, 63), ("dense", 8, 128, 1, 1), ("matmul", 64, 32, 2, 65), ("matmul", 16, 16, 8, 63),
              ("matmul_t", 32, 64, 2, 64), ("qkv", 8, 16, 2, 65)]  # (kind, K, N, seq, batch)


def accumulator_model(log_k):
    """Dense 2^log_k -> 2, every weight -128, no bias: on inputs of -128 every sum is 2^(log_k + 14)"""
    import deep_prove_amd as dpa
    k = 1 << log_k
    mb = dpa.models.ModelBuilder(k, 121)
    mb.dense(2, k, requant=False)
    mb.layers[0]["weights"] = np.full((2, k), -128, dtype=np.int64)
    mb.layers[0]["bias"] = np.zeros(2, dtype=np.int64)
    return mb


def maxpool_model():
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder((2, 16, 16), 122)
    mb.conv(3, 3).maxpool().flatten().dense(5)  # (no ReLU: the MaxPool sees the signed output of the Requant)
    return mb


def large_inputs_model():
    """the model of test_host_inference.py::test_large_inputs_take_the_64_bit_path"""
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder((8, 4), 5)
    mb.matmul(16, requant=False).matmul(8, bias=False, requant=False)
    return mb


# ---- (d) - (h) a layer at the last value it accepts and the first it refuses

def requant_model():
    """Dense 8 -> 8 with the identity matrix and no bias + its Requant (intermediate_bit_size 18): the Requant sees the model input"""
    import deep_prove_amd as dpa
    mb = dpa.models.ModelBuilder(8, 123)
    mb.dense(8, 8)
    mb.layers[0]["weights"] = np.eye(8, dtype=np.int64)
    mb.layers[0]["bias"] = np.zeros(8, dtype=np.int64)
    assert mb.layers[1]["intermediate_bit_size"] == 18
    return mb


def requant_rounding_inputs(mb):
    """multiples k of s = (1 << sh) // (2 m) + 1, k = -320 .. 320 and the four largest within the bit size on both signs: k s m / 2^sh lies
    just above k / 2, so the odd k sit at the rounding of a half (negative ones included) and |k| >= 254 reaches the clamp at +-127"""
    l = mb.layers[1]
    sh, m, lim = l["fp_scale"] + l["right_shift"], l["fixed_point_multiplier"], 1 << l["intermediate_bit_size"]
    s = (1 << sh) // (2 * m) + 1
    kmax = lim // s
    assert kmax > 320
    ks = list(range(-320, 321)) + [sign * (kmax - d) for sign in (1, -1) for d in range(4)]
    v = np.array(ks + [0] * (-len(ks) % 8), dtype=np.int64) * s
    assert np.abs(v).max() <= lim
    return v.reshape(-1, 8)


def gelu_edges(l):
    """(lowest, highest) input of the GELU's table: rows -edge .. edge - 1 of input * multiplier, edge as models.gelu_apply computes it"""
    m = l["multiplier"]
    edge = 1 << (7 + (m - 1).bit_length())
    return -(edge // m), (edge - 1) // m


def ln_table_input(l, a):
    """the inverse-square-root table input of a row that alternates +-a over the dim_size (even) live features: sum 0, sum of squares dim_size a^2"""
    n = l["dim_size"]
    return (n * l["multiplier"] * n * a * a) >> l["range_check_bits"]


def ln_amplitudes(l):
    """(the largest amplitude whose alternating row stays inside the table, in < 2^14; the next one up)"""
    a = 1
    while ln_table_input(l, a + 1) < (1 << 14):
        a += 1
    return a, a + 1


def _poked(x, index, value):
    y = np.array(x, dtype=np.int64).copy()
    y.reshape(-1)[index] = value
    return y


class Edge:
    """a model with the inputs it accepts (`good` [n][input_len]) and those it refuses (`bad`: (input, word of the class, fragment of the message))"""

    def __init__(self, name, mb, all_kinds, good, bad):
        self.name, self.mb, self.all_kinds, self.good, self.bad = name, mb, all_kinds, np.stack(good), bad


def requant_edge():
    mb = requant_model()
    lim = 1 << 18
    base = mb.input(1000)
    good = [base, _poked(base, 3, lim), _poked(base, 0, -lim), _poked(_poked(base, 7, lim), 6, -lim)] + list(requant_rounding_inputs(mb))
    bad = [(_poked(base, i, v), "requant", "requant") for i, v in ((3, lim + 1), (0, -lim - 1), (7, I64_MAX), (5, I64_MIN))]
    return Edge("requant", mb, False, good, bad)


def gelu_edge(in_scale=None):
    import deep_prove_amd as dpa
    mb = dpa.models.gelu_only(16, config=31) if in_scale is None else dpa.models.gelu_only(16, config=31, in_scale=in_scale)
    lo, hi = gelu_edges(mb.layers[0])
    base = mb.input(1000)
    good = [base, _poked(base, 0, lo), _poked(base, 15, hi), _poked(_poked(base, 7, hi), 8, lo), np.linspace(lo, hi, 16).astype(np.int64)]
    bad = [(_poked(base, 2, hi + 1), "gelu", "gelu"), (_poked(base, 15, lo - 1), "gelu", "gelu")]
    return Edge("gelu" if in_scale is None else "gelu_%g" % in_scale, mb, True, good, bad)


def layernorm_edge(features):
    """layernorm_mlp(4, features, 16): rows of `features` padded to a power of two. Row 1 of the four carries the pattern, the others the ordinary input"""
    import deep_prove_amd as dpa
    mb = dpa.models.layernorm_mlp(4, features, 16, config=33)
    l = mb.layers[0]
    fd, n = l["dim"], l["dim_size"]
    base = mb.input(1000).reshape(4, fd)

    def with_row(row):
        y = base.copy()
        y[1, :] = 0
        y[1, :n] = row
        return y.reshape(-1)
    alt = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int64)
    a_in, a_out = ln_amplitudes(l)
    pairs = [(a_in, a_out)]
    if features == 128:  # multiplier 1040, range_check_bits 26: +-200 gives the table input 10 156, +-400 four times that
        assert l["multiplier"] == 1040 and l["range_check_bits"] == 26 and ln_table_input(l, 200) == 10156
        pairs.append((200, 400))
    good = [base.reshape(-1), with_row(np.full(n, 100)), with_row(np.full(n, -(1 << 20))), with_row(np.zeros(n, dtype=np.int64))] + [with_row(alt * a) for a, _ in pairs] + [with_row(-alt * a_in)]
    table, rng_ = "leaves its table", "input out of range"
    bad = [(with_row(alt * a), "layernorm", table) for _, a in pairs]
    one = np.zeros(n, dtype=np.int64)
    one[n - 1] = 1
    lim = 1 << 20
    bad += [(with_row(one * lim), "layernorm", table), (with_row(-one * lim), "layernorm", table), (with_row(one * (lim + 1)), "layernorm", rng_), (with_row(-one * (lim + 1)), "layernorm", rng_)]
    return Edge("layernorm_%d" % features, mb, True, good, bad)


def softmax_edge(n, in_scale=None):
    import deep_prove_amd as dpa
    mb = dpa.models.softmax_only(2, n, config=35) if in_scale is None else dpa.models.softmax_only(2, n, config=35, in_scale=in_scale)
    lim = 1 << 24
    base = mb.input(1000)
    last = base.size - 1
    alt = np.where(np.arange(base.size) % 2 == 0, lim, -lim).astype(np.int64)
    good = [base, _poked(base, n + 1, lim), _poked(base, last, -lim), np.full(base.size, lim, dtype=np.int64), alt, -alt]
    bad = [(_poked(base, n + 1, lim + 1), "softmax", "softmax"), (_poked(base, last, -lim - 1), "softmax", "softmax")]
    return Edge("softmax_%d%s" % (n, "" if in_scale is None else "_zero_tables"), mb, True, good, bad)


def token_edge():
    """token_mlp(4, 5, 8): a vocabulary of 5 padded to 8 rows; tokens 5, 6 and 7 read the zero rows of the padding"""
    import deep_prove_amd as dpa
    mb = dpa.models.token_mlp(4, 5, 8, config=72)
    assert mb.layers[0]["nrows"] == 8
    base = mb.input(1000)
    good = [base, _poked(base, 3, 7), _poked(base, 0, 7), np.full(4, 7, dtype=np.int64)]
    bad = [(_poked(base, 3, 8), "vocabulary", "vocabulary"), (_poked(base, 0, -1), "vocabulary", "vocabulary"), (_poked(base, 1, I64_MIN), "vocabulary", "vocabulary")]
    return Edge("token", mb, False, good, bad)


EDGES = {"requant": requant_edge, "gelu": gelu_edge, "gelu_1.4": lambda: gelu_edge(1.4 / 128.0), "layernorm_128": lambda: layernorm_edge(128), "layernorm_200": lambda: layernorm_edge(200),
         "layernorm_2": lambda: layernorm_edge(2), "softmax_4": lambda: softmax_edge(4), "softmax_4_zero_tables": lambda: softmax_edge(4, 8.0 / 127.0), "softmax_64": lambda: softmax_edge(64),
         "token": token_edge}


if __name__ == "__main__":
    import deep_prove_amd as dpa
    z = np.load(sys.argv[1])
    nmodels, ncalls = int(z["nmodels"]), int(z["ncalls"])
    res = {}
    dev = dpa.Device(0)
    c = 0
    for m in range(nmodels):
        ctx = dpa.Context.generate(dev, z["blob_%d" % m])
        try:
            while c < ncalls and int(z["model_%d" % c]) == m:
                x, mode = z["x_%d" % c], int(z["mode_%d" % c])
                res["error_%d" % c] = np.array("")
                try:
                    if mode & CHECKED:
                        res["out_%d" % c], res["reasons_%d" % c], _ = ctx.infer_checked(x, all_kinds=bool(mode & ALL_KINDS))
                    else:
                        res["out_%d" % c], _ = ctx.infer(x, all_kinds=bool(mode & ALL_KINDS))
                except dpa.DeepProveError as e:
                    assert e.code == -1, str(e)
                    res["out_%d" % c], res["error_%d" % c] = np.zeros((0, 0), dtype=np.int64), np.array(str(e))
                c += 1
        finally:
            ctx.free()
    assert c == ncalls
    dev.close()
    np.savez(sys.argv[2], **res)
    print("infer edges child ok", ncalls)
