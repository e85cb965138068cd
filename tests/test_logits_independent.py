"""The verifier of Logits::Argmax (layer kind 18) a SECOND time: tests/support/logits_independent.py (Python, from logits.rs:580-730, on the
independent field / Poseidon2 / transcript, sumcheck and logup verifiers of l0 / l1 / l2_independent.py) follows the product's stream — made by
tests/support/logits_check over the CPU double — through the whole transcript, and every claim it ends with is checked against the polynomial
itself (the maxima, the Requant columns recomputed here by numpy, the constant matrix, the range and clamping multiplicities, the input) and
opened by the independent Basefold verifier (l3_independent.py). A misreading of the reference shared by prove_logits and the library's verify
branch — the row / column split of the point, the order of the sparse-matrix point, what is absorbed before the challenge, the bit order of a
token — would have to be repeated in this unrelated formulation to go unnoticed."""
import numpy as np
import pytest

from support import logits_cases as LC

P = 0xFFFFFFFF00000001


def _describe(mb, x):
    """the chain as logits_independent.verify_lm_chain wants it, the model polynomials, every committed witness column and every looked-up value
    from a plain numpy forward pass"""
    from deep_prove_amd import models as M
    cur = np.asarray(x, dtype=np.int64)
    layers, cols, polys, lk = [], {}, {}, {"range": [], "clamping": {}}
    for i, l in enumerate(mb.layers):
        if l["kind"] == M.L_MATMUL:
            assert l["bias"] is None and not l["transpose_b"]
            layers.append(dict(kind="matmul", nrows=l["nrows"], ncols=l["ncols"]))
            polys[(i, "MatMulWeight")] = l["weights"].reshape(-1)
            cur = (cur.reshape(-1, l["nrows"]) @ l["weights"]).reshape(-1)
        elif l["kind"] == M.L_REQUANT:
            shift = l["fp_scale"] + l["right_shift"]
            cs = l["intermediate_bit_size"] + int(l["fixed_point_multiplier"] - 1).bit_length() - shift
            layers.append(dict(kind="requant", clamping_size=cs, **{q: l[q] for q in ("fp_scale", "right_shift", "fixed_point_multiplier")}))
            tmp = cur * l["fixed_point_multiplier"] + (1 << (shift - 1))
            cin = tmp >> shift
            masked = tmp & ((1 << shift) - 1)
            chunks = [(masked >> (8 * j)) & 255 for j in range(shift // 8)]
            cols[i] = [cin, np.clip(cin, -127, 127)] + chunks
            lk["clamping"].setdefault(cs, []).extend(int(v) for v in cin)
            for c in chunks:
                lk["range"].extend(int(v) for v in c)
            cur = np.clip(cin, -127, 127)
        else:
            assert l["kind"] == M.L_LOGITS
            layers.append(dict(kind="logits", rows=l["rows"], K=l["K"]))
            m = cur.reshape(l["rows"], l["K"])
            cols[i] = [m.max(axis=1)]                                   # the one committed polynomial: the maxima
            lk["range"].extend(int(v) for v in (m.max(axis=1)[:, None] - m).reshape(-1))  # what is looked up: max - x
            cur = m.argmax(axis=1)
    return layers, cols, polys, lk, cur


def _verify(oracle, name, tmp_path, tokens=None):
    """the product's stream of a case through the independent verifier (with `tokens` in place of the true output, if given) -> everything the
    checks below need"""
    from deep_prove_amd import wire
    from support import logits_independent as V
    mb, x = LC.cases()[name]
    layers, cols, polys, lk, y = _describe(mb, x)
    assert (y == mb.run(x)).all()
    sp = str(tmp_path / (name + ".stream"))
    r = LC.run_check(LC.check_bin(), "run", *LC.write_case(tmp_path, name, mb.blob(), x), sp, str(tmp_path / (name + ".out")))
    assert r.returncode == 0, r.stdout + r.stderr
    tree = wire.parse_stream(np.fromfile(sp, dtype="<u8"))
    # the PCS parameters follow the largest committed polynomial: the model input, the model polynomials, the tables, the witness columns
    sizes = [mb.input_len, 256] + [p.size for p in polys.values()] + [c[0].size for c in cols.values()] + [1 << l["clamping_size"] for l in layers if l["kind"] == "requant"]
    max_poly = 1 << (max(sizes) - 1).bit_length()
    to_words = lambda v: np.asarray([int(t) % P for t in np.asarray(v).reshape(-1)], dtype=np.uint64)
    roots = {}
    for (i, pid), poly in polys.items():
        roots.setdefault(i, []).append((pid, oracle.pcs_commit_root(max_poly, to_words(poly), False)))
    out = [int(v) for v in (y if tokens is None else tokens)]
    claims, tr = V.verify_lm_chain(layers, roots, tree, [int(v) for v in x], out)
    return mb, cols, polys, lk, roots, tree, max_poly, claims, tr


@pytest.mark.parametrize("name", ["logits_only_4x8", "lm_head_4x8x16"])
def test_independent_verifier_accepts_the_products_stream_and_every_claim_is_true(oracle, tmp_path, name):
    from support import l0_independent as L, l3_independent as V3
    mb, cols, polys, lk, roots, tree, max_poly, claims, tr = _verify(oracle, name, tmp_path)
    fe = lambda v: (int(v) % P, 0)
    counts = {"model": 0, "witness": 0, "multiplicity": 0}
    for c in claims:
        counts[c[0]] += 1
        if c[0] == "model":
            _, node, pid, point, ev = c
            assert L.mle_eval([fe(v) for v in polys[(node, pid)]], point) == ev, f"model claim {node} {pid}"
        elif c[0] == "witness":
            _, node, k, comm, point, ev = c
            assert comm[1] == int(cols[node][k].size).bit_length() - 1
            assert L.mle_eval([fe(v) for v in cols[node][k]], point) == ev, f"witness claim of node {node}, column {k}"
        else:
            _, table, comm, point, ev = c
            lo, hi, data = (0, 256, lk["range"]) if table[0] == "range" else (-(1 << (table[1] - 1)), 1 << (table[1] - 1), lk["clamping"][table[1]])
            mult = [0] * (hi - lo)
            for v in data:
                mult[v - lo] += 1
            assert L.mle_eval([fe(v) for v in mult], point) == ev, f"multiplicity claim of table {table}"
    n_req = sum(l["kind"] == 1 for l in mb.layers)
    assert counts["model"] == len(polys) and counts["multiplicity"] == 1 + n_req and counts["witness"] >= 1 + 5 * n_req, counts
    # ... and the openings, by the independent Basefold verifier, on the same transcript
    root_of = {(node, pid): r for node, lst in roots.items() for pid, r in lst}
    uniform = []
    for c in claims:
        if c[0] == "model":
            uniform.append(({"root": root_of[(c[1], c[2])], "num_vars": int(polys[(c[1], c[2])].size).bit_length() - 1}, c[3], c[4]))
        elif c[0] == "witness":
            uniform.append(({"root": list(c[3][0]), "num_vars": c[3][1]}, c[4], c[5]))
        else:
            uniform.append(({"root": list(c[2][0]), "num_vars": c[2][1]}, c[3], c[4]))
    trivial = [u for u in uniform if len(u[1]) <= V3.BASECODE_LOG]
    batch = [u for u in uniform if len(u[1]) > V3.BASECODE_LOG]
    assert len(trivial) == len(tree["trivial_proofs"]) and len(trivial) >= 1  # (the maxima: a polynomial of `rows` entries is opened by showing it)
    for (comm, point, ev), tp in zip(trivial, tree["trivial_proofs"]):
        V3.trivial_verify(comm, point, ev, tp)
    assert len(batch) >= 1  # (the range table's multiplicities)
    V3.batch_verify(max_poly.bit_length() - 1, [u[0] for u in batch], [u[1] for u in batch], [u[2] for u in batch], tree["batch_proof"], tr)


@pytest.mark.parametrize("name", ["logits_only_4x8", "lm_head_4x8x16"])
def test_independent_verifier_refuses_wrong_tokens_at_the_output_evaluation(oracle, tmp_path, name):
    mb, x = LC.cases()[name]
    y = mb.run(x)
    k = mb.layers[-1]["K"]
    forged = [(0, (int(y[0]) + 1) % k)]  # a token of the row that is not its argmax
    if name == "logits_only_4x8":
        forged.append((1, 3))            # the SECOND occurrence of the tied maximum of row 1
    for row, token in forged:
        bad = y.copy()
        bad[row] = token
        with pytest.raises(AssertionError, match="Output claim evaluation check failed for Logits layer"):
            _verify(oracle, name, tmp_path, tokens=bad)
    bad = y.copy()
    bad[0] = k
    with pytest.raises(AssertionError, match="token outside the row"):
        _verify(oracle, name, tmp_path, tokens=bad)
