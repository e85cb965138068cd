"""TEST INFRASTRUCTURE — the verifier of Logits::Argmax a second time: LogitsCtx::verify and verify_output_evaluation written in Python from
zkml/src/layers/transformer/logits.rs:580-730 (split_claim_point :134-143, squeeze_challenge :147-156), on the independent field / Poseidon2 /
transcript of l0_independent.py, the sumcheck verifier of l1_independent.py and the helpers of l2_independent.py (verify_logup, identity_eval,
the table closed forms). Nothing here is derived from csrc/*: it is a second READING of the reference — which coordinates of the lookup's point
address the rows, the order of the sparse-matrix point, what is absorbed before the batching challenge, the division, the bit order of a token.
One deliberate difference from the reference's text, the one the library's verifier makes too: the output-claim challenges ARE drawn
(Verifier::verify would draw none for this layer outside cfg(test), logits.rs:680-690, while Prover::prove draws them, iop/prover.rs:423-435).
l2_independent.verify_chain / verify_graph cannot be extended from outside, so the preamble of Verifier::verify (iop/verifier.rs:72-318: model
roots, table challenges, the lookup fractions, the output claims, the table proofs, the input claim, the fraction sum) is restated here for
chains of MatMul (constant matrix) / Requant / Logits nodes, with the MatMul and Requant branches read again from layers/matrix_mul.rs:1048-1139
and layers/requant.rs:692-817. Like l2 it does not open commitments: it RETURNS every claim for the test to check on the polynomial itself."""
from . import l0_independent as L
from . import l1_independent as L1
from .l2_independent import (BIT_LEN, ONE, ZERO, add, append_ext, challenge, e, eq_xy_eval, fe, identity_eval, mul, read_challenges, sub, table_column_evals,
                             table_order_key, verify_logup)


def bits_le(v, n):
    """to_bit_sequence_le (logits.rs:717-719): bit k of v for k = 0 .. n - 1, as field elements"""
    return [fe((v >> k) & 1) for k in range(n)]


def verify_logits(lp, node, rows, k, constant, tr, tokens, out):
    """LogitsCtx::verify (logits.rs:580-678) on the parsed LogitsProof `lp`; `tokens`: the model's one output tensor (io.output[0]). Appends the
    witness claim on the maxima to `out` and returns the claim on the node's input"""
    claims, _, _ = verify_logup(lp["logup_proof"], 1, constant, ONE, tr)  # TableType::Range: column separation challenge one
    assert len(claims) == 1, "Expected 1 claim for logup when verifying Logits layer"
    point, ev = claims[0]["point"], claims[0]["eval"]
    nrv, nkv = rows.bit_length() - 1, k.bit_length() - 1
    assert len(point) == nrv + nkv
    row_point = point[len(point) - nrv:]  # split_claim_point: the row variables are the most significant ones
    max_eval = e(lp["max_eval"])
    input_claim = {"point": point, "eval": sub(max_eval, ev)}
    c = lp["max_commitment"]
    out.append(("witness", node, 0, (tuple(c["root"]), c["num_vars"]), row_point, max_eval))
    # the vector of maxima -> the sparse matrix of maxima: sum_j reduced_m(j) * 1 = max_eval (degree 2: the second factor is the all-ones table, which
    # evaluates to one everywhere, so the final claim of the sumcheck IS the evaluation of the matrix)
    s1_point = [e(v) for v in lp["sumcheck_proof"]["point"]]
    _, expected = L1.verify_sumcheck(max_eval, s1_point, lp["sumcheck_proof"]["proofs"], nkv, 2, tr)
    max_mat_eval = e(lp["max_mat_eval"])
    assert expected == max_mat_eval, "Sparse-matrix Sumcheck evaluation failed when verifying Logits layer"
    max_mat_point = s1_point + row_point
    # squeeze_challenge: the input claim's point, then its evaluation, then one challenge
    for v in input_claim["point"]:
        append_ext(tr, v)
    append_ext(tr, input_claim["eval"])
    ch = tr.read_challenge()
    s2_point = [e(v) for v in lp["hadamard_proof"]["point"]]
    _, expected = L1.verify_sumcheck(add(max_mat_eval, mul(ch, input_claim["eval"])), s2_point, lp["hadamard_proof"]["proofs"], nrv + nkv, 3, tr)
    beta_eval = identity_eval(max_mat_point, s2_point)
    input_eq_eval = identity_eval(input_claim["point"], s2_point)
    input_eval = e(lp["input_eval"])
    divisor = mul(beta_eval, input_eval)
    assert divisor != ZERO, "Logits: zero divisor"
    expected_output_eval = mul(sub(expected, mul(mul(ch, input_eval), input_eq_eval)), L.ext_inv(divisor))
    # verify_output_evaluation (logits.rs:693-731)
    assert len(tokens) == rows, "Expected 1 output tensor of `rows` tokens"
    column_point, row_part = s2_point[:len(s2_point) - nrv], s2_point[len(s2_point) - nrv:]
    computed = ZERO
    for i, token in enumerate(tokens):
        assert 0 <= token < k, "Logits: token outside the row"
        b1 = identity_eval(row_part, bits_le(i, nrv))  # compute_betas_eval(row_point)[i]
        computed = add(computed, mul(b1, identity_eval(column_point, bits_le(token, nkv))))
    assert computed == expected_output_eval, "Output claim evaluation check failed for Logits layer"
    return {"point": s2_point, "eval": input_eval}


def verify_lm_chain(layers, model_roots, tree, x, y, label=b"m2vec"):
    """Verifier::verify for a chain whose LAST node is Logits. layers: dicts with kind in {'matmul' (nrows = inner dimension, ncols, no bias, not
    transposed), 'requant' (clamping_size, fp_scale, right_shift, fixed_point_multiplier), 'logits' (rows, K)}; model_roots: {node: [(poly id, root
    words)]}; x: the padded input, y: the tokens. Returns (claims in the order the commitment verifier gets them, transcript): ('model', node, poly id,
    point, eval), ('witness', node, k, (root, num_vars), point, eval), ('multiplicity', table, (root, num_vars), point, eval)"""
    assert layers[-1]["kind"] == "logits" and all(l["kind"] != "logits" for l in layers[:-1])
    tr = L.Transcript(label)
    for node in sorted(model_roots):
        for _, root in sorted(model_roots[node]):
            tr.append_field_elements([int(w) for w in root])
    tables = {("range", 0)}  # Logits::step_info inserts TableType::Range (logits.rs:242)
    for l in layers:
        if l["kind"] == "requant":
            tables.add(("clamping", l["clamping_size"]))
    tables = sorted(tables, key=table_order_key)
    constant = challenge(tr, b"table_constant")
    chmap = {t: (ONE if t[0] == "range" else challenge(tr, b"Clamping")) for t in tables}
    steps = {node: (kind, lp) for node, kind, lp in tree["steps"]}
    assert sorted(steps) == list(range(len(layers)))
    nums, dens = [], []

    def fractions(lg):
        for r in lg["circuit_outputs"]:
            r = [e(v) for v in r]
            nums.append(add(mul(r[0], r[3]), mul(r[1], r[2])))
            dens.append(mul(r[2], r[3]))

    for node, l in enumerate(layers):
        if l["kind"] == "requant":
            fractions(steps[node][1]["clamping_lookup"])
            fractions(steps[node][1]["shifted_lookup"])
        elif l["kind"] == "logits":
            fractions(steps[node][1]["logup_proof"])  # LogitsProof::get_lookup_data (logits.rs:78-81)
    for tp in tree["table_proofs"]:
        fractions(tp["lookup"])
    # the output claim: drawn as the prover draws it; the Logits node does not use it
    read_challenges(tr, len(y).bit_length() - 1)
    out, cur = [], None
    for node in range(len(layers) - 1, -1, -1):
        l, (kind, lp) = layers[node], steps[node]
        if l["kind"] == "logits":
            assert kind == 18
            cur = verify_logits(lp, node, l["rows"], l["K"], constant, tr, [int(v) for v in y], out)
        elif l["kind"] == "requant":  # layers/requant.rs:692-817, recombine_claims :499-529
            ct = ("clamping", l["clamping_size"])
            shift = l["fp_scale"] + l["right_shift"]
            cclaims, _, _ = verify_logup(lp["clamping_lookup"], 1, constant, chmap[ct], tr)
            sclaims, _, _ = verify_logup(lp["shifted_lookup"], shift // BIT_LEN, constant, ONE, tr)
            b = challenge(tr, b"requant_batching")
            cpt, spt = cclaims[0]["point"], sclaims[0]["point"]
            init, chp = ZERO, ONE
            for v in [cur["eval"], cclaims[1]["eval"], cclaims[0]["eval"]] + [c["eval"] for c in sclaims]:
                init, chp = add(init, mul(chp, v)), mul(chp, b)
            acc_pt = [e(v) for v in lp["io_accumulation"]["point"]]
            _, expected = L1.verify_sumcheck(init, acc_pt, lp["io_accumulation"]["proofs"], len(cpt), 2, tr)
            ae = [e(v) for v in lp["accumulation_evals"]]
            lb, cb, sb = eq_xy_eval(cur["point"], acc_pt), eq_xy_eval(cpt, acc_pt), eq_xy_eval(spt, acc_pt)
            calc, comb = mul(add(lb, mul(b, cb)), ae[1]), mul(b, b)
            calc, comb = add(calc, mul(mul(comb, cb), ae[0])), mul(comb, b)
            for v in ae[2:]:
                calc, comb = add(calc, mul(mul(v, sb), comb)), mul(comb, b)
            assert calc == expected, f"requant {node}: accumulation evaluations do not recombine"
            full, pw = mul(fe(1 << shift), ae[0]), ONE
            for v in ae[2:]:
                full, pw = add(full, mul(v, pw)), mul(pw, fe(1 << BIT_LEN))
            nxt = mul(sub(full, fe(1 << (shift - 1))), L.ext_inv(fe(l["fixed_point_multiplier"])))
            assert len(lp["commitments"]) == len(ae)
            for q, (v, c) in enumerate(zip(ae, lp["commitments"])):
                out.append(("witness", node, q, (tuple(c["root"]), c["num_vars"]), acc_pt, v))
            cur = {"point": acc_pt, "eval": nxt}
        else:  # layers/matrix_mul.rs:1048-1139, constant right matrix, no bias
            assert l["kind"] == "matmul" and lp["bias_eval"] is None
            nvc = l["ncols"].bit_length() - 1
            cols, rows = cur["point"][:nvc], cur["point"][nvc:]
            sc_point = [e(v) for v in lp["sumcheck"]["point"]]
            _, expected = L1.verify_sumcheck(cur["eval"], sc_point, lp["sumcheck"]["proofs"], l["nrows"].bit_length() - 1, 2, tr)
            ic = [e(v) for v in lp["individual_claims"]]
            assert mul(ic[0], ic[1]) == expected, "matmul: sumcheck claim failed"
            out.append(("model", node, "MatMulWeight", cols + sc_point, ic[1]))
            cur = {"point": sc_point + rows, "eval": ic[0]}
    assert len(tree["table_proofs"]) == len(tables)
    for tp, t in zip(tree["table_proofs"], tables):
        claims, _, _ = verify_logup(tp["lookup"], 1, constant, chmap[t], tr)
        out.append(("multiplicity", t, (tuple(tp["multiplicity_commit"]["root"]), tp["multiplicity_commit"]["num_vars"]), claims[0]["point"], claims[0]["eval"]))
        expect = table_column_evals(t[0], t[1], claims[0]["point"])
        assert len(expect) == len(claims) - 1
        for cl, ex in zip(claims[1:], expect):
            assert cl["eval"] == ex, f"table {t}: claimed column evaluation is wrong"
    assert len(cur["point"]) == len(x).bit_length() - 1 and L.mle_eval([fe(v) for v in x], cur["point"]) == cur["eval"], "input claim is incorrect"
    fn, fd = ZERO, ONE
    for nu, de in zip(nums, dens):
        fn, fd = add(mul(fn, de), mul(nu, fd)), mul(fd, de)
    assert fn == ZERO, "final logup numerator is not zero"
    assert fd != ZERO, "final logup denominator is zero"
    return out, tr
