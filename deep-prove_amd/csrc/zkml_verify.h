// The verifier of the model proofs (zkml/src/iop/verifier.rs:72-318; the layers' verify fns; commit/context.rs:424-599) — host only, as in
// the reference. It has the prover's shape: VerifyState is the counterpart of ProverState, verify_<layer> of prove_<layer> — each takes the
// claim(s) on the node's output(s) and returns the claim(s) it makes on the node's input(s) — and verify() is the driver that prove() is.
// Every verify_<layer> begins (state, node id, layer description, its proof member) like its prove_<layer>; a parameter a layer does not
// read is left unnamed, so the signature shows what the function touches.
// zkml.h (the prover) includes this header at its end: includers of zkml.h need nothing more.
#pragma once
#include "zkml.h"

namespace dp {

struct IO { std::vector<int64_t> input, output; };

// what the layers' verify functions share: the transcript, the table challenges, the claims left to the opening, the model commitments not yet consumed
struct VerifyState {
  const VerifierContext& vc; const Proof& proof; Transcript& t;
  VerifyState(const VerifierContext& vc_, const Proof& proof_, Transcript& t_) : vc(vc_), proof(proof_), t(t_) {}
  Ext constant_challenge = ex_zero(); std::map<TableType, Ext> chmap;
  std::vector<VerifyClaim> claims, trivial_claims;
  std::map<size_t, std::map<std::string, Commitment>> unused;  // model commitments no layer has taken yet
  std::map<TableType, Commitment> unused_tables;               // the same for the committed table columns
  std::vector<size_t> lens, in_lens;                           // per node: the length of its output tensor / of its (first) input tensor
  void add_claim(const Commitment& c, const Claim& cl) {
    VerifyClaim v{c, cl.point, cl.eval};
    if (cl.point.size() <= PCS_BASECODE_LOG) trivial_claims.push_back(v); else claims.push_back(v);
  }
};

// the LogUpProofs of a step, per layer kind, in the order their fractions enter the global check
template <class F> inline void for_each_lookup(const LayerProof& lp, F f) {
  if (lp.kind == L_RELU || lp.kind == L_GELU) f(lp.act.lookup);
  if (lp.kind == L_REQUANT) { f(lp.req.clamping_lookup); f(lp.req.shifted_lookup); }
  if (lp.kind == L_MAXPOOL) f(lp.pool.lookup);
  if (lp.kind == L_LOGITS) f(lp.logits.logup_proof);
  if (lp.kind == L_LAYERNORM) for (auto& lg : lp.ln.logup_proofs) f(lg);
  if (lp.kind == L_SOFTMAX || lp.kind == L_MHA) for (auto& lg : lp.sm.logup_proofs) f(lg);
}

// the verifier's own same_poly (commit/same_poly.rs:157-183), used by the activations and QKV
inline Claim same_poly_verify(Transcript& t, const std::vector<Claim>& sp_claims, const SamePolyProof& sp, unsigned nv) {
  DP_REQUIRE(sp.evals.size() == 2, DP_ERR_VERIFY, "same_poly: shapes");
  for (auto& c : sp_claims) DP_REQUIRE(c.point.size() == nv, DP_ERR_VERIFY, "same_poly: invalid claim length");
  std::vector<Ext> a = t.read_challenges(sp_claims.size());
  Ext y = ex_zero();
  for (size_t i = 0; i < a.size(); i++) y = ex_add(y, ex_mul(sp_claims[i].eval, a[i]));
  SubClaim sub = sumcheck_verify(y, sp.sumcheck, nv, 2, t);
  Ext computed = ex_zero();
  for (size_t i = 0; i < a.size(); i++) computed = ex_add(computed, ex_mul(a[i], identity_eval(sp_claims[i].point, sp.sumcheck.point)));
  DP_REQUIRE(ex_eq(computed, sp.evals[0]), DP_ERR_VERIFY, "same_poly: beta evaluation mismatch");
  DP_REQUIRE(ex_eq(ex_mul(sp.evals[0], sp.evals[1]), sub.expected_evaluation), DP_ERR_VERIFY, "same_poly: final evals invalid");
  return {sp.sumcheck.point, sp.evals[1]};
}

// MatMulCtx::verify_matmul (matrix_mul.rs:1048-1139), both operands inputs: no commitment, two claims out
inline std::vector<Claim> verify_matmul2(VerifyState& vs, size_t id, const LayerSpec& l, const MatMulProof& mp, const Claim& cur) {
  const size_t s_ = l.nrows ? vs.in_lens[id] / l.nrows : 0;
  const unsigned nvc = dp_ceil_log2(l.ncols), nvr = dp_ceil_log2(s_);
  DP_REQUIRE(is_pow2(s_) && cur.point.size() == nvc + nvr && mp.individual_claims.size() == 2 && !mp.has_bias, DP_ERR_VERIFY, "matmul2: shapes");
  std::vector<Ext> cols(cur.point.begin(), cur.point.begin() + nvc), rows(cur.point.begin() + nvc, cur.point.end());
  SubClaim sub = sumcheck_verify(cur.eval, mp.sumcheck, dp_ceil_log2(l.nrows), 2, vs.t);
  DP_REQUIRE(ex_eq(ex_mul(mp.individual_claims[0], mp.individual_claims[1]), sub.expected_evaluation), DP_ERR_VERIFY, "matmul2: sumcheck claim failed");
  std::vector<Ext> pl = sub.point; pl.insert(pl.end(), rows.begin(), rows.end());
  std::vector<Ext> pr;
  if (l.mm_transpose) { pr = sub.point; pr.insert(pr.end(), cols.begin(), cols.end()); } else { pr = cols; pr.insert(pr.end(), sub.point.begin(), sub.point.end()); }
  return {{pl, mp.individual_claims[0]}, {pr, mp.individual_claims[1]}};
}

// AddCtx::verify (add.rs:586-625) without operand
inline std::vector<Claim> verify_add2(VerifyState&, size_t, const LayerSpec& l, const AddProof& ap, const Claim& cur, size_t out_len) {
  DP_REQUIRE(cur.point.size() == dp_ceil_log2(out_len) && l.add_left > 0 && l.add_right > 0, DP_ERR_VERIFY, "add2: shapes");
  const Ext sum = ex_add(ex_mul_base(ap.left_eval, gl_from_i64(l.add_left)), ex_mul_base(ap.right_eval, gl_from_i64(l.add_right)));
  DP_REQUIRE(ex_eq(sum, cur.eval), DP_ERR_VERIFY, "Add layer verification failed");
  return {{cur.point, ap.left_eval}, {cur.point, ap.right_eval}};
}

// ConcatMatMulCtx::verify (concat_matmul.rs:801-892)
inline std::vector<Claim> verify_concat_matmul(VerifyState& vs, size_t, const LayerSpec& l, const ConcatMatMulProof& cp, const Claim& cur) {
  const CmShape g = cm_shape(l);
  DP_REQUIRE(cp.individual_claims.size() == 3, DP_ERR_VERIFY, "concat matmul: shapes");
  const unsigned nvm = dp_ceil_log2(g.M), nvs = dp_ceil_log2(g.C * g.M);
  SubClaim sub = sumcheck_verify(cur.eval, cp.sumcheck, nvs, 3, vs.t);
  CmPoint p;
  try { p = cm_split_point(l, g, cur.point); } catch (const DpError&) { DP_REQUIRE(false, DP_ERR_VERIFY, "concat matmul: claim point length"); }
  const std::vector<Ext> s_mm(sub.point.begin(), sub.point.begin() + nvm), s_concat(sub.point.begin() + nvm, sub.point.end());
  DP_REQUIRE(ex_eq(identity_eval(s_concat, p.concat), cp.individual_claims[0]), DP_ERR_VERIFY, "concat matmul: wrong evaluation of the beta table");
  DP_REQUIRE(ex_eq(ex_mul(ex_mul(cp.individual_claims[0], cp.individual_claims[1]), cp.individual_claims[2]), sub.expected_evaluation), DP_ERR_VERIFY, "concat matmul: sumcheck claim failed");
  return {{cm_input_point(l.cm_left, s_concat, s_mm, p.row), cp.individual_claims[1]}, {cm_input_point(l.cm_right, s_concat, s_mm, p.col), cp.individual_claims[2]}};
}

// QKVCtx::verify (qkv.rs:680-810): `got` are the claims on Q, K and V
inline std::vector<Claim> verify_qkv(VerifyState& vs, size_t id, const LayerSpec& l, const QKVProof& qp, const std::vector<Claim>& got) {
  const size_t s_ = l.nrows ? vs.in_lens[id] / l.nrows : 0;
  const unsigned nvc = dp_ceil_log2(l.ncols), nvr = dp_ceil_log2(s_), nvk = dp_ceil_log2(l.nrows);
  DP_REQUIRE(got.size() == 3 && is_pow2(s_) && qp.pre_bias_evals.size() == 3 && qp.individual_claims.size() == 6, DP_ERR_VERIFY, "qkv: shapes");
  static const char* const wn[3] = {"WeightQ", "WeightK", "WeightV"}; static const char* const bn[3] = {"BiasQ", "BiasK", "BiasV"};
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.size() == 6, DP_ERR_VERIFY, "qkv: six commitments expected for the node");
  for (int w = 0; w < 3; w++) DP_REQUIRE(nit->second.count(wn[w]) && nit->second.count(bn[w]) && got[w].point.size() == nvc + nvr, DP_ERR_VERIFY, "qkv: commitments / claim point length");
  std::vector<Ext> rows[3], cols[3];
  for (int w = 0; w < 3; w++) { cols[w].assign(got[w].point.begin(), got[w].point.begin() + nvc); rows[w].assign(got[w].point.begin() + nvc, got[w].point.end()); }
  for (int w = 0; w < 3; w++) { vs.t.append_exts(got[w].point); vs.t.append_ext(qp.pre_bias_evals[w]); }
  const Ext coeff[3] = {ex_one(), vs.t.read_challenge(), vs.t.read_challenge()};
  Ext batched = ex_zero();
  for (int w = 0; w < 3; w++) batched = ex_add(batched, ex_mul(qp.pre_bias_evals[w], coeff[w]));
  SubClaim sub = sumcheck_verify(batched, qp.sumcheck, nvk, 2, vs.t);
  std::vector<Claim> on_input(3), on_weight(3);
  Ext virt = ex_zero();
  for (int w = 0; w < 3; w++) {
    on_input[w].point = sub.point; on_input[w].point.insert(on_input[w].point.end(), rows[w].begin(), rows[w].end()); on_input[w].eval = qp.individual_claims[2 * w];
    on_weight[w].point = cols[w]; on_weight[w].point.insert(on_weight[w].point.end(), sub.point.begin(), sub.point.end()); on_weight[w].eval = qp.individual_claims[2 * w + 1];
    virt = ex_add(virt, ex_mul(ex_mul(qp.individual_claims[2 * w], qp.individual_claims[2 * w + 1]), coeff[w]));
  }
  // add_common_claims: the node's polynomials in BTreeMap order
  for (int w : {1, 0, 2}) vs.add_claim(nit->second.at(bn[w]), {cols[w], ex_sub(got[w].eval, qp.pre_bias_evals[w])});
  for (int w : {1, 0, 2}) vs.add_claim(nit->second.at(wn[w]), on_weight[w]);
  vs.unused.erase(nit);
  DP_REQUIRE(ex_eq(virt, sub.expected_evaluation), DP_ERR_VERIFY, "qkv: sumcheck claim failed");
  return {same_poly_verify(vs.t, on_input, qp.aggregation, dp_ceil_log2(vs.in_lens[id]))};
}

// the chain of iFFT delegation sumchecks of a convolution (convolution.rs:1141-1386); `last_point` is the point of the clearing sumcheck
inline void verify_ifft_delegation(Transcript& t, const ConvProof& cp, unsigned lfs, unsigned l2n, const std::vector<Ext>& last_point) {
  const size_t iter = cp.ifft_delegation_proof.size();
  DP_REQUIRE(iter == lfs && cp.ifft_delegation_claims.size() == iter && cp.ifft_claims.size() == 2 && cp.ifft_proof.point.size() == l2n, DP_ERR_VERIFY, "Inconsistency in iFFT delegation proofs/aux size");
  Ext claim = cp.ifft_claims[1];
  std::vector<u64> exps = pow_two_omegas((unsigned)iter + 1, true);
  std::vector<Ext> prev_r = cp.ifft_proof.point;
  for (size_t i = 0; i < iter; i++) {
    const IOPProof& dpf = cp.ifft_delegation_proof[i];
    sumcheck_verify(claim, dpf, (unsigned)(lfs - i), 3, t);
    DP_REQUIRE(cp.ifft_delegation_claims[i].size() == 3 && dpf.point.size() == lfs - i, DP_ERR_VERIFY, "ifft delegation: shapes");
    DP_REQUIRE(ex_eq(identity_eval(dpf.point, prev_r), cp.ifft_delegation_claims[i][0]), DP_ERR_VERIFY, "Error in identity evaluation ifft delegation");
    DP_REQUIRE(ex_eq(phi_eval(dpf.point, ex_sub(ex_one(), last_point[i]), prev_r.back(), exps, false), cp.ifft_delegation_claims[i][1]), DP_ERR_VERIFY, "Error in phi computation ifft delegation");
    prev_r = dpf.point; claim = cp.ifft_delegation_claims[i][2];
  }
  Ext scale = ex_inv(ex_from_u64(u64(1) << (iter + 1)));
  DP_REQUIRE(ex_eq(claim, ex_add(ex_mul(scale, prev_r[0]), ex_mul(scale, ex_sub(ex_one(), prev_r[0])))), DP_ERR_VERIFY, "Error in final iFFT delegation step");
}

// one chain of FFT delegation sumchecks (convolution.rs:1085-1139), of the input or of the weights; `hadamard_point` is the point of the hadamard sumcheck
inline void verify_fft_delegation(Transcript& t, unsigned lfs, const std::vector<Ext>& hadamard_point, Ext claim, const std::vector<IOPProof>& dproofs, const std::vector<std::vector<Ext>>& dclaims, std::vector<Ext> prev_r) {
  size_t it2 = dproofs.size();
  DP_REQUIRE(it2 == lfs && dclaims.size() == it2, DP_ERR_VERIFY, "Inconsistency in FFT delegation proofs/aux size");
  std::vector<u64> exps = pow_two_omegas((unsigned)it2 + 1, false);
  for (size_t i = 0; i < it2; i++) {
    sumcheck_verify(claim, dproofs[i], (unsigned)(lfs - i), 3, t);
    DP_REQUIRE(dclaims[i].size() == 3 && dproofs[i].point.size() == lfs - i, DP_ERR_VERIFY, "fft delegation: shapes");
    DP_REQUIRE(ex_eq(identity_eval(dproofs[i].point, prev_r), dclaims[i][0]), DP_ERR_VERIFY, "Error in identity evaluation fft delegation");
    DP_REQUIRE(ex_eq(phi_eval(dproofs[i].point, hadamard_point[i], prev_r.back(), exps, i == 0), dclaims[i][1]), DP_ERR_VERIFY, "Error in phi computation fft delegation");
    claim = dclaims[i][2]; prev_r = dproofs[i].point;
  }
  Ext hp = hadamard_point[it2];
  DP_REQUIRE(ex_eq(claim, ex_sub(ex_add(ex_mul(ex_sub(ex_one(), ex_dbl(hp)), prev_r[0]), ex_one()), prev_r[0])), DP_ERR_VERIFY, "Error in final FFT delegation step");
}

// ConvCtx::verify_convolution (convolution.rs:1141-1386)
inline Claim verify_conv(VerifyState& vs, size_t id, const LayerSpec& l, const ConvProof& cp, const Claim& cur) {
  size_t fs = l.filter_size();
  unsigned lfs = dp_ceil_log2(fs), lkw = dp_ceil_log2(l.kw), lkx = dp_ceil_log2(l.kx), l2n = lfs + 1;
  // hadamard::verify of the garbage clearing (hadamard.rs:133-162); the clearing tensor is public
  DP_REQUIRE(cur.point.size() == lfs + lkw && cp.clearing_proof.individual_claim.size() == 2, DP_ERR_VERIFY, "conv: shapes");
  SubClaim hsub = sumcheck_verify(cur.eval, cp.clearing_proof.sumcheck, lfs + lkw, 3, vs.t);
  { std::vector<int64_t> clr = clearing_tensor(l); std::vector<Ext> cv(clr.size()); for (size_t i = 0; i < cv.size(); i++) cv[i] = ex_from_i64(clr[i]);
    DP_REQUIRE(ex_eq(host_mle_eval(cv, cp.clearing_proof.sumcheck.point), cp.clearing_proof.individual_claim[1]), DP_ERR_VERIFY, "Hadamard verification failed for v2 eval"); }
  Ext hbeta = eq_eval(cur.point.data(), cp.clearing_proof.sumcheck.point.data(), cur.point.size());
  DP_REQUIRE(ex_eq(ex_mul(ex_mul(hbeta, cp.clearing_proof.individual_claim[0]), cp.clearing_proof.individual_claim[1]), hsub.expected_evaluation), DP_ERR_VERIFY, "Hadamard verification failed for product eval");
  Claim last{cp.clearing_proof.sumcheck.point, cp.clearing_proof.individual_claim[0]};
  Ext conv_claim = ex_sub(last.eval, cp.bias_claim);
  // NOTE (reference behaviour, replicated): the sub-claims of the FFT / iFFT / delegation sumchecks are not compared
  // with the products of the claimed evaluations; only the identity / phi closed forms and the chaining are checked
  sumcheck_verify(conv_claim, cp.ifft_proof, l2n, 2, vs.t);
  verify_ifft_delegation(vs.t, cp, lfs, l2n, last.point);
  sumcheck_verify(cp.ifft_claims[0], cp.hadamard_proof, lkx + l2n, 3, vs.t);
  DP_REQUIRE(cp.hadamard_clams.size() == 3 && cp.hadamard_proof.point.size() == lkx + l2n, DP_ERR_VERIFY, "conv: hadamard shapes");
  DP_REQUIRE(ex_eq(cp.hadamard_clams[2], identity_eval(cp.ifft_proof.point, cp.hadamard_proof.point)), DP_ERR_VERIFY, "Error in Beta evaluation");
  sumcheck_verify(cp.hadamard_clams[1], cp.fft_proof, l2n, 2, vs.t);
  DP_REQUIRE(cp.fft_claims.size() == 2 && cp.fft_proof.point.size() == l2n, DP_ERR_VERIFY, "conv: fft shapes");
  verify_fft_delegation(vs.t, lfs, cp.hadamard_proof.point, cp.fft_claims[1], cp.fft_delegation_proof, cp.fft_delegation_claims, cp.fft_proof.point);
  sumcheck_verify(cp.hadamard_clams[0], cp.fft_proof_weights, l2n, 2, vs.t);
  DP_REQUIRE(cp.fft_weight_claims.size() == 2 && cp.fft_proof_weights.point.size() == l2n, DP_ERR_VERIFY, "conv: fft weights shapes");
  verify_fft_delegation(vs.t, lfs, cp.hadamard_proof.point, cp.fft_weight_claims[1], cp.fft_delegation_proof_weights, cp.fft_delegation_weights_claims, cp.fft_proof_weights.point);
  // the padded-weights claim from the partial evaluations
  std::vector<Ext> weights_point = cp.fft_proof_weights.point;
  Ext v = ex_inv(ex_sub(ex_one(), weights_point.back())); weights_point.pop_back();
  DP_REQUIRE(cp.partial_evals.size() == l.real_nw * l.real_nw, DP_ERR_VERIFY, "conv: partial evaluations");
  Ext yw = ex_zero();
  for (size_t a = 0; a < l.real_nw; a++) for (size_t b = 0; b < l.real_nw; b++) {
    size_t num = a * l.nw + b; unsigned bl = 2 * dp_ceil_log2(l.nw);
    std::vector<Ext> bits(bl); for (unsigned q = 0; q < bl; q++) bits[q] = ex_from_u64((num >> q) & 1);
    yw = ex_add(yw, ex_mul(cp.partial_evals[a * l.real_nw + b], identity_eval(bits, weights_point)));
  }
  DP_REQUIRE(ex_eq(ex_mul(cp.fft_weight_claims[0], v), yw), DP_ERR_VERIFY, "Error in padded_fft evaluation claim");
  std::vector<Ext> weights_rand = vs.t.read_challenges(dp_ceil_log2(l.real_nw * l.real_nw));
  std::vector<Ext> point = cp.hadamard_proof.point; point.insert(point.end(), last.point.begin() + lfs, last.point.end());
  Claim bias_claim{std::vector<Ext>(last.point.begin() + lfs, last.point.end()), cp.bias_claim};
  Claim filter_claim; filter_claim.point = weights_rand; filter_claim.point.insert(filter_claim.point.end(), point.begin() + l2n, point.end());
  filter_claim.eval = host_mle_eval(cp.partial_evals, weights_rand);
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("ConvBias") && nit->second.count("ConvFilter"), DP_ERR_VERIFY, "conv: no commitments for node");
  vs.add_claim(nit->second.at("ConvBias"), bias_claim);
  vs.add_claim(nit->second.at("ConvFilter"), filter_claim);
  vs.unused.erase(nit);
  std::vector<Ext> input_point = cp.fft_proof.point;
  v = ex_inv(ex_sub(ex_one(), input_point.back())); input_point.pop_back();
  for (auto& ip : input_point) ip = ex_sub(ex_one(), ip);
  input_point.insert(input_point.end(), cp.hadamard_proof.point.begin() + l2n, cp.hadamard_proof.point.end());
  return {input_point, ex_mul(cp.fft_claims[0], v)};
}

// PoolingCtx::verify_pooling (pooling.rs:528-660)
inline Claim verify_pooling(VerifyState& vs, size_t, const LayerSpec&, const PoolingProof& pp, const Claim& cur, size_t out_len) {
  TableType rt{2, 0};
  DP_REQUIRE(vs.chmap.count(rt), DP_ERR_VERIFY, "pooling: no challenge for the range table");
  LogUpVerifierClaim vcl = verify_logup_proof(pp.lookup, 4, vs.constant_challenge, vs.chmap[rt], vs.t, 0);
  unsigned nv = dp_ceil_log2(out_len);
  Ext bc = vs.t.get_and_append_challenge("batch_pooling");
  DP_REQUIRE(vcl.claims.size() == 4 && pp.zerocheck_evals.size() == 5 && pp.commitments.size() == 5 && cur.point.size() == nv, DP_ERR_VERIFY, "pooling: shapes");
  Ext init = ex_zero(), comb = bc;
  for (auto& c : vcl.claims) { init = ex_add(init, ex_mul(c.eval, comb)); comb = ex_mul(comb, bc); }
  init = ex_add(init, ex_mul(comb, cur.eval));
  SubClaim sub = sumcheck_verify(init, pp.sumcheck, nv, 5, vs.t);
  DP_REQUIRE(vcl.claims[0].point.size() == nv, DP_ERR_VERIFY, "pooling: lookup point size");
  Ext beta_eval = eq_eval(vcl.claims[0].point.data(), sub.point.data(), nv);
  Ext last_beta_eval = eq_eval(cur.point.data(), sub.point.data(), nv);
  const size_t ks = 4;
  Ext prod = beta_eval, sum = ex_zero(); comb = bc;
  for (size_t i = 0; i < ks; i++) { prod = ex_mul(prod, pp.zerocheck_evals[i]); sum = ex_add(sum, ex_mul(comb, pp.zerocheck_evals[i])); comb = ex_mul(comb, bc); }
  Ext output_eval = pp.zerocheck_evals[ks];
  Ext expected = ex_add(ex_add(prod, ex_mul(sum, beta_eval)), ex_mul(ex_mul(output_eval, last_beta_eval), comb));
  DP_REQUIRE(ex_eq(expected, sub.expected_evaluation), DP_ERR_VERIFY, "Expected pooling zerocheck claim did not equal the verifier claim");
  for (size_t i = 0; i <= ks; i++) vs.add_claim(pp.commitments[i], {sub.point, pp.zerocheck_evals[i]});
  Ext r1 = vs.t.get_and_append_challenge("input_batching"), r2 = r1;
  Ext om1 = ex_sub(ex_one(), r1), om2 = ex_sub(ex_one(), r2);
  Ext mult[4] = {ex_mul(om1, om2), ex_mul(om1, r2), ex_mul(r1, om2), ex_mul(r1, r2)};
  DP_REQUIRE(pp.variable_gap <= sub.point.size(), DP_ERR_VERIFY, "pooling: variable gap");
  Claim next; next.point.push_back(r1);
  next.point.insert(next.point.end(), sub.point.begin(), sub.point.begin() + pp.variable_gap);
  next.point.push_back(r2);
  next.point.insert(next.point.end(), sub.point.begin() + pp.variable_gap, sub.point.end());
  next.eval = ex_zero();
  for (size_t i = 0; i < ks; i++) next.eval = ex_add(next.eval, ex_mul(ex_sub(output_eval, pp.zerocheck_evals[i]), mult[i]));
  return next;
}

// LogitsCtx::verify (logits.rs:580-730). The claim on the node's output was drawn where the prover drew it and is dropped: the output is checked against io.output itself.
inline Claim verify_logits(VerifyState& vs, size_t id, const LayerSpec& l, const LogitsProof& gp, const IO& io) {
  const ModelSpec& m = vs.vc.shape;
  TableType rt{2, 0};
  DP_REQUIRE(vs.chmap.count(rt), DP_ERR_VERIFY, "logits: no challenge for the range table");
  LogUpVerifierClaim vcl = verify_logup_proof(gp.logup_proof, 1, vs.constant_challenge, vs.chmap[rt], vs.t, 0);
  const size_t rows = l.nrows, K = l.ncols;
  const unsigned nvr = dp_ceil_log2(rows), nvk = dp_ceil_log2(K), nv = nvr + nvk;
  DP_REQUIRE(is_pow2(rows) && is_pow2(K) && rows >= 2 && K >= 2 && vs.in_lens[id] == rows * K && vcl.claims.size() == 1 && vcl.claims[0].point.size() == nv, DP_ERR_VERIFY, "logits: shapes");
  const Claim& dc = vcl.claims[0];
  const std::vector<Ext> row_point(dc.point.begin() + nvk, dc.point.end());
  const Claim input_claim{dc.point, ex_sub(gp.max_eval, dc.eval)};
  vs.add_claim(gp.max_commitment, {row_point, gp.max_eval});
  // the vector of maxima -> the sparse matrix of maxima: the second factor is the all-ones table, which evaluates to 1 everywhere
  SubClaim s1 = sumcheck_verify(gp.max_eval, gp.sumcheck_proof, nvk, 2, vs.t);
  DP_REQUIRE(ex_eq(s1.expected_evaluation, gp.max_mat_eval), DP_ERR_VERIFY, "logits: sparse-matrix sumcheck evaluation failed");
  std::vector<Ext> claim_point = s1.point; claim_point.insert(claim_point.end(), row_point.begin(), row_point.end());
  vs.t.append_exts(input_claim.point); vs.t.append_ext(input_claim.eval);  // squeeze_challenge (logits.rs:147-156)
  const Ext challenge = vs.t.read_challenge();
  SubClaim s2 = sumcheck_verify(ex_add(gp.max_mat_eval, ex_mul(challenge, input_claim.eval)), gp.hadamard_proof, nv, 3, vs.t);
  const Ext beta_eval = identity_eval(claim_point, s2.point), input_eq_eval = identity_eval(input_claim.point, s2.point);
  const Ext divisor = ex_mul(beta_eval, gp.input_eval);
  DP_REQUIRE(!ex_is_zero(divisor), DP_ERR_VERIFY, "logits: zero divisor in the output evaluation");
  const Ext expected_output_eval = ex_mul(ex_sub(s2.expected_evaluation, ex_mul(ex_mul(challenge, gp.input_eval), input_eq_eval)), ex_inv(divisor));
  // verify_output_evaluation (logits.rs:693-731): the one-hot matrix of the tokens of io.output — the model's only output tensor — at s2's point
  DP_REQUIRE(output_edges(m).size() == 1 && output_edges(m)[0].from == (int)id && io.output.size() == rows, DP_ERR_VERIFY, "logits: the node's output must be the model's only output tensor");
  const std::vector<Ext> col_pt(s2.point.begin(), s2.point.begin() + nvk), row_pt(s2.point.begin() + nvk, s2.point.end());
  const std::vector<Ext> beta = host_eq_table(row_pt);
  Ext computed = ex_zero();
  for (size_t i = 0; i < rows; i++) {
    DP_REQUIRE(io.output[i] >= 0 && (uint64_t)io.output[i] < K, DP_ERR_VERIFY, "logits: token outside the row");
    Ext sel = beta[i];
    for (unsigned b = 0; b < nvk; b++) sel = ex_mul(sel, ((io.output[i] >> b) & 1) ? col_pt[b] : ex_sub(ex_one(), col_pt[b]));
    computed = ex_add(computed, sel);
  }
  DP_REQUIRE(ex_eq(computed, expected_output_eval), DP_ERR_VERIFY, "logits: output claim evaluation check failed");
  return {s2.point, gp.input_eval};
}

// DenseCtx::verify_dense (dense.rs:576-643)
inline Claim verify_dense(VerifyState& vs, size_t id, const LayerSpec& l, const DenseProof& dpf, const Claim& cur) {
  DP_REQUIRE(cur.point.size() == dp_ceil_log2(l.nrows) && dpf.individual_claims.size() == 2, DP_ERR_VERIFY, "dense: shapes");
  Ext eval_no_bias = ex_sub(cur.eval, dpf.bias_eval);
  SubClaim sub = sumcheck_verify(eval_no_bias, dpf.sumcheck, dp_ceil_log2(l.ncols), 2, vs.t);
  std::vector<Ext> pt = sub.point; pt.insert(pt.end(), cur.point.begin(), cur.point.end());
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end(), DP_ERR_VERIFY, "dense: no commitments for node");
  vs.add_claim(nit->second.at("DenseBias"), {cur.point, dpf.bias_eval});
  vs.add_claim(nit->second.at("DenseWeight"), {pt, dpf.individual_claims[0]});
  vs.unused.erase(nit);
  DP_REQUIRE(ex_eq(ex_mul(dpf.individual_claims[0], dpf.individual_claims[1]), sub.expected_evaluation), DP_ERR_VERIFY, "dense: sumcheck claim failed");
  return {sub.point, dpf.individual_claims[1]};
}

// PositionalCtx::verify (positional.rs:480-583) over AddCtx::verify (add.rs:586-625, two inputs)
inline Claim verify_positional(VerifyState& vs, size_t id, const LayerSpec& l, const PositionalProof& pp, const Claim& cur, size_t out_len) {
  const unsigned nv_sub = (unsigned)cur.point.size(), nv_all = dp_ceil_log2(l.nrows * l.ncols);
  DP_REQUIRE(nv_sub == dp_ceil_log2(out_len) && nv_all >= nv_sub && pp.sub_matrix_evals.size() == nv_all - nv_sub && l.add_left > 0 && l.add_right > 0, DP_ERR_VERIFY, "positional: shapes");
  const Ext sum = ex_add(ex_mul_base(pp.add_proof.left_eval, gl_from_i64(l.add_left)), ex_mul_base(pp.add_proof.right_eval, gl_from_i64(l.add_right)));
  DP_REQUIRE(ex_eq(sum, cur.eval), DP_ERR_VERIFY, "Add layer verification failed");
  vs.t.append_exts(cur.point); vs.t.append_ext(cur.eval); vs.t.append_exts(cur.point); vs.t.append_ext(pp.add_proof.right_eval);
  std::vector<Ext> point = cur.point;
  Ext acc = pp.add_proof.right_eval;
  for (size_t k = 0; k < pp.sub_matrix_evals.size(); k++) {
    const Ext c = vs.t.read_challenge();
    point.push_back(c);
  }
  for (size_t k = 0; k < pp.sub_matrix_evals.size(); k++) { const Ext c = point[nv_sub + k]; acc = ex_add(ex_mul(acc, ex_sub(ex_one(), c)), ex_mul(pp.sub_matrix_evals[k], c)); }
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("PositionalMatrix"), DP_ERR_VERIFY, "positional: no commitment for the table");
  vs.add_claim(nit->second.at("PositionalMatrix"), {point, acc});
  vs.unused.erase(nit);
  return {cur.point, pp.add_proof.left_eval};
}

// EmbeddingsCtx::verify (embeddings.rs:473-528); the one-hot claim is checked at the very end
inline Claim verify_embeddings(VerifyState& vs, size_t id, const LayerSpec& l, const MatMulProof& ep, const Claim& cur, size_t out_len) {
  DP_REQUIRE(id == 0 && l.ncols && out_len % l.ncols == 0, DP_ERR_VERIFY, "embeddings: shapes");
  const size_t ntok = out_len / l.ncols;
  const unsigned nvc = dp_ceil_log2(l.ncols), nvr = dp_ceil_log2(ntok);
  DP_REQUIRE(is_pow2(ntok) && cur.point.size() == nvc + nvr && ep.individual_claims.size() == 2, DP_ERR_VERIFY, "embeddings: shapes");
  std::vector<Ext> col_pt(cur.point.begin(), cur.point.begin() + nvc), row_pt(cur.point.begin() + nvc, cur.point.end());
  SubClaim sub = sumcheck_verify(cur.eval, ep.sumcheck, dp_ceil_log2(l.nrows), 2, vs.t);
  std::vector<Ext> one_hot_pt = sub.point; one_hot_pt.insert(one_hot_pt.end(), row_pt.begin(), row_pt.end());
  std::vector<Ext> table_pt = col_pt; table_pt.insert(table_pt.end(), sub.point.begin(), sub.point.end());
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("EmbeddingMat"), DP_ERR_VERIFY, "embeddings: no commitment for the table");
  vs.add_claim(nit->second.at("EmbeddingMat"), {table_pt, ep.individual_claims[1]});
  vs.unused.erase(nit);
  DP_REQUIRE(ex_eq(ex_mul(ep.individual_claims[0], ep.individual_claims[1]), sub.expected_evaluation), DP_ERR_VERIFY, "embeddings: sumcheck claim failed");
  return {one_hot_pt, ep.individual_claims[0]};
}

// AddCtx::verify (add.rs:586-625), static operand
inline Claim verify_add(VerifyState& vs, size_t id, const LayerSpec& l, const AddProof& ap, const Claim& cur, size_t out_len) {
  DP_REQUIRE(cur.point.size() == dp_ceil_log2(out_len) && l.add_left > 0 && l.add_right > 0, DP_ERR_VERIFY, "add: shapes");
  const Ext sum = ex_add(ex_mul_base(ap.left_eval, gl_from_i64(l.add_left)), ex_mul_base(ap.right_eval, gl_from_i64(l.add_right)));
  DP_REQUIRE(ex_eq(sum, cur.eval), DP_ERR_VERIFY, "Add layer verification failed");
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("255"), DP_ERR_VERIFY, "add: no commitment for the operand");
  vs.add_claim(nit->second.at("255"), {cur.point, ap.right_eval});
  vs.unused.erase(nit);
  return {cur.point, ap.left_eval};
}

// MatMulCtx::verify_matmul (matrix_mul.rs:1048-1139), (Input, Weight), right matrix not transposed
inline Claim verify_matmul(VerifyState& vs, size_t id, const LayerSpec& l, const MatMulProof& mp, const Claim& cur, size_t out_len) {
  DP_REQUIRE(l.nrows && out_len % l.ncols == 0, DP_ERR_VERIFY, "matmul: shapes");
  const size_t s_ = out_len / l.ncols;
  const unsigned nvc = dp_ceil_log2(l.ncols), nvr = dp_ceil_log2(s_);
  DP_REQUIRE(is_pow2(s_) && cur.point.size() == nvc + nvr && mp.individual_claims.size() == 2, DP_ERR_VERIFY, "matmul: shapes");
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("MatMulWeight"), DP_ERR_VERIFY, "matmul: no commitments for node");
  const bool hb = nit->second.count("MatMulBias") != 0;
  DP_REQUIRE(mp.has_bias == hb, DP_ERR_VERIFY, "matmul: bias evaluation missing or unexpected");
  std::vector<Ext> pt_right(cur.point.begin(), cur.point.begin() + nvc), pt_left(cur.point.begin() + nvc, cur.point.end());
  Ext eval = cur.eval;
  if (hb) { vs.add_claim(nit->second.at("MatMulBias"), {pt_right, mp.bias_eval}); eval = ex_sub(eval, mp.bias_eval); }
  SubClaim sub = sumcheck_verify(eval, mp.sumcheck, dp_ceil_log2(l.nrows), 2, vs.t);
  std::vector<Ext> point_left = sub.point; point_left.insert(point_left.end(), pt_left.begin(), pt_left.end());
  std::vector<Ext> point_right = l.mm_transpose ? sub.point : pt_right;
  if (l.mm_transpose) point_right.insert(point_right.end(), pt_right.begin(), pt_right.end()); else point_right.insert(point_right.end(), sub.point.begin(), sub.point.end());
  vs.add_claim(nit->second.at("MatMulWeight"), {point_right, mp.individual_claims[1]});
  vs.unused.erase(nit);
  DP_REQUIRE(ex_eq(ex_mul(mp.individual_claims[0], mp.individual_claims[1]), sub.expected_evaluation), DP_ERR_VERIFY, "matmul: sumcheck claim failed");
  return {point_left, mp.individual_claims[0]};
}

// SoftmaxCtx::verify (softmax.rs:1274-1586); `out_len`: heads x rows x columns
inline Claim verify_softmax(VerifyState& vs, size_t, const LayerSpec& l, const SoftmaxProof& q, const Claim& cur, size_t out_len) {
  const bool zero = l.sm_zero_chunks != 0;
  const TableType st = softmax_table(l), et = softmax_error_table(l), zt{6, l.sm_zero_vars};
  DP_REQUIRE(q.logup_proofs.size() == (zero ? 4u : 3u) && vs.chmap.count(st) && vs.chmap.count(et) && (!zero || vs.chmap.count(zt)), DP_ERR_VERIFY, "softmax: lookups");
  std::vector<LogUpVerifierClaim> lc;
  lc.push_back(verify_logup_proof(q.logup_proofs[0], 1, vs.constant_challenge, vs.chmap[st], vs.t, 0));
  lc.push_back(verify_logup_proof(q.logup_proofs[1], 2, vs.constant_challenge, ex_one(), vs.t, 0));
  lc.push_back(verify_logup_proof(q.logup_proofs[2], 1, vs.constant_challenge, ex_one(), vs.t, 0));
  if (zero) lc.push_back(verify_logup_proof(q.logup_proofs[3], l.sm_zero_chunks, vs.constant_challenge, vs.chmap[zt], vs.t, 0));
  const size_t nz = 2 * l.sm_zero_chunks;
  DP_REQUIRE(lc[0].claims.size() == 2 && lc[1].claims.size() == 2 && lc[2].claims.size() == 1 && (!zero || lc[3].claims.size() == nz) && q.evaluations.size() == 5 + nz && q.commitments.size() == 5 + nz, DP_ERR_VERIFY, "softmax: shapes");
  const Ext alpha = vs.t.get_and_append_challenge("batching_challenge");
  Ext sum = ex_zero(), bc = ex_one();
  auto fold_in = [&sum, &bc, &alpha](const std::vector<Claim>& cs) { for (auto& c : cs) { sum = ex_add(sum, ex_mul(bc, c.eval)); bc = ex_mul(bc, alpha); } };
  fold_in(lc[0].claims); fold_in(lc[1].claims); if (zero) fold_in(lc[3].claims); fold_in(lc[2].claims);
  sum = ex_add(sum, ex_mul(bc, cur.eval));
  const std::vector<Ext>& exp_point = lc[0].claims[0].point; const std::vector<Ext>& range_point = lc[1].claims[0].point; const std::vector<Ext>& error_point = lc[2].claims[0].point;
  const unsigned nv = (unsigned)exp_point.size();
  DP_REQUIRE(range_point.size() == nv && error_point.size() <= nv && cur.point.size() == nv && nv == dp_ceil_log2(out_len) && (!zero || lc[3].claims[0].point.size() == nv), DP_ERR_VERIFY, "softmax: point sizes");
  const size_t extra = nv - error_point.size();
  DP_REQUIRE(extra == dp_ceil_log2(l.sm_shape[2]), DP_ERR_VERIFY, "softmax: the error lookup does not range over the rows");
  const Ext two_inv = ex_inv(ex_from_u64(2)), two_mult = ex_from_u64(u64(1) << extra);
  std::vector<Ext> full_error(extra, two_inv); full_error.insert(full_error.end(), error_point.begin(), error_point.end());
  SubClaim acc = sumcheck_verify(sum, q.accumulation_proof, nv, zero ? l.sm_zero_chunks + 2 : 2, vs.t);
  const Ext last_beta = eq_eval(cur.point.data(), acc.point.data(), nv), exp_beta = eq_eval(exp_point.data(), acc.point.data(), nv), range_beta = eq_eval(range_point.data(), acc.point.data(), nv), error_beta = eq_eval(full_error.data(), acc.point.data(), nv);
  const std::vector<Ext>& ev = q.evaluations;
  Ext calc = ex_zero(); bc = ex_one();
  for (size_t k = 0; k < 2; k++) { calc = ex_add(calc, ex_mul(ev[k], bc)); bc = ex_mul(bc, alpha); }
  calc = ex_mul(exp_beta, calc);
  for (size_t k = 2; k < 4; k++) { calc = ex_add(calc, ex_mul(ex_mul(range_beta, ev[k]), bc)); bc = ex_mul(bc, alpha); }
  Ext out_eval = ev[1];
  if (zero) {
    const Ext zbeta = eq_eval(lc[3].claims[0].point.data(), acc.point.data(), nv);
    for (size_t k = 5; k < ev.size(); k++) { calc = ex_add(calc, ex_mul(ex_mul(zbeta, ev[k]), bc)); bc = ex_mul(bc, alpha); }
    for (size_t k = 6; k < ev.size(); k += 2) out_eval = ex_mul(out_eval, ev[k]);
  }
  calc = ex_add(calc, ex_mul(ex_mul(bc, out_eval), ex_add(ex_mul(error_beta, two_mult), ex_mul(alpha, last_beta))));
  DP_REQUIRE(ex_eq(calc, acc.expected_evaluation), DP_ERR_VERIFY, "softmax: accumulation claim mismatch");
  // |masked input| = low + 2^8 high + 2^16 exp_in + 2^(16 + table vars) (zero_in_0 + 2^zero_vars zero_in_1 + ..)
  Ext mask_in = ex_add(ex_add(ex_mul(ev[0], ex_from_u64(u64(1) << 16)), ex_mul(ev[3], ex_from_u64(u64(1) << 8))), ev[2]);
  if (zero) { Ext mul = ex_from_u64(u64(1) << (16 + l.sm_table_size)); for (size_t k = 5; k < ev.size(); k += 2) { mask_in = ex_add(mask_in, ex_mul(ev[k], mul)); mul = ex_mul(mul, ex_from_u64(u64(1) << l.sm_zero_vars)); } }
  SubClaim mk_ = sumcheck_verify(ex_neg(mask_in), q.mask_proof, nv, 3, vs.t);
  const Ext eqv = eq_eval(mk_.point.data(), acc.point.data(), nv);
  const unsigned cols_v = dp_ceil_log2(l.sm_shape[2]), rows_v = dp_ceil_log2(l.sm_shape[1]);
  Ext tril_eval = ex_one();  // eval_zeroifier_mle (mha.rs:894-901)
  for (unsigned k = 0; k < cols_v && k < rows_v; k++) { const Ext c = mk_.point[k], r = mk_.point[cols_v + k]; tril_eval = ex_add(ex_mul(tril_eval, ex_add(ex_sub(ex_sub(ex_one(), c), r), ex_mul(ex_from_u64(2), ex_mul(c, r)))), ex_mul(ex_sub(ex_one(), c), r)); }
  const Ext neg_inf = ex_from_i64(-(((l.sm_bkm >> 16) + 1) << 16));
  const Ext mult_tril = ex_mul(eqv, tril_eval), mult_bias = ex_mul(eqv, ex_mul(neg_inf, ex_sub(ex_one(), tril_eval)));
  DP_REQUIRE(!ex_is_zero(mult_tril), DP_ERR_VERIFY, "softmax: degenerate mask point");
  const Ext shifted = ex_mul(ex_sub(mk_.expected_evaluation, mult_bias), ex_inv(mult_tril));
  const Ext input_eval = ex_mul(ex_sub(shifted, ev[4]), ex_inv(ex_from_i64(l.sm_scalar)));
  for (size_t k = 0; k < 4; k++) vs.add_claim(q.commitments[k], {acc.point, ev[k]});
  vs.add_claim(q.commitments[4], {std::vector<Ext>(mk_.point.begin() + extra, mk_.point.end()), ev[4]});
  for (size_t k = 5; k < ev.size(); k++) vs.add_claim(q.commitments[k], {acc.point, ev[k]});
  return {mk_.point, input_eval};
}

// LayerNormCtx::verify (layernorm.rs:1230-1505)
inline Claim verify_layernorm(VerifyState& vs, size_t id, const LayerSpec& l, const LayerNormProof& q, const Claim& cur) {
  const TableType it = layernorm_table(l);
  DP_REQUIRE(vs.chmap.count(it) && q.logup_proofs.size() == 2, DP_ERR_VERIFY, "layernorm: lookups");
  const size_t nrc = (l.ln_range_check_bits - 1) / Q_BIT_LEN + 1;
  LogUpVerifierClaim ic_ = verify_logup_proof(q.logup_proofs[0], 1, vs.constant_challenge, vs.chmap[it], vs.t, 0);
  LogUpVerifierClaim rc_ = verify_logup_proof(q.logup_proofs[1], nrc, vs.constant_challenge, ex_one(), vs.t, 0);
  DP_REQUIRE(ic_.claims.size() == 2 && rc_.claims.size() == nrc && q.acc_evals.size() == 2 + nrc && q.evaluations.size() == 4 + nrc && q.commitments.size() == 2 + nrc, DP_ERR_VERIFY, "layernorm: shapes");
  std::vector<Ext> bc; for (unsigned k = 0; k < dp_ceil_log2(2 + nrc); k++) bc.push_back(vs.t.get_and_append_challenge("batching"));
  const std::vector<Ext> rlc = host_eq_table(bc);
  Ext acc_init = ex_zero();
  for (size_t k = 0; k < 2 + nrc; k++) acc_init = ex_add(acc_init, ex_mul(k < 2 ? ic_.claims[k].eval : rc_.claims[k - 2].eval, rlc[k]));
  const unsigned nv = (unsigned)ic_.claims[0].point.size(), sdv = dp_ceil_log2(l.ln_dim_size);
  DP_REQUIRE(rc_.claims[0].point.size() == nv && cur.point.size() == nv + sdv, DP_ERR_VERIFY, "layernorm: point sizes");
  SubClaim acc = sumcheck_verify(acc_init, q.accumulation_proof, nv, 2, vs.t);
  const Ext eq_sqrt = eq_eval(ic_.claims[0].point.data(), acc.point.data(), nv), eq_range = eq_eval(rc_.claims[0].point.data(), acc.point.data(), nv);
  Ext calc = ex_zero();
  for (size_t k = 0; k < 2 + nrc; k++) calc = ex_add(calc, ex_mul(ex_mul(q.acc_evals[k], k < 2 ? eq_sqrt : eq_range), rlc[k]));
  DP_REQUIRE(ex_eq(calc, acc.expected_evaluation), DP_ERR_VERIFY, "layernorm: accumulation claim mismatch");
  // STRICTER THAN THE REFERENCE (layernorm.rs:1341-1480 has the same gap): the evaluations the two sumchecks reason about (acc_evals) must be
  // the ones opened against the witness commitments at acc.point (evaluations) — otherwise the inverse-square-root input and the range
  // chunks the protocol constrains are not bound to the committed columns. Honest proofs set them equal; the transcript is unchanged.
  for (size_t k = 0; k < 2 + nrc; k++) if (k != 1) DP_REQUIRE(ex_eq(q.acc_evals[k], q.evaluations[k]), DP_ERR_VERIFY, "layernorm: accumulation evaluation not bound to its commitment");
  const Ext c1 = vs.t.get_and_append_challenge("batching"), c2 = vs.t.get_and_append_challenge("batching");
  const Ext first = ex_mul(ex_sub(ex_one(), c1), ex_sub(ex_one(), c2)), second = ex_mul(c1, ex_sub(ex_one(), c2)), third = ex_mul(ex_sub(ex_one(), c1), c2);
  // the inverse-square-root input, shifted back up, plus the range-checked chunks (the top one divided by its scalar)
  Ext partial = ex_mul(q.acc_evals[0], ex_from_u64(u64(1) << l.ln_range_check_bits)), pw = ex_one();
  for (size_t k = 0; k + 1 < nrc; k++) { partial = ex_add(partial, ex_mul(q.acc_evals[2 + k], pw)); pw = ex_mul(pw, ex_from_u64(u64(1) << Q_BIT_LEN)); }
  const Ext top_inv = ex_inv(ex_from_u64(u64(1) << l.ln_top_chunk_scalar_log));
  const Ext io_init = ex_add(ex_add(ex_mul(first, ex_add(partial, ex_mul(ex_mul(q.acc_evals.back(), top_inv), pw))), ex_mul(second, cur.eval)), ex_mul(q.acc_evals[1], third));
  SubClaim io = sumcheck_verify(io_init, q.io_proof, nv + sdv, 4, vs.t);
  const Ext input_io = q.evaluations[q.evaluations.size() - 2], mean_io = q.evaluations.back(), inv_ev = q.evaluations[1];
  const Ext n_f = ex_from_u64(l.ln_dim_size), two_inv = ex_inv(ex_from_u64(2)), two_mul = ex_from_u64(u64(1) << sdv), mult_f = ex_from_i64(l.ln_multiplier);
  std::vector<Ext> full_point(sdv, two_inv); full_point.insert(full_point.end(), acc.point.begin(), acc.point.end());
  const Ext input_eq = eq_eval(full_point.data(), io.point.data(), io.point.size()), last_eq = eq_eval(cur.point.data(), io.point.data(), io.point.size());
  const Ext p1 = ex_mul(ex_mul(ex_mul(first, mult_f), input_eq), ex_sub(ex_mul(ex_mul(n_f, two_mul), ex_mul(input_io, input_io)), ex_mul(mean_io, mean_io)));
  const Ext p2 = ex_mul(ex_mul(second, last_eq), ex_add(ex_mul(ex_mul(inv_ev, q.gamma_eval), ex_sub(ex_mul(n_f, input_io), mean_io)), q.beta_eval));
  const Ext p3 = ex_mul(ex_mul(third, input_eq), inv_ev);
  DP_REQUIRE(ex_eq(ex_add(ex_add(p1, p2), p3), io.expected_evaluation), DP_ERR_VERIFY, "layernorm: io claim mismatch");
  const Ext ich = vs.t.get_and_append_challenge("batching");
  SubClaim in = sumcheck_verify(ex_add(input_io, ex_mul(ich, ex_sub(mean_io, input_io))), q.input_proof, nv + sdv, 2, vs.t);
  std::vector<Ext> sum_io(sdv, two_inv); sum_io.insert(sum_io.end(), io.point.begin() + sdv, io.point.end());
  const Ext eq_io = eq_eval(io.point.data(), in.point.data(), in.point.size()), eq_sum = eq_eval(sum_io.data(), in.point.data(), in.point.size());
  const Ext non_input = ex_add(eq_io, ex_mul(ich, ex_sub(ex_mul(two_mul, eq_sum), eq_io)));
  DP_REQUIRE(!ex_is_zero(non_input), DP_ERR_VERIFY, "layernorm: degenerate input point");
  for (size_t k = 0; k < 2 + nrc; k++) vs.add_claim(q.commitments[k], k == 1 ? Claim{std::vector<Ext>(io.point.begin() + sdv, io.point.end()), q.evaluations[k]} : Claim{acc.point, q.evaluations[k]});
  auto nit = vs.unused.find(id);
  DP_REQUIRE(nit != vs.unused.end() && nit->second.count("LayerNormBeta") && nit->second.count("LayerNormGamma"), DP_ERR_VERIFY, "layernorm: no commitments for node");
  const std::vector<Ext> gp(io.point.begin(), io.point.begin() + sdv);
  vs.add_claim(nit->second.at("LayerNormBeta"), {gp, q.beta_eval}); vs.add_claim(nit->second.at("LayerNormGamma"), {gp, q.gamma_eval});
  vs.unused.erase(nit);
  return {in.point, ex_mul(in.expected_evaluation, ex_inv(non_input))};
}

// verify_requant (requant.rs:692-817)
inline Claim verify_requant(VerifyState& vs, size_t, const LayerSpec& l, const RequantProof& rp, const Claim& cur) {
  TableType ct{3, l.clamping_size()};
  DP_REQUIRE(vs.chmap.count(ct), DP_ERR_VERIFY, "requant: no challenge for clamping table");
  size_t inst = l.shift() / Q_BIT_LEN;
  LogUpVerifierClaim cc = verify_logup_proof(rp.clamping_lookup, 1, vs.constant_challenge, vs.chmap[ct], vs.t, 0);
  LogUpVerifierClaim scl = verify_logup_proof(rp.shifted_lookup, inst, vs.constant_challenge, ex_one(), vs.t, 0);
  Ext b = vs.t.get_and_append_challenge("requant_batching");
  DP_REQUIRE(cc.claims.size() == 2 && scl.claims.size() == inst && rp.accumulation_evals.size() == 2 + inst && rp.commitments.size() == 2 + inst, DP_ERR_VERIFY, "requant: shapes");
  const std::vector<Ext>& cpt = cc.claims[0].point; const std::vector<Ext>& spt = scl.claims[0].point;
  Ext init = ex_zero(), chal = ex_one();
  std::vector<Ext> vals = {cur.eval, cc.claims[1].eval, cc.claims[0].eval};
  for (auto& c : scl.claims) vals.push_back(c.eval);
  for (const Ext& v : vals) { init = ex_add(init, ex_mul(chal, v)); chal = ex_mul(chal, b); }
  SubClaim sub = sumcheck_verify(init, rp.io_accumulation, (unsigned)cpt.size(), 2, vs.t);
  DP_REQUIRE(cur.point.size() == sub.point.size() && cpt.size() == sub.point.size() && spt.size() == sub.point.size(), DP_ERR_VERIFY, "requant: point sizes");
  Ext lb = eq_eval(cur.point.data(), sub.point.data(), sub.point.size());
  Ext cb = eq_eval(cpt.data(), sub.point.data(), sub.point.size());
  Ext sb = eq_eval(spt.data(), sub.point.data(), sub.point.size());
  const std::vector<Ext>& ae = rp.accumulation_evals;
  Ext calc = ex_mul(ex_add(lb, ex_mul(b, cb)), ae[1]);
  Ext comb = ex_mul(b, b);
  calc = ex_add(calc, ex_mul(ex_mul(comb, cb), ae[0]));
  comb = ex_mul(comb, b);
  for (size_t i = 2; i < ae.size(); i++) { calc = ex_add(calc, ex_mul(ex_mul(ae[i], sb), comb)); comb = ex_mul(comb, b); }
  DP_REQUIRE(ex_eq(calc, sub.expected_evaluation), DP_ERR_VERIFY, "requant: accumulation claim mismatch");
  Ext next = recombine_claims(l, ae[0], &ae[2], ae.size() - 2);
  for (size_t i = 0; i < ae.size(); i++) vs.add_claim(rp.commitments[i], {sub.point, ae[i]});
  return {sub.point, next};
}

// verify_activation (activation.rs:459-517): ReLU and GELU
inline Claim verify_activation(VerifyState& vs, size_t, const LayerSpec& l, const ActivationProof& ap, const Claim& cur, size_t out_len) {
  DP_REQUIRE(l.kind == L_RELU || l.kind == L_GELU, DP_ERR_VERIFY, "unknown layer kind");
  TableType rt = l.kind == L_GELU ? gelu_table(l) : TableType{0, 0};
  DP_REQUIRE(vs.chmap.count(rt), DP_ERR_VERIFY, "relu: no challenge for table");
  LogUpVerifierClaim vcl = verify_logup_proof(ap.lookup, 1, vs.constant_challenge, vs.chmap[rt], vs.t, 0);
  DP_REQUIRE(vcl.claims.size() == 2 && ap.commits.size() == 2 && ap.io_accumulation.evals.size() == 2, DP_ERR_VERIFY, "relu: shapes");
  // the claim on the output and the lookup's claim on it are two claims on one committed column
  const Claim new_out = same_poly_verify(vs.t, {cur, vcl.claims[1]}, ap.io_accumulation, dp_ceil_log2(out_len));
  vs.add_claim(ap.commits[0], vcl.claims[0]);
  vs.add_claim(ap.commits[1], new_out);
  Claim on_input = vcl.claims[0];
  if (l.kind == L_GELU) on_input.eval = ex_mul(on_input.eval, ex_inv(ex_from_i64(l.fixed_point_multiplier)));  // the claim on the input itself (:507-515)
  return on_input;
}

// MhaCtx::verify (mha.rs:792-893) is the verification of its three sub-layers one after the other — final_mul on the node's output claim, the
// softmax on final_mul's first claim, qk on the softmax's claim — handing on the claims on Q, K (from qk) and V (from final_mul)
inline std::vector<Claim> verify_mha(VerifyState& vs, size_t id, const LayerSpec& l, const LayerProof& mp, const Claim& cur) {
  // (the two size checks cannot fire — verify_concat_matmul returns two claims — and are kept with their messages as the reference has them)
  const std::vector<Claim> fm = verify_concat_matmul(vs, id, mha_final_spec(l), mp.mha_final, cur);
  DP_REQUIRE(fm.size() == 2, DP_ERR_VERIFY, "mha: final_mul claims");
  const Claim sc = verify_softmax(vs, id, mha_softmax_spec(l), mp.sm, fm[0], l.mha_shape[1] * l.mha_shape[0] * l.mha_shape[0]);
  const std::vector<Claim> qk = verify_concat_matmul(vs, id, mha_qk_spec(l), mp.mha_qk, sc);
  DP_REQUIRE(qk.size() == 2 && fm.size() == 2, DP_ERR_VERIFY, "mha: qk claims");
  return {qk[0], qk[1], fm[1]};
}

// table proofs (verifier.rs:320-383)
inline void verify_table_proofs(VerifyState& vs) {
  const VerifierContext& vc = vs.vc; const Proof& proof = vs.proof;
  DP_REQUIRE(proof.table_proofs.size() == vc.tables.size(), DP_ERR_VERIFY, "wrong number of table proofs");
  vs.unused_tables = vc.table_comms;
  for (size_t i = 0; i < vc.tables.size(); i++) {
    const TableType& tt = vc.tables[i];
    const TableProof& tp = proof.table_proofs[i];
    LogUpVerifierClaim v = verify_logup_proof(tp.lookup, 1, vs.constant_challenge, vs.chmap[tt], vs.t, 1);
    vs.add_claim(tp.multiplicity_commit, v.claims[0]);
    if (tt.committed_column()) {  // the claim on the committed column is left to the opening (verifier.rs:352-362)
      auto ti = vs.unused_tables.find(tt);
      DP_REQUIRE(ti != vs.unused_tables.end() && v.claims.size() >= 2, DP_ERR_VERIFY, "table: no commitment for its column");
      vs.add_claim(ti->second, v.claims.back());
      vs.unused_tables.erase(ti);
      v.claims.pop_back();
    }
    const std::vector<Ext>& pt = v.claims[0].point;
    DP_REQUIRE(pt.size() == tt.vars(), DP_ERR_VERIFY, "table: point size");
    std::vector<Ext> expect;  // evaluate_table_columns (lookup/context.rs:302-462)
    Ext idx = ex_zero();
    for (size_t k = 0; k < pt.size(); k++) idx = ex_add(idx, ex_mul(pt[k], ex_from_u64(u64(1) << k)));
    if (tt.kind == 2) expect = {idx};
    else if (tt.kind == 1) expect = {ex_sub(idx, ex_from_u64(u64(1) << (tt.size - 1)))};  // GELU: the input column, the output column is committed (context.rs:364-378)
    else if (tt.kind == 7) expect = {ex_sub(idx, ex_from_u64(u64(1) << (2 * (Q_BIT_LEN - 1))))};  // (context.rs:445-462)
    else if (tt.kind == 4) expect = {idx};   // Softmax: the input column (context.rs:409-423)
    else if (tt.kind == 5) expect = {};      // ErrorTable: nothing but the committed column (:424)
    else if (tt.kind == 6) { Ext o = ex_one(); for (size_t k = 0; k < pt.size(); k++) o = ex_mul(o, ex_sub(ex_one(), pt[k])); expect = {idx, o}; }  // ZeroTable (:425-443)
    else if (tt.kind == 0) {
      Ext second = ex_zero();
      for (size_t k = 0; k + 1 < pt.size(); k++) second = ex_add(second, ex_mul(ex_mul(pt[k], ex_from_u64(u64(1) << k)), pt.back()));
      expect = {ex_sub(idx, ex_from_u64(u64(1) << (Q_BIT_LEN - 1))), second};
    } else {
      int64_t mx = int64_t(1) << (tt.size - 1);
      std::vector<Ext> col; for (int64_t x = -mx; x < mx; x++) col.push_back(ex_from_i64(q_clamp(x)));
      expect = {ex_sub(idx, ex_from_u64(u64(1) << (tt.size - 1))), host_mle_eval(col, pt)};
    }
    DP_REQUIRE(expect.size() + 1 == v.claims.size(), DP_ERR_VERIFY, "table: number of column claims");
    for (size_t k = 0; k < expect.size(); k++) DP_REQUIRE(ex_eq(v.claims[k + 1].eval, expect[k]), DP_ERR_VERIFY, "table: claimed column evaluation is wrong");
  }
}

// input claim (provable/mod.rs:542-565); behind an Embeddings layer it is a claim on the one-hot encoding of the tokens:
// sum_i beta(i, r2) * eq(r1, bits(token_i)), r1 = the vocabulary part of the point (verify_input_claim, embeddings.rs:530-571)
// every input tensor of the model against the claim its reader made on it (ModelCtx::input_claims, provable/mod.rs:272-311)
inline void verify_input_claims(const ModelSpec& m, const IO& io, const std::map<size_t, std::vector<Claim>>& made) {
  const std::vector<size_t> in_tensors = input_tensor_lens(m);
  if (in_tensors.size() > 1 || !m.layers[0].inputs.empty()) {
    size_t off = 0;
    for (size_t q = 0; q < in_tensors.size(); q++) {
      const Reader_ rd = reader_of(m, -1, (int)q);
      DP_REQUIRE(rd.to >= 0 && m.layers[(size_t)rd.to].kind != L_EMBED, DP_ERR_VERIFY, "input tensor without a reader (Embeddings is only supported as node 0 of a chain)");
      const Claim& c = made.at((size_t)rd.to).at((size_t)rd.port);
      std::vector<Ext> iv(in_tensors[q]); for (size_t i = 0; i < iv.size(); i++) iv[i] = ex_from_i64(io.input[off + i]);
      DP_REQUIRE(c.point.size() == dp_ceil_log2(iv.size()) && ex_eq(host_mle_eval(iv, c.point), c.eval), DP_ERR_VERIFY, "input claim is incorrect");
      off += in_tensors[q];
    }
  } else {
    const Claim& cur = made.at(0).at(0);
    if (m.layers[0].kind == L_EMBED) {
      const unsigned vnv = dp_ceil_log2(m.layers[0].nrows);
      DP_REQUIRE(cur.point.size() == vnv + dp_ceil_log2(io.input.size()), DP_ERR_VERIFY, "input claim is incorrect");
      std::vector<Ext> r1(cur.point.begin(), cur.point.begin() + vnv), r2(cur.point.begin() + vnv, cur.point.end());
      std::vector<Ext> beta = host_eq_table(r2);
      Ext sum = ex_zero();
      for (size_t i = 0; i < io.input.size(); i++) {
        DP_REQUIRE(io.input[i] >= 0 && (size_t)io.input[i] < m.layers[0].nrows, DP_ERR_VERIFY, "token outside the vocabulary");
        Ext sel = beta[i];
        for (unsigned b = 0; b < vnv; b++) sel = ex_mul(sel, ((io.input[i] >> b) & 1) ? r1[b] : ex_sub(ex_one(), r1[b]));
        sum = ex_add(sum, sel);
      }
      DP_REQUIRE(ex_eq(sum, cur.eval), DP_ERR_VERIFY, "one hot encoding claim is incorrect");
    } else
    { std::vector<Ext> iv(io.input.size()); for (size_t i = 0; i < iv.size(); i++) iv[i] = ex_from_i64(io.input[i]);
      DP_REQUIRE(cur.point.size() == dp_ceil_log2(iv.size()) && ex_eq(host_mle_eval(iv, cur.point), cur.eval), DP_ERR_VERIFY, "input claim is incorrect"); }
  }
}

// the output claims: one per output tensor, in the order of the model's outputs (io.output = their concatenation)
inline std::vector<Claim> draw_output_claims(VerifyState& vs, const IO& io) {
  const ModelSpec& m = vs.vc.shape;
  DP_REQUIRE(io.input.size() == m.input_len && io.output.size() == model_output_len(m), DP_ERR_VERIFY, "io shapes");
  std::vector<Claim> on_outputs;
  size_t off = 0;
  for (const Edge& e : output_edges(m)) {
    const size_t n = vs.lens.at((size_t)e.from);
    DP_REQUIRE(is_pow2(n), DP_ERR_VERIFY, "io shapes");
    Claim c; c.point = vs.t.read_challenges(dp_ceil_log2(n));
    std::vector<Ext> ov(n); for (size_t i = 0; i < n; i++) ov[i] = ex_from_i64(io.output[off + i]);
    c.eval = host_mle_eval(ov, c.point);
    on_outputs.push_back(std::move(c)); off += n;
  }
  return on_outputs;
}

// Verifier::verify (verifier.rs:72-318)
inline void verify(const VerifierContext& vc, const Proof& proof, const IO& io, Transcript& t) {
  const ModelSpec& m = vc.shape;
  VerifyState vs(vc, proof, t);
  for (auto& kv : vc.model_comms) for (auto& pc : kv.second) t.append_digest(pc.second.root);
  if (!vc.tables.empty()) {
    vs.constant_challenge = t.get_and_append_challenge("table_constant");
    for (auto& tt : vc.tables) vs.chmap[tt] = tt.label() ? t.get_and_append_challenge(tt.label()) : ex_one();
  }
  // every provable node has its step and no other step is there; the fractions of all lookups, for the global check
  std::vector<Ext> nums, dens;
  auto add_fracs = [&nums, &dens](const LogUpProof& p) {
    for (auto& e : p.circuit_outputs) { DP_REQUIRE(e.size() == 4, DP_ERR_VERIFY, "circuit outputs"); nums.push_back(ex_add(ex_mul(e[0], e[3]), ex_mul(e[1], e[2]))); dens.push_back(ex_mul(e[2], e[3])); }
  };
  size_t n_provable = 0;
  for (size_t id = 0; id < m.layers.size(); id++) {
    if (m.layers[id].kind == L_FLATTEN) continue;  // not provable: no proof (verifier.rs:92-96)
    n_provable++;
    auto it = proof.steps.find(id);
    DP_REQUIRE(it != proof.steps.end() && it->second.kind == m.layers[id].kind, DP_ERR_VERIFY, "missing or mistyped layer proof");
    for_each_lookup(it->second, add_fracs);
  }
  DP_REQUIRE(proof.steps.size() == n_provable, DP_ERR_VERIFY, "unexpected layer proofs");
  for (auto& tp : proof.table_proofs) add_fracs(tp.lookup);
  tensor_lens(m, vs.lens, &vs.in_lens);
  const std::vector<Claim> on_outputs = draw_output_claims(vs, io);
  // the nodes in proving order, each receiving the claims its readers made on its outputs and making one claim per input
  vs.unused = vc.model_comms;
  std::map<size_t, std::vector<Claim>> made;  // node -> the claims on its inputs
  for (size_t id : proving_order(m)) {
    const LayerSpec& l = m.layers[id];
    std::vector<Claim> got;
    for (size_t j = 0; j < out_degree(l); j++) { const Reader_ rd = reader_of(m, (int)id, (int)j); got.push_back(rd.to < 0 ? on_outputs.at((size_t)rd.port) : made.at((size_t)rd.to).at((size_t)rd.port)); }
    const Claim& cur = got[0];
    const size_t out_len = vs.lens[id];
    if (l.kind == L_FLATTEN) { made[id] = {cur}; continue; }  // claims pass through a non-provable node unchanged (verifier.rs:205-209)
    const LayerProof& lp = proof.steps.at(id);
    if (l.kind == L_MATMUL2) made[id] = verify_matmul2(vs, id, l, lp.matmul, cur);
    else if (l.kind == L_ADD2) made[id] = verify_add2(vs, id, l, lp.add, cur, out_len);
    else if (l.kind == L_CONCAT_MATMUL) made[id] = verify_concat_matmul(vs, id, l, lp.cmm, cur);
    else if (l.kind == L_QKV) made[id] = verify_qkv(vs, id, l, lp.qkv, got);
    else if (l.kind == L_MHA) made[id] = verify_mha(vs, id, l, lp, cur);
    else if (l.kind == L_CONV) made[id] = {verify_conv(vs, id, l, lp.conv, cur)};
    else if (l.kind == L_MAXPOOL) made[id] = {verify_pooling(vs, id, l, lp.pool, cur, out_len)};
    else if (l.kind == L_LOGITS) made[id] = {verify_logits(vs, id, l, lp.logits, io)};
    else if (l.kind == L_DENSE) made[id] = {verify_dense(vs, id, l, lp.dense, cur)};
    else if (l.kind == L_POSITIONAL) made[id] = {verify_positional(vs, id, l, lp.pos, cur, out_len)};
    else if (l.kind == L_EMBED) made[id] = {verify_embeddings(vs, id, l, lp.matmul, cur, out_len)};
    else if (l.kind == L_ADD) made[id] = {verify_add(vs, id, l, lp.add, cur, out_len)};
    else if (l.kind == L_MATMUL) made[id] = {verify_matmul(vs, id, l, lp.matmul, cur, out_len)};
    else if (l.kind == L_SOFTMAX) made[id] = {verify_softmax(vs, id, l, lp.sm, cur, out_len)};
    else if (l.kind == L_LAYERNORM) made[id] = {verify_layernorm(vs, id, l, lp.ln, cur)};
    else if (l.kind == L_REQUANT) made[id] = {verify_requant(vs, id, l, lp.req, cur)};
    else made[id] = {verify_activation(vs, id, l, lp.act, cur, out_len)};  // (refuses every kind but ReLU and GELU)
  }
  verify_table_proofs(vs);
  verify_input_claims(m, io, made);
  // commitment openings (commit/context.rs:520-598)
  DP_REQUIRE(vs.unused.empty(), DP_ERR_VERIFY, "not all model commitments have been used");
  DP_REQUIRE(vs.unused_tables.empty(), DP_ERR_VERIFY, "not all table commitments have been used");
  DP_REQUIRE(vs.trivial_claims.size() == proof.trivial_proofs.size(), DP_ERR_VERIFY, "number of trivial proofs");
  for (size_t i = 0; i < vs.trivial_claims.size(); i++) pcs_verify_trivial(vs.trivial_claims[i].comm, vs.trivial_claims[i].point, vs.trivial_claims[i].eval, proof.trivial_proofs[i]);
  VerifierParams vp; vp.full_log = vc.full_log;
  { const bool timing = getenv("DP_TIMING") && atoi(getenv("DP_TIMING")); auto t0 = std::chrono::steady_clock::now();
    pcs_batch_verify(vp, vs.claims, proof.batch_proof, t);
    if (timing) fprintf(stderr, "[dp timing] verify: batch opening (without its Merkle paths) %8.3f ms, %zu claims\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), vs.claims.size()); }
  // global logup check (verifier.rs:273-291)
  Ext fn = ex_zero(), fd = ex_one();
  for (size_t i = 0; i < nums.size(); i++) { fn = ex_add(ex_mul(fn, dens[i]), ex_mul(nums[i], fd)); fd = ex_mul(fd, dens[i]); }
  DP_REQUIRE(ex_is_zero(fn), DP_ERR_VERIFY, "final logup numerator is non-zero");
  DP_REQUIRE(!ex_is_zero(fd), DP_ERR_VERIFY, "final logup denominator is zero");
}

// ---- serialisable verifier context (what dp_model_verifier_blob hands out and dp_verify consumes)
constexpr int N_POLY_IDS = 17;
inline const char* const* poly_ids() { static const char* const ids[N_POLY_IDS] = {"DenseBias", "DenseWeight", "ConvBias", "ConvFilter", "MatMulBias", "MatMulWeight", "255", "EmbeddingMat", "PositionalMatrix", "BiasK", "BiasQ", "BiasV", "WeightK", "WeightQ", "WeightV", "LayerNormBeta", "LayerNormGamma"}; return ids; }
constexpr u64 VCTX_GRAPH_MARK = 0x0048504152475044ULL;  // "DPGRAPH": the optional trailing section of a verifier blob (edges, multi-tensor io, ConcatMatMul geometry)
inline bool is_plain_chain(const ModelSpec& m) {
  if (!m.input_lens.empty() || !m.outputs.empty()) return false;
  for (auto& l : m.layers) if (!l.inputs.empty() || l.kind == L_CONCAT_MATMUL) return false;
  return true;
}
inline std::vector<u64> vctx_to_words(const VerifierContext& v) {
  std::vector<u64> w;
  w.push_back(0x3158544356504444ULL); w.push_back(v.full_log); w.push_back(v.shape.input_len); w.push_back(v.shape.layers.size());
  for (auto& l0 : v.shape.layers) {
    LayerSpec l = l0;
    if (l.kind == L_SOFTMAX) {  // a Softmax in the slots of Requant / Conv: table size, zero chunks, multiplier, 1 / temperature bits, zero table vars, bkm, allowable error, shape
      l.right_shift = l.sm_table_size; l.fp_scale = l.sm_zero_chunks; l.fixed_point_multiplier = l.sm_scalar; l.intermediate_bit_size = l.sm_temp_bits;
      l.kw = l.sm_zero_vars; l.kx = (size_t)l.sm_bkm; l.real_nw = (size_t)l.sm_allowable_error; for (int k = 0; k < 3; k++) l.unp_out[k] = l.sm_shape[k];
    }
    if (l.kind == L_MHA) {  // an Mha node: its softmax in the same slots, (seq, heads, head_dim) where a Softmax has its shape
      l.right_shift = l.sm_table_size; l.fp_scale = l.sm_zero_chunks; l.fixed_point_multiplier = l.sm_scalar; l.intermediate_bit_size = l.sm_temp_bits;
      l.kw = l.sm_zero_vars; l.kx = (size_t)l.sm_bkm; l.real_nw = (size_t)l.sm_allowable_error; for (int k = 0; k < 3; k++) l.unp_out[k] = l.mha_shape[k];
    }
    if (l.kind == L_LAYERNORM) {  // a LayerNorm rides in the slots of a Requant: N, range check bits, log2 of the top chunk scalar, multiplier, epsilon bits
      l.ncols = l.ln_dim_size; l.right_shift = l.ln_range_check_bits; l.fp_scale = l.ln_top_chunk_scalar_log; l.fixed_point_multiplier = l.ln_multiplier; l.intermediate_bit_size = l.ln_eps_bits;
    }
    w.push_back(l.kind); w.push_back(l.nrows); w.push_back(l.ncols); w.push_back(l.right_shift); w.push_back(l.fp_scale);
    const bool adds = l.kind == L_ADD || l.kind == L_ADD2 || l.kind == L_POSITIONAL, mm = l.kind == L_MATMUL || l.kind == L_MATMUL2;
    w.push_back(adds ? (u64)l.add_left : (u64)l.fixed_point_multiplier);  // (an Add carries its two multipliers in the requant multiplier / kx slots)
    w.push_back(l.intermediate_bit_size);
    w.push_back(mm ? (l.mm_transpose ? 1 : 0) : l.kw);  // (a MatMul has no filter count: the slot carries its transpose flag)
    w.push_back(adds ? (u64)l.add_right : l.kx); w.push_back(l.real_nw); w.push_back(l.nw);
    for (int k = 0; k < 3; k++) w.push_back(l.unp_out[k]);
    for (int k = 0; k < 3; k++) w.push_back(l.pin[k]);
  }
  w.push_back(v.model_comms.size());
  for (auto& kv : v.model_comms) {
    w.push_back(kv.first); w.push_back(kv.second.size());
    for (auto& pc : kv.second) {
      int code = -1; for (int q = 0; q < N_POLY_IDS; q++) if (pc.first == poly_ids()[q]) code = q;
      DP_REQUIRE(code >= 0, DP_ERR_ARG, "unknown model polynomial id");
      const Commitment& c = pc.second; w.push_back((u64)code); for (int k = 0; k < 4; k++) w.push_back(c.root.v[k]); w.push_back(c.num_vars); w.push_back(c.is_base);
    }
  }
  w.push_back(v.tables.size());
  for (auto& t : v.tables) {
    w.push_back(t.kind); w.push_back(t.size);
    if (t.committed_column()) {  // (only these entries are longer: the table's other parameters and the commitment of its column)
      w.push_back(t.aux); w.push_back((u64)t.aux2);
      auto it = v.table_comms.find(t); DP_REQUIRE(it != v.table_comms.end(), DP_ERR_ARG, "verifier context: table without its commitment");
      const Commitment& c = it->second; for (int k = 0; k < 4; k++) w.push_back(c.root.v[k]); w.push_back(c.num_vars); w.push_back(c.is_base);
    }
  }
  if (!is_plain_chain(v.shape)) {
    w.push_back(VCTX_GRAPH_MARK);
    w.push_back(v.shape.input_lens.size()); for (size_t n : v.shape.input_lens) w.push_back(n);
    w.push_back(v.shape.outputs.size()); for (const Edge& e : v.shape.outputs) { w.push_back((u64)(e.from + 1)); w.push_back((u64)e.slot); }
    for (auto& l : v.shape.layers) {
      w.push_back(l.inputs.size()); for (const Edge& e : l.inputs) { w.push_back((u64)(e.from + 1)); w.push_back((u64)e.slot); }
      if (l.kind == L_CONCAT_MATMUL) {
        for (int d = 0; d < 3; d++) w.push_back(l.cm_a[d]);
        for (int d = 0; d < 3; d++) w.push_back(l.cm_b[d]);
        for (int d = 0; d < 3; d++) w.push_back((u64)l.cm_left[d]);
        for (int d = 0; d < 3; d++) w.push_back((u64)l.cm_right[d]);
        w.push_back(l.cm_perm.size()); for (int x : l.cm_perm) w.push_back((u64)x);
      }
    }
  }
  return w;
}
inline VerifierContext vctx_from_words(const u64* w, size_t n) {
  size_t pos = 0;
  auto rd = [&]() { DP_REQUIRE(pos < n, DP_ERR_ARG, "verifier blob truncated"); return w[pos++]; };
  VerifierContext v;
  DP_REQUIRE(rd() == 0x3158544356504444ULL, DP_ERR_ARG, "bad verifier blob magic");
  v.full_log = (unsigned)rd(); v.shape.input_len = (size_t)rd(); size_t nl = (size_t)rd();
  DP_REQUIRE(nl < 4096, DP_ERR_ARG, "verifier blob: layer count");
  for (size_t i = 0; i < nl; i++) {
    LayerSpec l; l.kind = (int)rd(); l.nrows = (size_t)rd(); l.ncols = (size_t)rd(); l.right_shift = (unsigned)rd(); l.fp_scale = (unsigned)rd(); l.fixed_point_multiplier = (int64_t)rd(); l.intermediate_bit_size = (unsigned)rd();
    l.kw = (size_t)rd(); l.kx = (size_t)rd(); l.real_nw = (size_t)rd(); l.nw = (size_t)rd();
    for (int k = 0; k < 3; k++) l.unp_out[k] = (size_t)rd();
    for (int k = 0; k < 3; k++) l.pin[k] = (size_t)rd();
    DP_REQUIRE(l.kind >= L_DENSE && l.kind <= L_LOGITS, DP_ERR_ARG, "verifier blob: layer kind");
    if (l.kind == L_LOGITS) DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2 && l.nrows <= (size_t(1) << 24) && l.ncols <= (size_t(1) << 24), DP_ERR_ARG, "verifier blob: logits shape");
    if (l.kind == L_GELU) DP_REQUIRE(l.fixed_point_multiplier >= 1 && l.fixed_point_multiplier <= (int64_t(1) << 12), DP_ERR_ARG, "verifier blob: gelu multiplier");
    if (l.kind == L_MHA) {
      l.sm_table_size = l.right_shift; l.sm_zero_chunks = l.fp_scale; l.sm_scalar = l.fixed_point_multiplier; l.sm_temp_bits = (uint32_t)l.intermediate_bit_size;
      l.sm_zero_vars = (unsigned)l.kw; l.sm_bkm = (int64_t)l.kx; l.sm_allowable_error = (int64_t)l.real_nw; for (int k = 0; k < 3; k++) { l.mha_shape[k] = l.unp_out[k]; l.unp_out[k] = 0; }
      l.right_shift = l.fp_scale = l.intermediate_bit_size = 0; l.fixed_point_multiplier = 0; l.kw = l.kx = l.real_nw = 0;
      DP_REQUIRE(is_pow2(l.mha_shape[0]) && is_pow2(l.mha_shape[1]) && is_pow2(l.mha_shape[2]) && l.mha_shape[0] >= 2 && l.mha_shape[2] >= 2 && l.mha_shape[0] <= (size_t(1) << 12) && l.mha_shape[1] <= (size_t(1) << 12) && l.mha_shape[2] <= (size_t(1) << 12)
                 && l.sm_scalar >= 1 && l.sm_bkm >= (int64_t(1) << 17) && l.sm_bkm < (int64_t(1) << 40) && l.sm_table_size == dp_ceil_log2((size_t)(l.sm_bkm >> 16)) && l.sm_zero_chunks <= 3 && l.sm_zero_vars <= 22
                 && (l.sm_zero_chunks == 0) == (l.sm_zero_vars == 0) && l.sm_allowable_error >= 1 && l.sm_allowable_error <= (1 << 11), DP_ERR_ARG, "verifier blob: mha parameters");
    }
    if (l.kind == L_SOFTMAX) {
      l.sm_table_size = l.right_shift; l.sm_zero_chunks = l.fp_scale; l.sm_scalar = l.fixed_point_multiplier; l.sm_temp_bits = (uint32_t)l.intermediate_bit_size;
      l.sm_zero_vars = (unsigned)l.kw; l.sm_bkm = (int64_t)l.kx; l.sm_allowable_error = (int64_t)l.real_nw; for (int k = 0; k < 3; k++) { l.sm_shape[k] = l.unp_out[k]; l.unp_out[k] = 0; }
      l.right_shift = l.fp_scale = l.intermediate_bit_size = 0; l.fixed_point_multiplier = 0; l.kw = l.kx = l.real_nw = 0;
      DP_REQUIRE(is_pow2(l.sm_shape[0]) && is_pow2(l.sm_shape[1]) && l.sm_shape[1] == l.sm_shape[2] && l.sm_shape[0] <= (size_t(1) << 20) && l.sm_shape[1] <= (size_t(1) << 20) && l.sm_scalar >= 1 && l.sm_bkm >= (int64_t(1) << 17) && l.sm_bkm < (int64_t(1) << 40)
                 && l.sm_table_size == dp_ceil_log2((size_t)(l.sm_bkm >> 16)) && l.sm_zero_chunks <= 3 && l.sm_zero_vars <= 22 && (l.sm_zero_chunks == 0) == (l.sm_zero_vars == 0) && l.sm_allowable_error >= 1 && l.sm_allowable_error <= (1 << 11), DP_ERR_ARG, "verifier blob: softmax parameters");
    }
    if (l.kind == L_LAYERNORM) {
      l.ln_dim_size = l.ncols; l.ln_range_check_bits = l.right_shift; l.ln_top_chunk_scalar_log = l.fp_scale; l.ln_multiplier = l.fixed_point_multiplier; l.ln_eps_bits = (uint32_t)l.intermediate_bit_size;
      l.ncols = 0; l.right_shift = l.fp_scale = l.intermediate_bit_size = 0; l.fixed_point_multiplier = 0;
      DP_REQUIRE(is_pow2(l.nrows) && l.nrows >= 2 && l.nrows <= (size_t(1) << 24) && l.ln_dim_size >= 1 && next_pow2(l.ln_dim_size) == l.nrows && l.ln_multiplier >= 1 && l.ln_range_check_bits >= 1 && l.ln_range_check_bits <= 40 && l.ln_top_chunk_scalar_log < Q_BIT_LEN, DP_ERR_ARG, "verifier blob: layernorm parameters");
    }
    if (l.kind == L_MATMUL2) { DP_REQUIRE(l.kw <= 1, DP_ERR_ARG, "verifier blob: matmul flags"); l.mm_transpose = l.kw != 0; l.kw = 0; }
    if (l.kind == L_ADD || l.kind == L_ADD2 || l.kind == L_POSITIONAL) { l.add_left = l.fixed_point_multiplier; l.add_right = (int64_t)l.kx; l.fixed_point_multiplier = 0; l.kx = 0; DP_REQUIRE(l.add_left > 0 && l.add_right > 0, DP_ERR_ARG, "verifier blob: add multipliers"); }
    if (l.kind == L_MATMUL) { DP_REQUIRE(l.kw <= 1, DP_ERR_ARG, "verifier blob: matmul flags"); l.mm_transpose = l.kw != 0; l.kw = 0; }
    if (l.kind == L_CONV) DP_REQUIRE(is_pow2(l.kw) && is_pow2(l.kx) && is_pow2(l.real_nw) && is_pow2(l.nw) && l.kw <= (1u << 16) && l.kx <= (1u << 16) && l.nw <= (1u << 12) && 2 * l.real_nw <= l.nw && l.unp_out[0] <= l.kw && l.unp_out[1] <= l.nw && l.unp_out[2] <= l.nw, DP_ERR_ARG, "verifier blob: conv shape");
    if (l.kind == L_MAXPOOL) DP_REQUIRE(is_pow2(l.pin[0]) && is_pow2(l.pin[1]) && is_pow2(l.pin[2]) && l.pin[2] >= 2, DP_ERR_ARG, "verifier blob: maxpool shape");
    v.shape.layers.push_back(l);
  }
  size_t nc = (size_t)rd(); DP_REQUIRE(nc <= nl, DP_ERR_ARG, "verifier blob: commitments");
  for (size_t i = 0; i < nc; i++) {
    size_t id = (size_t)rd(); size_t np = (size_t)rd();
    DP_REQUIRE(np <= 6, DP_ERR_ARG, "verifier blob: polynomials per node");
    for (size_t q = 0; q < np; q++) { u64 code = rd(); DP_REQUIRE(code < (u64)N_POLY_IDS, DP_ERR_ARG, "verifier blob: polynomial id"); Commitment c; for (int k = 0; k < 4; k++) c.root.v[k] = rd(); c.num_vars = (unsigned)rd(); c.is_base = rd() != 0; v.model_comms[id][poly_ids()[code]] = c; }
  }
  size_t nt = (size_t)rd(); DP_REQUIRE(nt < 64, DP_ERR_ARG, "verifier blob: tables");
  for (size_t i = 0; i < nt; i++) {
    TableType t; t.kind = (int)rd(); t.size = (unsigned)rd();
    DP_REQUIRE(t.kind >= 0 && t.kind <= 7, DP_ERR_ARG, "verifier blob: table kind");
    DP_REQUIRE(t.kind != 6 || (t.size >= 1 && t.size <= 22), DP_ERR_ARG, "verifier blob: zero table size");
    if (t.committed_column()) {
      u64 a = rd(), a2 = rd(); DP_REQUIRE(a <= 0xFFFFFFFFull && t.size <= 40 && a2 < (u64(1) << 40), DP_ERR_ARG, "verifier blob: table parameters"); t.aux = (uint32_t)a; t.aux2 = (int64_t)a2;
      DP_REQUIRE(t.kind != 5 || (t.aux2 >= 1 && t.aux2 <= (1 << 11)), DP_ERR_ARG, "verifier blob: error table");
      DP_REQUIRE(t.kind != 4 || (t.size >= 1 && t.size <= 22), DP_ERR_ARG, "verifier blob: softmax table");
      DP_REQUIRE(t.kind != 1 || (t.aux2 >= 1 && t.aux2 <= (int64_t(1) << 12) && t.size == gelu_table_vars(t.aux2) && t.aux == 0), DP_ERR_ARG, "verifier blob: gelu table");
      Commitment c; for (int k = 0; k < 4; k++) c.root.v[k] = rd(); c.num_vars = (unsigned)rd(); c.is_base = rd() != 0; v.table_comms[t] = c;
    }
    v.tables.push_back(t);
  }
  if (pos < n) {
    DP_REQUIRE(rd() == VCTX_GRAPH_MARK, DP_ERR_ARG, "verifier blob: trailing words");
    auto rd_edge = [&]() { Edge e; u64 f = rd(); DP_REQUIRE(f <= nl, DP_ERR_ARG, "verifier blob: edge"); e.from = (int)f - 1; u64 sl = rd(); DP_REQUIRE(sl < 4096, DP_ERR_ARG, "verifier blob: edge"); e.slot = (int)sl; return e; };
    size_t ni = (size_t)rd(); DP_REQUIRE(ni < 4096, DP_ERR_ARG, "verifier blob: inputs");
    for (size_t i = 0; i < ni; i++) v.shape.input_lens.push_back((size_t)rd());
    size_t no = (size_t)rd(); DP_REQUIRE(no < 4096, DP_ERR_ARG, "verifier blob: outputs");
    for (size_t i = 0; i < no; i++) v.shape.outputs.push_back(rd_edge());
    for (auto& l : v.shape.layers) {
      size_t k = (size_t)rd(); DP_REQUIRE(k <= 3, DP_ERR_ARG, "verifier blob: node inputs");
      for (size_t i = 0; i < k; i++) l.inputs.push_back(rd_edge());
      if (l.kind == L_CONCAT_MATMUL) {
        for (int d = 0; d < 3; d++) { l.cm_a[d] = (size_t)rd(); DP_REQUIRE(is_pow2(l.cm_a[d]) && l.cm_a[d] <= (size_t(1) << 24), DP_ERR_ARG, "verifier blob: concat matmul shape"); }
        for (int d = 0; d < 3; d++) { l.cm_b[d] = (size_t)rd(); DP_REQUIRE(is_pow2(l.cm_b[d]) && l.cm_b[d] <= (size_t(1) << 24), DP_ERR_ARG, "verifier blob: concat matmul shape"); }
        for (int d = 0; d < 3; d++) { u64 x = rd(); DP_REQUIRE(x < 3, DP_ERR_ARG, "verifier blob: concat matmul axes"); l.cm_left[d] = (int)x; }
        for (int d = 0; d < 3; d++) { u64 x = rd(); DP_REQUIRE(x < 3, DP_ERR_ARG, "verifier blob: concat matmul axes"); l.cm_right[d] = (int)x; }
        size_t np_ = (size_t)rd(); DP_REQUIRE(np_ == 0 || np_ == 3, DP_ERR_ARG, "verifier blob: concat matmul permutation");
        for (size_t i = 0; i < np_; i++) { u64 x = rd(); DP_REQUIRE(x < 3, DP_ERR_ARG, "verifier blob: concat matmul permutation"); l.cm_perm.push_back((int)x); }
      }
    }
    DP_REQUIRE(pos == n, DP_ERR_ARG, "verifier blob: trailing words");
  }
  return v;
}

}  // namespace dp
