// The zkml proving surface for the Dense / Requant / ReLU graph on top of device ops:
//   Context::generate (zkml/src/iop/context.rs:109-215, commit/context.rs:59-115)
//   Prover::prove     (zkml/src/iop/prover.rs:401-488) with Dense::prove_step (layers/dense.rs:423-561),
//                     Requant::prove_step (layers/requant.rs:531-690), Activation::prove_step (layers/activation.rs:385-456),
//                     generate_lookup_witnesses (lookup/context.rs:631-781), prove_tables (iop/prover.rs:110-157),
//                     CommitmentProver::prove (commit/context.rs:355-418)
//   verify            (zkml/src/iop/verifier.rs:72-318) — host only, as in the reference: zkml_verify.h, included at the end of this header.
// A model is an already padded / quantised chain with node ids Dense, Requant, Relu, Dense, ... as produced by
// Model::random_with_rng (zkml/src/model/mod.rs:596-665); the ONNX / float front-end is out of scope.
#pragma once
#include "logup.h"
#include "pcs.h"
#include "cnn.h"
#include <unordered_map>
#include <mutex>
#include <algorithm>
#include <memory>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

namespace dp {

constexpr unsigned Q_BIT_LEN = 8;
constexpr int64_t Q_MIN = -127, Q_MAX = 127;
constexpr int64_t COLUMN_SEPARATOR = int64_t(1) << 32;

// Edge of the model graph (Edge, layers/provable/mod.rs:195-229): tensor `slot` produced by node `from`; from < 0: input tensor `slot` of the model
struct Edge { int from = -1; int slot = 0; };
struct LayerSpec {
  int kind = L_DENSE;
  // the node's input edges (Node::inputs); empty = the chain form (output 0 of the node before, the model input for node 0). Nodes are
  // stored in a topological order: an edge always comes from a smaller id.
  std::vector<Edge> inputs;
  // matmul2 (layers/matrix_mul.rs, both operands inputs): [s][nrows] x [nrows][ncols] ([ncols][nrows] under mm_transpose), no bias.
  // add2 (layers/add.rs, no operand): add_left * a + add_right * b.
  // qkv (layers/transformer/qkv.rs): weights = W_q | W_k | W_v ([nrows][ncols] each), bias = b_q | b_k | b_v ([ncols] each); outputs Q, K, V.
  // concat matmul (layers/concat_matmul.rs): rank-3 inputs of shapes cm_a, cm_b; cm_left / cm_right = (concat, mat_mul, output) dimension of
  // each input; cm_perm = permutation of the [concat][rows][cols] result, empty for none.
  size_t cm_a[3] = {0, 0, 0}, cm_b[3] = {0, 0, 0};
  int cm_left[3] = {0, 2, 1}, cm_right[3] = {0, 1, 2};
  std::vector<int> cm_perm;
  size_t nrows = 0, ncols = 0;
  std::vector<int64_t> weights, bias;  // dense: row major / padded bias; conv: filter [kw][kx][real_nw][real_nw], bias [kw]
  // matmul (layers/matrix_mul.rs, MatMul::new_constant: Input x Weight [+ bias]): the constant RIGHT matrix is weights[nrows][ncols] row major,
  // the input a row-major [s][nrows] matrix (s = its length / nrows), bias [ncols] or empty; the output is [s][ncols]. mm_transpose
  // (Config::TransposeB, matrix_mul.rs:36-39): the constant matrix is stored as [ncols][nrows] and used transposed
  bool mm_transpose = false;
  // positional (layers/transformer/positional.rs, Positional::Learned): weights = the [nrows = positions][ncols = embedding size] table;
  // out = add_left * x + add_right * table[0 .. tokens) for a [tokens][ncols] activation, tokens <= nrows
  // embeddings (layers/transformer/embeddings.rs): only as the FIRST layer; the input is a vector of token ids, weights the
  // [nrows = vocabulary][ncols = embedding size] table, the output [tokens][ncols]
  // add (layers/add.rs, Add::new_with(operand)): out = add_left * x + add_right * operand; the operand — a constant tensor as long as the
  // input, e.g. learned positional embeddings — is `weights`; the multipliers are QuantInfo::left/right_multiplier (add.rs:271-283)
  int64_t add_left = 1, add_right = 1;
  // conv (layers/convolution.rs:52-83, tensor.rs:409-431): padded filter count kw, padded input channels kx, padded kernel
  // side real_nw, padded input side nw; unp_out = conv2d_shape of the unpadded tensors (for the garbage-clearing tensor)
  size_t kw = 0, kx = 0, real_nw = 0, nw = 0;
  size_t unp_out[3] = {0, 0, 0};
  size_t pin[3] = {0, 0, 0};  // maxpool: padded input shape [c, h, w]
  std::shared_ptr<const std::vector<u64>> wfft;  // conv: FFT of every zero-padded kernel, [kw][kx][2 nw^2] (prepare_conv)
  // dense: the weights once more as int16 when they all fit (quantised models: |w| <= 127) — the inference that precedes
  // every proof then streams a quarter of the bytes and its dot products vectorise (pmaddwd); w16_max = max |w|
  std::shared_ptr<const std::vector<int16_t>> w16; int64_t w16_max = 0;
  size_t filter_size() const { return nw * nw; }
  // layernorm (layers/transformer/layernorm.rs:74-101): gamma = weights, beta = bias, both [nrows = the padded normalisation dimension];
  // QuantisedLayerNormData: N = ln_dim_size, the multiplier of the inverse-square-root input, the f32 bits of the rescaled epsilon (the table's
  // identity together with ln_range_check_bits), the bits shifted away and range checked, log2 of the scalar of their top chunk
  size_t ln_dim_size = 0; int64_t ln_multiplier = 0; uint32_t ln_eps_bits = 0; unsigned ln_range_check_bits = 0, ln_top_chunk_scalar_log = 0;
  // softmax (layers/transformer/softmax.rs:66-99; QuantisedSoftmaxData, SoftmaxCtx :1153-1169) over the last dimension of a padded [sm_shape[0]]
  // [sm_shape[1]][sm_shape[2]] tensor under a causal mask (the last two dimensions are equal): the multiplier that brings the input to the scale
  // 2^24; the f32 bits of 1 / temperature and of the input scale (the prover's row shifts are computed in floating point, as in the reference);
  // the exponential table (2^sm_table_size entries, zero from sm_bkm on); the zero tables for the bits above; the allowable error of a row sum
  int64_t sm_scalar = 0, sm_bkm = 0, sm_allowable_error = 0; uint32_t sm_temp_bits = 0, sm_in_scale_bits = 0; unsigned sm_table_size = 0, sm_zero_chunks = 0, sm_zero_vars = 0;
  size_t sm_shape[3] = {0, 0, 0};
  // mha (layers/transformer/mha.rs:133-186, Mha::new): ONE node with the inputs Q, K, V — padded [seq][heads * head_dim] matrices read as
  // [seq][heads][head_dim] — that bundles qk = ConcatMatMul (1,2,0) x (1,2,0) -> [heads][seq][seq], the Softmax described by the sm_* fields
  // (sm_shape unused) straight on the products, final_mul = ConcatMatMul (0,2,1) x (1,0,2), permuted (1,0,2) -> [seq][heads][head_dim]
  size_t mha_shape[3] = {0, 0, 0};  // seq, heads, head_dim
  // logits (layers/transformer/logits.rs, Logits::Argmax): the input is a padded [nrows = rows][ncols = K] tensor, the output the `rows` indices of
  // the first maximum of every row. The argmax runs over the PADDED row (logits.rs:90-125 ignores the unpadded shapes): a front end that pads a
  // vocabulary must keep its padding columns from winning. Only as the model's single output tensor (verify_output_evaluation, logits.rs:693-731).
  unsigned right_shift = 0, fp_scale = 0, intermediate_bit_size = 0;
  int64_t fixed_point_multiplier = 0;
  unsigned shift() const { return fp_scale + right_shift; }
  unsigned clamping_size() const { return intermediate_bit_size + dp_ceil_log2((size_t)fixed_point_multiplier) - shift(); }
};
// input_lens: the input tensors of the model (empty: a single one of input_len words; otherwise input_len is their sum and an input vector
// their concatenation); outputs: the edges that are the model's output tensors (empty: output 0 of the last node), concatenated likewise
struct ModelSpec { size_t input_len = 0; std::vector<LayerSpec> layers; std::vector<size_t> input_lens; std::vector<Edge> outputs; };
inline size_t out_degree(const LayerSpec& l) { return l.kind == L_QKV ? 3 : 1; }
inline size_t in_degree(const LayerSpec& l) { return l.kind == L_MHA ? 3 : l.kind == L_MATMUL2 || l.kind == L_ADD2 || l.kind == L_CONCAT_MATMUL ? 2 : 1; }
// the sub-layers of an Mha node (Mha::new, mha.rs:147-186)
inline LayerSpec mha_qk_spec(const LayerSpec& l) {
  LayerSpec s; s.kind = L_CONCAT_MATMUL;
  static const int dims[3] = {1, 2, 0};
  for (int d = 0; d < 3; d++) { s.cm_a[d] = s.cm_b[d] = l.mha_shape[d]; s.cm_left[d] = s.cm_right[d] = dims[d]; }
  return s;
}
inline LayerSpec mha_softmax_spec(const LayerSpec& l) {
  LayerSpec s; s.kind = L_SOFTMAX;
  s.sm_scalar = l.sm_scalar; s.sm_bkm = l.sm_bkm; s.sm_allowable_error = l.sm_allowable_error; s.sm_temp_bits = l.sm_temp_bits; s.sm_in_scale_bits = l.sm_in_scale_bits;
  s.sm_table_size = l.sm_table_size; s.sm_zero_chunks = l.sm_zero_chunks; s.sm_zero_vars = l.sm_zero_vars;
  s.sm_shape[0] = l.mha_shape[1]; s.sm_shape[1] = s.sm_shape[2] = l.mha_shape[0];
  return s;
}
inline LayerSpec mha_final_spec(const LayerSpec& l) {
  LayerSpec s; s.kind = L_CONCAT_MATMUL;
  static const int dl[3] = {0, 2, 1}, dr[3] = {1, 0, 2};
  s.cm_a[0] = l.mha_shape[1]; s.cm_a[1] = s.cm_a[2] = l.mha_shape[0];
  for (int d = 0; d < 3; d++) { s.cm_b[d] = l.mha_shape[d]; s.cm_left[d] = dl[d]; s.cm_right[d] = dr[d]; }
  s.cm_perm = {1, 0, 2};
  return s;
}
inline std::vector<Edge> edges_in(const ModelSpec& m, size_t id) {
  if (!m.layers[id].inputs.empty()) return m.layers[id].inputs;
  Edge e; e.from = (int)id - 1; e.slot = 0;  // (node 0: from = -1, the model input)
  return {e};
}
inline std::vector<Edge> output_edges(const ModelSpec& m) {
  if (!m.outputs.empty()) return m.outputs;
  Edge e; e.from = (int)m.layers.size() - 1;
  return {e};
}
inline std::vector<size_t> input_tensor_lens(const ModelSpec& m) { if (m.input_lens.empty()) return {m.input_len}; return m.input_lens; }
// Who reads tensor (node, slot): input `port` of node `to`, or — to < 0 — output number `port` of the model. The reference proves graphs in
// which every tensor has exactly one reader (claims_for_node, provable/mod.rs:235-270); anything else is refused.
struct Reader_ { int to = -1; int port = 0; };
inline Reader_ reader_of(const ModelSpec& m, int node, int slot) {
  Reader_ r; int n = 0;
  for (size_t id = 0; id < m.layers.size(); id++) { const std::vector<Edge> in = edges_in(m, id); for (size_t q = 0; q < in.size(); q++) if (in[q].from == node && in[q].slot == slot) { r.to = (int)id; r.port = (int)q; n++; } }
  const std::vector<Edge> outs = output_edges(m);
  for (size_t q = 0; q < outs.size(); q++) if (outs[q].from == node && outs[q].slot == slot) { r.to = -1; r.port = (int)q; n++; }
  DP_REQUIRE(n == 1, DP_ERR_SHAPE, "model graph: every tensor needs exactly one reader");
  return r;
}
// The order in which Prover::prove and verify walk the nodes (NodeIterator<_, false>, model/iterator.rs:152-185): repeatedly the SMALLEST id
// among the nodes all of whose readers have been handled. For a chain: last node first.
inline std::vector<size_t> proving_order(const ModelSpec& m) {
  const size_t n = m.layers.size();
  std::vector<char> handled(n, 0);
  std::vector<size_t> order;
  while (order.size() < n) {
    size_t pick = n;
    for (size_t id = 0; id < n && pick == n; id++) {
      if (handled[id]) continue;
      bool ok = true;
      for (size_t j = 0; j < out_degree(m.layers[id]) && ok; j++) { const Reader_ r = reader_of(m, (int)id, (int)j); ok = r.to < 0 || handled[(size_t)r.to]; }
      if (ok) pick = id;
    }
    DP_REQUIRE(pick < n, DP_ERR_SHAPE, "model graph: cycle");
    handled[pick] = 1; order.push_back(pick);
  }
  return order;
}
// Tensor::permute3d (tensor.rs:1769-1800): axis d of the result is axis order[d] of x
template <class T> inline std::vector<T> transpose3(const std::vector<T>& x, const size_t dims[3], const int order[3]) {
  const size_t nd[3] = {dims[order[0]], dims[order[1]], dims[order[2]]};
  std::vector<T> y(x.size());
  size_t at[3];
  for (at[0] = 0; at[0] < dims[0]; at[0]++) for (at[1] = 0; at[1] < dims[1]; at[1]++) for (at[2] = 0; at[2] < dims[2]; at[2]++)
    y[(at[order[0]] * nd[1] + at[order[1]]) * nd[2] + at[order[2]]] = x[(at[0] * dims[1] + at[1]) * dims[2] + at[2]];
  return y;
}
// ConcatMatMul geometry: an input described by (concat, mat_mul, output) axes is brought to the axes `want` by the order this returns
// (InputMatrixDimensions::compute_permutation, concat_matmul.rs:101-114); `identity` when nothing moves
inline void cm_axes_to(const int have[3], const int want[3], int order[3], bool& identity) {
  identity = have[0] == want[0] && have[1] == want[1] && have[2] == want[2];
  order[0] = 0; order[1] = 1; order[2] = 2;
  if (!identity) for (int q = 0; q < 3; q++) order[want[q]] = have[q];
}
constexpr int CM_WANT_LEFT[3] = {0, 2, 1}, CM_WANT_RIGHT[3] = {0, 1, 2};  // [concat][rows][inner] times [concat][inner][cols] (concat_matmul.rs:443-465)
struct CmShape { size_t C, R, M, N; size_t out[3]; };  // chunks, rows, inner, columns; the (permuted) shape of the result
inline CmShape cm_shape(const LayerSpec& l) {
  CmShape g;
  g.C = l.cm_a[l.cm_left[0]]; g.R = l.cm_a[l.cm_left[2]]; g.M = l.cm_a[l.cm_left[1]]; g.N = l.cm_b[l.cm_right[2]];
  const size_t r[3] = {g.C, g.R, g.N};
  for (int d = 0; d < 3; d++) g.out[d] = l.cm_perm.empty() ? r[d] : r[l.cm_perm[d]];
  return g;
}

struct TableType {
  // 0 Relu, 1 GELU{multiplier = aux2, table_size = size: GELUQuantData's min / max are -+2^(size - 1)}, 2 Range, 3 Clamping(size), 4 Softmax{float_bits = aux, table_size = size, bkm = aux2}, 5 ErrorTable(4096, allowable_error = aux2),
  // 6 ZeroTable(size), 7 InverseSQRT{eps_bits = aux, range_check_bits = size}  (derive(Ord) order of lookup/context.rs:55-72; SoftmaxTableData
  // :74-84 ordered by (float_bits, table_size, bkm), InverseSQRTTableData :124-131 by (eps_bits, range_check_bits))
  int kind; unsigned size; uint32_t aux = 0; int64_t aux2 = 0;
  bool operator<(const TableType& o) const { return kind != o.kind ? kind < o.kind : aux != o.aux ? aux < o.aux : size != o.size ? size < o.size : aux2 < o.aux2; }
  bool operator==(const TableType& o) const { return kind == o.kind && size == o.size && aux == o.aux && aux2 == o.aux2; }
  unsigned vars() const { return kind == 1 || kind == 3 || kind == 4 || kind == 6 ? size : kind == 5 ? dp_ceil_log2((size_t)(2 * aux2)) : kind == 7 ? 2 * (Q_BIT_LEN - 1) + 1 : Q_BIT_LEN; }  // multiplicity_poly_vars (context.rs:481-492)
  const char* label() const { return kind == 0 ? "Relu" : kind == 1 ? "GELU" : kind == 3 ? "Clamping" : kind == 4 ? "Softmax" : kind == 6 ? "Zero" : kind == 7 ? "InverseSQRT" : nullptr; }
  // committed_columns (context.rs:495-545): the output column of these tables (the only column of an ErrorTable) is a commitment of the context
  bool committed_column() const { return kind == 7 || kind == 4 || kind == 5 || kind == 1; }
};
constexpr unsigned SM_LOG_SCALE = 24; constexpr int64_t SM_OUT_ONE = 1 << 12;  // SCALE_FACTOR, OUTPUT_SCALE_FACTOR (softmax.rs:56-60)
// SoftmaxTableData::table_output (lookup/context.rs:111-122), f32 exp as there
inline int64_t softmax_lut(uint32_t temp_bits, int64_t bkm, int64_t j) {
  float temp; memcpy(&temp, &temp_bits, 4);
  const int64_t prod = (int64_t(1) << (SM_LOG_SCALE - 8)) * j;
  if (prod >= bkm) return 0;
  return (int64_t)roundf(expf((float)(-prod) / ((float)(1u << SM_LOG_SCALE) * temp)) * (float)SM_OUT_ONE);
}
constexpr unsigned LN_LOG_SCALE = 24, LN_LOG_OUT_SCALE = 10;  // LAYERNORM_SCALE_FACTOR, LAYERNORM_OUTPUT_SCALE_FACTOR (layernorm.rs:61-65)
// InverseSQRTTableData::table_output (lookup/context.rs:147-157), in f32 as there; a negative argument gives NaN, which `as Element` turns into 0
inline int64_t inv_sqrt_lut(uint32_t eps_bits, unsigned range_check_bits, int64_t j) {
  float eps; memcpy(&eps, &eps_bits, 4);
  const float arg = (float)(j * (int64_t(1) << range_check_bits)) / (float)(1u << LN_LOG_SCALE) + eps;
  const float r = roundf((1.0f / sqrtf(arg)) * (float)(1u << LN_LOG_OUT_SCALE));
  if (r != r) return 0;
  if (r >= 9.2e18f) return INT64_MAX;
  if (r <= -9.2e18f) return INT64_MIN;
  return (int64_t)r;
}
// GELUQuantData::table_output (layers/activation.rs:582-588) with gelu_float (:623-627), in f32 and in that order of operations; the argument is the
// SCALED input (input * multiplier), the table's unit 2^-12 (GELU_SCALE_FACTOR, :42-43). Every intermediate goes through a volatile float: no
// compiler may fuse x + 0.044715 x^3 into one rounding (the reference's code is not contracted).
constexpr unsigned GELU_LOG_SCALE = 12;
inline int64_t gelu_lut(int64_t scaled) {
  volatile float x = (float)scaled / (float)(1u << GELU_LOG_SCALE);
  volatile float x2 = x * x;
  volatile float x3 = x2 * x;
  volatile float c = 0.044715f * x3;
  volatile float s = x + c;
  volatile float k = sqrtf(2.0f / 3.14159265358979323846f);
  volatile float inner = k * s;
  volatile float th = tanhf(inner);
  volatile float one_plus = 1.0f + th;
  volatile float hx = 0.5f * x;
  volatile float g = hx * one_plus;
  volatile float q = g * (float)Q_MAX;
  return (int64_t)roundf(q);
}
inline unsigned gelu_table_vars(int64_t multiplier) { return Q_BIT_LEN + dp_ceil_log2((size_t)multiplier); }  // min = -2^(7 + ceil_log2(multiplier)), max = -min (GELU::quantize, :629-659)
inline int64_t q_clamp(int64_t x) { return x < Q_MIN ? Q_MIN : x > Q_MAX ? Q_MAX : x; }
inline int64_t q_relu(int64_t x) { return x < 0 ? 0 : x; }
inline void table_columns(const TableType& tt, std::vector<int64_t>& merged, std::vector<std::vector<int64_t>>& cols) {
  merged.clear(); cols.clear();
  if (tt.kind == 0) { cols.resize(2); for (int64_t i = Q_MIN - 1; i <= Q_MAX; i++) { int64_t o = q_relu(i); merged.push_back(i + o * COLUMN_SEPARATOR); cols[0].push_back(i); cols[1].push_back(o); } }
  else if (tt.kind == 1) { cols.resize(2); int64_t mx = int64_t(1) << (tt.size - 1); for (int64_t i = -mx; i < mx; i++) { int64_t o = gelu_lut(i); merged.push_back(i + o * COLUMN_SEPARATOR); cols[0].push_back(i); cols[1].push_back(o); } }  // GELUQuantData::table: min .. max, max excluded (:579-581)
  else if (tt.kind == 2) { cols.resize(1); for (int64_t i = 0; i < (int64_t(1) << Q_BIT_LEN); i++) { merged.push_back(i); cols[0].push_back(i); } }
  else if (tt.kind == 4) { cols.resize(2); for (int64_t j = 0; j < (int64_t(1) << tt.size); j++) { int64_t o = softmax_lut(tt.aux, tt.aux2, j); merged.push_back(j + o * COLUMN_SEPARATOR); cols[0].push_back(j); cols[1].push_back(o); } }
  else if (tt.kind == 5) {  // one - error ..= one + error, cut / zero padded to 2^ceil_log2(2 error) entries (context.rs:248-264)
    cols.resize(1); const size_t n = size_t(1) << tt.vars();
    for (int64_t v = SM_OUT_ONE - tt.aux2; v <= SM_OUT_ONE + tt.aux2 && merged.size() < n; v++) { merged.push_back(v); cols[0].push_back(v); }
    while (merged.size() < n) { merged.push_back(0); cols[0].push_back(0); }
  }
  else if (tt.kind == 6) { cols.resize(2); for (int64_t i = 0; i < (int64_t(1) << tt.size); i++) { int64_t o = i != 0 ? 0 : 1; merged.push_back(i + o * COLUMN_SEPARATOR); cols[0].push_back(i); cols[1].push_back(o); } }
  else if (tt.kind == 7) { cols.resize(2); int64_t mx = int64_t(1) << (2 * (Q_BIT_LEN - 1)); for (int64_t i = -mx; i < mx; i++) { int64_t o = inv_sqrt_lut(tt.aux, tt.size, i); merged.push_back(i + o * COLUMN_SEPARATOR); cols[0].push_back(i); cols[1].push_back(o); } }
  else { cols.resize(2); int64_t mx = int64_t(1) << (tt.size - 1); for (int64_t i = -mx; i < mx; i++) { int64_t o = q_clamp(i); merged.push_back(i + o * COLUMN_SEPARATOR); cols[0].push_back(i); cols[1].push_back(o); } }
}

inline TableType gelu_table(const LayerSpec& l) { TableType t{1, gelu_table_vars(l.fixed_point_multiplier)}; t.aux2 = l.fixed_point_multiplier; return t; }  // (a GELU node keeps its multiplier where a Requant keeps its own)
// Activation::Gelu on Elements (GELU::apply, activation.rs:661-671): the table is looked up at input * multiplier. The reference accepts scaled == max, which is
// no row of its table (the lookup argument then fails): refused here
inline int64_t gelu_op(const LayerSpec& l, int64_t v) {
  const int64_t mx = int64_t(1) << (gelu_table_vars(l.fixed_point_multiplier) - 1), scaled = v * l.fixed_point_multiplier;
  DP_REQUIRE(v >= -(int64_t(1) << 20) && v <= (int64_t(1) << 20) && scaled >= -mx && scaled < mx, DP_ERR_ARG, "gelu: input out of range");
  return gelu_lut(scaled);
}
inline TableType layernorm_table(const LayerSpec& l) { TableType t{7, l.ln_range_check_bits}; t.aux = l.ln_eps_bits; return t; }
// LayerNorm::evaluate on Elements (layernorm.rs:394-470): per row, multiplier (N sum x^2 - (sum x)^2) is split into the bits that are range
// checked and the input of the inverse-square-root table; out = gamma (N x - sum x) lut(input) + beta
struct LayerNormTrace { std::vector<int64_t> lookup_input, lookup_output, range_check, row_sum; };
inline std::vector<int64_t> layernorm_op(const LayerSpec& l, const std::vector<int64_t>& x, LayerNormTrace* d) {
  const size_t fd = l.weights.size();
  DP_REQUIRE((fd && !(fd & (fd - 1))) && l.bias.size() == fd && x.size() % fd == 0 && l.ln_dim_size >= 1 && l.ln_dim_size <= fd, DP_ERR_SHAPE, "layernorm: shapes");
  const int64_t n = (int64_t)l.ln_dim_size, mask = (int64_t(1) << l.ln_range_check_bits) - 1, tmax = int64_t(1) << (2 * (Q_BIT_LEN - 1));
  std::vector<int64_t> o(x.size());
  for (size_t c = 0; c < x.size() / fd; c++) {
    int64_t sq = 0, sum = 0;
    for (size_t i = 0; i < fd; i++) { const int64_t v = x[c * fd + i]; DP_REQUIRE(v >= -(int64_t(1) << 20) && v <= (int64_t(1) << 20), DP_ERR_ARG, "layernorm: input out of range"); sq += v * v; sum += v; }
    const int64_t full = n * l.ln_multiplier * sq - l.ln_multiplier * sum * sum;
    const int64_t in = full >> l.ln_range_check_bits;
    DP_REQUIRE(in >= -tmax && in < tmax, DP_ERR_ARG, "layernorm: the inverse square root input leaves its table");
    const int64_t inv = inv_sqrt_lut(l.ln_eps_bits, l.ln_range_check_bits, in);
    if (d) { d->lookup_input.push_back(in); d->lookup_output.push_back(inv); d->range_check.push_back(full & mask); d->row_sum.push_back(sum); }
    for (size_t i = 0; i < fd; i++) o[c * fd + i] = l.weights[i] * (n * x[c * fd + i] - sum) * inv + l.bias[i];
  }
  return o;
}

inline TableType softmax_table(const LayerSpec& l) { TableType t{4, l.sm_table_size}; t.aux = l.sm_temp_bits; t.aux2 = l.sm_bkm; return t; }
inline TableType softmax_error_table(const LayerSpec& l) { TableType t{5, 0}; t.aux2 = l.sm_allowable_error; return t; }
// Softmax::evaluate on Elements (softmax.rs:455-566) with calculate_shift_data (:250-320: per row, minus the logarithm of the sum of the
// exponentials of its unmasked entries, computed in f32 — a WITNESS, any shift whose row sum lands in the error table is accepted) and the causal
// AttentionMask (:1590-1750). |masked input| = low byte | high byte | exponential table input | zero table inputs
struct SoftmaxTrace {
  std::vector<int64_t> shift, shifted_input, tril, bias, low, high, exp_in, exp_out, row_sums;
  std::vector<std::vector<int64_t>> zero_in, zero_out;
};
// the shift of one row whose first `take` entries the causal mask keeps (the entries already range checked). The only data-dependent floating
// point of the inference: softmax_op and the shift step of dp_model_infer_ex (infer.h) both call it, so the two paths share its roundings
inline int64_t softmax_row_shift(const LayerSpec& l, const int64_t* row, size_t take) {
  if (take == 1) return -row[0] * l.sm_scalar;
  float inv_temp, in_scale; memcpy(&inv_temp, &l.sm_temp_bits, 4); memcpy(&in_scale, &l.sm_in_scale_bits, 4);
  int64_t mx = row[0]; for (size_t j = 1; j < take; j++) mx = std::max(mx, row[j]);
  float sum = 0.0f;
  for (size_t j = 0; j < take; j++) sum += expf(((float)(row[j] - mx) * in_scale) / inv_temp);
  return -(int64_t)roundf((float)(1u << SM_LOG_SCALE) * inv_temp * logf(sum)) - mx * l.sm_scalar;
}
inline std::vector<int64_t> softmax_op(const LayerSpec& l, const std::vector<int64_t>& x, SoftmaxTrace* out) {
  const size_t C = l.sm_shape[0], R = l.sm_shape[1], K = l.sm_shape[2];
  DP_REQUIRE(C && R && R == K && x.size() == C * R * K, DP_ERR_SHAPE, "softmax: shapes");
  SoftmaxTrace d;
  const int64_t neg_inf = -(((l.sm_bkm >> 16) + 1) << 16);
  for (size_t i = 0; i < C * R; i++) {
    const int64_t* row = &x[i * K]; const size_t take = i % R + 1;
    for (size_t j = 0; j < K; j++) DP_REQUIRE(row[j] >= -(int64_t(1) << 24) && row[j] <= (int64_t(1) << 24), DP_ERR_ARG, "softmax: input out of range");
    d.shift.push_back(softmax_row_shift(l, row, take));
  }
  d.tril.resize(x.size()); d.bias.resize(x.size()); d.shifted_input.resize(x.size());
  for (size_t i = 0; i < C * R; i++) for (size_t j = 0; j < K; j++) {
    const bool keep = j <= i % R;
    d.tril[i * K + j] = keep ? 1 : 0; d.bias[i * K + j] = keep ? 0 : neg_inf;
    d.shifted_input[i * K + j] = x[i * K + j] * l.sm_scalar + d.shift[i];
  }
  const unsigned tv = l.sm_table_size;
  const int64_t tmask = (int64_t(1) << tv) - 1, zmask = (int64_t(1) << l.sm_zero_vars) - 1;
  d.zero_in.resize(l.sm_zero_chunks); d.zero_out.resize(l.sm_zero_chunks);
  std::vector<int64_t> o; o.reserve(x.size());
  for (size_t q = 0; q < x.size(); q++) {
    const int64_t masked = d.shifted_input[q] * d.tril[q] + d.bias[q];
    int64_t r = masked < 0 ? -masked : masked;
    d.low.push_back(r & 255); r >>= 8; d.high.push_back(r & 255); r >>= 8;
    const int64_t lk = r & tmask, ev = softmax_lut(l.sm_temp_bits, l.sm_bkm, lk);
    d.exp_in.push_back(lk); d.exp_out.push_back(ev); r >>= tv;
    int64_t acc = ev;
    for (unsigned z = 0; z < l.sm_zero_chunks; z++) { const int64_t zi = r & zmask, zo = zi != 0 ? 0 : 1; d.zero_in[z].push_back(zi); d.zero_out[z].push_back(zo); r >>= l.sm_zero_vars; acc *= zo; }
    o.push_back(acc);
  }
  for (size_t i = 0; i < C * R; i++) { int64_t a = 0; for (size_t j = 0; j < K; j++) a += o[i * K + j]; d.row_sums.push_back(a); }
  if (out) *out = std::move(d);
  return o;
}

// ---- inference (the reference's Model::run; CPU pre-processing outside "proving time", zkml/src/bin/bench.rs:341-352)
// ConvData (tensor.rs:326-372) in the base field: what the FFT convolution computes on the way, kept for the prover
struct ConvTrace {
  std::vector<u64> input_pad;   // [kx][2n^2]: every input channel reversed (index_x) and zero-padded to the FFT length
  std::vector<u64> input_fft;   // [kx][2n^2]
  std::vector<u64> prod;        // [kw][2n^2]: sum_j FFT(x_j) o FFT(w_ij)
  std::vector<int64_t> output_as_element;  // conv output after the bias, before clearing (convolution.rs:311-316)
};
// per node: first input, first output; in2 = second input of a two-input node; more_out = the outputs after the first (QKV: K, V)
// MhaData (mha.rs:45-52): the products Q K^T the softmax reads and the probabilities final_mul reads (its output is the node's: final_reshape moves nothing)
struct MhaTrace { std::vector<int64_t> softmax_in, softmax_out; };
// ArgmaxData (logits.rs:48-51): the row maxima of every Logits node (its output holds the indices)
struct Trace {
  std::vector<std::vector<int64_t>> in, out, in2, in3; std::vector<std::vector<std::vector<int64_t>>> more_out; std::vector<ConvTrace> conv; std::map<size_t, MhaTrace> mha;
  std::map<size_t, std::vector<int64_t>> argmax_max;
  const std::vector<int64_t>& tensor(int node, int slot) const { return slot == 0 ? out[(size_t)node] : more_out[(size_t)node][(size_t)slot - 1]; }
};
// FFT of every kernel of a convolution, zero-padded to 2 nw^2 (index_w, tensor.rs:236-254): computed once per model —
// the reference recomputes these kw*kx transforms at every inference (tensor.rs:494-507)
inline std::shared_ptr<const std::vector<u64>> conv_weight_fft(const LayerSpec& l) {
  size_t N = 2 * l.nw * l.nw, fsz = l.real_nw * l.real_nw;
  auto w = std::make_shared<std::vector<u64>>(l.kw * l.kx * N, 0);
  for (size_t ij = 0; ij < l.kw * l.kx; ij++) {
    u64* o = w->data() + ij * N;
    for (size_t a = 0; a < l.real_nw; a++) for (size_t b = 0; b < l.real_nw; b++) o[a * l.nw + b] = gl_from_i64(l.weights[ij * fsz + a * l.real_nw + b]);
    gl_fft(o, N, false);
  }
  return w;
}
// Tensor::fft_conv (tensor.rs:458-523) + Convolution::op (convolution.rs:303-336)
inline std::vector<int64_t> conv_op(const LayerSpec& l, const std::vector<int64_t>& x, ConvTrace& ct) {
  size_t nn = l.nw * l.nw, N = 2 * nn;
  DP_REQUIRE(x.size() == l.kx * nn, DP_ERR_SHAPE, "conv: input size mismatch");
  std::shared_ptr<const std::vector<u64>> wf = l.wfft ? l.wfft : conv_weight_fft(l);
  ct.input_pad.assign(l.kx * N, 0);
  for (size_t j = 0; j < l.kx; j++) for (size_t t = 0; t < nn; t++) ct.input_pad[j * N + t] = gl_from_i64(x[j * nn + nn - 1 - t]);
  ct.input_fft = ct.input_pad;
  for (size_t j = 0; j < l.kx; j++) gl_fft(ct.input_fft.data() + j * N, N, false);
  ct.prod.assign(l.kw * N, 0);
  for (size_t i = 0; i < l.kw; i++) {
    u64* o = ct.prod.data() + i * N;
    for (size_t j = 0; j < l.kx; j++) {
      const u64* xf = ct.input_fft.data() + j * N; const u64* w = wf->data() + (i * l.kx + j) * N;
      for (size_t k = 0; k < N; k++) o[k] = gl_add(o[k], gl_mul(xf[k], w[k]));
    }
  }
  std::vector<u64> out = ct.prod;
  std::vector<int64_t> o(l.kw * nn);
  for (size_t i = 0; i < l.kw; i++) {
    gl_fft(out.data() + i * N, N, true);
    for (size_t p = 0; p < nn; p++) o[i * nn + p] = gl_to_element(out[i * N + nn - 1 - p]) + l.bias[i];  // index_u + add_bias
  }
  ct.output_as_element = o;
  for (size_t i = 0; i < l.kw; i++) for (size_t j = 0; j < l.nw; j++) for (size_t k = 0; k < l.nw; k++)  // clear_garbage
    if (!(i < l.unp_out[0] && j < l.unp_out[1] && k < l.unp_out[2])) o[i * nn + j * l.nw + k] = 0;
  return o;
}
// new_clearing_tensor (convolution.rs:1508-1529)
inline std::vector<int64_t> clearing_tensor(const LayerSpec& l) {
  std::vector<int64_t> d(l.kw * l.nw * l.nw, 0);
  for (size_t i = 0; i < l.unp_out[0]; i++) for (size_t j = 0; j < l.unp_out[1]; j++) for (size_t k = 0; k < l.unp_out[2]; k++) d[(i * l.nw + j) * l.nw + k] = 1;
  return d;
}
// Tensor::maxpool2d, kernel = stride = 2 (tensor.rs:1335-1383)
inline std::vector<int64_t> maxpool_op(const LayerSpec& l, const std::vector<int64_t>& x) {
  size_t c = l.pin[0], h = l.pin[1], w = l.pin[2], oh = h / 2, ow = w / 2;
  DP_REQUIRE(x.size() == c * h * w, DP_ERR_SHAPE, "maxpool: input size mismatch");
  std::vector<int64_t> o(c * oh * ow);
  for (size_t n = 0; n < c; n++) for (size_t i = 0; i < oh; i++) for (size_t j = 0; j < ow; j++) {
    const int64_t* p = &x[n * h * w + 2 * i * w + 2 * j];
    o[(n * oh + i) * ow + j] = std::max(std::max(p[0], p[1]), std::max(p[w], p[w + 1]));
  }
  return o;
}
// Maxpool2D::compute_polys (pooling.rs:686-767): output - input at the kernel offsets (dy,dx) = (0,0),(1,0),(0,1),(1,1)
inline std::vector<std::vector<int64_t>> maxpool_diff_polys(const LayerSpec& l, const std::vector<int64_t>& x, const std::vector<int64_t>& out) {
  size_t c = l.pin[0], h = l.pin[1], w = l.pin[2], oh = h / 2, ow = w / 2;
  std::vector<std::vector<int64_t>> cols(4, std::vector<int64_t>(out.size()));
  static const size_t dy[4] = {0, 1, 0, 1}, dx[4] = {0, 0, 1, 1};
  for (int q = 0; q < 4; q++)
    for (size_t n = 0; n < c; n++) for (size_t i = 0; i < oh; i++) for (size_t j = 0; j < ow; j++) {
      size_t oi = (n * oh + i) * ow + j;
      cols[q][oi] = out[oi] - x[n * h * w + (2 * i + dy[q]) * w + 2 * j + dx[q]];
    }
  return cols;
}
// length of the model's output tensor (the shape propagation of run_model without the arithmetic)
// lens[id] = length of (each of) node id's output tensors; in_len[id] = length of its first input
inline void tensor_lens(const ModelSpec& m, std::vector<size_t>& lens, std::vector<size_t>* in_len = nullptr, std::vector<size_t>* in2_len = nullptr, std::vector<size_t>* in3_len = nullptr) {
  const std::vector<size_t> ins = input_tensor_lens(m);
  lens.assign(m.layers.size(), 0);
  if (in_len) in_len->assign(m.layers.size(), 0);
  if (in2_len) in2_len->assign(m.layers.size(), 0);
  if (in3_len) in3_len->assign(m.layers.size(), 0);
  for (size_t id = 0; id < m.layers.size(); id++) {
    const LayerSpec& l = m.layers[id];
    const std::vector<Edge> e = edges_in(m, id);
    DP_REQUIRE(e.size() == in_degree(l), DP_ERR_SHAPE, "model graph: wrong number of inputs for a node");
    size_t got[3] = {0, 0, 0};
    for (size_t q = 0; q < e.size(); q++) {
      DP_REQUIRE(e[q].from < (int)id && (e[q].from >= 0 ? e[q].slot >= 0 && (size_t)e[q].slot < out_degree(m.layers[(size_t)e[q].from]) : e[q].slot >= 0 && (size_t)e[q].slot < ins.size()), DP_ERR_SHAPE, "model graph: an edge must come from an earlier node or a model input");
      got[q] = e[q].from < 0 ? ins[(size_t)e[q].slot] : lens[(size_t)e[q].from];
    }
    size_t cur = got[0];
    if (in_len) (*in_len)[id] = got[0];
    if (in2_len) (*in2_len)[id] = got[1];
    if (in3_len) (*in3_len)[id] = got[2];
    if (l.kind == L_DENSE) cur = l.nrows;
    else if (l.kind == L_MATMUL || l.kind == L_MATMUL2 || l.kind == L_QKV) cur = l.nrows ? cur / l.nrows * l.ncols : 0;
    else if (l.kind == L_EMBED) cur = cur * l.ncols;
    else if (l.kind == L_CONV) cur = l.kw * l.nw * l.nw;
    else if (l.kind == L_MAXPOOL) cur = l.pin[0] * (l.pin[1] / 2) * (l.pin[2] / 2);
    else if (l.kind == L_CONCAT_MATMUL) { const CmShape g = cm_shape(l); cur = g.out[0] * g.out[1] * g.out[2]; }
    else if (l.kind == L_LOGITS) cur = l.nrows;
    lens[id] = cur;
  }
}
inline size_t model_output_len(const ModelSpec& m) {
  std::vector<size_t> lens; tensor_lens(m, lens);
  size_t n = 0; for (const Edge& e : output_edges(m)) n += lens.at((size_t)e.from);
  return n;
}
// the two inner loops of the int16 inference paths, cloned for the vector ISAs of the host (resolved once at load time): the library is
// built for baseline x86-64, where 32-bit multiplies do not vectorise
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define DP_HOST_CLONES __attribute__((target_clones("avx512f", "avx2", "default")))
#else
#define DP_HOST_CLONES
#endif
DP_HOST_CLONES inline int32_t dot_i16(const int16_t* a, const int16_t* b, size_t n) { int32_t s = 0; for (size_t i = 0; i < n; i++) s += (int32_t)a[i] * (int32_t)b[i]; return s; }
DP_HOST_CLONES inline void axpy_i16(int32_t* acc, int32_t x, const int16_t* w, size_t n) { for (size_t j = 0; j < n; j++) acc[j] += x * (int32_t)w[j]; }
// the weights of a Dense / MatMul layer once more as int16 when they all fit (quantised models: |w| <= 127): the inference that precedes
// every proof then streams a quarter of the bytes and its multiply-adds vectorise in 32-bit lanes
// |v| without the overflow of -INT64_MIN (2^63 as an unsigned value: beyond every bound it is compared with)
inline uint64_t abs_u64(int64_t v) { return v < 0 ? 0 - (uint64_t)v : (uint64_t)v; }
inline void prepare_fast_inference(LayerSpec& l) {
  if (l.kind != L_DENSE && l.kind != L_MATMUL && l.kind != L_QKV) return;
  uint64_t wm = 0; for (int64_t v : l.weights) wm = std::max(wm, abs_u64(v));
  if (wm > 32767) return;
  auto w16 = std::make_shared<std::vector<int16_t>>(l.weights.size());
  for (size_t j = 0; j < l.weights.size(); j++) (*w16)[j] = (int16_t)l.weights[j];
  l.w16 = w16; l.w16_max = (int64_t)wm;
}
// [s][k] activations (as int16) times a constant [k][n] matrix (or its transpose [n][k]) kept as int16, exact in int32 (the caller has checked the bound), + bias:
// eight rows of the activation share every pass over the matrix — a row of W (2 KB at n = 1024) is read once per eight tokens
inline void matmul_w16(const int16_t* x16, size_t s_, size_t k, size_t n, const int16_t* w16, bool transposed, const int64_t* bias, int64_t* o) {
  const size_t TB = 8;
  std::vector<int32_t> acc(TB * n);
  for (size_t i0 = 0; i0 < s_; i0 += TB) {
    const size_t tb = std::min(TB, s_ - i0);
    if (transposed) { for (size_t j = 0; j < n; j++) { const int16_t* w = w16 + j * k; for (size_t t = 0; t < tb; t++) acc[t * n + j] = dot_i16(&x16[(i0 + t) * k], w, k); } }
    else {
      std::fill(acc.begin(), acc.begin() + tb * n, 0);
      for (size_t q = 0; q < k; q++) { const int16_t* w = w16 + q * n; for (size_t t = 0; t < tb; t++) { const int32_t xv = x16[(i0 + t) * k + q]; if (xv) axpy_i16(&acc[t * n], xv, w, n); } }
    }
    for (size_t t = 0; t < tb; t++) { int64_t* row = &o[(i0 + t) * n]; const int32_t* a = &acc[t * n]; for (size_t j = 0; j < n; j++) row[j] = (int64_t)a[j] + (bias ? bias[j] : 0); }
  }
}
// the model's output tensors, concatenated (ModelSpec::outputs order)
inline std::vector<int64_t> model_output(const ModelSpec& m, const Trace& tr) {
  const std::vector<Edge> outs = output_edges(m);
  if (outs.size() == 1) return tr.tensor(outs[0].from, outs[0].slot);
  std::vector<int64_t> o;
  for (const Edge& e : outs) { const std::vector<int64_t>& v = tr.tensor(e.from, e.slot); o.insert(o.end(), v.begin(), v.end()); }
  return o;
}
// plain integer products of the two-input nodes (tiny next to the proving that follows)
inline std::vector<int64_t> matmul_i64(const int64_t* a, const int64_t* b, size_t s_, size_t k, size_t n, bool b_transposed) {
  std::vector<int64_t> o(s_ * n, 0);
  for (size_t i = 0; i < s_; i++) {
    int64_t* row = &o[i * n];
    if (b_transposed) for (size_t j = 0; j < n; j++) { int64_t acc = 0; for (size_t q = 0; q < k; q++) acc += a[i * k + q] * b[j * k + q]; row[j] = acc; }
    else for (size_t q = 0; q < k; q++) { const int64_t x = a[i * k + q]; const int64_t* w = b + q * n; for (size_t j = 0; j < n; j++) row[j] += x * w[j]; }
  }
  return o;
}
// ConcatMatMul::evaluate (concat_matmul.rs:568-616)
inline std::vector<int64_t> concat_matmul_op(const LayerSpec& l, const std::vector<int64_t>& cur, const std::vector<int64_t>& b0) {
  std::vector<int64_t> o;
    DP_REQUIRE(cur.size() == l.cm_a[0] * l.cm_a[1] * l.cm_a[2] && b0.size() == l.cm_b[0] * l.cm_b[1] * l.cm_b[2], DP_ERR_SHAPE, "concat matmul: input shapes");
    const CmShape g = cm_shape(l);
    int order[3]; bool same;
    cm_axes_to(l.cm_left, CM_WANT_LEFT, order, same);
    const std::vector<int64_t> a = same ? cur : transpose3(cur, l.cm_a, order);
    cm_axes_to(l.cm_right, CM_WANT_RIGHT, order, same);
    const std::vector<int64_t> b = same ? b0 : transpose3(b0, l.cm_b, order);
    std::vector<int64_t> r;
    for (size_t c = 0; c < g.C; c++) { std::vector<int64_t> y = matmul_i64(&a[c * g.R * g.M], &b[c * g.M * g.N], g.R, g.M, g.N, false); r.insert(r.end(), y.begin(), y.end()); }
    if (l.cm_perm.empty()) o = std::move(r);
    else { const size_t rs[3] = {g.C, g.R, g.N}; const int po[3] = {l.cm_perm[0], l.cm_perm[1], l.cm_perm[2]}; o = transpose3(r, rs, po); }
  return o;
}
// max_in_slice (zkml/src/lib.rs:194-206) on every row of a [rows][K] tensor: a fold from (MIN, 0) that moves on a STRICTLY greater value — the index
// of the first maximum, 0 for a row of equal values
inline std::vector<int64_t> argmax_rows(const std::vector<int64_t>& x, size_t rows, size_t K, std::vector<int64_t>& maxima) {
  std::vector<int64_t> idx(rows); maxima.resize(rows);
  for (size_t r = 0; r < rows; r++) {
    int64_t best = INT64_MIN; size_t at = 0;
    for (size_t j = 0; j < K; j++) if (x[r * K + j] > best) { best = x[r * K + j]; at = j; }
    idx[r] = (int64_t)at; maxima[r] = best;
  }
  return idx;
}
inline Trace run_model(const ModelSpec& m, const std::vector<int64_t>& input) {
  Trace tr;
  DP_REQUIRE(input.size() == m.input_len, DP_ERR_SHAPE, "input length mismatch");
  const std::vector<size_t> in_lens = input_tensor_lens(m);
  auto fetch = [&](const Edge& e) -> std::vector<int64_t> {
    if (e.from >= 0) { DP_REQUIRE((size_t)e.from < tr.out.size(), DP_ERR_SHAPE, "model graph: an edge must come from an earlier node"); return tr.tensor(e.from, e.slot); }
    size_t off = 0; for (int q = 0; q < e.slot; q++) off += in_lens.at((size_t)q);
    DP_REQUIRE((size_t)e.slot < in_lens.size() && off + in_lens[(size_t)e.slot] <= input.size(), DP_ERR_SHAPE, "model graph: input tensor");
    return std::vector<int64_t>(input.begin() + off, input.begin() + off + in_lens[(size_t)e.slot]);
  };
  tr.in2.resize(m.layers.size()); tr.in3.resize(m.layers.size()); tr.more_out.resize(m.layers.size());
  for (size_t id = 0; id < m.layers.size(); id++) {
    const LayerSpec& l = m.layers[id];
    const std::vector<Edge> edges = edges_in(m, id);
    DP_REQUIRE(edges.size() == in_degree(l), DP_ERR_SHAPE, "model graph: wrong number of inputs for a node");
    std::vector<int64_t> cur = m.layers[id].inputs.empty() && id > 0 ? tr.out[id - 1] : fetch(edges[0]);
    tr.in.push_back(cur);
    if (edges.size() > 1) tr.in2[id] = fetch(edges[1]);
    if (edges.size() > 2) tr.in3[id] = fetch(edges[2]);
    std::vector<int64_t> o;
    if (l.kind == L_MATMUL2) {  // MatMul::op (matrix_mul.rs:230-311) on two inputs
      const std::vector<int64_t>& b = tr.in2[id];
      DP_REQUIRE(l.nrows && cur.size() % l.nrows == 0 && b.size() == l.nrows * l.ncols, DP_ERR_SHAPE, "matmul2: input shapes");
      o = matmul_i64(cur.data(), b.data(), cur.size() / l.nrows, l.nrows, l.ncols, l.mm_transpose);
    } else if (l.kind == L_ADD2) {  // Add::evaluate (add.rs:184-210) without operand
      const std::vector<int64_t>& b = tr.in2[id];
      DP_REQUIRE(cur.size() == b.size(), DP_ERR_SHAPE, "add2: inputs of different lengths");
      o.resize(cur.size());
      for (size_t i = 0; i < cur.size(); i++) o[i] = l.add_left * cur[i] + l.add_right * b[i];
    } else if (l.kind == L_QKV) {  // QKV::evaluate (qkv.rs:275-340, no cache)
      const size_t k = l.nrows, n = l.ncols;
      DP_REQUIRE(k && cur.size() % k == 0 && l.weights.size() == 3 * k * n && l.bias.size() == 3 * n, DP_ERR_SHAPE, "qkv: shapes");
      uint64_t xmax = 0; for (int64_t v : cur) xmax = std::max(xmax, abs_u64(v));
      const bool fast = l.w16 && xmax <= 32767 && (double)xmax * (double)l.w16_max * (double)k < 2.0e9;  // exact in int32: the same integers as matmul_i64 gives
      std::vector<int16_t> x16; if (fast) { x16.resize(cur.size()); for (size_t j = 0; j < cur.size(); j++) x16[j] = (int16_t)cur[j]; }
      for (size_t w = 0; w < 3; w++) {
        std::vector<int64_t> y;
        if (fast) { y.resize(cur.size() / k * n); matmul_w16(x16.data(), cur.size() / k, k, n, l.w16->data() + w * k * n, false, &l.bias[w * n], y.data()); }
        else { y = matmul_i64(cur.data(), &l.weights[w * k * n], cur.size() / k, k, n, false); for (size_t i = 0; i < y.size(); i++) y[i] += l.bias[w * n + i % n]; }
        if (w == 0) o = std::move(y); else tr.more_out[id].push_back(std::move(y));
      }
    } else if (l.kind == L_CONCAT_MATMUL) o = concat_matmul_op(l, cur, tr.in2[id]);
    else if (l.kind == L_MHA) {  // Mha::evaluate_with_intermediate_outputs (mha.rs:216-300): qk, softmax, final_mul on the reshaped inputs
      const size_t n = l.mha_shape[0] * l.mha_shape[1] * l.mha_shape[2];
      DP_REQUIRE(cur.size() == n && tr.in2[id].size() == n && tr.in3[id].size() == n, DP_ERR_SHAPE, "mha: input shapes");
      MhaTrace d;
      d.softmax_in = concat_matmul_op(mha_qk_spec(l), cur, tr.in2[id]);
      d.softmax_out = softmax_op(mha_softmax_spec(l), d.softmax_in, nullptr);
      o = concat_matmul_op(mha_final_spec(l), d.softmax_out, tr.in3[id]);
      tr.mha[id] = std::move(d);
    } else
    if (l.kind == L_DENSE) {
      DP_REQUIRE(cur.size() == l.ncols, DP_ERR_SHAPE, "dense input size mismatch");
      o.resize(l.nrows);
      uint64_t xmax = 0; for (int64_t v : cur) xmax = std::max(xmax, abs_u64(v));
      if (l.w16 && xmax <= 32767 && (double)xmax * (double)l.w16_max * (double)l.ncols < 2.0e9) {  // exact in int32: same integers as below
        std::vector<int16_t> x16(cur.size()); for (size_t j = 0; j < cur.size(); j++) x16[j] = (int16_t)cur[j];
        const int16_t* xp = x16.data();
        for (size_t i = 0; i < l.nrows; i++) o[i] = (int64_t)dot_i16(l.w16->data() + i * l.ncols, xp, l.ncols) + l.bias[i];
      } else
      for (size_t i = 0; i < l.nrows; i++) { int64_t a = 0; const int64_t* w = &l.weights[i * l.ncols]; for (size_t j = 0; j < l.ncols; j++) a += w[j] * cur[j]; o[i] = a + l.bias[i]; }
    } else if (l.kind == L_MATMUL) {  // MatMul::op (matrix_mul.rs:230-311): [s][k] times the constant [k][n], the bias added to every row
      const size_t k = l.nrows, n = l.ncols;
      DP_REQUIRE(k && cur.size() % k == 0, DP_ERR_SHAPE, "matmul input size mismatch");
      const size_t s_ = cur.size() / k;
      o.assign(s_ * n, 0);
      uint64_t xmax = 0; for (int64_t v : cur) xmax = std::max(xmax, abs_u64(v));
      if (l.w16 && xmax <= 32767 && (double)xmax * (double)l.w16_max * (double)k < 2.0e9) {  // exact in int32: the same integers as the int64 loops below
        std::vector<int16_t> x16(cur.size()); for (size_t j = 0; j < cur.size(); j++) x16[j] = (int16_t)cur[j];
        matmul_w16(x16.data(), s_, k, n, l.w16->data(), l.mm_transpose, l.bias.empty() ? nullptr : l.bias.data(), o.data());
      } else
      for (size_t i = 0; i < s_; i++) {
        int64_t* row = &o[i * n];
        if (l.mm_transpose) for (size_t j = 0; j < n; j++) { const int64_t* w = &l.weights[j * k]; const int64_t* x = &cur[i * k]; int64_t a = 0; for (size_t q = 0; q < k; q++) a += x[q] * w[q]; row[j] = a; }
        else for (size_t q = 0; q < k; q++) { const int64_t x = cur[i * k + q]; const int64_t* w = &l.weights[q * n]; for (size_t j = 0; j < n; j++) row[j] += x * w[j]; }
        if (!l.bias.empty()) for (size_t j = 0; j < n; j++) row[j] += l.bias[j];
      }
    } else if (l.kind == L_EMBED) {  // Embeddings::evaluate (embeddings.rs:197-236): row x[i] of the table for every token
      o.resize(cur.size() * l.ncols);
      for (size_t i = 0; i < cur.size(); i++) {
        DP_REQUIRE(cur[i] >= 0 && (size_t)cur[i] < l.nrows, DP_ERR_ARG, "embeddings: token outside the vocabulary");
        memcpy(&o[i * l.ncols], &l.weights[(size_t)cur[i] * l.ncols], l.ncols * sizeof(int64_t));
      }
    } else if (l.kind == L_POSITIONAL) {  // Positional::evaluate (positional.rs:157-185): the Add layer on (x, the first rows of the table)
      DP_REQUIRE(l.ncols && cur.size() % l.ncols == 0 && cur.size() <= l.weights.size(), DP_ERR_SHAPE, "positional: input shape");
      o.resize(cur.size());
      for (size_t i = 0; i < cur.size(); i++) o[i] = l.add_left * cur[i] + l.add_right * l.weights[i];
    } else if (l.kind == L_ADD) {  // Add::evaluate (add.rs:184-210)
      DP_REQUIRE(cur.size() == l.weights.size(), DP_ERR_SHAPE, "add: operand size mismatch");
      o.resize(cur.size());
      for (size_t i = 0; i < cur.size(); i++) o[i] = l.add_left * cur[i] + l.add_right * l.weights[i];
    } else if (l.kind == L_REQUANT) {
      unsigned sh = l.shift();
      for (int64_t v : cur) {
        DP_REQUIRE(abs_u64(v) <= (uint64_t(1) << l.intermediate_bit_size), DP_ERR_ARG, "requant: value exceeds intermediate bit size");
        o.push_back(q_clamp((v * l.fixed_point_multiplier + (int64_t(1) << (sh - 1))) >> sh));
      }
    } else if (l.kind == L_RELU) for (int64_t v : cur) o.push_back(q_relu(v));
    else if (l.kind == L_GELU) for (int64_t v : cur) o.push_back(gelu_op(l, v));
    else if (l.kind == L_LAYERNORM) o = layernorm_op(l, cur, nullptr);
    else if (l.kind == L_SOFTMAX) o = softmax_op(l, cur, nullptr);
    else if (l.kind == L_CONV) { tr.conv.resize(m.layers.size()); o = conv_op(l, cur, tr.conv[tr.in.size() - 1]); }
    else if (l.kind == L_MAXPOOL) o = maxpool_op(l, cur);
    else if (l.kind == L_FLATTEN) o = cur;
    else if (l.kind == L_LOGITS) {  // Logits::evaluate_with_argmax_data (logits.rs:90-125)
      DP_REQUIRE(l.nrows && l.ncols && cur.size() == l.nrows * l.ncols, DP_ERR_SHAPE, "logits: input shape");
      o = argmax_rows(cur, l.nrows, l.ncols, tr.argmax_max[id]);
    }
    else DP_REQUIRE(false, DP_ERR_ARG, "unknown layer kind");
    tr.out.push_back(std::move(o));
  }
  return tr;
}

inline size_t next_pow2(size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; }
inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

// ---- what the verifier needs (the serialisable part of Context)
struct VerifierContext {
  ModelSpec shape;  // weights/bias vectors left empty
  unsigned full_log = 0;
  std::map<size_t, std::map<std::string, Commitment>> model_comms;
  std::vector<TableType> tables;
  std::map<TableType, Commitment> table_comms;
};

struct Context {
  Dev* dev = nullptr;
  ModelSpec model;
  unsigned full_log = 0;
  size_t max_poly_len = 0;
  std::map<size_t, std::map<std::string, DevCommit>> model_comms;  // BTreeMap<NodeId, BTreeMap<PolyId, ..>>
  std::map<size_t, DBuf> weights_dev;                              // base-field weight matrices kept for K2
  struct ConvDev { DBuf wfft, clearing; };                          // conv: kernel FFTs [kw][kx*2n^2] and the 0/1 clearing tensor
  std::map<size_t, ConvDev> conv_dev;
  std::vector<TableType> tables;
  std::map<TableType, DevCommit> table_comms;  // the committed columns of the tables that have one (commit/context.rs:105-107)
  // The columns of a lookup table are a property of the MODEL: built once per context (a softmax table is 2^size calls of expf, an inverse-square-root
  // table 2^14 of sqrt), not once per proof as until round 4. inv_cnt[i] = 1 / (number of rows of the table that hold merged[i]) — the zero padding
  // of an error table repeats a row —, so that a proof's multiplicity of row i is count(merged[i]) * inv_cnt[i]. Shared by the workers of a batch.
  struct TableData { std::vector<int64_t> merged; std::vector<std::vector<int64_t>> cols; std::vector<u64> inv_cnt; };
  // ... and they live ON THE DEVICE for the life of the context, as the weights do (round 5): until then the tables' columns rode in every proof's witness
  // upload — 68 352 of the 113 444 words of a Dense-4M proof, 307 k of 649 k for CNN-264k, 330 k of 1.87 M for the transformer layer. Base-field columns in
  // commit order of the table's proof; read-only, shared by the workers of a batch (persistent buffers belong to the device).
  std::map<TableType, std::vector<DBuf>> table_cols_dev;
  mutable std::mutex table_data_mu; mutable std::map<TableType, std::unique_ptr<TableData>> table_data_;
  const TableData& table_data(const TableType& tt) const {
    std::lock_guard<std::mutex> g(table_data_mu);
    auto it = table_data_.find(tt);
    if (it != table_data_.end()) return *it->second;
    std::unique_ptr<TableData> d(new TableData);
    table_columns(tt, d->merged, d->cols);
    std::unordered_map<int64_t, u64> cnt; cnt.reserve(d->merged.size());
    for (int64_t v : d->merged) cnt[v] += 1;
    d->inv_cnt.resize(d->merged.size());
    for (size_t i = 0; i < d->merged.size(); i++) { const u64 c = cnt[d->merged[i]]; d->inv_cnt[i] = c != 1 ? gl_inv(gl_from_u64(c)) : 1; }
    return *(table_data_[tt] = std::move(d));
  }
  VerifierContext verifier_ctx() const {
    VerifierContext v; v.full_log = full_log; v.tables = tables;
    for (auto& kv : table_comms) v.table_comms[kv.first] = pure_commitment(kv.second); v.shape.input_len = model.input_len; v.shape.input_lens = model.input_lens; v.shape.outputs = model.outputs;
    for (auto& l : model.layers) { LayerSpec s = l; s.weights.clear(); s.bias.clear(); s.wfft.reset(); s.w16.reset(); v.shape.layers.push_back(s); }
    for (auto& kv : model_comms) for (auto& pc : kv.second) v.model_comms[kv.first][pc.first] = pure_commitment(pc.second);
    return v;
  }
  ~Context() {
    if (!dev) return;
    for (auto& kv : model_comms) for (auto& pc : kv.second) dev->free_commit(pc.second);
    for (auto& kv : table_comms) dev->free_commit(kv.second);
    for (auto& kv : conv_dev) { dev->free_persistent(kv.second.wfft); dev->free_persistent(kv.second.clearing); }
    for (auto& kv : table_cols_dev) for (DBuf& b : kv.second) dev->free_persistent(b);
  }
};

inline void validate_model(const ModelSpec& m) {
  DP_REQUIRE(!m.layers.empty() && m.layers.size() < 4096, DP_ERR_SHAPE, "model: no layers");
  { size_t tot = 0; for (size_t n : input_tensor_lens(m)) { DP_REQUIRE(is_pow2(n), DP_ERR_SHAPE, "model: input length must be a power of two"); tot += n; }
    DP_REQUIRE(tot == m.input_len, DP_ERR_SHAPE, "model: the input tensors do not add up to input_len"); }
  std::vector<size_t> lens, in_len, in2_len, in3_len;
  tensor_lens(m, lens, &in_len, &in2_len, &in3_len);
  for (const Edge& e : output_edges(m)) DP_REQUIRE(e.from >= 0 && (size_t)e.from < m.layers.size() && e.slot >= 0 && (size_t)e.slot < out_degree(m.layers[(size_t)e.from]), DP_ERR_SHAPE, "model graph: output edge");
  // a Logits node is checked against io.output by the verifier itself, which wants exactly one output tensor (verify_output_evaluation, logits.rs:693-701):
  // its output is the model's only output tensor and no node reads it
  for (size_t id = 0; id < m.layers.size(); id++) if (m.layers[id].kind == L_LOGITS) {
    const std::vector<Edge> outs = output_edges(m);
    bool read = false;
    for (size_t q = 0; q < m.layers.size(); q++) for (const Edge& e : edges_in(m, q)) read = read || e.from == (int)id;
    DP_REQUIRE(outs.size() == 1 && outs[0].from == (int)id && outs[0].slot == 0 && !read, DP_ERR_ARG, "node " + std::to_string(id) + " (kind 18, logits): its output must be the model's only output tensor, read by no node");
  }
  for (size_t id = 0; id < m.layers.size(); id++) for (size_t j = 0; j < out_degree(m.layers[id]); j++) reader_of(m, (int)id, (int)j);  // exactly one reader each
  { std::vector<size_t> ins = input_tensor_lens(m); for (size_t q = 0; q < ins.size(); q++) reader_of(m, -1, (int)q); }
  auto check_softmax = [](const LayerSpec& l, size_t cur) {
    DP_REQUIRE(is_pow2(l.sm_shape[0]) && is_pow2(l.sm_shape[1]) && l.sm_shape[1] == l.sm_shape[2] && l.sm_shape[1] >= 2 && cur == l.sm_shape[0] * l.sm_shape[1] * l.sm_shape[2] && l.sm_shape[0] * l.sm_shape[1] >= 4, DP_ERR_SHAPE, "softmax: a padded [c][n][n] input with at least four rows");
    DP_REQUIRE(l.sm_scalar >= 1 && l.sm_scalar < (int64_t(1) << 30) && l.sm_bkm >= (int64_t(1) << 17) && l.sm_bkm < (int64_t(1) << 40) && l.sm_table_size == dp_ceil_log2((size_t)(l.sm_bkm >> 16)) && l.sm_table_size <= 22, DP_ERR_ARG, "softmax: multiplier / bkm / table size");
    DP_REQUIRE(l.sm_zero_chunks <= 3 && (l.sm_zero_chunks == 0) == (l.sm_zero_vars == 0) && l.sm_zero_vars <= 22 && l.sm_allowable_error >= 1 && l.sm_allowable_error <= (1 << 11), DP_ERR_ARG, "softmax: zero tables / allowable error");
    // (the lookup argument here wants columns of at least four entries, logup.h: a one-bit zero table or an error table of two entries is
    // refused; a front end can always widen the zero table by a bit — the value it holds just has a zero on top)
    DP_REQUIRE((l.sm_zero_vars == 0 || l.sm_zero_vars >= 2) && l.sm_allowable_error >= 2, DP_ERR_ARG, "softmax: tables of fewer than four entries are not supported");
  };
  for (size_t id = 0; id < m.layers.size(); id++) {
    const LayerSpec& l = m.layers[id];
    size_t cur = in_len[id];
    if (l.kind == L_MATMUL2) {
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2 && cur % l.nrows == 0 && cur / l.nrows >= 2 && is_pow2(cur) && in2_len[id] == l.nrows * l.ncols && l.weights.empty() && l.bias.empty(), DP_ERR_SHAPE, "matmul2: [s][k] x [k][n] with powers of two >= 2");
    } else if (l.kind == L_ADD2) {
      DP_REQUIRE(cur >= 2 && in2_len[id] == cur && l.add_left > 0 && l.add_right > 0 && l.add_left < (int64_t(1) << 40) && l.add_right < (int64_t(1) << 40), DP_ERR_SHAPE, "add2: two inputs of one length, positive multipliers");
    } else if (l.kind == L_QKV) {
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2 && cur % l.nrows == 0 && cur / l.nrows >= 2 && is_pow2(cur) && l.weights.size() == 3 * l.nrows * l.ncols && l.bias.size() == 3 * l.ncols, DP_ERR_SHAPE, "qkv: [s][k] input, three [k][n] matrices and [n] biases, powers of two >= 2");
    } else if (l.kind == L_CONCAT_MATMUL) {
      for (int d = 0; d < 3; d++) DP_REQUIRE(is_pow2(l.cm_a[d]) && is_pow2(l.cm_b[d]), DP_ERR_SHAPE, "concat matmul: padded shapes must be powers of two");
      auto is_perm = [](const int* p) { return p[0] >= 0 && p[0] < 3 && p[1] >= 0 && p[1] < 3 && p[2] >= 0 && p[2] < 3 && p[0] != p[1] && p[0] != p[2] && p[1] != p[2]; };
      DP_REQUIRE(is_perm(l.cm_left) && is_perm(l.cm_right) && (l.cm_perm.empty() || (l.cm_perm.size() == 3 && is_perm(l.cm_perm.data()))), DP_ERR_SHAPE, "concat matmul: dimension triples must be permutations of 0, 1, 2");
      DP_REQUIRE(cur == l.cm_a[0] * l.cm_a[1] * l.cm_a[2] && in2_len[id] == l.cm_b[0] * l.cm_b[1] * l.cm_b[2], DP_ERR_SHAPE, "concat matmul: input lengths");
      DP_REQUIRE(l.cm_a[l.cm_left[0]] == l.cm_b[l.cm_right[0]] && l.cm_a[l.cm_left[1]] == l.cm_b[l.cm_right[1]] && l.cm_a[l.cm_left[1]] >= 2, DP_ERR_SHAPE, "concat matmul: concat / mat_mul dimensions of the two inputs differ");
      DP_REQUIRE(lens[id] >= 2, DP_ERR_SHAPE, "concat matmul: output of one entry");
    } else
    if (l.kind == L_DENSE) {
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2, DP_ERR_SHAPE, "dense: padded dimensions must be powers of two >= 2");
      DP_REQUIRE(l.ncols == cur && l.weights.size() == l.nrows * l.ncols && l.bias.size() == l.nrows, DP_ERR_SHAPE, "dense: tensor sizes");
      cur = l.nrows;
    } else if (l.kind == L_MATMUL) {
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2, DP_ERR_SHAPE, "matmul: padded dimensions must be powers of two >= 2");
      DP_REQUIRE(cur % l.nrows == 0 && cur / l.nrows >= 2 && l.weights.size() == l.nrows * l.ncols && (l.bias.empty() || l.bias.size() == l.ncols), DP_ERR_SHAPE, "matmul: tensor sizes (the input is [s][nrows], s >= 2)");
      cur = cur / l.nrows * l.ncols;
    } else if (l.kind == L_EMBED) {
      DP_REQUIRE(&l == &m.layers[0], DP_ERR_SHAPE, "embeddings: only as the first layer (its input claim is checked against the public tokens)");
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2 && l.weights.size() == l.nrows * l.ncols && cur >= 2, DP_ERR_SHAPE, "embeddings: padded table dimensions must be powers of two >= 2");
      cur = cur * l.ncols;
    } else if (l.kind == L_POSITIONAL) {
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.ncols >= 2 && l.weights.size() == l.nrows * l.ncols && cur % l.ncols == 0 && cur <= l.weights.size() && cur >= 2
                 && l.add_left > 0 && l.add_right > 0 && l.add_left < (int64_t(1) << 40) && l.add_right < (int64_t(1) << 40), DP_ERR_SHAPE, "positional: the table is [positions][embedding size] with at least as many positions as the input has rows");
      // KNOWN SOUNDNESS GAP, replicated from the reference for transcript compatibility (positional.rs:80-126, 480-583): when the table
      // has more rows than the input has tokens, the coordinates that lift the slice claim to the whole table are drawn BEFORE the
      // sub-matrix evaluations are absorbed, so a prover that sees them can choose right_eval and solve for sub_matrix_evals[0]: the
      // positional addend is forgeable. DP_STRICT_POSITIONAL=1 refuses such models (table rows == tokens: nothing to lift, no gap).
      static const bool strict_positional = getenv("DP_STRICT_POSITIONAL") && atoi(getenv("DP_STRICT_POSITIONAL"));
      DP_REQUIRE(!strict_positional || cur == l.weights.size(), DP_ERR_ARG, "positional: table longer than the sequence (DP_STRICT_POSITIONAL: the reference's lifting of the slice claim is not sound)");
    } else if (l.kind == L_ADD) {
      DP_REQUIRE(l.weights.size() == cur && cur >= 2 && l.add_left > 0 && l.add_right > 0 && l.add_left < (int64_t(1) << 40) && l.add_right < (int64_t(1) << 40), DP_ERR_SHAPE, "add: the operand must be as long as the input, the multipliers positive");
    } else if (l.kind == L_REQUANT) {
      DP_REQUIRE(l.fixed_point_multiplier > 0 && l.shift() % Q_BIT_LEN == 0 && l.shift() >= Q_BIT_LEN && l.shift() < 63, DP_ERR_ARG, "requant: shift must be a positive multiple of BIT_LEN");
      DP_REQUIRE(l.intermediate_bit_size + l.fp_scale <= 63, DP_ERR_ARG, "requant: intermediate_bit_size + fp_scale > 63");
      unsigned cs = l.clamping_size();
      DP_REQUIRE(cs >= 1 && cs <= 24 && cur >= 4, DP_ERR_ARG, "requant: unsupported clamping table size / tensor length");
    } else if (l.kind == L_RELU) { DP_REQUIRE(cur >= 4, DP_ERR_SHAPE, "relu: tensor length must be >= 4"); }
    else if (l.kind == L_GELU) { DP_REQUIRE(cur >= 4 && l.fixed_point_multiplier >= 1 && l.fixed_point_multiplier <= (int64_t(1) << 12), DP_ERR_ARG, "gelu: tensor length must be >= 4, the table at most 2^20 rows (activation.rs:643-648)"); }
    else if (l.kind == L_SOFTMAX) check_softmax(l, cur);
    else if (l.kind == L_MHA) {  // three equally long inputs; the sub-layers' own conditions (head_dim is the mat_mul dimension of qk, seq of final_mul)
      const size_t S = l.mha_shape[0], H = l.mha_shape[1], D = l.mha_shape[2];
      DP_REQUIRE(is_pow2(S) && is_pow2(H) && is_pow2(D) && S >= 2 && D >= 2 && S <= (size_t(1) << 12) && H <= (size_t(1) << 12) && D <= (size_t(1) << 12) && cur == S * H * D && in2_len[id] == cur && in3_len[id] == cur, DP_ERR_SHAPE, "mha: Q, K, V of [seq >= 2][heads][head_dim >= 2] entries each, powers of two");
      check_softmax(mha_softmax_spec(l), H * S * S);
    }
    else if (l.kind == L_LAYERNORM) {
      const size_t fd = l.weights.size();
      DP_REQUIRE(is_pow2(fd) && fd >= 2 && l.bias.size() == fd && l.nrows == fd && is_pow2(cur) && cur % fd == 0 && cur / fd >= 4, DP_ERR_SHAPE, "layernorm: [rows >= 4][dim >= 2] input, gamma and beta of the padded dimension");
      DP_REQUIRE(l.ln_dim_size >= 1 && next_pow2(l.ln_dim_size) == fd && l.ln_multiplier >= 1 && l.ln_multiplier < (int64_t(1) << 30), DP_ERR_ARG, "layernorm: dim_size / multiplier");
      DP_REQUIRE(l.ln_range_check_bits >= 1 && l.ln_range_check_bits <= 40 && l.ln_top_chunk_scalar_log == (l.ln_range_check_bits % Q_BIT_LEN ? Q_BIT_LEN - l.ln_range_check_bits % Q_BIT_LEN : 0), DP_ERR_ARG, "layernorm: range check bits and the scalar of their top chunk");
    }
    else if (l.kind == L_CONV) {
      DP_REQUIRE(is_pow2(l.kw) && is_pow2(l.kx) && is_pow2(l.real_nw) && is_pow2(l.nw) && l.kw >= 2 && l.nw >= 2 && 2 * l.real_nw <= l.nw, DP_ERR_SHAPE, "conv: padded dimensions must be powers of two, padded kernel <= half the padded input side");
      DP_REQUIRE(cur == l.kx * l.nw * l.nw && l.weights.size() == l.kw * l.kx * l.real_nw * l.real_nw && l.bias.size() == l.kw, DP_ERR_SHAPE, "conv: tensor sizes");
      DP_REQUIRE(l.unp_out[0] >= 1 && l.unp_out[0] <= l.kw && l.unp_out[1] >= 1 && l.unp_out[1] <= l.nw && l.unp_out[2] >= 1 && l.unp_out[2] <= l.nw, DP_ERR_SHAPE, "conv: unpadded output shape");
      cur = l.kw * l.nw * l.nw;
    } else if (l.kind == L_MAXPOOL) {
      DP_REQUIRE(is_pow2(l.pin[0]) && is_pow2(l.pin[1]) && is_pow2(l.pin[2]) && l.pin[1] >= 2 && l.pin[2] >= 4 && cur == l.pin[0] * l.pin[1] * l.pin[2] && cur >= 16, DP_ERR_SHAPE, "maxpool: padded input shape");
      cur /= 4;
    } else if (l.kind == L_FLATTEN) {}
    else if (l.kind == L_LOGITS) {
      const std::string who = "node " + std::to_string(id) + " (kind 18, logits): ";
      DP_REQUIRE(is_pow2(l.nrows) && is_pow2(l.ncols) && l.nrows >= 2 && l.ncols >= 2 && l.nrows <= (size_t(1) << 24) && l.ncols <= (size_t(1) << 24), DP_ERR_ARG, who + "rows and K must be powers of two >= 2");
      DP_REQUIRE(cur == l.nrows * l.ncols, DP_ERR_ARG, who + "the input must have rows * K entries");
    }
    else DP_REQUIRE(false, DP_ERR_ARG, "unknown layer kind");
  }
}

inline std::unique_ptr<Context> context_generate(Dev& dev, const ModelSpec& m) {
  validate_model(m);
  std::unique_ptr<Context> ctx(new Context());
  ctx->dev = &dev; ctx->model = m;
  size_t mpl = 0;
  for (size_t n : input_tensor_lens(m)) mpl = std::max(mpl, n);
  std::vector<TableType> ts;
  auto add = [&](TableType t) { for (auto& x : ts) if (x == t) return; ts.push_back(t); };
  std::vector<size_t> lens; tensor_lens(m, lens);
  for (size_t id = 0; id < m.layers.size(); id++) {
    // an Mha node brings the tables of its softmax and witness polynomials as long as the [heads][seq][seq] products (Mha::step_info, mha.rs:432-503)
    const LayerSpec& l0 = m.layers[id];
    const LayerSpec sub = l0.kind == L_MHA ? mha_softmax_spec(l0) : LayerSpec();
    const LayerSpec& l = l0.kind == L_MHA ? sub : l0;
    const size_t cur = l0.kind == L_MHA ? sub.sm_shape[0] * sub.sm_shape[1] * sub.sm_shape[2] : lens[id];  // (Requant / Relu: also the length of the input; MaxPool: of the output, as the committed polynomials are)
    if (l.kind == L_REQUANT) { add({2, 0}); add({3, l.clamping_size()}); mpl = std::max(mpl, next_pow2(cur)); }
    else if (l.kind == L_RELU) { add({0, 0}); mpl = std::max(mpl, next_pow2(cur)); }
    else if (l.kind == L_GELU) { add(gelu_table(l)); mpl = std::max(mpl, next_pow2(cur)); }
    else if (l.kind == L_MAXPOOL) { add({2, 0}); mpl = std::max(mpl, next_pow2(cur)); }
    else if (l.kind == L_LOGITS) { add({2, 0}); mpl = std::max(mpl, next_pow2(cur)); }  // (the committed polynomial is the vector of maxima, as long as the output; logits.rs:242)
    else if (l.kind == L_LAYERNORM) { add({2, 0}); add(layernorm_table(l)); mpl = std::max(mpl, next_pow2(cur)); }  // layernorm.rs:587-618
    else if (l.kind == L_SOFTMAX) { add({2, 0}); add(softmax_table(l)); add(softmax_error_table(l)); if (l.sm_zero_vars) add({6, l.sm_zero_vars}); mpl = std::max(mpl, next_pow2(cur)); }  // softmax.rs:1205-1245
  }
  std::sort(ts.begin(), ts.end());
  for (auto& t : ts) mpl = std::max(mpl, size_t(1) << t.vars());
  for (auto& l : m.layers) if (l.kind == L_QKV) mpl = std::max(mpl, std::max(next_pow2(l.weights.size() / 3), next_pow2(l.bias.size() / 3)));
  for (auto& l : m.layers) if (l.kind == L_DENSE || l.kind == L_CONV || l.kind == L_MATMUL || l.kind == L_ADD || l.kind == L_EMBED || l.kind == L_POSITIONAL || l.kind == L_LAYERNORM) mpl = std::max(mpl, std::max(next_pow2(l.weights.size()), next_pow2(l.bias.size())));
  mpl = next_pow2(mpl);
  ctx->max_poly_len = mpl; ctx->full_log = dp_ceil_log2(mpl); ctx->tables = ts;
  dev.pcs_init(ctx->full_log);
  for (size_t id = 0; id < m.layers.size(); id++) {
    LayerSpec& l = ctx->model.layers[id];
    if (l.kind == L_QKV) {  // six model polynomials (qkv.rs:388-418); the three weight matrices stay on the device side by side for the prover
      const size_t kn = l.nrows * l.ncols, n = l.ncols;
      static const char* const wn[3] = {"WeightQ", "WeightK", "WeightV"}; static const char* const bn[3] = {"BiasQ", "BiasK", "BiasV"};
      for (size_t q = 0; q < 3; q++) {  // (each commitment owns its evaluation table: the prover reads the matrices from there)
        DBuf w = dev.alloc_persistent(kn, false), b = dev.alloc_persistent(n, false);
        dev.upload_i64(w, &l.weights[q * kn]); dev.upload_i64(b, &l.bias[q * n]);
        ctx->model_comms[id][wn[q]] = dev.commit(w, true); ctx->model_comms[id][bn[q]] = dev.commit(b, true);
      }
      prepare_fast_inference(l);
      continue;
    }
    if (l.kind == L_LAYERNORM) {  // gamma and beta are model polynomials (layernorm.rs:67-68,603-613)
      DBuf g = dev.alloc_persistent(l.weights.size(), false), b = dev.alloc_persistent(l.bias.size(), false);
      dev.upload_i64(g, l.weights.data()); dev.upload_i64(b, l.bias.data());
      ctx->model_comms[id]["LayerNormGamma"] = dev.commit(g, true); ctx->model_comms[id]["LayerNormBeta"] = dev.commit(b, true);
      continue;
    }
    if (l.kind != L_DENSE && l.kind != L_CONV && l.kind != L_MATMUL && l.kind != L_ADD && l.kind != L_EMBED && l.kind != L_POSITIONAL) continue;
    if (l.kind == L_POSITIONAL) {  // the whole table is the model polynomial (positional.rs:229,243-251)
      DBuf w = dev.alloc_persistent(l.weights.size(), false);
      dev.upload_i64(w, l.weights.data());
      ctx->model_comms[id]["PositionalMatrix"] = dev.commit(w, true);
      ctx->weights_dev[id] = w;
      continue;
    }
    if (l.kind == L_EMBED) {  // the embedding table is a model polynomial (embeddings.rs:271,284-291)
      DBuf w = dev.alloc_persistent(l.weights.size(), false);
      dev.upload_i64(w, l.weights.data());
      ctx->model_comms[id]["EmbeddingMat"] = dev.commit(w, true);
      ctx->weights_dev[id] = w;
      continue;
    }
    if (l.kind == L_ADD) {  // the static operand is a model polynomial: OPERAND_POLY_ID = 0xff, to_string() (add.rs:32,518-522)
      DBuf w = dev.alloc_persistent(l.weights.size(), false);
      dev.upload_i64(w, l.weights.data());
      ctx->model_comms[id]["255"] = dev.commit(w, true);
      ctx->weights_dev[id] = w;
      continue;
    }
    if (l.kind == L_MATMUL) {  // model polys of a MatMul with a constant matrix (matrix_mul.rs:947-963)
      DBuf w = dev.alloc_persistent(l.weights.size(), false);
      dev.upload_i64(w, l.weights.data());
      prepare_fast_inference(l);
      ctx->model_comms[id]["MatMulWeight"] = dev.commit(w, true);
      if (!l.bias.empty()) { DBuf b = dev.alloc_persistent(l.bias.size(), false); dev.upload_i64(b, l.bias.data()); ctx->model_comms[id]["MatMulBias"] = dev.commit(b, true); }
      ctx->weights_dev[id] = w;
      continue;
    }
    DBuf w = dev.alloc_persistent(l.weights.size(), false), b = dev.alloc_persistent(l.bias.size(), false);
    dev.upload_i64(w, l.weights.data()); dev.upload_i64(b, l.bias.data());
    if (l.kind == L_DENSE) {
      prepare_fast_inference(l);
      ctx->model_comms[id]["DenseWeight"] = dev.commit(w, true);
      ctx->model_comms[id]["DenseBias"] = dev.commit(b, true);
    } else {  // model polys of a convolution (convolution.rs:452-453,546-553)
      ctx->model_comms[id]["ConvFilter"] = dev.commit(w, true);
      ctx->model_comms[id]["ConvBias"] = dev.commit(b, true);
      l.wfft = conv_weight_fft(l);
      Context::ConvDev cd;
      cd.wfft = dev.alloc_persistent(l.wfft->size(), false); dev.upload(cd.wfft, l.wfft->data());
      std::vector<int64_t> clr = clearing_tensor(l);
      cd.clearing = dev.alloc_persistent(clr.size(), false); dev.upload_i64(cd.clearing, clr.data());
      ctx->conv_dev[id] = cd;
    }
    ctx->weights_dev[id] = w;
  }
  for (const TableType& tt : ts) if (tt.committed_column()) {  // commit/context.rs:105-107
    std::vector<int64_t> merged; std::vector<std::vector<int64_t>> tc;
    table_columns(tt, merged, tc);
    DBuf col = dev.alloc_persistent(tc.back().size(), false);  // (the output column; the only column of an ErrorTable)
    dev.upload_i64(col, tc.back().data());
    ctx->table_comms[tt] = dev.commit(col, true);
  }
  for (const TableType& tt : ts) {  // the columns of every lookup table of the model: built once (Context::table_data), resident from here on
    const Context::TableData& td = ctx->table_data(tt);
    std::vector<DBuf>& dc = ctx->table_cols_dev[tt];
    for (const std::vector<int64_t>& c : td.cols) { DBuf b = dev.alloc_persistent(c.size(), false); dev.upload_i64(b, c.data()); dc.push_back(b); }
  }
  return ctx;
}

// ---- prover
struct LogUpWitness {
  bool is_table = false;
  std::vector<DevCommit> commits;
  std::vector<DBuf> columns;
  std::vector<DBuf> extra_columns;  // committed alongside the lookup columns but not looked up (maxpool output)
  size_t columns_per_instance = 1;
  TableType table_type{0, 0};
  DBuf multiplicities;
};
struct CommitClaim { DevCommit comm; Claim claim; };
struct ProverState {
  Context* ctx; Dev* dev; Transcript* t;
  std::map<size_t, LayerProof> proofs;
  std::vector<CommitClaim> claims, trivial_claims;
  std::map<size_t, std::vector<LogUpWitness>> lookup_witness;
  std::vector<LogUpWitness> table_witness;
  Ext constant_challenge; std::map<TableType, Ext> challenge_map;
  // activations the layer proofs read as extension tables (Dense inputs, ReLU outputs), already on the device: they rode in the
  // witness upload instead of costing one upload launch each inside the layer loop
  std::map<size_t, DBuf> staged_in, staged_out;
  std::map<size_t, SoftmaxTrace> sm_trace;    // SoftmaxData of every Softmax node, likewise
  std::map<size_t, LayerNormTrace> ln_trace;  // LayerNormData of every LayerNorm node (kept from the witness generation for its prover)
  struct LogitsDev { DBuf in, onehot; };       // the input of every Logits node and the one-hot matrix of its output (base columns, instantiate_witness_ctx)
  std::map<size_t, LogitsDev> logits_dev;
  void add_witness_claim(const DevCommit& c, Claim cl) {
    if (c.nv <= PCS_BASECODE_LOG) trivial_claims.push_back({c, std::move(cl)}); else claims.push_back({c, std::move(cl)});
  }
  LogUpInputDev logup_input(const LogUpWitness& w) const {
    LogUpInputDev in; in.is_table = w.is_table; in.columns = w.columns; in.multiplicities = w.multiplicities;
    in.constant_challenge = constant_challenge; in.column_separation_challenge = challenge_map.at(w.table_type);
    in.columns_per_instance = w.columns_per_instance; return in;
  }
};

struct PhaseTimer {  // DP_TIMING=1 prints the host-side wall time of each proving phase to stderr
  bool on; std::chrono::steady_clock::time_point t0; const char* name;
  PhaseTimer() : on(getenv("DP_TIMING") && atoi(getenv("DP_TIMING"))), t0(std::chrono::steady_clock::now()), name(nullptr) {}
  void lap(const char* what) {
    if (!on) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[dp timing] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};
// generate_lookup_witnesses (lookup/context.rs:631-781) with gen_lookup_witness of requant.rs:208-345 / activation.rs:238-318.
// All witness columns of the inference are produced on the host (tiny integer work on activation vectors), shipped to
// the device in ONE upload and committed in ONE batched call (the reference commits them one by one on rayon threads).
// The HOST half of it — everything that is a function of (context, trace) alone: the lookup columns, what each lookup hits in its table, the tables'
// multiplicities, all of it flattened for the two uploads. No device, no transcript: dp_model_prove_batch computes it for the next inputs on helper threads
// while the proofs in flight wait for the device (capi.cpp), every other caller inside prove().
struct WitnessHost {
  std::map<TableType, std::unordered_map<int64_t, u64>> counts;
  struct Col { std::vector<int64_t> v; };
  // col_ids: committed columns, in commit order; the first n_lookup_cols of them (all, if 0) are the lookup's columns. late >= 0: the lookup's
  // only column is `lates[late]`, a column that is NOT committed (Softmax's row sums), and every committed column is an extra one
  // logits_in >= 0 (a Logits node): the lookup's only column is MADE ON THE DEVICE (Dev::logits_columns) from lates[logits_in], the node's input, the
  // committed column (the row maxima) and lates[logits_idx], the chosen indices; the committed column is an extra one
  struct Pending { size_t node; int which; std::vector<size_t> col_ids; size_t cpi; TableType tt; size_t n_lookup_cols = 0; int late = -1; int logits_in = -1, logits_idx = -1; };
  struct TabInfo { TableType tt; std::vector<size_t> col_ids; std::vector<u64> mult; };
  struct Act { size_t node; bool is_out; size_t n; size_t off; };
  std::vector<Pending> pend; std::vector<size_t> late_ids; std::vector<TabInfo> tabs; std::vector<Act> acts;
  size_t n_witness_cols = 0;
  std::vector<size_t> col_len, offs, moffs;  // per i64 column: length and offset in `flat`; per table: offset of its multiplicities in `mflat`
  std::vector<int64_t> flat; std::vector<u64> mflat;
  std::map<size_t, SoftmaxTrace> sm_trace; std::map<size_t, LayerNormTrace> ln_trace;
};
inline WitnessHost witness_host(const Context& ctx, const Trace& tr) {
  WitnessHost wh;
  if (ctx.tables.empty()) return wh;
  PhaseTimer wt;
  using Col = WitnessHost::Col; using Pending = WitnessHost::Pending; using TabInfo = WitnessHost::TabInfo; using Act = WitnessHost::Act;
  std::map<TableType, std::unordered_map<int64_t, u64>>& counts = wh.counts;
  // the range table's keys are 0 .. 2^Q_BIT_LEN - 1 and most lookups of a proof go there: counted in an array, merged into `counts` once at the end
  // (the entry of the range table is created where the first lookup into it is met, as before: the ORDER of `counts` is the order of the table proofs)
  std::vector<u64> range_hist(size_t(1) << Q_BIT_LEN, 0);
  bool range_used = false;
  auto count_range = [&](int64_t v) {  // (a value outside the table keeps its own key, as before: it is no row of the table and the lookup argument will not hold)
    range_used = true;
    if (v >= 0 && v < (int64_t(1) << Q_BIT_LEN)) range_hist[(size_t)v] += 1; else counts[TableType{2, 0}][v] += 1;
  };
  std::vector<Col> cols;                       // every i64 column that goes to the device, in commit order first
  std::vector<Pending>& pend = wh.pend;
  std::vector<std::vector<int64_t>> lates; std::vector<size_t>& late_ids = wh.late_ids;
  for (size_t id = 0; id < ctx.model.layers.size(); id++) {
    // Mha::gen_lookup_witness (mha.rs:706-719): the witness of its softmax on the products Q K^T, under the node's own id
    const LayerSpec& l0 = ctx.model.layers[id];
    const LayerSpec sub = l0.kind == L_MHA ? mha_softmax_spec(l0) : LayerSpec();
    const LayerSpec& l = l0.kind == L_MHA ? sub : l0;
    if (l.kind == L_REQUANT) {
      unsigned shift = l.shift(); int64_t rounding = int64_t(1) << (shift - 1), mask = (int64_t(1) << shift) - 1;
      std::vector<int64_t> cin, cout, shifted;
      for (int64_t v : tr.in[id]) { int64_t tmp = v * l.fixed_point_multiplier + rounding; int64_t c = tmp >> shift; cin.push_back(c); cout.push_back(q_clamp(c)); shifted.push_back(tmp & mask); }
      unsigned nchunks = shift / Q_BIT_LEN; int64_t rmask = (int64_t(1) << Q_BIT_LEN) - 1;
      TableType ct{3, l.clamping_size()}, rt{2, 0};
      int64_t cmax = int64_t(1) << (ct.size - 1);
      std::unordered_map<int64_t, u64>& cct = counts[ct];
      for (size_t i = 0; i < cin.size(); i++) {
        DP_REQUIRE(cin[i] >= -cmax && cin[i] < cmax, DP_ERR_ARG, "requant: value falls outside the clamping table");
        cct[cin[i] + cout[i] * COLUMN_SEPARATOR] += 1;
      }
      Pending pc{id, 0, {}, 2, ct}, pr{id, 1, {}, 1, rt};
      pc.col_ids = {cols.size(), cols.size() + 1};
      cols.push_back({cin}); cols.push_back({cout});
      for (unsigned j = 0; j < nchunks; j++) {
        std::vector<int64_t> ch; ch.reserve(shifted.size());
        for (int64_t sft : shifted) { int64_t v = (sft >> (j * Q_BIT_LEN)) & rmask; ch.push_back(v); count_range(v); }
        pr.col_ids.push_back(cols.size()); cols.push_back({std::move(ch)});
      }
      pend.push_back(pc); pend.push_back(pr);
    } else if (l.kind == L_GELU) {  // Activation::gen_lookup_witness (activation.rs:238-318): the first column is the SCALED input, what the table is indexed by
      TableType gt = gelu_table(l);
      std::vector<int64_t> a; a.reserve(tr.in[id].size());
      for (int64_t v : tr.in[id]) a.push_back(v * l.fixed_point_multiplier);
      const auto& b = tr.out[id];
      std::unordered_map<int64_t, u64>& cg = counts[gt];
      for (size_t i = 0; i < a.size(); i++) cg[a[i] + COLUMN_SEPARATOR * b[i]] += 1;
      Pending p{id, 0, {cols.size(), cols.size() + 1}, 2, gt};
      cols.push_back({std::move(a)}); cols.push_back({b});
      pend.push_back(p);
    } else if (l.kind == L_RELU) {
      TableType rt{0, 0};
      const auto& a = tr.in[id]; const auto& b = tr.out[id];
      std::unordered_map<int64_t, u64>& crl = counts[rt];
      for (size_t i = 0; i < a.size(); i++) crl[a[i] + COLUMN_SEPARATOR * b[i]] += 1;
      Pending p{id, 0, {cols.size(), cols.size() + 1}, 2, rt};
      cols.push_back({a}); cols.push_back({b});
      pend.push_back(p);
    } else if (l.kind == L_LAYERNORM) {  // LayerNorm::lookup_witness (layernorm.rs:1103-1218): (input, output) of the inverse square root, then the range-checked chunks
      LayerNormTrace& d = wh.ln_trace[id];
      layernorm_op(l, tr.in[id], &d);
      const unsigned nrc = (l.ln_range_check_bits - 1) / Q_BIT_LEN + 1;
      const int64_t rmask = (int64_t(1) << Q_BIT_LEN) - 1, top = int64_t(1) << l.ln_top_chunk_scalar_log;
      TableType it = layernorm_table(l), rt{2, 0};
      std::unordered_map<int64_t, u64>& cit = counts[it];
      for (size_t i = 0; i < d.lookup_input.size(); i++) cit[d.lookup_input[i] + d.lookup_output[i] * COLUMN_SEPARATOR] += 1;
      Pending pi{id, 0, {cols.size(), cols.size() + 1}, 2, it}, pr{id, 1, {}, 1, rt};
      cols.push_back({d.lookup_input}); cols.push_back({d.lookup_output});
      for (unsigned j = 0; j < nrc; j++) {
        std::vector<int64_t> ch; ch.reserve(d.range_check.size());
        for (int64_t v : d.range_check) { int64_t c = ((v >> (j * Q_BIT_LEN)) & rmask) * (j + 1 == nrc ? top : 1); ch.push_back(c); count_range(c); }
        pr.col_ids.push_back(cols.size()); cols.push_back({std::move(ch)});
      }
      pend.push_back(pi); pend.push_back(pr);
    } else if (l.kind == L_SOFTMAX) {  // Softmax::lookup_witness (softmax.rs:890-1066)
      SoftmaxTrace& d = wh.sm_trace[id];
      softmax_op(l, l0.kind == L_MHA ? tr.mha.at(id).softmax_in : tr.in[id], &d);
      TableType st = softmax_table(l), rt{2, 0}, et = softmax_error_table(l), zt{6, l.sm_zero_vars};
      for (int64_t v : d.low) count_range(v);
      for (int64_t v : d.high) count_range(v);
      std::unordered_map<int64_t, u64>& cst = counts[st];
      for (size_t i = 0; i < d.exp_in.size(); i++) cst[d.exp_in[i] + d.exp_out[i] * COLUMN_SEPARATOR] += 1;
      std::unordered_map<int64_t, u64>& cet = counts[et];
      for (int64_t v : d.row_sums) cet[v] += 1;
      Pending pe{id, 0, {cols.size(), cols.size() + 1}, 2, st}; cols.push_back({d.exp_in}); cols.push_back({d.exp_out});
      Pending pr{id, 1, {cols.size(), cols.size() + 1}, 1, rt}; cols.push_back({d.low}); cols.push_back({d.high});
      Pending px{id, 2, {cols.size()}, 1, et}; cols.push_back({d.shift});  // the SHIFT polynomial is committed with this lookup, the row sums are what is looked up
      px.late = (int)lates.size(); lates.push_back(d.row_sums);
      pend.push_back(pe); pend.push_back(pr); pend.push_back(px);
      if (l.sm_zero_chunks) {
        Pending pz{id, 3, {}, 2, zt};
        for (unsigned z = 0; z < l.sm_zero_chunks; z++) {
          std::unordered_map<int64_t, u64>& czt = counts[zt];
          for (size_t i = 0; i < d.zero_in[z].size(); i++) czt[d.zero_in[z][i] + d.zero_out[z][i] * COLUMN_SEPARATOR] += 1;
          pz.col_ids.push_back(cols.size()); cols.push_back({d.zero_in[z]}); pz.col_ids.push_back(cols.size()); cols.push_back({d.zero_out[z]});
        }
        pend.push_back(pz);
      }
    } else if (l.kind == L_MAXPOOL) {  // Pooling::gen_lookup_witness (pooling.rs:206-262): 4 difference columns + the output
      TableType rt{2, 0};
      std::vector<std::vector<int64_t>> diffs = maxpool_diff_polys(l, tr.in[id], tr.out[id]);
      Pending p{id, 0, {}, 1, rt};
      for (auto& d : diffs) {
        for (int64_t v : d) { DP_REQUIRE(v >= 0 && v < (int64_t(1) << Q_BIT_LEN), DP_ERR_ARG, "maxpool: difference outside the range table"); count_range(v); }
        p.col_ids.push_back(cols.size()); cols.push_back({std::move(d)});
      }
      p.col_ids.push_back(cols.size()); cols.push_back({tr.out[id]});  // committed, but not a lookup column
      p.n_lookup_cols = 4;
      pend.push_back(p);
    } else if (l.kind == L_LOGITS) {  // Logits::gen_lookup_witness (logits.rs:474-552): the maxima are committed, max - input is looked up in the range table
      const std::vector<int64_t>& x = tr.in[id]; const std::vector<int64_t>& mx = tr.argmax_max.at(id);
      const size_t K = l.ncols;
      DP_REQUIRE(x.size() == mx.size() * K && tr.out[id].size() == mx.size(), DP_ERR_SHAPE, "logits: trace shapes");
      for (size_t i = 0; i < x.size(); i++) {
        const int64_t d = mx[i / K] - x[i];  // (>= 0: mx is the row's maximum)
        DP_REQUIRE(d < (int64_t(1) << Q_BIT_LEN), DP_ERR_ARG, "logits: a row spreads beyond the range table");
        count_range(d);
      }
      Pending p{id, 0, {cols.size()}, 1, TableType{2, 0}}; cols.push_back({mx});
      p.logits_in = (int)lates.size(); lates.push_back(x);
      p.logits_idx = (int)lates.size(); lates.push_back(tr.out[id]);
      pend.push_back(p);
    }
  }
  wh.n_witness_cols = cols.size();
  for (auto& v : lates) { late_ids.push_back(cols.size()); cols.push_back({std::move(v)}); }  // uploaded with the rest, not committed
  if (range_used) { std::unordered_map<int64_t, u64>& crt = counts[TableType{2, 0}]; for (size_t v = 0; v < range_hist.size(); v++) if (range_hist[v]) crt[(int64_t)v] += range_hist[v]; }
  wt.lap("  witness: host columns");
  // the tables' multiplicities (their columns are resident: Context::table_cols_dev)
  std::vector<TabInfo>& tabs = wh.tabs;
  for (auto& kv : counts) {
    const TableType& tt = kv.first;
    const Context::TableData& td = ctx.table_data(tt);  // the table's columns and the inverse repetition of its rows: per context, not per proof
    const std::vector<int64_t>& merged = td.merged;
    TabInfo ti; ti.tt = tt; ti.mult.resize(merged.size());
    for (size_t i = 0; i < merged.size(); i++) {
      auto it = kv.second.find(merged[i]);
      ti.mult[i] = it == kv.second.end() ? 0 : td.inv_cnt[i] == 1 ? gl_from_u64(it->second) : gl_mul(gl_from_u64(it->second), td.inv_cnt[i]);
    }
    if (!ctx.table_cols_dev.count(tt))  // (a table the setup did not foresee: its columns ride in the upload as they did until round 4)
      for (auto& c : td.cols) { ti.col_ids.push_back(cols.size()); cols.push_back({c}); }
    tabs.push_back(std::move(ti));
  }
  wt.lap("  witness: multiplicities");
  // flattened for ONE upload of all i64 columns and ONE of all multiplicity vectors
  size_t total = 0; for (auto& c : cols) total += c.v.size();
  std::vector<int64_t>& flat = wh.flat; flat.reserve(total);
  for (auto& c : cols) { wh.offs.push_back(flat.size()); wh.col_len.push_back(c.v.size()); flat.insert(flat.end(), c.v.begin(), c.v.end()); }
  size_t mtotal = 0; for (auto& t : tabs) mtotal += t.mult.size();
  std::vector<u64>& mflat = wh.mflat; mflat.reserve(mtotal);
  for (auto& t : tabs) { wh.moffs.push_back(mflat.size()); mflat.insert(mflat.end(), t.mult.begin(), t.mult.end()); }
  // ... and the activations of the layer loop, as extension words behind the multiplicities (16-byte aligned)
  std::vector<std::pair<Act, const std::vector<int64_t>*>> acts;
  for (size_t id = 0; id < ctx.model.layers.size(); id++) {
    const int kind = ctx.model.layers[id].kind;
    if (kind == L_DENSE) acts.push_back({Act{id, false, tr.in[id].size(), 0}, &tr.in[id]});
    else if (kind == L_RELU || kind == L_GELU) acts.push_back({Act{id, true, tr.out[id].size(), 0}, &tr.out[id]});
  }
  if (mflat.size() & 1) mflat.push_back(0);
  for (auto& av : acts) { av.first.off = mflat.size(); mflat.reserve(mflat.size() + 2 * av.second->size()); for (int64_t x : *av.second) { mflat.push_back(gl_from_i64(x)); mflat.push_back(0); } wh.acts.push_back(av.first); }
  wt.lap("  witness: flatten");
  return wh;
}
// the device half: two uploads, one batched commit, the witnesses of the layer lookups and of the tables, the table challenges
inline void instantiate_witness_ctx(ProverState& ps, const Trace& tr, WitnessHost* prepared = nullptr) {
  Context& ctx = *ps.ctx; Dev& dev = *ps.dev;
  if (ctx.tables.empty()) return;
  WitnessHost local;
  if (!prepared) local = witness_host(ctx, tr);
  WitnessHost& wh = prepared ? *prepared : local;
  PhaseTimer wt;
  ps.sm_trace = std::move(wh.sm_trace); ps.ln_trace = std::move(wh.ln_trace);
  const std::vector<WitnessHost::Pending>& pend = wh.pend; const std::vector<size_t>& late_ids = wh.late_ids; const std::vector<WitnessHost::TabInfo>& tabs = wh.tabs;
  const size_t n_witness_cols = wh.n_witness_cols;
  const std::vector<size_t>& moffs = wh.moffs;
  DBuf big = dev.alloc(wh.flat.size(), false);
  dev.upload_i64(big, wh.flat.data());
  std::vector<DBuf> dcol;
  for (size_t i = 0; i < wh.col_len.size(); i++) dcol.push_back(big.slice(wh.offs[i], wh.col_len[i]));
  DBuf mbig = dev.alloc(wh.mflat.size(), false);
  dev.upload(mbig, wh.mflat.data());
  for (const WitnessHost::Act& a : wh.acts) { DBuf b; b.p = (char*)mbig.p + a.off * 8; b.n = a.n; b.ext = true; (a.is_out ? ps.staged_out : ps.staged_in)[a.node] = b; }
  wt.lap("  witness: uploads");
  // one batched commit: witness columns in order, then the table multiplicities
  std::vector<DBuf> to_commit(dcol.begin(), dcol.begin() + n_witness_cols);
  for (size_t i = 0; i < tabs.size(); i++) to_commit.push_back(mbig.slice(moffs[i], tabs[i].mult.size()));
  std::vector<DevCommit> comms = dev.commit_many(to_commit, false);
  wt.lap("  witness: commit_many");
  for (auto& p : pend) {
    LogUpWitness w; w.columns_per_instance = p.cpi; w.table_type = p.tt;
    for (size_t q = 0; q < p.col_ids.size(); q++) {
      size_t cid = p.col_ids[q];
      if (p.late < 0 && (!p.n_lookup_cols || q < p.n_lookup_cols)) w.columns.push_back(dcol[cid]); else w.extra_columns.push_back(dcol[cid]);
      w.commits.push_back(comms[cid]);
    }
    if (p.late >= 0) w.columns.push_back(dcol[late_ids[(size_t)p.late]]);
    if (p.logits_in >= 0) {  // (the arena allocations of a proof live until prove() releases its mark)
      const DBuf in = dcol[late_ids[(size_t)p.logits_in]], mx = dcol[p.col_ids.at(0)];
      DBuf diff = dev.alloc(in.n, false), onehot = dev.alloc(in.n, false);
      dev.logits_columns(in, mx, dcol[late_ids[(size_t)p.logits_idx]], diff, onehot);
      w.columns = {diff}; w.extra_columns = {mx};
      ps.logits_dev[p.node] = {in, onehot};
    }
    ps.lookup_witness[p.node].push_back(std::move(w));
  }
  for (size_t i = 0; i < tabs.size(); i++) {
    LogUpWitness w; w.is_table = true; w.table_type = tabs[i].tt;
    w.multiplicities = to_commit[n_witness_cols + i];
    auto res = ctx.table_cols_dev.find(tabs[i].tt);
    if (res != ctx.table_cols_dev.end()) w.columns = res->second;  // resident since Context::generate
    else for (size_t cid : tabs[i].col_ids) w.columns.push_back(dcol[cid]);
    w.columns_per_instance = w.columns.size();
    w.commits.push_back(comms[n_witness_cols + i]);
    ps.table_witness.push_back(std::move(w));
  }
  ps.constant_challenge = ps.t->get_and_append_challenge("table_constant");
  for (auto& kv : wh.counts) ps.challenge_map[kv.first] = kv.first.label() ? ps.t->get_and_append_challenge(kv.first.label()) : ex_one();
}

// Positional::prove, Learned (layers/transformer/positional.rs:327-452). The Add layer on (input, the first `tokens` rows of the table): both
// evaluated at the claim's point (Dev::mle_eval_batch; add.rs:81-145 with two inputs: no transcript traffic). Then the slice claim is lifted
// to the whole committed table: the output claim and the slice claim are absorbed, one coordinate per doubling is drawn (:80-99), the
// evaluation of every upper-half sub-matrix (rows [tokens 2^k, tokens 2^(k+1)): a contiguous slice of the table on the device) at the
// point's prefix is sent, and table(point | extras) follows by folding (:106-126).
inline Claim prove_positional(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  const size_t n = input.size();
  DP_REQUIRE((size_t(1) << last.point.size()) == n && n <= l.weights.size(), DP_ERR_SHAPE, "positional: claim point length");
  size_t mk = dev.mark();
  const DBuf& table = ps.ctx->weights_dev.at(id);
  DBuf in = dev.alloc(n, false);
  dev.upload_i64(in, input.data());
  const unsigned nv_sub = (unsigned)last.point.size(), diff = dp_ceil_log2(l.weights.size()) - nv_sub;
  DBuf both[2] = {in, table.slice(0, n)};
  Ext ev2[2];
  dev.mle_eval_batch(both, 2, last.point.data(), nv_sub, ev2);
  PositionalProof pp; pp.add_proof.left_eval = ev2[0]; pp.add_proof.right_eval = ev2[1];
  Transcript& t = *ps.t;
  t.append_exts(last.point); t.append_ext(last.eval); t.append_exts(last.point); t.append_ext(ev2[1]);
  std::vector<Ext> point = last.point;
  for (unsigned k = 0; k < diff; k++) point.push_back(t.read_challenge());
  Ext acc = ev2[1];
  for (unsigned k = 0; k < diff; k++) {
    const size_t len = n << k;
    DBuf sm = table.slice(len, len);
    Ext ev;
    dev.mle_eval_batch(&sm, 1, point.data(), nv_sub + k, &ev);
    pp.sub_matrix_evals.push_back(ev);
    const Ext c = point[nv_sub + k];
    acc = ex_add(ex_mul(acc, ex_sub(ex_one(), c)), ex_mul(ev, c));
  }
  ps.add_witness_claim(ps.ctx->model_comms.at(id).at("PositionalMatrix"), {point, acc});
  LayerProof lp; lp.kind = L_POSITIONAL; lp.pos = pp;
  ps.proofs[id] = lp;
  dev.release(mk);
  return {last.point, pp.add_proof.left_eval};
}

// Embeddings::prove (layers/transformer/embeddings.rs:359-462): the matmul protocol on (one-hot(tokens), table) without the one-hot
// matrix — its row variables fixed at the row part of the claim are reduced[x[i]] += beta(i, row part), a vocabulary-long vector built on
// the host from the (few) tokens and uploaded; the table's column variables fixed on the device (Dev::fix_low); one degree-2 sumcheck over
// the vocabulary. The table claim [column part | sumcheck point] goes to the commitment; the one-hot claim [sumcheck point | row part]
// is the model's input claim, which the verifier checks against the public tokens.
inline Claim prove_embeddings(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& tokens) {
  Dev& dev = *ps.dev;
  const unsigned nvc = dp_ceil_log2(l.ncols), nvr = dp_ceil_log2(tokens.size());
  DP_REQUIRE(is_pow2(tokens.size()) && last.point.size() == nvc + nvr, DP_ERR_SHAPE, "embeddings: claim point length");
  size_t mk = dev.mark();
  std::vector<Ext> col_pt(last.point.begin(), last.point.begin() + nvc), row_pt(last.point.begin() + nvc, last.point.end());
  std::vector<Ext> beta = host_eq_table(row_pt), reduced(l.nrows, ex_zero());
  for (size_t i = 0; i < tokens.size(); i++) reduced[(size_t)tokens[i]] = ex_add(reduced[(size_t)tokens[i]], beta[i]);
  DBuf in = dev.alloc(l.nrows, true), table = dev.alloc(l.nrows, true);
  dev.upload(in, (const u64*)reduced.data());
  dev.fix_low(table, ps.ctx->weights_dev.at(id), l.nrows, l.ncols, col_pt.data());
  DevVP vp(dp_ceil_log2(l.nrows));
  vp.add_mle_list({in, table}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, *ps.t);
  std::vector<Ext> one_hot_pt = sc.proof.point; one_hot_pt.insert(one_hot_pt.end(), row_pt.begin(), row_pt.end());
  std::vector<Ext> table_pt = col_pt; table_pt.insert(table_pt.end(), sc.proof.point.begin(), sc.proof.point.end());
  ps.add_witness_claim(ps.ctx->model_comms.at(id).at("EmbeddingMat"), {table_pt, sc.finals[1]});
  LayerProof lp; lp.kind = L_EMBED; lp.matmul.sumcheck = sc.proof; lp.matmul.individual_claims = sc.finals;
  ps.proofs[id] = lp;
  dev.release(mk);
  return {one_hot_pt, sc.finals[0]};
}

// Add::prove_step with a static operand (layers/add.rs:81-145): no sumcheck, no transcript traffic. The input's evaluation at the claim's
// point (one Dev::mle_eval_batch over the uploaded activation); the operand's evaluation follows from out(r) = M1 x(r) + M2 c(r) and
// becomes a claim on the operand's commitment; the input claim goes to the previous layer.
inline Claim prove_add(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  DP_REQUIRE((size_t(1) << last.point.size()) == input.size(), DP_ERR_SHAPE, "add: claim point length");
  size_t mk = dev.mark();
  DBuf in = dev.alloc(input.size(), false);
  dev.upload_i64(in, input.data());
  Ext left_eval;
  dev.mle_eval_batch(&in, 1, last.point.data(), (unsigned)last.point.size(), &left_eval);
  const Ext scaled = ex_mul_base(left_eval, gl_from_i64(l.add_left));
  const Ext right_eval = ex_mul_base(ex_sub(last.eval, scaled), gl_inv(gl_from_i64(l.add_right)));
  ps.add_witness_claim(ps.ctx->model_comms.at(id).at("255"), {last.point, right_eval});
  LayerProof lp; lp.kind = L_ADD; lp.add.left_eval = left_eval; lp.add.right_eval = right_eval;
  ps.proofs[id] = lp;
  dev.release(mk);
  return {last.point, left_eval};
}

// MatMul::prove_step (layers/matrix_mul.rs:701-873), (Input, Weight) arrangement, right matrix not transposed. split_claim (:339-356):
// the low variables of the output point address the columns (-> right matrix), the high ones the rows (-> left matrix). The bias is
// evaluated on the column part; left = input with its row variables fixed (Dev::fix_high over the [s][k] activation), right = the
// constant matrix with its column variables fixed (Dev::fix_low); one degree-2 sumcheck over the inner dimension. full_points
// (:364-383): the input claim [sumcheck point | row part] goes to the previous layer, the weight claim [column part | sumcheck point]
// to the batch opening.
inline Claim prove_matmul(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  const size_t k = l.nrows, n = l.ncols, s_ = input.size() / k;
  const unsigned nvc = dp_ceil_log2(n), nvr = dp_ceil_log2(s_);
  DP_REQUIRE(is_pow2(s_) && s_ * k == input.size() && last.point.size() == nvc + nvr, DP_ERR_SHAPE, "matmul: claim point length");
  size_t mk = dev.mark();
  const auto& comms = ps.ctx->model_comms.at(id);
  const bool hb = !l.bias.empty();
  std::vector<Ext> pt_right(last.point.begin(), last.point.begin() + nvc), pt_left(last.point.begin() + nvc, last.point.end());
  Ext bias_eval = ex_zero();
  if (hb) dev.mle_eval_batch(&comms.at("MatMulBias").evals, 1, pt_right.data(), nvc, &bias_eval);
  DBuf in = dev.alloc(input.size(), false);
  dev.upload_i64(in, input.data());
  DBuf left = dev.alloc(k, true), right = dev.alloc(k, true);
  dev.fix_high(left, in, s_, k, pt_left.data());
  // not transposed: [k][n], its column variables are the low ones; transposed: stored [n][k], the variables of its rows are the high ones (:815-824)
  if (l.mm_transpose) dev.fix_high(right, ps.ctx->weights_dev.at(id), n, k, pt_right.data());
  else dev.fix_low(right, ps.ctx->weights_dev.at(id), k, n, pt_right.data());
  DevVP vp(dp_ceil_log2(k));
  vp.add_mle_list({left, right}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, *ps.t);
  std::vector<Ext> point_left = sc.proof.point; point_left.insert(point_left.end(), pt_left.begin(), pt_left.end());
  std::vector<Ext> point_right = l.mm_transpose ? sc.proof.point : pt_right;
  if (l.mm_transpose) point_right.insert(point_right.end(), pt_right.begin(), pt_right.end()); else point_right.insert(point_right.end(), sc.proof.point.begin(), sc.proof.point.end());
  if (hb) ps.add_witness_claim(comms.at("MatMulBias"), {pt_right, bias_eval});   // BTreeMap order: "MatMulBias" < "MatMulWeight"
  ps.add_witness_claim(comms.at("MatMulWeight"), {point_right, sc.finals[1]});
  LayerProof lp; lp.kind = L_MATMUL; lp.matmul.sumcheck = sc.proof; lp.matmul.individual_claims = sc.finals; lp.matmul.has_bias = hb; lp.matmul.bias_eval = bias_eval;
  ps.proofs[id] = lp;
  dev.release(mk);
  return {point_left, sc.finals[0]};
}

// ---- nodes with two inputs or several outputs (the model as a graph, layers/provable/mod.rs:195-565)
// MatMul::prove_step (layers/matrix_mul.rs:701-873) when BOTH operands are inputs of the node: the same degree-2 sumcheck over the inner
// dimension; nothing is committed, both final evaluations leave as claims — [sumcheck point | row part] for the left input,
// [column part | sumcheck point] (or [sumcheck point | column part] under TransposeB) for the right one.
inline std::vector<Claim> prove_matmul2(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
  Dev& dev = *ps.dev;
  const size_t k = l.nrows, n = l.ncols, s_ = a.size() / k;
  const unsigned nvc = dp_ceil_log2(n), nvr = dp_ceil_log2(s_);
  DP_REQUIRE(is_pow2(s_) && s_ * k == a.size() && b.size() == k * n && last.point.size() == nvc + nvr, DP_ERR_SHAPE, "matmul2: claim point length");
  size_t mk = dev.mark();
  std::vector<Ext> cols(last.point.begin(), last.point.begin() + nvc), rows(last.point.begin() + nvc, last.point.end());
  DBuf da = dev.alloc(a.size(), false), db = dev.alloc(b.size(), false);
  dev.upload_i64(da, a.data()); dev.upload_i64(db, b.data());
  DBuf left = dev.alloc(k, true), right = dev.alloc(k, true);
  dev.fix_high(left, da, s_, k, rows.data());
  if (l.mm_transpose) dev.fix_high(right, db, n, k, cols.data()); else dev.fix_low(right, db, k, n, cols.data());
  DevVP vp(dp_ceil_log2(k));
  vp.add_mle_list({left, right}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, *ps.t);
  dev.release(mk);
  std::vector<Ext> pl = sc.proof.point; pl.insert(pl.end(), rows.begin(), rows.end());
  std::vector<Ext> pr;
  if (l.mm_transpose) { pr = sc.proof.point; pr.insert(pr.end(), cols.begin(), cols.end()); } else { pr = cols; pr.insert(pr.end(), sc.proof.point.begin(), sc.proof.point.end()); }
  LayerProof lp; lp.kind = L_MATMUL2; lp.matmul.sumcheck = sc.proof; lp.matmul.individual_claims = sc.finals; lp.matmul.has_bias = false;
  ps.proofs[id] = lp;
  return {{pl, sc.finals[0]}, {pr, sc.finals[1]}};
}
// Add::prove_step without operand (layers/add.rs:81-145): both inputs at the claim's point in one Dev::mle_eval_batch
inline std::vector<Claim> prove_add2(ProverState& ps, size_t id, const Claim& last, const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
  Dev& dev = *ps.dev;
  DP_REQUIRE((size_t(1) << last.point.size()) == a.size() && a.size() == b.size(), DP_ERR_SHAPE, "add2: claim point length");
  size_t mk = dev.mark();
  DBuf tabs[2] = {dev.alloc(a.size(), false), dev.alloc(b.size(), false)};
  dev.upload_i64(tabs[0], a.data()); dev.upload_i64(tabs[1], b.data());
  Ext ev[2];
  dev.mle_eval_batch(tabs, 2, last.point.data(), (unsigned)last.point.size(), ev);
  dev.release(mk);
  LayerProof lp; lp.kind = L_ADD2; lp.add.left_eval = ev[0]; lp.add.right_eval = ev[1];
  ps.proofs[id] = lp;
  return {{last.point, ev[0]}, {last.point, ev[1]}};
}
// The point of ConcatMatMul's output claim by axis (MatrixPermutations::split_output_claim_point, concat_matmul.rs:295-343): the last axis of
// the (permuted) output owns the low coordinates; returned for the axes of the un-permuted [concat][rows][cols] result
struct CmPoint { std::vector<Ext> concat, row, col; };
inline CmPoint cm_split_point(const LayerSpec& l, const CmShape& g, const std::vector<Ext>& point) {
  size_t nv[3], total = 0;
  for (int d = 0; d < 3; d++) { nv[d] = dp_ceil_log2(g.out[d]); total += nv[d]; }
  DP_REQUIRE(point.size() == total, DP_ERR_SHAPE, "concat matmul: claim point length");
  std::vector<Ext> by_axis[3];
  size_t end = point.size();
  for (int d = 0; d < 3; d++) { by_axis[d].assign(point.begin() + (end - nv[d]), point.begin() + end); end -= nv[d]; }
  int at[3] = {0, 1, 2};  // at[axis of the plain result] = where the permutation put it
  if (!l.cm_perm.empty()) for (int i = 0; i < 3; i++) at[l.cm_perm[i]] = i;
  return {by_axis[at[0]], by_axis[at[1]], by_axis[at[2]]};
}
// InputMatrixDimensions::input_mle_for_proving (concat_matmul.rs:134-166) on the device: the rank-3 input with the coordinates of its
// OUTPUT axis fixed at `pt`; the table that is left runs over [concat][mat_mul]. Whether the tensor is re-laid first follows the reference
// (it decides which axis the remaining variables see as low).
inline DBuf cm_fix_output_axis(Dev& dev, const std::vector<int64_t>& x, const size_t dims[3], const int axes[3], const std::vector<Ext>& pt) {
  const int concat = axes[0], mm = axes[1], outa = axes[2];
  const size_t O = dims[outa], rest = x.size() / O;
  DP_REQUIRE((size_t(1) << pt.size()) == O && O >= 2, DP_ERR_SHAPE, "concat matmul: output axis of fewer than two entries");
  DBuf in = dev.alloc(x.size(), false), out = dev.alloc(rest, true);
  if (concat > mm || outa == 1) {
    const int order[3] = {concat, mm, outa};
    const std::vector<int64_t> y = transpose3(x, dims, order);
    dev.upload_i64(in, y.data());
    dev.fix_low(out, in, rest, O, pt.data());
  } else {
    dev.upload_i64(in, x.data());
    if (outa == 0) dev.fix_high(out, in, O, rest, pt.data()); else dev.fix_low(out, in, rest, O, pt.data());
  }
  return out;
}
// InputMatrixDimensions::build_point_for_input (concat_matmul.rs:116-132): the sub-points in the order of the input's axes, last axis first
inline std::vector<Ext> cm_input_point(const int axes[3], const std::vector<Ext>& p_concat, const std::vector<Ext>& p_mm, const std::vector<Ext>& p_out) {
  const std::vector<Ext>* of_axis[3] = {nullptr, nullptr, nullptr};
  of_axis[axes[0]] = &p_concat; of_axis[axes[1]] = &p_mm; of_axis[axes[2]] = &p_out;
  std::vector<Ext> pt;
  for (int d = 2; d >= 0; d--) pt.insert(pt.end(), of_axis[d]->begin(), of_axis[d]->end());
  return pt;
}
// ConcatMatMul::prove_step (concat_matmul.rs:467-566): one degree-3 sumcheck over (chunk, inner index) of beta(chunk) * A_chunk[row point][.]
// * B_chunk[.][column point]; two claims out, one per input
inline std::vector<Claim> prove_concat_matmul(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
  Dev& dev = *ps.dev;
  const CmShape g = cm_shape(l);
  const CmPoint p = cm_split_point(l, g, last.point);
  size_t mk = dev.mark();
  DBuf left = cm_fix_output_axis(dev, a, l.cm_a, l.cm_left, p.row), right = cm_fix_output_axis(dev, b, l.cm_b, l.cm_right, p.col);
  DP_REQUIRE(left.n == g.C * g.M && right.n == left.n, DP_ERR_SHAPE, "concat matmul: reduced tables");
  std::vector<Ext> bc = host_eq_table(p.concat), bw(g.C * g.M);  // beta(chunk), repeated along the inner axis
  for (size_t c = 0; c < g.C; c++) for (size_t j = 0; j < g.M; j++) bw[c * g.M + j] = bc[c];
  DBuf beta = dev.alloc(bw.size(), true);
  dev.upload(beta, (const u64*)bw.data());
  DevVP vp(dp_ceil_log2(left.n));
  vp.add_mle_list({beta, left, right}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, *ps.t);
  dev.release(mk);
  const unsigned nvm = dp_ceil_log2(g.M);  // split_sumcheck_point (:256-281): the inner coordinates come first
  const std::vector<Ext> s_mm(sc.proof.point.begin(), sc.proof.point.begin() + nvm), s_concat(sc.proof.point.begin() + nvm, sc.proof.point.end());
  LayerProof lp; lp.kind = L_CONCAT_MATMUL; lp.cmm.sumcheck = sc.proof; lp.cmm.individual_claims = sc.finals;
  ps.proofs[id] = lp;
  return {{cm_input_point(l.cm_left, s_concat, s_mm, p.row), sc.finals[1]}, {cm_input_point(l.cm_right, s_concat, s_mm, p.col), sc.finals[2]}};
}
inline SamePolyProof same_poly_prove(Dev& dev, const std::vector<Claim>& claims, const DBuf& poly, Transcript& t);
// QKV::prove (layers/transformer/qkv.rs:462-630): X W_q, X W_k, X W_v proven by ONE sumcheck (coefficients 1, c1, c2 drawn after the output
// points and the bias-free evaluations have been absorbed), the three resulting claims on X merged by same_poly; six claims go to the
// commitments of the weights and biases
inline std::vector<Claim> prove_qkv(ProverState& ps, size_t id, const LayerSpec& l, const std::vector<Claim>& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  const size_t k = l.nrows, n = l.ncols, s_ = input.size() / k;
  const unsigned nvc = dp_ceil_log2(n), nvr = dp_ceil_log2(s_);
  DP_REQUIRE(last.size() == 3 && is_pow2(s_) && s_ * k == input.size(), DP_ERR_SHAPE, "qkv: three output claims expected");
  static const char* const wn[3] = {"WeightQ", "WeightK", "WeightV"}; static const char* const bn[3] = {"BiasQ", "BiasK", "BiasV"};
  const auto& comms = ps.ctx->model_comms.at(id);
  size_t mk = dev.mark();
  std::vector<Ext> rows[3], cols[3];
  Ext bias_eval[3], pre[3];
  for (int w = 0; w < 3; w++) {
    DP_REQUIRE(last[w].point.size() == nvc + nvr, DP_ERR_SHAPE, "qkv: claim point length");
    cols[w].assign(last[w].point.begin(), last[w].point.begin() + nvc); rows[w].assign(last[w].point.begin() + nvc, last[w].point.end());  // split_claim_point (:173-184)
    dev.mle_eval_batch(&comms.at(bn[w]).evals, 1, cols[w].data(), nvc, &bias_eval[w]);
    pre[w] = ex_sub(last[w].eval, bias_eval[w]);
  }
  for (int w = 0; w < 3; w++) { ps.t->append_exts(last[w].point); ps.t->append_ext(pre[w]); }  // challenges_for_batched_sumcheck (:210-232)
  const Ext coeff[3] = {ex_one(), ps.t->read_challenge(), ps.t->read_challenge()};
  DBuf in = dev.alloc(input.size(), false);
  dev.upload_i64(in, input.data());
  DevVP vp(dp_ceil_log2(k));
  for (int w = 0; w < 3; w++) {
    DBuf x = dev.alloc(k, true), wm = dev.alloc(k, true);
    dev.fix_high(x, in, s_, k, rows[w].data());
    dev.fix_low(wm, comms.at(wn[w]).evals, k, n, cols[w].data());
    vp.add_mle_list({x, wm}, coeff[w]);
  }
  SumcheckOut sc = sumcheck_prove(dev, vp, *ps.t);
  DP_REQUIRE(sc.finals.size() == 6, DP_ERR_SHAPE, "qkv: six final evaluations expected");
  std::vector<Claim> on_input(3), on_weight(3);
  for (int w = 0; w < 3; w++) {  // build_points (:193-204)
    on_input[w].point = sc.proof.point; on_input[w].point.insert(on_input[w].point.end(), rows[w].begin(), rows[w].end()); on_input[w].eval = sc.finals[2 * w];
    on_weight[w].point = cols[w]; on_weight[w].point.insert(on_weight[w].point.end(), sc.proof.point.begin(), sc.proof.point.end()); on_weight[w].eval = sc.finals[2 * w + 1];
  }
  // add_common_claims walks the node's polynomials in BTreeMap order: BiasK, BiasQ, BiasV, WeightK, WeightQ, WeightV
  for (int w : {1, 0, 2}) ps.add_witness_claim(comms.at(bn[w]), {cols[w], bias_eval[w]});
  for (int w : {1, 0, 2}) ps.add_witness_claim(comms.at(wn[w]), on_weight[w]);
  DBuf xin = dev.alloc(input.size(), true);
  { std::vector<u64> ww(2 * input.size()); for (size_t i = 0; i < input.size(); i++) { ww[2 * i] = gl_from_i64(input[i]); ww[2 * i + 1] = 0; } dev.upload(xin, ww.data()); }
  SamePolyProof agg = same_poly_prove(dev, on_input, xin, *ps.t);
  dev.release(mk);
  LayerProof lp; lp.kind = L_QKV; lp.qkv.sumcheck = sc.proof; lp.qkv.aggregation = agg; lp.qkv.pre_bias_evals.assign(pre, pre + 3); lp.qkv.individual_claims = sc.finals;
  ps.proofs[id] = lp;
  return {{agg.sumcheck.point, agg.evals[1]}};
}

inline std::vector<u64> ext_words_from_i64(const std::vector<int64_t>& v) { std::vector<u64> w(2 * v.size()); for (size_t i = 0; i < v.size(); i++) { w[2 * i] = gl_from_i64(v[i]); w[2 * i + 1] = 0; } return w; }

inline Claim prove_dense(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  DP_REQUIRE((size_t(1) << last.point.size()) == l.nrows, DP_ERR_SHAPE, "dense: claim point length");
  size_t mk = dev.mark();
  const auto& comms = ps.ctx->model_comms.at(id);
  Ext bias_eval;
  DBuf in;  // trace.into_fields(): i64 -> Ext (model/trace.rs:50-92)
  if (ps.staged_in.count(id) && ps.staged_in[id].n == input.size()) in = ps.staged_in[id];
  else { in = dev.alloc(input.size(), true); std::vector<u64> w = ext_words_from_i64(input); dev.upload(in, w.data()); }
  SumcheckOut sc;
  Dev::DenseTailOut dto;
  // a device that keeps the sponge to itself does the bias evaluation, fix_high and the sumcheck in one go (Dev::dense_tail)
  if (dev.dense_tail(comms.at("DenseBias").evals, ps.ctx->weights_dev.at(id), l.nrows, l.ncols, in, last.point.data(), ps.t->challenger(), dto)) {
    bias_eval = dto.bias_eval;
    sc.proof.proofs = dto.msgs; sc.proof.point = dto.point; sc.finals = {dto.finals[0], dto.finals[1]};
  } else {
    dev.mle_eval_batch(&comms.at("DenseBias").evals, 1, last.point.data(), (unsigned)last.point.size(), &bias_eval);
    DBuf mat = dev.alloc(l.ncols, true);
    dev.fix_high(mat, ps.ctx->weights_dev.at(id), l.nrows, l.ncols, last.point.data());
    DevVP vp(dp_ceil_log2(l.ncols));
    vp.add_mle_list({mat, in}, ex_one());
    sc = sumcheck_prove(dev, vp, *ps.t);
  }
  std::vector<Ext> point = sc.proof.point; point.insert(point.end(), last.point.begin(), last.point.end());
  ps.add_witness_claim(comms.at("DenseBias"), {last.point, bias_eval});   // BTreeMap order: "DenseBias" < "DenseWeight"
  ps.add_witness_claim(comms.at("DenseWeight"), {point, sc.finals[0]});
  LayerProof lp; lp.kind = L_DENSE; lp.dense.sumcheck = sc.proof; lp.dense.bias_eval = bias_eval; lp.dense.individual_claims = sc.finals;
  ps.proofs[id] = lp;
  dev.release(mk);
  return {sc.proof.point, sc.finals[1]};
}
inline Ext recombine_claims(const LayerSpec& l, Ext clamping_claim, const Ext* shifted, size_t ns) {
  Ext full = ex_mul(ex_from_u64(u64(1) << l.shift()), clamping_claim), pw = ex_one();
  for (size_t i = 0; i < ns; i++) { full = ex_add(full, ex_mul(shifted[i], pw)); pw = ex_mul(pw, ex_from_u64(u64(1) << Q_BIT_LEN)); }
  return ex_mul(ex_sub(full, ex_from_u64(u64(1) << (l.shift() - 1))), ex_inv(ex_from_i64(l.fixed_point_multiplier)));
}
inline Claim prove_requant(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last) {
  Dev& dev = *ps.dev;
  std::vector<LogUpWitness>& ws = ps.lookup_witness.at(id);
  LogUpWitness& cw = ws[0]; LogUpWitness& sw = ws[1];
  LogUpProof cproof = logup_batch_prove(dev, ps.logup_input(cw), *ps.t);
  LogUpProof sproof = logup_batch_prove(dev, ps.logup_input(sw), *ps.t);
  size_t mk = dev.mark();
  size_t n = cw.columns[0].n; unsigned nv = dp_ceil_log2(n);
  DBuf clamp_in = cw.columns[0], clamp_out = cw.columns[1];
  DBuf cbeta = dev.alloc(n, true), lbeta = dev.alloc(n, true), sbeta = dev.alloc(n, true);
  DP_REQUIRE(last.point.size() == nv, DP_ERR_SHAPE, "requant: claim point length");
  std::vector<EqAcc> eqs = {{cbeta, cproof.output_claims[0].point, ex_one(), false}, {lbeta, last.point, ex_one(), false}, {sbeta, sproof.output_claims[0].point, ex_one(), false}};
  Ext b = ps.t->get_and_append_challenge("requant_batching");
  DevVP vp(nv);
  vp.add_mle_list({clamp_out, lbeta}, ex_one());
  vp.add_mle_list({clamp_out, cbeta}, b);
  Ext comb = ex_mul(b, b);
  vp.add_mle_list({clamp_in, cbeta}, comb);
  comb = ex_mul(comb, b);
  for (auto& m : sw.columns) { vp.add_mle_list({sbeta, m}, comb); comb = ex_mul(comb, b); }
  SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, *ps.t);
  dev.release(mk);
  const std::vector<Ext>& fin = sc.finals;
  Ext cout_eval = fin[0], cin_eval = fin[3];
  size_t ns = fin.size() - 5;
  Ext combined = recombine_claims(l, cin_eval, &fin[5], ns);
  RequantProof rp; rp.io_accumulation = sc.proof; rp.clamping_lookup = cproof; rp.shifted_lookup = sproof;
  std::vector<Ext> evs = {cin_eval, cout_eval}; evs.insert(evs.end(), fin.begin() + 5, fin.end());
  std::vector<DevCommit> cm = cw.commits; cm.insert(cm.end(), sw.commits.begin(), sw.commits.end());
  for (size_t i = 0; i < evs.size(); i++) { rp.commitments.push_back(pure_commitment(cm[i])); ps.add_witness_claim(cm[i], {sc.proof.point, evs[i]}); rp.accumulation_evals.push_back(evs[i]); }
  LayerProof lp; lp.kind = L_REQUANT; lp.req = rp; ps.proofs[id] = lp;
  return {sc.proof.point, combined};
}
// same_poly::Prover::prove (commit/same_poly.rs:88-122)
inline SamePolyProof same_poly_prove(Dev& dev, const std::vector<Claim>& claims, const DBuf& poly, Transcript& t) {
  size_t mk = dev.mark();
  unsigned nv = dp_ceil_log2(poly.n);
  std::vector<Ext> a = t.read_challenges(claims.size());
  DBuf beta = dev.alloc(poly.n, true);
  std::vector<EqAcc> eqs;
  for (size_t i = 0; i < claims.size(); i++) {
    DP_REQUIRE(claims[i].point.size() == nv, DP_ERR_SHAPE, "same_poly: claim point length");
    eqs.push_back({beta, claims[i].point, a[i], i > 0});
  }
  DevVP vp(nv);
  vp.add_mle_list({beta, poly}, ex_one());
  SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, t);
  dev.release(mk);
  return {sc.proof, sc.finals};
}
// Activation::prove_step (activation.rs:385-456) for both activations. GELU (`multiplier` > 0): the first lookup column holds input * multiplier, the claim
// handed on is the lookup's claim times 1 / multiplier (:405-413). The COMMITTED column is the scaled one, and the verifier opens it at the lookup's own claim
// (verify_activation, :495-505: `verifier_claims.claims().iter().take(1)`). The reference's prover hands its commitment prover the DESCALED claim instead
// (:419-421 shadow `input_claim` before the `commits` array is built): its batch opening then starts from a wrong sum and cannot verify, except where the
// claim is never used — polynomials of at most 2^7 entries, opened by showing them (`_eval` of Basefold::open, mpcs/src/basefold.rs:466-483; the size of
// the reference's own test, activation.rs:686-697) — or multiplier = 1. Here the commitment gets the claim the verifier will check; the proof stream is
// the reference's wherever the reference produces one that verifies.
inline bool gelu_reference_letter() { const char* e = getenv("DP_GELU_REFERENCE_LETTER"); return e && atoi(e) != 0; }  // (read per proof: a host may switch between proofs)
inline Claim prove_relu(ProverState& ps, size_t id, const Claim& last, const std::vector<int64_t>& output, int64_t multiplier = 0) {
  Dev& dev = *ps.dev;
  LogUpWitness& w = ps.lookup_witness.at(id)[0];
  LogUpProof lproof = logup_batch_prove(dev, ps.logup_input(w), *ps.t);
  Claim input_claim = lproof.output_claims[0], output_claim = lproof.output_claims[1];
  size_t mk = dev.mark();
  DBuf out;
  if (ps.staged_out.count(id) && ps.staged_out[id].n == output.size()) out = ps.staged_out[id];
  else { out = dev.alloc(output.size(), true); std::vector<u64> ww = ext_words_from_i64(output); dev.upload(out, ww.data()); }
  SamePolyProof sp = same_poly_prove(dev, {last, output_claim}, out, *ps.t);
  dev.release(mk);
  ActivationProof ap; ap.io_accumulation = sp; ap.lookup = lproof;
  Claim descaled = input_claim;
  if (multiplier) descaled.eval = ex_mul(input_claim.eval, ex_inv(ex_from_i64(multiplier)));
  // DP_GELU_REFERENCE_LETTER=1: the commitment of the scaled column gets the DESCALED claim, as the reference's prover files it (:419-430) — the reference
  // prover's byte stream for every GELU model; it only verifies where the reference's own does (columns of <= 2^7 entries, or multiplier 1)
  ps.add_witness_claim(w.commits[0], multiplier && gelu_reference_letter() ? descaled : input_claim); ap.commits.push_back(pure_commitment(w.commits[0]));
  ps.add_witness_claim(w.commits[1], {sp.sumcheck.point, sp.evals[1]}); ap.commits.push_back(pure_commitment(w.commits[1]));
  LayerProof lp; lp.kind = multiplier ? L_GELU : L_RELU; lp.act = ap; ps.proofs[id] = lp;
  return descaled;
}

// LayerNorm::prove + prove_step (layers/transformer/layernorm.rs:729-1100). After the two lookups, three sumchecks: (1) all lookup claims to ONE
// point; (2) at (1/2, .., 1/2 | that point) — a sum over the normalisation dimension is 2^k times the evaluation with 1/2 in its coordinates —
// the inverse-square-root input, recombined with its range-checked chunks, is multiplier (N sum x^2 - (sum x)^2); the output claim is gamma (N x -
// sum x) inv_sqrt + beta; the inv_sqrt column of both is the committed one: three statements batched by two challenges, degree 4;
// (3) `mean` is the row sum of the input. All tables are built on the host from the trace (row sums, repeated gamma / beta / lookup output) and
// uploaded as base-field columns; the eq tables are made on the device.
inline Claim prove_layernorm(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last, const std::vector<int64_t>& input) {
  Dev& dev = *ps.dev;
  const size_t fd = l.weights.size(), n = input.size(), rows = n / fd;
  const unsigned sdv = dp_ceil_log2(fd), nv_full = dp_ceil_log2(n);
  DP_REQUIRE(last.point.size() == nv_full, DP_ERR_SHAPE, "layernorm: claim point length");
  std::vector<LogUpWitness>& ws = ps.lookup_witness.at(id);
  DP_REQUIRE(ws.size() == 2, DP_ERR_SHAPE, "layernorm: two lookups expected");
  const LayerNormTrace& d = ps.ln_trace.at(id);
  LayerNormProof pr;
  for (auto& w : ws) pr.logup_proofs.push_back(logup_batch_prove(dev, ps.logup_input(w), *ps.t));
  const std::vector<Claim>& inv_claims = pr.logup_proofs[0].output_claims; const std::vector<Claim>& range_claims = pr.logup_proofs[1].output_claims;
  const unsigned nv = (unsigned)inv_claims[0].point.size();
  DP_REQUIRE(inv_claims.size() == 2 && range_claims.size() == ws[1].columns.size() && nv + sdv == nv_full, DP_ERR_SHAPE, "layernorm: lookup claims");
  std::vector<Ext> bc; for (unsigned q = 0; q < dp_ceil_log2(inv_claims.size() + range_claims.size()); q++) bc.push_back(ps.t->get_and_append_challenge("batching"));
  const std::vector<Ext> rlc = host_eq_table(bc);
  std::vector<DBuf> columns = ws[0].columns; columns.insert(columns.end(), ws[1].columns.begin(), ws[1].columns.end());
  std::vector<DevCommit> commits = ws[0].commits; commits.insert(commits.end(), ws[1].commits.begin(), ws[1].commits.end());
  size_t mk = dev.mark();
  {
    DBuf sqrt_eq = dev.alloc(rows, true), range_eq = dev.alloc(rows, true);
    std::vector<EqAcc> eqs = {{sqrt_eq, inv_claims[0].point, ex_one(), false}, {range_eq, range_claims[0].point, ex_one(), false}};
    DevVP vp(nv);
    for (size_t q = 0; q < columns.size(); q++) vp.add_mle_list({columns[q], q < 2 ? sqrt_eq : range_eq}, rlc.at(q));
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, *ps.t);
    pr.accumulation_proof = sc.proof;
    const std::vector<Ext>& fin = sc.finals;  // sqrt_in, sqrt_eq, sqrt_out, range_0, range_eq, range_1, ..
    pr.acc_evals = {fin[0], fin[2], fin[3]}; pr.acc_evals.insert(pr.acc_evals.end(), fin.begin() + 5, fin.end());
  }
  dev.release(mk);
  const std::vector<Ext> sc_point = pr.accumulation_proof.point;
  const Ext two_inv = ex_inv(ex_from_u64(2)), two_mul = ex_from_u64(u64(1) << sdv);
  const Ext c1 = ps.t->get_and_append_challenge("batching"), c2 = ps.t->get_and_append_challenge("batching");
  const Ext first = ex_mul(ex_sub(ex_one(), c1), ex_sub(ex_one(), c2)), second = ex_mul(c1, ex_sub(ex_one(), c2)), third = ex_mul(ex_sub(ex_one(), c1), c2);
  std::vector<Ext> full_point(sdv, two_inv); full_point.insert(full_point.end(), sc_point.begin(), sc_point.end());
  const Ext n_f = ex_from_u64(l.ln_dim_size), mult_f = ex_from_i64(l.ln_multiplier);
  // input | mean | gamma repeated | beta repeated | lookup output repeated, one upload
  std::vector<int64_t> host(5 * n);
  for (size_t c = 0; c < rows; c++) for (size_t i = 0; i < fd; i++) {
    const size_t j = c * fd + i;
    host[j] = input[j]; host[n + j] = d.row_sum[c]; host[2 * n + j] = l.weights[i]; host[3 * n + j] = l.bias[i]; host[4 * n + j] = d.lookup_output[c];
  }
  DBuf all = dev.alloc(5 * n, false);
  dev.upload_i64(all, host.data());
  DBuf input_poly = all.slice(0, n), mean_poly = all.slice(n, n), gamma_poly = all.slice(2 * n, n), beta_poly = all.slice(3 * n, n), inv_poly = all.slice(4 * n, n);
  Ext input_eval, mean_eval, inv_eval;
  {
    size_t mk2 = dev.mark();
    DBuf input_eq = dev.alloc(n, true), last_eq = dev.alloc(n, true);
    std::vector<EqAcc> eqs = {{input_eq, full_point, ex_one(), false}, {last_eq, last.point, ex_one(), false}};
    DevVP vp(nv_full);
    vp.add_mle_list({input_eq, input_poly, input_poly}, ex_mul(ex_mul(first, mult_f), ex_mul(n_f, two_mul)));
    vp.add_mle_list({input_eq, mean_poly, mean_poly}, ex_neg(ex_mul(first, mult_f)));
    vp.add_mle_list({last_eq, gamma_poly, input_poly, inv_poly}, ex_mul(second, n_f));
    vp.add_mle_list({last_eq, gamma_poly, mean_poly, inv_poly}, ex_neg(second));
    vp.add_mle_list({last_eq, beta_poly}, second);
    vp.add_mle_list({input_eq, inv_poly}, third);
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, *ps.t);
    pr.io_proof = sc.proof;
    const std::vector<Ext>& fin = sc.finals;  // input_eq, input, mean, last_eq, gamma, inv_sqrt_out, beta
    input_eval = fin[1]; mean_eval = fin[2]; pr.gamma_eval = fin[4]; inv_eval = fin[5]; pr.beta_eval = fin[6];
    dev.release(mk2);
  }
  const std::vector<Ext> io_point = pr.io_proof.point;
  const Ext ic = ps.t->get_and_append_challenge("batching");
  Claim input_claim;
  {
    std::vector<Ext> sum_io(sdv, two_inv); sum_io.insert(sum_io.end(), io_point.begin() + sdv, io_point.end());
    DBuf eq_io = dev.alloc(n, true), eq_sum = dev.alloc(n, true);
    std::vector<EqAcc> eqs = {{eq_io, io_point, ex_one(), false}, {eq_sum, sum_io, ex_one(), false}};
    dev.upload_i64(input_poly, input.data());  // (the io sumcheck folded its copy away)
    DevVP vp(nv_full);
    vp.add_mle_list({input_poly, eq_io}, ex_sub(ex_one(), ic));
    vp.add_mle_list({input_poly, eq_sum}, ex_mul(ic, two_mul));
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, *ps.t);
    pr.input_proof = sc.proof;
    input_claim = {sc.proof.point, sc.finals[0]};
  }
  dev.release(mk);
  // witness claims: the lookup input at the accumulation point, the lookup output at the tail of the io point, the chunks at the accumulation point
  std::vector<Claim> cl = {{sc_point, pr.acc_evals[0]}, {std::vector<Ext>(io_point.begin() + sdv, io_point.end()), inv_eval}};
  for (size_t q = 2; q < pr.acc_evals.size(); q++) cl.push_back({sc_point, pr.acc_evals[q]});
  DP_REQUIRE(cl.size() == commits.size(), DP_ERR_SHAPE, "layernorm: claims and commitments");
  for (size_t q = 0; q < cl.size(); q++) { pr.commitments.push_back(pure_commitment(commits[q])); pr.evaluations.push_back(cl[q].eval); ps.add_witness_claim(commits[q], cl[q]); }
  pr.evaluations.push_back(input_eval); pr.evaluations.push_back(mean_eval);
  // add_common_claims walks the node's BTreeMap: "LayerNormBeta" then "LayerNormGamma"
  const std::vector<Ext> gp(io_point.begin(), io_point.begin() + sdv);
  auto& comms = ps.ctx->model_comms.at(id);
  ps.add_witness_claim(comms.at("LayerNormBeta"), {gp, pr.beta_eval});
  ps.add_witness_claim(comms.at("LayerNormGamma"), {gp, pr.gamma_eval});
  LayerProof lp; lp.kind = L_LAYERNORM; lp.ln = pr; ps.proofs[id] = lp;
  return input_claim;
}

// Softmax::prove_step (layers/transformer/softmax.rs:573-888): the lookups (exponential table; the two low bytes; the row sums against the values
// within the allowable error of one; the bits above the exponential's input against the zero table), ONE sumcheck that brings every lookup
// claim to a single point and ties both the output claim and the row sums (1/2 in the coordinates of the normalised dimension, times 2^k) to
// exp_out * prod zero_out, and the mask sumcheck eq (shifted_input tril + bias). The claim handed on is the one the verifier derives,
// (shifted - shift) / scalar (:1541-1543); the reference's prover keeps the undivided value (:748-749), which nothing downstream reads.
inline Claim prove_softmax(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last) {
  Dev& dev = *ps.dev;
  const SoftmaxTrace& d = ps.sm_trace.at(id);
  std::vector<LogUpWitness>& ws = ps.lookup_witness.at(id);
  const bool zero = l.sm_zero_chunks != 0;
  DP_REQUIRE(ws.size() == (zero ? 4u : 3u), DP_ERR_SHAPE, "softmax: lookup witnesses");
  SoftmaxProof pr;
  for (auto& w : ws) pr.logup_proofs.push_back(logup_batch_prove(dev, ps.logup_input(w), *ps.t));
  const std::vector<Ext> exp_point = pr.logup_proofs[0].output_claims.at(0).point, range_point = pr.logup_proofs[1].output_claims.at(0).point, error_point = pr.logup_proofs[2].output_claims.at(0).point;
  const size_t n = d.exp_in.size(); const unsigned nv = dp_ceil_log2(n);
  DP_REQUIRE(exp_point.size() == nv && range_point.size() == nv && error_point.size() <= nv && last.point.size() == nv, DP_ERR_SHAPE, "softmax: claim points");
  const size_t extra = nv - error_point.size();
  const Ext two_inv = ex_inv(ex_from_u64(2)), two_mult = ex_from_u64(u64(1) << extra);
  std::vector<Ext> full_error(extra, two_inv); full_error.insert(full_error.end(), error_point.begin(), error_point.end());
  const Ext alpha = ps.t->get_and_append_challenge("batching_challenge");
  size_t mk = dev.mark();
  std::vector<Ext> all;
  {
    DBuf exp_beta = dev.alloc(n, true), range_beta = dev.alloc(n, true), error_beta = dev.alloc(n, true), last_beta = dev.alloc(n, true), zbeta;
    std::vector<EqAcc> eqs = {{exp_beta, exp_point, ex_one(), false}, {range_beta, range_point, ex_one(), false}, {error_beta, full_error, ex_one(), false}, {last_beta, last.point, ex_one(), false}};
    if (zero) { zbeta = dev.alloc(n, true); eqs.push_back({zbeta, pr.logup_proofs[3].output_claims.at(0).point, ex_one(), false}); }
    DevVP vp(nv);
    Ext bc = ex_one();
    for (auto& c : ws[0].columns) { vp.add_mle_list({c, exp_beta}, bc); bc = ex_mul(bc, alpha); }
    for (auto& c : ws[1].columns) { vp.add_mle_list({c, range_beta}, bc); bc = ex_mul(bc, alpha); }
    const DBuf exp_out = ws[0].columns[1];
    if (zero) {
      for (auto& c : ws[3].columns) { vp.add_mle_list({zbeta, c}, bc); bc = ex_mul(bc, alpha); }
      std::vector<DBuf> prod; for (size_t q = 1; q < ws[3].columns.size(); q += 2) prod.push_back(ws[3].columns[q]);
      prod.push_back(exp_out);
      std::vector<DBuf> err = prod, outp = prod; err.push_back(error_beta); outp.push_back(last_beta);
      vp.add_mle_list(err, ex_mul(bc, two_mult));
      vp.add_mle_list(outp, ex_mul(bc, alpha));
    } else {
      vp.add_mle_list({exp_out, error_beta}, ex_mul(bc, two_mult));
      vp.add_mle_list({exp_out, last_beta}, ex_mul(bc, alpha));
    }
    // (tables are de-duplicated here: exp_in, exp_beta, exp_out, low, range_beta, high, [zero_beta, zero columns..], error_beta, last_beta)
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, *ps.t);
    pr.accumulation_proof = sc.proof; all = sc.finals;
  }
  dev.release(mk);
  const std::vector<Ext> sc_point = pr.accumulation_proof.point;
  Ext shifted_eval;
  {
    std::vector<int64_t> host(3 * n);
    std::copy(d.shifted_input.begin(), d.shifted_input.end(), host.begin()); std::copy(d.tril.begin(), d.tril.end(), host.begin() + n); std::copy(d.bias.begin(), d.bias.end(), host.begin() + 2 * n);
    DBuf buf = dev.alloc(3 * n, false);
    dev.upload_i64(buf, host.data());
    DBuf meq = dev.alloc(n, true);
    std::vector<EqAcc> eqs = {{meq, sc_point, ex_one(), false}};
    DevVP mv(nv);
    mv.add_mle_list({buf.slice(0, n), buf.slice(n, n), meq}, ex_one());
    mv.add_mle_list({buf.slice(2 * n, n), meq}, ex_one());
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, mv, *ps.t);
    pr.mask_proof = sc.proof; shifted_eval = sc.finals[0];
  }
  dev.release(mk);
  const DevCommit& shift_c = ws[2].commits[0];
  const std::vector<Ext> mask_point = pr.mask_proof.point;
  const std::vector<Ext> shift_point(mask_point.begin() + (mask_point.size() - shift_c.nv), mask_point.end());
  std::vector<Ext> shift_ext(d.shift.size()); for (size_t i = 0; i < d.shift.size(); i++) shift_ext[i] = ex_from_i64(d.shift[i]);
  const Ext shift_eval = host_mle_eval(shift_ext, shift_point);
  const Ext evs4[4] = {all[0], all[2], all[3], all[5]};
  for (size_t q = 0; q < 4; q++) { const DevCommit& c = q < 2 ? ws[0].commits[q] : ws[1].commits[q - 2]; ps.add_witness_claim(c, {sc_point, evs4[q]}); pr.commitments.push_back(pure_commitment(c)); pr.evaluations.push_back(evs4[q]); }
  ps.add_witness_claim(shift_c, {shift_point, shift_eval}); pr.commitments.push_back(pure_commitment(shift_c)); pr.evaluations.push_back(shift_eval);
  if (zero) for (size_t q = 0; q < ws[3].commits.size(); q++) { ps.add_witness_claim(ws[3].commits[q], {sc_point, all[7 + q]}); pr.commitments.push_back(pure_commitment(ws[3].commits[q])); pr.evaluations.push_back(all[7 + q]); }
  LayerProof lp; lp.kind = L_SOFTMAX; lp.sm = pr; ps.proofs[id] = lp;
  return {mask_point, ex_mul(ex_sub(shifted_eval, shift_eval), ex_inv(ex_from_i64(l.sm_scalar)))};
}

// ---- convolution (zkCNN FFT protocol, layers/convolution.rs:697-1080 with the helpers of iop/prover.rs:164-399)
inline DBuf upload_exts(Dev& dev, const std::vector<Ext>& v) {
  DBuf b = dev.alloc(v.size(), true);
  dev.upload(b, (const u64*)v.data());
  return b;
}
struct MatrixEval { std::vector<IOPProof> proofs; std::vector<std::vector<Ext>> claims; };
// delegate_matrix_evaluation (iop/prover.rs:164-211): the tables of every round are a few hundred elements; beta is
// built on the device, phi and the intermediate FFT-matrix table ride up in one upload per round
inline MatrixEval delegate_matrix_evaluation(Dev& dev, Transcript& t, const std::vector<std::vector<Ext>>& f_middle, const std::vector<Ext>& r1, std::vector<Ext> r2, bool is_fft) {
  std::vector<u64> omegas = phi_pow_init((unsigned)r1.size(), is_fft);
  MatrixEval me;
  size_t fm = f_middle.size();
  {  // a device that keeps the sponge to itself runs the whole chain in one launch (Dev::deleg_tail)
    Dev::DelegTailArgs da{&f_middle, r1.data(), (unsigned)r1.size(), r2.data(), omegas.data(), omegas.size(), is_fft};
    Dev::DelegTailOut dout;
    if (r2.size() == r1.size() && dev.deleg_tail(da, t.challenger(), dout)) {
      DP_REQUIRE(dout.msgs.size() == fm && dout.points.size() == fm && dout.finals.size() == fm, DP_ERR_SHAPE, "deleg_tail: one sumcheck per intermediate table expected");
      for (size_t q = 0; q < fm; q++) { IOPProof p; p.point = dout.points[q]; p.proofs = dout.msgs[q]; me.proofs.push_back(std::move(p)); me.claims.push_back(dout.finals[q]); }
      return me;
    }
  }
  for (size_t l = r1.size() - 1; l-- > 0;) {
    size_t mk = dev.mark();
    size_t len = f_middle[l].size();
    unsigned nv = dp_ceil_log2(len);
    DP_REQUIRE(r2.size() == nv + 1, DP_ERR_SHAPE, "delegation: point length");
    std::vector<Ext> both = delegation_phi(len, l, fm, r1, r2.back(), omegas, is_fft);
    both.insert(both.end(), f_middle[l].begin(), f_middle[l].end());
    DBuf pf = upload_exts(dev, both);
    DBuf beta = dev.alloc(len, true);
    DevVP vp(nv);
    vp.add_mle_list({beta, pf.slice(0, len), pf.slice(len, len)}, ex_one());
    SumcheckOut sc = sumcheck_prove_with_eq(dev, {{beta, std::vector<Ext>(r2.begin(), r2.begin() + nv), ex_one(), false}}, vp, t);
    dev.release(mk);
    r2 = sc.proof.point;
    me.proofs.push_back(sc.proof); me.claims.push_back(sc.finals);
  }
  return me;
}
struct BatchFFTProof { IOPProof proof; std::vector<Ext> claims; MatrixEval matrix_eval; std::vector<Ext> partial_evals; };
// prove_batch_fft / prove_batch_ifft (iop/prover.rs:290-398): Y(r1, r2) = sum_i F(r1, i) X(i, r2). X is a base-field
// matrix [rows][cols] on the device (rows = channels): X(., r2) is one pass of K2 (Dev::fix_high).
inline BatchFFTProof prove_batch_fft_dev(Dev& dev, Transcript& t, const std::vector<Ext>& r, const DBuf& X, size_t rows, size_t cols, bool inverse) {
  unsigned l1 = dp_ceil_log2(cols), l2 = dp_ceil_log2(rows);
  DP_REQUIRE(r.size() >= l1 + l2 && X.n == rows * cols && l1 >= 2, DP_ERR_SHAPE, "batch fft: shapes");
  std::vector<Ext> r1(r.begin(), r.begin() + l1), r2(r.begin() + l1, r.begin() + l1 + l2);
  if (inverse) DP_REQUIRE(ex_is_zero(r1[l1 - 1]), DP_ERR_ARG, "Error in randomness init batch ifft");
  std::vector<Ext> w_red(cols, ex_zero()); std::vector<std::vector<Ext>> f_middle(l1 - 1);
  phi_g_init(w_red, f_middle, r1, inverse ? ex_inv(ex_from_u64(cols)) : ex_one(), l1, inverse);
  size_t mk = dev.mark();
  DBuf fr = upload_exts(dev, w_red);
  DBuf fmx = dev.alloc(cols, true);
  dev.fix_high(fmx, X, rows, cols, r2.data());
  DevVP vp(l1);
  vp.add_mle_list({fmx, fr}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, t);
  dev.release(mk);
  BatchFFTProof out; out.proof = sc.proof; out.claims = sc.finals;
  out.matrix_eval = delegate_matrix_evaluation(dev, t, f_middle, r1, sc.proof.point, inverse);
  return out;
}
// Convolution::prove_batch_fft_weights (convolution.rs:358-443)
inline BatchFFTProof prove_batch_fft_weights(ProverState& ps, size_t id, const LayerSpec& l, const std::vector<Ext>& r) {
  Dev& dev = *ps.dev; Transcript& t = *ps.t;
  size_t padded_rows = 2 * l.nw * l.nw, fsz = l.real_nw * l.real_nw;
  unsigned l1 = dp_ceil_log2(padded_rows);
  std::vector<Ext> r1(r.begin(), r.begin() + l1), r2(r.begin() + l1, r.end());
  DP_REQUIRE(r2.size() == dp_ceil_log2(l.kw * l.kx), DP_ERR_SHAPE, "fft weights: point length");
  std::vector<Ext> w_red(padded_rows, ex_zero()); std::vector<std::vector<Ext>> f_middle(l1 - 1);
  phi_g_init(w_red, f_middle, r1, ex_one(), l1, false);
  size_t mk = dev.mark();
  // w1_reduced[k] = sum_{i,j} beta(r2)[i*kx + j] * filter[i][j][k]: K2 on the committed filter table
  DBuf red = dev.alloc(fsz, true);
  dev.fix_high(red, ps.ctx->weights_dev.at(id), l.kw * l.kx, fsz, r2.data());
  BatchFFTProof out; out.partial_evals.resize(fsz);
  dev.download(red, (u64*)out.partial_evals.data());
  std::vector<Ext> padded(padded_rows, ex_zero());  // index_wf (convolution.rs:1535-1550)
  for (size_t a = 0; a < l.real_nw; a++) for (size_t b = 0; b < l.real_nw; b++) padded[a * l.nw + b] = out.partial_evals[a * l.real_nw + b];
  std::vector<Ext> both = padded; both.insert(both.end(), w_red.begin(), w_red.end());
  DBuf pf = upload_exts(dev, both);
  DevVP vp(l1);
  vp.add_mle_list({pf.slice(0, padded_rows), pf.slice(padded_rows, padded_rows)}, ex_one());
  SumcheckOut sc = sumcheck_prove(dev, vp, t);
  dev.release(mk);
  out.proof = sc.proof; out.claims = sc.finals;
  out.matrix_eval = delegate_matrix_evaluation(dev, t, f_middle, r1, sc.proof.point, false);
  return out;
}
inline Claim prove_conv(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last_in, const ConvTrace& ct) {
  Dev& dev = *ps.dev; Transcript& t = *ps.t;
  const Context::ConvDev& cd = ps.ctx->conv_dev.at(id);
  const auto& comms = ps.ctx->model_comms.at(id);
  size_t fs = l.filter_size(), N = 2 * fs;
  unsigned lfs = dp_ceil_log2(fs), lkw = dp_ceil_log2(l.kw), l2n = lfs + 1;
  DP_REQUIRE(last_in.point.size() == lfs + lkw, DP_ERR_SHAPE, "conv: claim point length");
  size_t mk = dev.mark();
  // the tables of this inference: one upload for the three base-field matrices
  DBuf big = dev.alloc(ct.input_pad.size() + ct.input_fft.size() + ct.prod.size(), false);
  { std::vector<u64> flat; flat.reserve(big.n); flat.insert(flat.end(), ct.input_pad.begin(), ct.input_pad.end()); flat.insert(flat.end(), ct.input_fft.begin(), ct.input_fft.end()); flat.insert(flat.end(), ct.prod.begin(), ct.prod.end()); dev.upload(big, flat.data()); }
  DBuf input_pad = big.slice(0, ct.input_pad.size()), input_fft = big.slice(ct.input_pad.size(), ct.input_fft.size()), prod = big.slice(ct.input_pad.size() + ct.input_fft.size(), ct.prod.size());
  // 1. garbage clearing: hadamard::prove (hadamard.rs:83-130) on (conv output after bias) o (0/1 clearing tensor)
  HadamardProof clearing_proof;
  {
    size_t mk2 = dev.mark();
    DBuf v1 = dev.alloc(ct.output_as_element.size(), false);
    dev.upload_i64(v1, ct.output_as_element.data());
    DBuf beta = dev.alloc(v1.n, true);
    DevVP vp((unsigned)last_in.point.size());
    vp.add_mle_list({v1, cd.clearing, beta}, ex_one());
    SumcheckOut sc = sumcheck_prove_with_eq(dev, {{beta, last_in.point, ex_one(), false}}, vp, t);
    clearing_proof.sumcheck = sc.proof; clearing_proof.individual_claim = {sc.finals[0], sc.finals[1]};
    dev.release(mk2);
  }
  Claim last{clearing_proof.sumcheck.point, clearing_proof.individual_claim[0]};
  std::vector<Ext> r(last.point.size() + 1, ex_zero()), bias_point(lkw, ex_zero());
  for (unsigned i = 0; i < lfs; i++) r[i] = ex_sub(ex_one(), last.point[i]);
  for (unsigned i = 0; i < lkw; i++) { r[i + lfs + 1] = last.point[i + lfs]; bias_point[i] = last.point[i + lfs]; }
  Ext bias_eval = ex_zero();
  dev.mle_eval_batch(&comms.at("ConvBias").evals, 1, bias_point.data(), lkw, &bias_eval);
  // 2. Y = iFFT(prod)
  BatchFFTProof ifft = prove_batch_fft_dev(dev, t, r, prod, l.kw, N, true);
  DP_REQUIRE(ifft.proof.point.size() == lfs + 1, DP_ERR_SHAPE, "Error in ifft sumcheck");
  std::vector<Ext> r_ifft = ifft.proof.point;
  for (size_t i = l2n; i < r.size(); i++) r_ifft.push_back(r[i]);
  std::vector<Ext> r1(r_ifft.begin() + l2n, r_ifft.end()), r2(r_ifft.begin(), r_ifft.begin() + l2n);
  // 3. prod = sum_j FFT(x_j) o FFT(w_ij): cubic sumcheck over (aggregated filter FFT, input FFT, beta). The aggregated
  //    filter sum_i beta1[i] w[i][j] is transformed by the reference (kx extension-field FFTs); the transform is linear,
  //    so it equals sum_i beta1[i] FFT(w[i][j]) — one K2 pass over the kernel FFTs kept from setup.
  IOPProof hadamard_proof; std::vector<Ext> hadamard_claims;
  {
    size_t mk2 = dev.mark();
    DBuf f1 = dev.alloc(l.kx * N, true), f3 = dev.alloc(l.kx * N, true);
    dev.fix_high(f1, cd.wfft, l.kw, l.kx * N, r1.data());
    dev.eq_table_tiled(f3, r2.data(), l2n);
    DevVP vp(dp_ceil_log2(l.kx * N));
    vp.add_mle_list({f1, input_fft, f3}, ex_one());
    SumcheckOut sc = sumcheck_prove(dev, vp, t);
    hadamard_proof = sc.proof; hadamard_claims = sc.finals;
    dev.release(mk2);
  }
  std::vector<Ext> point = hadamard_proof.point; point.insert(point.end(), r1.begin(), r1.end());
  // 4. FFT of the input and of the weights
  BatchFFTProof fftp = prove_batch_fft_dev(dev, t, hadamard_proof.point, input_pad, l.kx, N, false);
  BatchFFTProof wp = prove_batch_fft_weights(ps, id, l, point);
  std::vector<Ext> weights_rand = t.read_challenges(dp_ceil_log2(l.real_nw * l.real_nw));
  Claim bias_claim{bias_point, bias_eval};
  Claim filter_claim; filter_claim.point = weights_rand; filter_claim.point.insert(filter_claim.point.end(), point.begin() + l2n, point.end());
  filter_claim.eval = host_mle_eval(wp.partial_evals, weights_rand);
  ps.add_witness_claim(comms.at("ConvBias"), bias_claim);  // add_common_claims: BTreeMap order "ConvBias" < "ConvFilter"
  ps.add_witness_claim(comms.at("ConvFilter"), filter_claim);
  LayerProof lp; lp.kind = L_CONV; ConvProof& cp = lp.conv;
  cp.fft_proof = fftp.proof; cp.fft_claims = fftp.claims; cp.fft_proof_weights = wp.proof; cp.ifft_proof = ifft.proof;
  cp.fft_delegation_proof = fftp.matrix_eval.proofs; cp.fft_delegation_proof_weights = wp.matrix_eval.proofs; cp.ifft_delegation_proof = ifft.matrix_eval.proofs;
  cp.hadamard_proof = hadamard_proof; cp.ifft_claims = ifft.claims; cp.fft_weight_claims = wp.claims;
  cp.fft_delegation_claims = fftp.matrix_eval.claims; cp.fft_delegation_weights_claims = wp.matrix_eval.claims; cp.ifft_delegation_claims = ifft.matrix_eval.claims;
  cp.hadamard_clams = hadamard_claims; cp.bias_claim = bias_eval; cp.partial_evals = wp.partial_evals; cp.clearing_proof = clearing_proof;
  ps.proofs[id] = lp;
  dev.release(mk);
  std::vector<Ext> input_point = fftp.proof.point;
  Ext v = ex_inv(ex_sub(ex_one(), input_point.back())); input_point.pop_back();
  for (auto& ip : input_point) ip = ex_sub(ex_one(), ip);
  Claim fin; fin.point = input_point;
  fin.point.insert(fin.point.end(), hadamard_proof.point.begin() + l2n, hadamard_proof.point.end());
  fin.eval = ex_mul(fftp.claims[0], v);
  return fin;
}
// Pooling::prove_pooling (pooling.rs:342-520)
inline Claim prove_pooling(ProverState& ps, size_t id, const LayerSpec& l, const Claim& last) {
  Dev& dev = *ps.dev; Transcript& t = *ps.t;
  std::vector<LogUpWitness>& ws = ps.lookup_witness.at(id);
  DP_REQUIRE(ws.size() == 1 && ws[0].columns.size() == 4 && ws[0].extra_columns.size() == 1 && ws[0].commits.size() == 5, DP_ERR_ARG, "pooling: lookup witness shape");
  LogUpWitness& w = ws[0];
  LogUpProof lproof = logup_batch_prove(dev, ps.logup_input(w), t);
  size_t n = w.columns[0].n; unsigned nv = dp_ceil_log2(n);
  DP_REQUIRE(last.point.size() == nv, DP_ERR_SHAPE, "pooling: claim point length");
  size_t mk = dev.mark();
  Ext batch = t.get_and_append_challenge("batch_pooling");
  DBuf beta = dev.alloc(n, true), last_beta = dev.alloc(n, true);
  std::vector<EqAcc> eqs = {{beta, lproof.output_claims[0].point, ex_one(), false}, {last_beta, last.point, ex_one(), false}};
  DevVP vp(nv);
  std::vector<DBuf> all = w.columns; all.push_back(beta);
  vp.add_mle_list(all, ex_one());  // zero check: prod_i (out - in_i) * eq
  Ext comb = batch;
  for (auto& d : w.columns) { vp.add_mle_list({d, beta}, comb); comb = ex_mul(comb, batch); }
  vp.add_mle_list({w.extra_columns[0], last_beta}, comb);  // the output (committed base column == trace output as field elements)
  SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, t);  // (degree 5: fused devices decline, the tables are then built one by one)
  dev.release(mk);
  const std::vector<Ext>& evals = sc.finals;
  const size_t ks = 4;
  Ext output_eval = evals[ks + 1];
  LayerProof lp; lp.kind = L_MAXPOOL; PoolingProof& pp = lp.pool;
  pp.sumcheck = sc.proof; pp.lookup = lproof;
  for (size_t i = 0; i <= ks; i++) {
    pp.commitments.push_back(pure_commitment(w.commits[i]));
    ps.add_witness_claim(w.commits[i], {sc.proof.point, i < ks ? evals[i] : output_eval});
  }
  unsigned row_log = dp_ceil_log2(l.pin[2]);
  Ext r1 = t.get_and_append_challenge("input_batching"), r2 = r1;  // `[challenge; 2]`: ONE challenge used twice (pooling.rs:459-462)
  Ext om1 = ex_sub(ex_one(), r1), om2 = ex_sub(ex_one(), r2);
  Ext mult[4] = {ex_mul(om1, om2), ex_mul(om1, r2), ex_mul(r1, om2), ex_mul(r1, r2)};
  Ext zc = ex_zero();
  for (size_t i = 0; i < ks; i++) zc = ex_add(zc, ex_mul(mult[i], ex_sub(output_eval, evals[i])));
  Claim next; next.point.push_back(r1);
  next.point.insert(next.point.end(), sc.proof.point.begin(), sc.proof.point.begin() + (row_log - 1));
  next.point.push_back(r2);
  next.point.insert(next.point.end(), sc.proof.point.begin() + (row_log - 1), sc.proof.point.end());
  next.eval = zc;
  pp.zerocheck_evals.assign(evals.begin(), evals.begin() + ks); pp.zerocheck_evals.push_back(output_eval);
  pp.variable_gap = row_log - 1;
  ps.proofs[id] = lp;
  return next;
}

// Logits::prove, Argmax (layers/transformer/logits.rs:306-472). The lookup shows max[i] - x[i][j] in 0..255 for every entry (the maximum bounds its
// row); what remains is that the maximum is ATTAINED at the claimed index: with M[i][j] = max[i] * [j == idx[i]], a first sumcheck over the columns
// turns the committed maxima at the row point into M at (s1 | row point), and the second one proves M = input o onehot there, batched (by a challenge
// drawn after the lookup's claim is absorbed) with the lookup's own claim on the input. The claim `last` that prove() drew on the output tensor is
// drawn and NOT used, as in the reference (`_last_claims`): the verifier evaluates the one-hot matrix of io.output itself.
// The second sumcheck lists `input` once per product in the reference (two Arcs of one polynomial): here the table is shared — the round messages are
// sums over the same values and final evaluation [0] is the input's either way.
inline Claim prove_logits(ProverState& ps, size_t id, const LayerSpec& l, const std::vector<int64_t>& output, const std::vector<int64_t>& maxima) {
  Dev& dev = *ps.dev; Transcript& t = *ps.t;
  std::vector<LogUpWitness>& ws = ps.lookup_witness.at(id);
  DP_REQUIRE(ws.size() == 1 && ws[0].columns.size() == 1 && ws[0].commits.size() == 1, DP_ERR_ARG, "logits: lookup witness shape");
  const ProverState::LogitsDev& ld = ps.logits_dev.at(id);
  const size_t rows = l.nrows, K = l.ncols, n = rows * K;
  const unsigned nvr = dp_ceil_log2(rows), nvk = dp_ceil_log2(K), nv = nvr + nvk;
  DP_REQUIRE(output.size() == rows && maxima.size() == rows && ld.in.n == n, DP_ERR_SHAPE, "logits: shapes");
  LogitsProof pr;
  pr.logup_proof = logup_batch_prove(dev, ps.logup_input(ws[0]), t);
  const Claim diff_claim = pr.logup_proof.output_claims.at(0);
  DP_REQUIRE(diff_claim.point.size() == nv, DP_ERR_SHAPE, "logits: lookup claim point");
  const std::vector<Ext> row_point(diff_claim.point.begin() + nvk, diff_claim.point.end());  // split_claim_point: the rows are the most significant variables
  std::vector<Ext> mx(rows); for (size_t i = 0; i < rows; i++) mx[i] = ex_from_i64(maxima[i]);
  pr.max_eval = host_mle_eval(mx, row_point);
  pr.max_commitment = pure_commitment(ws[0].commits[0]);
  ps.add_witness_claim(ws[0].commits[0], {row_point, pr.max_eval});
  const Claim input_claim{diff_claim.point, ex_sub(pr.max_eval, diff_claim.eval)};
  size_t mk = dev.mark();
  {  // the sparse matrix M with its row variables fixed at row_point: `rows` terms, made on the host
    const std::vector<Ext> beta = host_eq_table(row_point);
    std::vector<Ext> reduced(K, ex_zero());
    for (size_t i = 0; i < rows; i++) { DP_REQUIRE(output[i] >= 0 && (size_t)output[i] < K, DP_ERR_SHAPE, "logits: index outside the row"); reduced[(size_t)output[i]] = ex_add(reduced[(size_t)output[i]], ex_mul(beta[i], mx[i])); }
    DevVP vp(nvk);
    vp.add_mle_list({upload_exts(dev, reduced), upload_exts(dev, std::vector<Ext>(K, ex_one()))}, ex_one());
    SumcheckOut sc = sumcheck_prove(dev, vp, t);
    pr.sumcheck_proof = sc.proof; pr.max_mat_eval = sc.finals[0];
  }
  dev.release(mk);
  std::vector<Ext> claim_point = pr.sumcheck_proof.point; claim_point.insert(claim_point.end(), row_point.begin(), row_point.end());
  t.append_exts(input_claim.point); t.append_ext(input_claim.eval);  // squeeze_challenge (logits.rs:147-156)
  const Ext challenge = t.read_challenge();
  {
    DBuf beta = dev.alloc(n, true), input_eq = dev.alloc(n, true);
    std::vector<EqAcc> eqs = {{beta, claim_point, ex_one(), false}, {input_eq, input_claim.point, ex_one(), false}};
    DevVP vp(nv);
    vp.add_mle_list({ld.in, ld.onehot, beta}, ex_one());
    vp.add_mle_list({input_eq, ld.in}, challenge);
    SumcheckOut sc = sumcheck_prove_with_eq(dev, eqs, vp, t);
    pr.hadamard_proof = sc.proof; pr.input_eval = sc.finals[0];
  }
  dev.release(mk);
  LayerProof lp; lp.kind = L_LOGITS; lp.logits = pr; ps.proofs[id] = lp;
  return {pr.hadamard_proof.point, pr.input_eval};
}

// Mha::prove (mha.rs:633-704): final_mul on (probabilities, V), the softmax, qk on (Q, K); the claims on Q, K, V in this order
inline std::vector<Claim> prove_mha(ProverState& ps, size_t id, const LayerSpec& l, const Claim& cur, const MhaTrace& d, const std::vector<int64_t>& q, const std::vector<int64_t>& k, const std::vector<int64_t>& v) {
  LayerProof lp; lp.kind = L_MHA;
  std::vector<Claim> fm = prove_concat_matmul(ps, id, mha_final_spec(l), cur, d.softmax_out, v);
  lp.mha_final = ps.proofs.at(id).cmm;
  const Claim sc = prove_softmax(ps, id, mha_softmax_spec(l), fm[0]);
  lp.sm = ps.proofs.at(id).sm;
  std::vector<Claim> qk = prove_concat_matmul(ps, id, mha_qk_spec(l), sc, q, k);
  lp.mha_qk = ps.proofs.at(id).cmm;
  ps.proofs[id] = lp;
  return {qk[0], qk[1], fm[1]};
}

// Prover::prove(trace). `tr` comes from run_model (inference is not part of proving time in the reference either).
// `dev` may be any device context on the GPU that holds `ctx` (the model commitments are only read), so several proofs
// can be in flight at once, each on its own stream/arena (dp_model_prove_batch).
// `prepared`: the host half of the witness generation of THIS trace, made ahead of time (witness_host; consumed)
inline Proof prove(Context& ctx, Dev& dev, const Trace& tr, Transcript& t, WitnessHost* prepared = nullptr) {
  PhaseTimer pt;
  sc_stats() = ScStats();
  size_t mk = dev.mark();
  ProverState ps; ps.ctx = &ctx; ps.dev = &dev; ps.t = &t;
  for (auto& kv : ctx.model_comms) for (auto& pc : kv.second) t.append_digest(pc.second.tree.root);
  instantiate_witness_ctx(ps, tr, prepared);
  pt.lap("witness columns + commits");
  // a claim per output tensor (iop/prover.rs:419-435); then the nodes in proving order, each node receiving the claims its readers made on
  // its outputs and making one claim per input (claims_for_node, provable/mod.rs:235-270). A chain: one claim walking from the last node back.
  const ModelSpec& model = ctx.model;
  std::vector<Claim> on_outputs;
  for (const Edge& e : output_edges(model)) {
    const std::vector<int64_t>& out = tr.tensor(e.from, e.slot);
    Claim c; c.point = t.read_challenges(dp_ceil_log2(out.size()));
    std::vector<Ext> ov(out.size()); for (size_t i = 0; i < out.size(); i++) ov[i] = ex_from_i64(out[i]);
    c.eval = host_mle_eval(ov, c.point);
    on_outputs.push_back(std::move(c));
  }
  const bool chain = model.outputs.empty() && std::all_of(model.layers.begin(), model.layers.end(), [](const LayerSpec& l) { return l.inputs.empty(); });
  std::map<size_t, std::vector<Claim>> made;  // node -> the claims it made on its inputs
  std::vector<size_t> order;
  if (chain) for (size_t id = model.layers.size(); id-- > 0;) order.push_back(id); else order = proving_order(model);
  for (size_t id : order) {
    const LayerSpec& l = model.layers[id];
    std::vector<Claim> got;
    for (size_t j = 0; j < out_degree(l); j++) {
      Reader_ r; if (chain) { r.to = id + 1 < model.layers.size() ? (int)id + 1 : -1; r.port = 0; } else r = reader_of(model, (int)id, (int)j);
      got.push_back(r.to < 0 ? on_outputs.at((size_t)r.port) : made.at((size_t)r.to).at((size_t)r.port));
    }
    Claim cur = got[0];
    if (l.kind == L_MATMUL2) { made[id] = prove_matmul2(ps, id, l, cur, tr.in[id], tr.in2[id]); continue; }
    if (l.kind == L_ADD2) { made[id] = prove_add2(ps, id, cur, tr.in[id], tr.in2[id]); continue; }
    if (l.kind == L_CONCAT_MATMUL) { made[id] = prove_concat_matmul(ps, id, l, cur, tr.in[id], tr.in2[id]); continue; }
    if (l.kind == L_QKV) { made[id] = prove_qkv(ps, id, l, got, tr.in[id]); continue; }
    if (l.kind == L_MHA) { made[id] = prove_mha(ps, id, l, cur, tr.mha.at(id), tr.in[id], tr.in2[id], tr.in3[id]); continue; }
    if (l.kind == L_DENSE) cur = prove_dense(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_MATMUL) cur = prove_matmul(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_ADD) cur = prove_add(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_EMBED) cur = prove_embeddings(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_POSITIONAL) cur = prove_positional(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_REQUANT) cur = prove_requant(ps, id, l, cur);
    else if (l.kind == L_RELU) cur = prove_relu(ps, id, cur, tr.out[id]);
    else if (l.kind == L_GELU) cur = prove_relu(ps, id, cur, tr.out[id], l.fixed_point_multiplier);
    else if (l.kind == L_LAYERNORM) cur = prove_layernorm(ps, id, l, cur, tr.in[id]);
    else if (l.kind == L_SOFTMAX) cur = prove_softmax(ps, id, l, cur);
    else if (l.kind == L_CONV) cur = prove_conv(ps, id, l, cur, tr.conv.at(id));
    else if (l.kind == L_MAXPOOL) cur = prove_pooling(ps, id, l, cur);
    else if (l.kind == L_LOGITS) cur = prove_logits(ps, id, l, tr.out[id], tr.argmax_max.at(id));
    // L_FLATTEN is not provable: the claim passes through unchanged (iop/prover.rs:449-456)
    if (pt.on) { char b[64]; snprintf(b, sizeof b, "layer %zu (kind %d)", id, l.kind); pt.lap(b); }
    made[id] = {cur};
    if (chain && id + 1 < model.layers.size()) made.erase(id + 1);
  }
  Proof proof;
  for (auto& tw : ps.table_witness) {
    LogUpProof tp = logup_batch_prove(dev, ps.logup_input(tw), t);
    ps.add_witness_claim(tw.commits[0], tp.output_claims[0]);
    // table_claims (lookup/context.rs:548-563): the claim on a committed table column (the last one) goes to the opening as well
    if (tw.table_type.committed_column()) ps.add_witness_claim(ctx.table_comms.at(tw.table_type), tp.output_claims.back());
    proof.table_proofs.push_back({pure_commitment(tw.commits[0]), tp});
  }
  pt.lap("table proofs");
  for (auto& c : ps.trivial_claims) proof.trivial_proofs.push_back(pcs_open_trivial(dev, c.comm));
  pt.lap("trivial openings");
  std::vector<OpenClaim> oc;
  for (auto& c : ps.claims) oc.push_back({&c.comm, c.claim.point, c.claim.eval});
  proof.batch_proof = pcs_batch_open(dev, ctx.full_log, oc, t);
  pt.lap("batch_open");
  if (pt.on) fprintf(stderr, "[dp timing] sumcheck rounds %zu: device wait %.3f ms, host transcript+algebra %.3f ms\n", sc_stats().rounds, sc_stats().dev_ms, sc_stats().host_ms);
  proof.steps = ps.proofs;
  dev.release(mk);
  return proof;
}

inline Proof prove(Context& ctx, const Trace& tr, Transcript& t) { return prove(ctx, *ctx.dev, tr, t); }

}  // namespace dp

#include "zkml_verify.h"  // the verifier
