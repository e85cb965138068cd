// Batched quantised inference on the device (dp_model_infer, include/deep_prove_hip_infer.h): Model::run for many independent inputs.
// The host flattens a ModelSpec into an InferProgram (infer_plan below: tensors, constants, one op per launch) once per model; hip_infer_run
// (infer_kernels.inc, compiled into hip_dev.hip) executes it for a batch: activations are [batch][tensor], one launch serves the whole batch.
// Which products take the i8 MFMA is decided here, statically: the weights within -128..127, K * 128 * 128 < 2^31 and the input produced by
// a Requant (through ReLU / MaxPool / Flatten) or a model input the host has range-checked at upload. Everything else is 64-bit multiply-add
// with the host's wrap-around.
// INFER_ALL_KINDS (dp_model_infer_ex, DP_INFER_ALL_KINDS) adds LayerNorm, Softmax, Mha and GELU. Their tables are constants of the model, made
// here by the functions the prover uses (gelu_lut, inv_sqrt_lut, softmax_lut); on the device the three layers are integer work. The one float
// computation that depends on the data, the shift of a Softmax row, stays on the host: at an IO_SOFTMAX hip_infer_run downloads the input of
// the chunk, calls InferProgram::shifts (infer_softmax_shifts below: softmax_row_shift of zkml.h, the function softmax_op calls) and uploads
// one shift per row. An Mha node is three ops: the product Q K^T, the Softmax, the product with V.
// Data the host would refuse: one status word per sample of the chunk holds the class (INFER_BAD_*) of the first op that refused the sample; the
// shift step works sample by sample and never reads the rows of a sample that is already refused. The two kinds of call differ only in what
// hip_infer_run does with the words: with `reasons` (dp_model_infer_checked) it refuses inputs one by one, without (dp_model_infer_ex) the
// first chunk that holds a refused sample ends the call with the host's message for its class. Program and constants are the same for both.
// Tap mode (dp_model_infer_trace; `rows` of hip_infer_run): the trace row of every input (trace_row.h) comes back with its outputs. The planner
// records for every entry of trace_layout the tensor that holds it (InferProgram::taps); after the last op of a chunk ONE launch of
// k_infer_tap_pack gathers them into a sample-major image [sample][row_words], which travels to the host in one copy beside the outputs.
#pragma once
#include "dev.h"
#ifdef DP_INFER_PLANNER
#include "trace_row.h"
#endif
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <thread>
#include <vector>

namespace dp {

enum InferQ { IQ_NO = 0, IQ_YES = 1, IQ_IF_INPUTS = 2 };  // every value of the tensor within -128..127: never / always / iff the model inputs of the call are
struct InferTensor { size_t len = 0; int q = IQ_NO; };
// a constant of the model. h64 points into the ModelSpec (it lives as long as the dp_model); w8 = the same matrix as int8, transposed to [N][K]
// (both operands of k_infer_gemm_i8 are read along K), empty when a weight does not fit. Uploaded at the first launch that reads it.
// A table (GELU, inverse square root, exponential) is made by the planner and lives in `own`.
struct InferConst {
  const int64_t* h64 = nullptr; size_t n = 0; std::vector<int8_t> w8; std::vector<int64_t> own;
  const int64_t* data() const { return own.empty() ? h64 : own.data(); }
};
constexpr uint32_t INFER_ALL_KINDS = 1;  // (DP_INFER_ALL_KINDS of the public header)
// the status of one input (DP_INFER_OK, DP_INFER_BAD_* of the public header): which kind of node refused it first
constexpr uint32_t INFER_OK = 0, INFER_BAD_REQUANT = 1, INFER_BAD_TOKEN = 2, INFER_BAD_GELU = 3, INFER_BAD_LAYERNORM = 4, INFER_BAD_SOFTMAX = 5;
// internal only: a LayerNorm's inverse square root input leaves its table (the host has a message of its own for it; INFER_BAD_LAYERNORM in `reasons`)
constexpr uint32_t INFER_BAD_LAYERNORM_TABLE = 6;
enum InferOpKind { IO_GEMM = 0, IO_GEMM2, IO_REQUANT, IO_RELU, IO_ADDC, IO_ADD2, IO_EMBED, IO_MAXPOOL, IO_CONV, IO_GELU, IO_LAYERNORM, IO_SOFTMAX, IO_ARGMAX, IO_KINDS };
// out[b][c*sOc + r*sOr + n*sOn] = sum_m A[b][c*sAc + r*sAr + m*sAm] * B[(B a tensor: b)][c*sBc + m*sBm + n*sBn] (+ bias[n])
struct InferGemmShape { size_t C = 1, R = 0, K = 0, N = 0; size_t sAc = 0, sAr = 0, sAm = 0, sBc = 0, sBm = 0, sBn = 0, sOc = 0, sOr = 0, sOn = 0; };
struct InferOp {
  int kind = IO_GEMM, node = 0;
  int in0 = -1, in1 = -1, out = -1;  // tensors
  int w = -1, bias = -1;             // constants (IO_LAYERNORM: gamma, beta)
  int table = -1;                    // constant: the table of IO_GELU (rows -max .. max - 1), IO_LAYERNORM (rows -2^14 .. 2^14 - 1), IO_SOFTMAX (2^table bits rows)
  InferGemmShape g;                  // IO_GEMM (B = constant w; the i8 form when in0 is q and w has an int8 copy), IO_GEMM2 (B = tensor in1)
  int64_t left = 1, right = 1;       // IO_ADDC: left * x + right * w[i]; IO_ADD2: left * a + right * b; IO_REQUANT, IO_GELU, IO_LAYERNORM: left = multiplier; IO_SOFTMAX: left = scalar, right = bkm
  unsigned shift = 0, bits = 0;      // IO_REQUANT; IO_LAYERNORM: shift = range_check_bits; IO_SOFTMAX: bits = table bits
  // IO_EMBED: vocabulary, embedding size; IO_MAXPOOL: c, h, w; IO_CONV: kw, kx, real_nw, nw, unp_out[3]; IO_GELU: max; IO_LAYERNORM: row length, N;
  // IO_SOFTMAX: C, R, K, zero chunks, zero vars (in1 = the shift buffer of the chunk, a tensor of C * R words per sample); IO_ARGMAX: rows, K
  size_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
struct InferTap { int tensor = -1; size_t len = 0, off = 0; };  // words off .. off + len of a trace row are tensor `tensor`
struct InferProgram {
  size_t input_len = 0, output_len = 0;
  std::vector<InferTap> taps; size_t row_words = 0;  // one tap per entry of trace_layout(model), in its order
  std::vector<InferTensor> tensors;
  std::vector<int> inputs, outputs;  // tensor ids of the model's input / output tensors, in the order they are concatenated
  std::vector<InferConst> consts;
  std::vector<InferOp> ops;
  // the shift step of an IO_SOFTMAX: x = its input for nb samples; shifts: nb x C * R words; status: nb words. A sample whose word is set is not
  // read and gets zero shifts, a sample with an input beyond 2^24 gets INFER_BAD_SOFTMAX and zero shifts
  std::function<void(const InferOp& o, const int64_t* x, size_t nb, int64_t* shifts, uint32_t* status)> shifts;
};
struct InferDeviceState;  // the constants on the device (made at the first call, freed with the model)
InferDeviceState* hip_infer_state_new(int device);
void hip_infer_state_free(InferDeviceState* s);
// inputs: ninputs x p.input_len words; outputs: ninputs x out_stride words (the first p.output_len of each row are written). Throws DpError.
// reasons (ninputs words) not null: checked mode — bad data refuses its input (reasons[i] = INFER_BAD_*, the output row zeros), not the call, and
// every chunk is processed. Null: the first chunk with a refused sample ends the call (DP_ERR_ARG, the host's message), none of its rows is written.
// rows not null: tap mode — row i of `rows` (ninputs x row_stride words, the first p.row_words of each written) is the trace row of input i; zeros
// for an input refused in checked mode.
void hip_infer_run(Dev* d, const InferProgram& p, InferDeviceState* st, const int64_t* inputs, size_t ninputs, int64_t* outputs, size_t out_stride, double* wall_ms, uint32_t* reasons = nullptr,
                   int64_t* rows = nullptr, size_t row_stride = 0);

// ---- Decode (dp_model_decode, include/deep_prove_hip_decode.h): greedy generation for a model that maps `seq` tokens to the `seq` tokens its
// Logits node chose. The state of one prompt is (tokens[seq], length, stop); limit = prompt_len + max_new (never above seq). One step: test
// the limits, infer the whole padded window, take out[length - 1]; the end-of-sequence token stops the prompt and is NOT appended, any other
// token is. decode_step below is that step for one prompt, given the inference of its tokens; the host loop (dp_model_decode_host) and
// k_infer_next_token (infer_kernels.inc) both call it.
constexpr uint32_t DECODE_STOP_EOS = 1, DECODE_STOP_WINDOW = 2, DECODE_STOP_MAX_NEW = 3, DECODE_STOP_REFUSED = 4;  // (DP_DECODE_STOP_* of the public header; 0: still decoding)
// the limits alone (steps 1 and 2): what stops a prompt of this length before any inference, or 0. (length 0 is refused by every caller; it
// stops here so that no index is ever formed from it)
DP_HD uint32_t decode_limit(uint32_t length, uint32_t limit, uint32_t seq) {
  return length == 0 || length >= seq ? DECODE_STOP_WINDOW : length >= limit ? DECODE_STOP_MAX_NEW : 0;
}
// One step of one prompt. status: the status word of the inference of `tokens` (INFER_OK or a class: the prompt is refused as it stands);
// out: the Logits row of that inference, read at length - 1 only, and only when no limit stops the prompt first (a caller that knows
// decode_limit() != 0 need not infer: out is not read then). The token goes to tokens[length] once length < seq is established, and the limits
// are tested again on the new length: that is the head of the next step, taken here so that a prompt never costs an inference it cannot use.
// A prompt whose stop is set is left alone.
DP_HD void decode_step(uint32_t& length, uint32_t& stop, uint32_t limit, uint32_t seq, int64_t eos, uint32_t status, const int64_t* out, int64_t* tokens) {
  if (stop) return;
  if (status) { stop = DECODE_STOP_REFUSED; return; }
  if ((stop = decode_limit(length, limit, seq))) return;
  const int64_t t = out[length - 1];  // (1 <= length < seq)
  if (eos >= 0 && t == eos) { stop = DECODE_STOP_EOS; return; }
  tokens[length] = t;
  length += 1;
  stop = decode_limit(length, limit, seq);
}
// prompts: nprompts x seq words (row i read up to prompt_len[i]); tokens, outputs (nullable): nprompts x seq; length, stop, reasons: nprompts
// words. The caller has checked that p is decodable (seq = p.input_len = p.output_len, one input, one output, no IO_SOFTMAX), 1 <= prompt_len
// <= seq and pad. Throws DpError.
void hip_infer_decode(Dev* d, const InferProgram& p, InferDeviceState* st, const int64_t* prompts, const uint32_t* prompt_len, size_t nprompts, uint32_t max_new, int64_t eos, int64_t pad,
                      int64_t* tokens, uint32_t* length, uint32_t* stop, uint32_t* reasons, int64_t* outputs, double* wall_ms);

#ifdef DP_INFER_PLANNER  // (capi.cpp, after zkml.h)
// Whether dp_model_decode can drive the model: the length of its window, or DP_ERR_ARG with the condition that fails. vocab: the Embeddings vocabulary
inline size_t decode_window(const ModelSpec& m, size_t* vocab) {
  DP_REQUIRE(input_tensor_lens(m).size() == 1, DP_ERR_ARG, "dp_model_decode: the model must have exactly one input tensor (it has " + std::to_string(input_tensor_lens(m).size()) + ")");
  const size_t seq = m.input_len;
  const std::vector<Edge> e0 = m.layers.empty() ? std::vector<Edge>() : edges_in(m, 0);
  DP_REQUIRE(!m.layers.empty() && m.layers[0].kind == L_EMBED && e0.size() == 1 && e0[0].from < 0 && e0[0].slot == 0, DP_ERR_ARG, "dp_model_decode: node 0 must be an Embeddings layer that reads the input tokens");
  const std::vector<Edge> outs = output_edges(m);
  DP_REQUIRE(outs.size() == 1 && outs[0].from >= 0 && m.layers[(size_t)outs[0].from].kind == L_LOGITS, DP_ERR_ARG, "dp_model_decode: the only output of the model must be a Logits node");
  const LayerSpec& lg = m.layers[(size_t)outs[0].from];
  DP_REQUIRE(lg.nrows == seq, DP_ERR_ARG, "dp_model_decode: the Logits node must choose one token per input position (rows " + std::to_string(lg.nrows) + ", window " + std::to_string(seq) + ")");
  DP_REQUIRE(lg.ncols <= m.layers[0].nrows, DP_ERR_ARG, "dp_model_decode: the Logits node chooses among " + std::to_string(lg.ncols) + " tokens, the Embeddings vocabulary has " + std::to_string(m.layers[0].nrows));
  for (size_t id = 0; id < m.layers.size(); id++)
    DP_REQUIRE(m.layers[id].kind != L_SOFTMAX && m.layers[id].kind != L_MHA, DP_ERR_ARG, "dp_model_decode: node " + std::to_string(id) + " holds a Softmax, whose row shifts need a host step in every decode step: not decodable yet");
  if (vocab) *vocab = m.layers[0].nrows;
  return seq;
}
inline const char* infer_kind_name(int k) {
  static const char* names[] = {"Dense", "Requant", "ReLU", "Conv", "MaxPool", "Flatten", "MatMul", "Add", "Embeddings", "Positional", "MatMul2", "Add2", "ConcatMatMul", "QKV", "LayerNorm", "Softmax", "Mha", "GELU", "Logits"};
  return k >= 0 && k < 19 ? names[k] : "unknown";
}
// the shifts of every Softmax row of nb samples, sample by sample over at most DP_HOST_THREADS threads (never more than 16). A sample whose
// status word is set (any class) was refused by an earlier op: its rows hold whatever the later kernels made of it and are NOT read (no value of
// theirs reaches expf, logf or the conversion to an integer); it gets zero shifts and keeps its word. Every other sample is range checked as a
// whole before its first shift is made — softmax_op's order — and gets INFER_BAD_SOFTMAX and zero shifts when an element lies beyond 2^24
inline void infer_softmax_shifts(const LayerSpec& sm, const int64_t* x, size_t nb, int64_t* shifts, uint32_t* status) {
  const size_t C = sm.sm_shape[0], R = sm.sm_shape[1], K = sm.sm_shape[2], rows = C * R;
  const char* te = getenv("DP_HOST_THREADS");
  size_t nth = te ? (size_t)std::max(1, atoi(te)) : (size_t)std::max(1.0, host_cpu_budget() - 2.0);
  nth = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::min<size_t>(nth, 16), nb * rows / 256), nb));
  auto part = [&](size_t t) {
    for (size_t b = nb * t / nth, e = nb * (t + 1) / nth; b < e; b++) {
      const int64_t* xs = x + b * rows * K;
      int64_t* sh = shifts + b * rows;
      bool in = !status[b];
      for (size_t j = 0; j < rows * K && in; j++) in = xs[j] >= -(int64_t(1) << 24) && xs[j] <= (int64_t(1) << 24);
      if (!in) { if (!status[b]) status[b] = INFER_BAD_SOFTMAX; std::fill(sh, sh + rows, int64_t(0)); continue; }
      for (size_t i = 0; i < rows; i++) sh[i] = softmax_row_shift(sm, xs + i * K, i % R + 1);
    }
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < nth; t++) th.emplace_back(part, t);
  part(0);
  for (std::thread& t : th) t.join();
}
inline InferProgram infer_plan(const ModelSpec& m, uint32_t flags = 0) {
  for (size_t id = 0; id < m.layers.size(); id++) {
    const int k = m.layers[id].kind;
    if ((flags & INFER_ALL_KINDS) && k >= L_LAYERNORM && k <= L_GELU) continue;
    if (k == L_LOGITS) continue;  // (integer work without tables: inferred under every flag)
    DP_REQUIRE(k >= L_DENSE && k <= L_QKV, DP_ERR_ARG, "dp_model_infer: node " + std::to_string(id) + " is a " + infer_kind_name(k) + " layer (kind " + std::to_string(k) +
               "): LayerNorm, Softmax, Mha and GELU are not inferred on the device yet");
  }
  InferProgram p;
  p.input_len = m.input_len; p.output_len = model_output_len(m);
  std::vector<size_t> lens; tensor_lens(m, lens);
  auto new_tensor = [&](size_t len, int q) { InferTensor t; t.len = len; t.q = q; p.tensors.push_back(t); return (int)p.tensors.size() - 1; };
  auto new_const = [&](const int64_t* h, size_t n) { InferConst c; c.h64 = h; c.n = n; p.consts.push_back(std::move(c)); return (int)p.consts.size() - 1; };
  for (size_t n : input_tensor_lens(m)) p.inputs.push_back(new_tensor(n, IQ_IF_INPUTS));
  std::vector<std::vector<int>> slot(m.layers.size());  // tensor of (node, output slot)
  std::map<size_t, std::pair<int, int>> mha_inner;      // Mha node -> (the products its Softmax reads, the probabilities)
  auto tensor_of = [&](const Edge& e) { return e.from < 0 ? p.inputs.at((size_t)e.slot) : slot.at((size_t)e.from).at((size_t)e.slot); };
  // the constant [K][N] matrix (b_is_nk: stored [N][K]) of a product, with its int8 copy [N][K] when every weight fits and K * 128 * 128 < 2^31
  auto weight_const = [&](const int64_t* h, size_t K, size_t N, bool b_is_nk) {
    const int c = new_const(h, K * N);
    bool fits = (double)K * 128.0 * 128.0 < 2147483648.0;
    for (size_t i = 0; i < K * N && fits; i++) fits = h[i] >= -128 && h[i] <= 127;
    if (fits) {
      std::vector<int8_t>& w8 = p.consts[(size_t)c].w8;
      w8.resize(K * N);
      for (size_t n = 0; n < N; n++) for (size_t k = 0; k < K; k++) w8[n * K + k] = (int8_t)(b_is_nk ? h[n * K + k] : h[k * N + n]);
    }
    return c;
  };
  auto const_gemm = [&](size_t id, int in, const int64_t* h, size_t s, size_t K, size_t N, bool b_is_nk, const int64_t* bias) {
    InferOp o; o.kind = IO_GEMM; o.node = (int)id; o.in0 = in; o.out = new_tensor(s * N, IQ_NO);
    o.w = weight_const(h, K, N, b_is_nk); o.bias = bias ? new_const(bias, N) : -1;
    o.g.C = 1; o.g.R = s; o.g.K = K; o.g.N = N; o.g.sAr = K; o.g.sAm = 1; o.g.sBm = b_is_nk ? 1 : N; o.g.sBn = b_is_nk ? K : 1; o.g.sOr = N; o.g.sOn = 1;
    p.ops.push_back(o);
    return o.out;
  };
  // a table of the model: the output column, made once per (kind, parameters)
  std::map<TableType, int> tables;
  auto table_const = [&](const TableType& tt) {
    auto it = tables.find(tt);
    if (it != tables.end()) return it->second;
    InferConst c;
    if (tt.kind == 1) { const int64_t mx = int64_t(1) << (tt.size - 1); for (int64_t i = -mx; i < mx; i++) c.own.push_back(gelu_lut(i)); }
    else if (tt.kind == 7) { const int64_t mx = int64_t(1) << (2 * (Q_BIT_LEN - 1)); for (int64_t i = -mx; i < mx; i++) c.own.push_back(inv_sqrt_lut(tt.aux, tt.size, i)); }
    else for (int64_t j = 0; j < (int64_t(1) << tt.size); j++) c.own.push_back(softmax_lut(tt.aux, tt.aux2, j));
    c.n = c.own.size();
    p.consts.push_back(std::move(c));
    return tables[tt] = (int)p.consts.size() - 1;
  };
  // the product of two tensors a ConcatMatMul describes (also the two products of an Mha node)
  auto cm_gemm = [&](size_t id, const LayerSpec& l, int a, int b) {
    InferOp o; o.kind = IO_GEMM2; o.node = (int)id; o.in0 = a; o.in1 = b;
    DP_REQUIRE(p.tensors[(size_t)a].len == l.cm_a[0] * l.cm_a[1] * l.cm_a[2] && p.tensors[(size_t)b].len == l.cm_b[0] * l.cm_b[1] * l.cm_b[2], DP_ERR_SHAPE, "concat matmul: input shapes");
    const CmShape g = cm_shape(l);
    const size_t sa[3] = {l.cm_a[1] * l.cm_a[2], l.cm_a[2], 1}, sb[3] = {l.cm_b[1] * l.cm_b[2], l.cm_b[2], 1};
    o.g.C = g.C; o.g.R = g.R; o.g.K = g.M; o.g.N = g.N;
    o.g.sAc = sa[l.cm_left[0]]; o.g.sAm = sa[l.cm_left[1]]; o.g.sAr = sa[l.cm_left[2]];
    o.g.sBc = sb[l.cm_right[0]]; o.g.sBm = sb[l.cm_right[1]]; o.g.sBn = sb[l.cm_right[2]];
    // axis d of the permuted result is axis perm[d] of [C][R][N]
    size_t so[3] = {g.R * g.N, g.N, 1};
    if (!l.cm_perm.empty()) { const size_t st[3] = {g.out[1] * g.out[2], g.out[2], 1}; for (int d = 0; d < 3; d++) so[l.cm_perm[d]] = st[d]; }
    o.g.sOc = so[0]; o.g.sOr = so[1]; o.g.sOn = so[2];
    o.out = new_tensor(o.g.C * o.g.R * o.g.N, IQ_NO);
    p.ops.push_back(o);
    return o.out;
  };
  auto softmax = [&](size_t id, const LayerSpec& l, int a) {
    const size_t C = l.sm_shape[0], R = l.sm_shape[1], K = l.sm_shape[2];
    DP_REQUIRE(C && R && R == K && p.tensors[(size_t)a].len == C * R * K, DP_ERR_SHAPE, "softmax: shapes");
    DP_REQUIRE(l.sm_table_size <= 24 && 16 + l.sm_table_size + l.sm_zero_chunks * l.sm_zero_vars <= 63, DP_ERR_ARG, "softmax: table sizes");
    InferOp o; o.kind = IO_SOFTMAX; o.node = (int)id; o.in0 = a; o.in1 = new_tensor(C * R, IQ_NO);
    o.table = table_const(softmax_table(l)); o.left = l.sm_scalar; o.right = l.sm_bkm; o.bits = l.sm_table_size;
    o.d[0] = C; o.d[1] = R; o.d[2] = K; o.d[3] = l.sm_zero_chunks; o.d[4] = l.sm_zero_vars;
    o.out = new_tensor(C * R * K, IQ_NO);
    p.ops.push_back(o);
    return o.out;
  };
  for (size_t id = 0; id < m.layers.size(); id++) {
    const LayerSpec& l = m.layers[id];
    const std::vector<Edge> e = edges_in(m, id);
    DP_REQUIRE(e.size() == in_degree(l), DP_ERR_SHAPE, "model graph: wrong number of inputs for a node");
    const int a = tensor_of(e[0]);
    const size_t alen = p.tensors[(size_t)a].len;
    InferOp o; o.node = (int)id; o.in0 = a;
    if (l.kind == L_FLATTEN) { slot[id] = {a}; continue; }
    if (l.kind == L_DENSE) { DP_REQUIRE(alen == l.ncols, DP_ERR_SHAPE, "dense input size mismatch"); slot[id] = {const_gemm(id, a, l.weights.data(), 1, l.ncols, l.nrows, true, l.bias.data())}; continue; }
    if (l.kind == L_MATMUL) {
      DP_REQUIRE(l.nrows && alen % l.nrows == 0, DP_ERR_SHAPE, "matmul input size mismatch");
      slot[id] = {const_gemm(id, a, l.weights.data(), alen / l.nrows, l.nrows, l.ncols, l.mm_transpose, l.bias.empty() ? nullptr : l.bias.data())};
      continue;
    }
    if (l.kind == L_QKV) {
      const size_t k = l.nrows, n = l.ncols;
      DP_REQUIRE(k && alen % k == 0 && l.weights.size() == 3 * k * n && l.bias.size() == 3 * n, DP_ERR_SHAPE, "qkv: shapes");
      for (size_t w = 0; w < 3; w++) slot[id].push_back(const_gemm(id, a, &l.weights[w * k * n], alen / k, k, n, false, &l.bias[w * n]));
      continue;
    }
    if (l.kind == L_CONCAT_MATMUL) { slot[id] = {cm_gemm(id, l, a, tensor_of(e[1]))}; continue; }
    if (l.kind == L_MHA) {  // qk on (Q, K), the Softmax straight on the products, final_mul on (probabilities, V)
      const size_t n = l.mha_shape[0] * l.mha_shape[1] * l.mha_shape[2];
      const int kt = tensor_of(e[1]), vt = tensor_of(e[2]);
      DP_REQUIRE(alen == n && p.tensors[(size_t)kt].len == n && p.tensors[(size_t)vt].len == n, DP_ERR_SHAPE, "mha: input shapes");
      const int qk = cm_gemm(id, mha_qk_spec(l), a, kt), pr = softmax(id, mha_softmax_spec(l), qk);
      mha_inner[id] = {qk, pr};
      slot[id] = {cm_gemm(id, mha_final_spec(l), pr, vt)};
      DP_REQUIRE(p.tensors[(size_t)slot[id][0]].len == lens[id], DP_ERR_SHAPE, "dp_model_infer: tensor length");
      continue;
    }
    if (l.kind == L_SOFTMAX) { slot[id] = {softmax(id, l, a)}; continue; }
    if (l.kind == L_MATMUL2) {
      o.kind = IO_GEMM2; o.in1 = tensor_of(e[1]);
      const size_t blen = p.tensors[(size_t)o.in1].len;
      DP_REQUIRE(l.nrows && alen % l.nrows == 0 && blen == l.nrows * l.ncols, DP_ERR_SHAPE, "matmul2: input shapes");
      o.g.C = 1; o.g.R = alen / l.nrows; o.g.K = l.nrows; o.g.N = l.ncols; o.g.sAr = l.nrows; o.g.sAm = 1;
      o.g.sBm = l.mm_transpose ? 1 : l.ncols; o.g.sBn = l.mm_transpose ? l.nrows : 1; o.g.sOr = l.ncols; o.g.sOn = 1;
      o.out = new_tensor(o.g.C * o.g.R * o.g.N, IQ_NO);
      p.ops.push_back(o); slot[id] = {o.out};
      continue;
    }
    if (l.kind == L_REQUANT) {
      o.kind = IO_REQUANT; o.left = l.fixed_point_multiplier; o.shift = l.shift(); o.bits = l.intermediate_bit_size;
      o.out = new_tensor(alen, IQ_YES);
    } else if (l.kind == L_RELU) { o.kind = IO_RELU; o.out = new_tensor(alen, p.tensors[(size_t)a].q); }
    else if (l.kind == L_ADD || l.kind == L_POSITIONAL) {
      if (l.kind == L_ADD) DP_REQUIRE(alen == l.weights.size(), DP_ERR_SHAPE, "add: operand size mismatch");
      else DP_REQUIRE(l.ncols && alen % l.ncols == 0 && alen <= l.weights.size(), DP_ERR_SHAPE, "positional: input shape");
      o.kind = IO_ADDC; o.left = l.add_left; o.right = l.add_right; o.w = new_const(l.weights.data(), alen); o.out = new_tensor(alen, IQ_NO);
    } else if (l.kind == L_ADD2) {
      o.kind = IO_ADD2; o.in1 = tensor_of(e[1]); o.left = l.add_left; o.right = l.add_right;
      DP_REQUIRE(alen == p.tensors[(size_t)o.in1].len, DP_ERR_SHAPE, "add2: inputs of different lengths");
      o.out = new_tensor(alen, IQ_NO);
    } else if (l.kind == L_EMBED) {
      o.kind = IO_EMBED; o.w = new_const(l.weights.data(), l.nrows * l.ncols); o.d[0] = l.nrows; o.d[1] = l.ncols; o.out = new_tensor(alen * l.ncols, IQ_NO);
    } else if (l.kind == L_MAXPOOL) {
      DP_REQUIRE(alen == l.pin[0] * l.pin[1] * l.pin[2], DP_ERR_SHAPE, "maxpool: input size mismatch");
      o.kind = IO_MAXPOOL; o.d[0] = l.pin[0]; o.d[1] = l.pin[1]; o.d[2] = l.pin[2]; o.out = new_tensor(alen / 4, p.tensors[(size_t)a].q);
    } else if (l.kind == L_CONV) {
      DP_REQUIRE(alen == l.kx * l.nw * l.nw, DP_ERR_SHAPE, "conv: input size mismatch");
      o.kind = IO_CONV; o.w = new_const(l.weights.data(), l.weights.size()); o.bias = new_const(l.bias.data(), l.bias.size());
      o.d[0] = l.kw; o.d[1] = l.kx; o.d[2] = l.real_nw; o.d[3] = l.nw; o.d[4] = l.unp_out[0]; o.d[5] = l.unp_out[1]; o.d[6] = l.unp_out[2];
      o.out = new_tensor(l.kw * l.nw * l.nw, IQ_NO);
    } else if (l.kind == L_GELU) {
      const TableType tt = gelu_table(l);
      o.kind = IO_GELU; o.table = table_const(tt); o.left = l.fixed_point_multiplier; o.d[0] = size_t(1) << (tt.size - 1); o.out = new_tensor(alen, IQ_NO);
    } else if (l.kind == L_LOGITS) {  // the index of the first maximum of every row (argmax_rows); reads the int8 copy of a Requant's output where there is one
      DP_REQUIRE(l.nrows && l.ncols && alen == l.nrows * l.ncols, DP_ERR_SHAPE, "logits: input shape");
      o.kind = IO_ARGMAX; o.d[0] = l.nrows; o.d[1] = l.ncols; o.out = new_tensor(l.nrows, IQ_NO);
    } else if (l.kind == L_LAYERNORM) {
      const size_t fd = l.weights.size();
      DP_REQUIRE((fd && !(fd & (fd - 1))) && l.bias.size() == fd && alen % fd == 0 && l.ln_dim_size >= 1 && l.ln_dim_size <= fd && l.ln_range_check_bits < 64, DP_ERR_SHAPE, "layernorm: shapes");
      o.kind = IO_LAYERNORM; o.w = new_const(l.weights.data(), fd); o.bias = new_const(l.bias.data(), fd); o.table = table_const(layernorm_table(l));
      o.left = l.ln_multiplier; o.shift = l.ln_range_check_bits; o.d[0] = fd; o.d[1] = l.ln_dim_size; o.out = new_tensor(alen, IQ_NO);
    }
    DP_REQUIRE(p.tensors[(size_t)o.out].len == lens[id], DP_ERR_SHAPE, "dp_model_infer: tensor length");
    p.ops.push_back(o); slot[id] = {o.out};
  }
  for (const Edge& e : output_edges(m)) p.outputs.push_back(tensor_of(e));
  // the taps: the tensor behind every entry of the trace row, in the layout's order (a Flatten node's entry is the tensor it passes on)
  const TraceLayout lay = trace_layout(m);
  for (const TraceEntry& e : lay.entries) {
    const size_t id = (size_t)e.node;
    InferTap t; t.len = (size_t)e.len; t.off = (size_t)e.off;
    t.tensor = e.role == TRACE_ROLE_MHA_IN ? mha_inner.at(id).first : e.role == TRACE_ROLE_MHA_OUT ? mha_inner.at(id).second : slot.at(id).at((size_t)e.role);
    DP_REQUIRE(p.tensors[(size_t)t.tensor].len == t.len, DP_ERR_SHAPE, "dp_model_infer: tap length");
    p.taps.push_back(t);
  }
  p.row_words = lay.row_words;
  // (m is the model of the dp_model that keeps this program: it outlives it)
  p.shifts = [&m](const InferOp& o, const int64_t* x, size_t nb, int64_t* shifts, uint32_t* status) {
    const LayerSpec& l = m.layers[(size_t)o.node];
    infer_softmax_shifts(l.kind == L_MHA ? mha_softmax_spec(l) : l, x, nb, shifts, status);
  };
  return p;
}
#endif

}  // namespace dp
