// Batched quantised inference on the device (dp_model_infer, include/deep_prove_hip_infer.h): Model::run for many independent inputs.
// The host flattens a ModelSpec into an InferProgram (infer_plan below: tensors, constants, one op per launch) once per model; hip_infer_run
// (infer_kernels.inc, compiled into hip_dev.hip) executes it for a batch: activations are [batch][tensor], one launch serves the whole batch.
// Which products take the i8 MFMA is decided here, statically: the weights within -128..127, K * 128 * 128 < 2^31 and the input produced by
// a Requant (through ReLU / MaxPool / Flatten), a model input the host has range-checked at upload, or a tensor whose values are bounded
// whatever the data is (infer_range_plan below: the entries of a GELU or Embeddings table and sums of such): within -128..127 it gets an int8
// copy, within -16384..16383 two int8 planes, the left operand of k_infer_gemm_i8_pl. A convolution is such a product too
// (k_infer_conv_i8, on the packed filter image of infer_conv_pack) at every padded kernel side the kernel has a form for: 1 (a pointwise layer,
// staged as a GEMM in K slices whatever the number of channels), 2, 4, 8 and 16 (whole input spans in LDS where they fit, channel slices where they
// do not: infer_conv_slice). Everything else is 64-bit
// multiply-add with the host's wrap-around. The product of two tensors of the batch (IO_GEMM2: MatMul2, ConcatMatMul, the two products of an Mha node)
// takes k_infer_gemm2_i8 when infer_gemm2_plan below finds a form for both operands and both have int8 copies; the left one may instead be a
// two-plane tensor (IQ_PLANES: the probabilities a Softmax writes, when every entry of its table lies in 0..16383, or a tensor of infer_range_plan).
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

// every value of the tensor within -128..127: never / always / iff the model inputs of the call are; IQ_PLANES: every value within -16384..16383,
// the tensor has two int8 planes (lo = v & 127 in 0..127, hi = v >> 7 arithmetic in -128..127: v = 128 * hi + lo exactly) and NO int8 copy — only
// the left operand of k_infer_gemm2_i8 and of k_infer_gemm_i8_pl reads them
enum InferQ { IQ_NO = 0, IQ_YES = 1, IQ_IF_INPUTS = 2, IQ_PLANES = 3 };
struct InferTensor { size_t len = 0; int q = IQ_NO; };
// what ReLU / MaxPool make of their input's form: they keep -128..127 and write the int8 copy themselves; they write no planes
inline int infer_q_through(int q) { return q == IQ_PLANES ? (int)IQ_NO : q; }
// a constant of the model. h64 points into the ModelSpec (it lives as long as the dp_model); w8 = the same matrix as int8, transposed to [N][K]
// (both operands of k_infer_gemm_i8 are read along K), empty when a weight does not fit. Uploaded at the first launch that reads it.
// A conv's filter: w8 = its packed int8 image [kw][K] (infer_conv_pack below), the operand of k_infer_conv_i8, under the same rule.
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
  InferGemmShape g;                  // IO_GEMM (B = constant w; the i8 form when in0 is q and w has an int8 copy), IO_GEMM2 (B = tensor in1); IO_CONV: g.K = the packed K of the int8 filter image
  int64_t left = 1, right = 1;       // IO_ADDC: left * x + right * w[i]; IO_ADD2: left * a + right * b; IO_REQUANT, IO_GELU, IO_LAYERNORM: left = multiplier; IO_SOFTMAX: left = scalar, right = bkm
  unsigned shift = 0, bits = 0;      // IO_REQUANT; IO_LAYERNORM: shift = range_check_bits; IO_SOFTMAX: bits = table bits
  // IO_EMBED: vocabulary, embedding size; IO_MAXPOOL: c, h, w; IO_CONV: kw, kx, real_nw, nw, unp_out[3], ra (the filter rows of the int8 image; 0: none, the op stays on k_infer_conv); IO_GELU: max; IO_LAYERNORM: row length, N;
  // IO_SOFTMAX: C, R, K, zero chunks, zero vars (in1 = the shift buffer of the chunk, a tensor of C * R words per sample); IO_ARGMAX: rows, K;
  // IO_GEMM2: d[0] = infer_gemm2_plan (IG2_*; 0: the op stays on k_infer_gemm_i64); IO_GEMM: d[0] = the ops behind it that k_infer_gemm_i8_rq
  // absorbs (infer_fuse_plan: 0 none, 1 its Requant, 2 the Requant and a ReLU), d[1], d[2] = their indices in InferProgram::ops.
  // An IO_GEMM2 at the head of a chain of k_infer_gemm2_i8_rq (nfused = 1, fused[0] = its Requant): d[1] = IG2_OW | IG2_SM* (the wide store; with
  // IG2_SM the Softmax in front of it is made on the way into LDS), d[2] = that Softmax's index in InferProgram::ops. The IO_SOFTMAX such a chain serves: d[5] = 1 + the index of the chain's IO_GEMM2 (0: none)
  size_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // IO_CONV: the ops behind it that the epilogue of k_infer_conv_i8_rq absorbs (infer_fuse_plan), as indices in InferProgram::ops in chain
  // order: its Requant, then a ReLU and / or a MaxPool; nfused = 0: none. IO_GEMM2: the Requant the epilogue of k_infer_gemm2_i8_rq absorbs
  int nfused = 0, fused[3] = {-1, -1, -1};
  // IO_CONV: the input channels of a slice (infer_conv_slice) where the int8 image is served by the channel-sliced kernels; 0: unsliced
  unsigned jc = 0;
};
// k_infer_conv_i8 (infer_kernels.inc): a workgroup computes IC_TC output channels of a strip of IC_TP consecutive pixels of one sample's plane; the
// filter tile goes through LDS in K slices of IC_TK bytes (row pitch IC_LDA). Its dynamic LDS, in this order: the filter slice, one word per
// filter row of the packed K (where the row's input bytes start), and per input channel the span of int8 inputs the strip can touch —
// IC_TP + (ra - 1) * nw + rn - 1 bytes, + 4 so that every fragment can be cut from whole aligned words, rounded up to 16.
// A pointwise layer (rn == 1, infer_conv_tile<1>) has no table and no spans: behind the filter slice lies the input slice, IC_TP pixels x IC_TK
// channels at row pitch IC_LDA — 23040 bytes whatever kx is.
// The channel-sliced form (rn >= 2, infer_conv_tile_sl) serves the layers whose kx spans do not fit: the input channels go through LDS in slices
// of jc channels — jc * ra * rn consecutive k of the image —, two span buffers of jc spans each (rounded up to whole rounds of 256 words, one per thread of the
// workgroup) behind a row table of jc * ra words that holds for every slice. infer_conv_slice is the slice rule: jc = the largest power of two with jc * pitch <= IC_SL_MAX (a slice is at most 4096 words: 16
// per thread), jc * ra * rn a multiple of IC_TK (no K slice of the filter straddles two span slices; K = kx * ra * rn then, without padding) and
// kx a multiple of jc; 0 where there is none (a very wide plane: the pitch alone passes IC_SL_MAX, or so few spans fit that they hold no whole K
// slice). jc <= 64 (a pitch is at least 144), so its LDS is at most 4608 + 4 * 64 * 16 + 2 * IC_SL_MAX = 41472 bytes whatever kx is.
// infer_conv_lds is the one rule (jc = 0: the whole-span form): infer_conv_pack admits by it, infer_launch sizes by it
constexpr unsigned IC_TC = 32, IC_TP = 128, IC_TK = 128, IC_LDA = IC_TK + 16, IC_LDS_MAX = 48 * 1024, IC_SL_MAX = 16 * 1024;
DP_HD unsigned infer_conv_pitch(unsigned nw, unsigned ra, unsigned rn) { return (IC_TP + (ra - 1) * nw + rn + 3 + 15) & ~15u; }
DP_HD unsigned infer_conv_tab_words(unsigned K, unsigned rn) { return rn == 1 ? 0u : (K / rn + 3) & ~3u; }
DP_HD unsigned infer_conv_slice(unsigned kx, unsigned nw, unsigned ra, unsigned rn) {
  if (rn < 2 || !kx) return 0;
  const unsigned fit = IC_SL_MAX / infer_conv_pitch(nw, ra, rn);
  unsigned jc = kx & (0u - kx);  // (the largest power of two that divides kx)
  while (jc > fit) jc >>= 1;
  return jc && jc * ra * rn % IC_TK == 0 ? jc : 0;  // (a smaller power of two has fewer factors of two still)
}
DP_HD size_t infer_conv_lds(size_t kx, unsigned nw, unsigned ra, unsigned rn, unsigned K, unsigned jc = 0) {
  if (rn == 1) return (size_t)(IC_TC + IC_TP) * IC_LDA;
  if (jc) return (size_t)IC_TC * IC_LDA + 4 * (size_t)infer_conv_tab_words(jc * ra * rn, rn) + 2 * (((size_t)jc * infer_conv_pitch(nw, ra, rn) + 1023) & ~size_t(1023));
  return (size_t)IC_TC * IC_LDA + 4 * (size_t)infer_conv_tab_words(K, rn) + kx * infer_conv_pitch(nw, ra, rn);
}
// The static half of "does this IO_GEMM2 take k_infer_gemm2_i8" (the other half, at the launch: both tensors have their int8 form in this call).
// Each operand needs a unit stride along m (IG2_*K: staged with loads along K) or along its other matrix axis, r for A / n for B (IG2_*T: read along
// that axis and transposed on the way into LDS); one whose unit stride is the concat axis is not served. K * 128 * 128 < 2^31 keeps the 32-bit
// accumulator exact (the rule of weight_const). IG2_*W: the wide loads of the form — 16 bytes along K, 4 bytes along r / n — are aligned for every
// (sample, concat index, row) and never leave the matrix: the int8 copy of a tensor starts 256-aligned, so the per-sample length, the concat and
// row strides and the extent along the load must all be multiples of the load. lenA / lenB: the words of a sample of the two tensors.
constexpr unsigned IG2_OK = 1, IG2_AT = 2, IG2_BT = 4, IG2_AW = 8, IG2_BW = 16;
inline unsigned infer_gemm2_plan(const InferGemmShape& g, size_t lenA, size_t lenB) {
  if (!g.C || !g.R || !g.K || !g.N || !((double)g.K * 128.0 * 128.0 < 2147483648.0)) return 0;
  auto form = [&](size_t sK, size_t sX, size_t sC, size_t X, size_t len, unsigned T, unsigned W) -> int {
    const bool t = sK != 1;
    if (t && sX != 1) return -1;
    const size_t w = t ? 4 : 16, along = t ? X : g.K, across = t ? sK : sX;
    return (int)((t ? T : 0) | (along % w == 0 && across % w == 0 && (g.C == 1 || sC % w == 0) && len % w == 0 ? W : 0));
  };
  const int a = form(g.sAm, g.sAr, g.sAc, g.R, lenA, IG2_AT, IG2_AW), b = form(g.sBm, g.sBn, g.sBc, g.N, lenB, IG2_BT, IG2_BW);
  return a < 0 || b < 0 ? 0 : IG2_OK | (unsigned)a | (unsigned)b;
}
// k_infer_gemm2_i8_rq (InferOp::d[1] of the chain's IO_GEMM2; the kernel takes d[0] | d[1]). IG2_OW: the int8 tile leaves in 16-byte vectors along n
// (sOn == 1 and N, the row and concat strides and the words of a sample are multiples of 16: the int8 copy of a tensor starts 256-aligned).
// IG2_SM: the left operand is made from the Softmax's int64 input; IG2_SM_LDS: its exponential table is staged in LDS as 16-bit entries
// (infer_gemm2_rq_table_lds; otherwise the 16-bit table is gathered through global memory); IG2_SM_SKIP: a masked element is 0, so the K slices
// wholly above the diagonal of the tile's rows are skipped
constexpr unsigned IG2_OW = 32, IG2_SM = 64, IG2_SM_LDS = 128, IG2_SM_SKIP = 256;
// the LDS of k_infer_gemm2_i8_rq: three (SM: two planes of A, and B) or two operand slices of 64 rows at pitch 80, and behind them the table
constexpr size_t IG2_RQ_LDS_MAX = 48 * 1024, IG2_RQ_OPERANDS = 3 * 64 * 80;
// (tv <= 14. A diagnostic build with -DDP_IG2_TABLE_GATHER gathers every table through global memory: the measurement of the other form)
#ifdef DP_IG2_TABLE_GATHER
DP_HD bool infer_gemm2_rq_table_lds(unsigned) { return false; }
#else
DP_HD bool infer_gemm2_rq_table_lds(unsigned tv) { return tv >= 3 && IG2_RQ_OPERANDS + (size_t(2) << tv) <= IG2_RQ_LDS_MAX; }
#endif
// Softmax::evaluate on one element after the mask and the shift (called by k_infer_softmax, by k_infer_gemm2_i8_rq and by the planner: the arithmetic exists once): |masked| = low byte | high
// byte | exponential table index (tv bits) | zero chunks (zc groups of zv bits). The index, and whether every zero chunk is zero: the value is
// table[index] then, else 0. The index is masked: nothing is read outside the table, whatever the data
DP_HD bool infer_softmax_index(int64_t masked, unsigned tv, unsigned zc, unsigned zv, size_t* index) {
  int64_t r = masked < 0 ? (int64_t)(0 - (uint64_t)masked) : masked;
  r >>= 16;
  *index = (size_t)(r & ((int64_t(1) << tv) - 1));
  r >>= tv;
  bool keep = true;
  for (unsigned z = 0; z < zc; z++) { keep = keep && (r & ((int64_t(1) << zv) - 1)) == 0; r >>= zv; }
  return keep;
}
DP_HD int64_t infer_softmax_neg_inf(int64_t bkm) { return -(((bkm >> 16) + 1) << 16); }
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
// The tiles of k_infer_gemm2_i8 (64 x 64 per workgroup, one (sample, concat index) each) for nb samples: its grid, which must fit 31 bits
inline size_t infer_gemm2_tiles(const InferGemmShape& g, size_t nb) { return nb * g.C * ((g.R + 63) / 64) * ((g.N + 63) / 64); }
// THE predicate "op o reads only the int8 form of tensor t in this call": o is a product that takes an MFMA kernel (k_infer_gemm_i8 /
// k_infer_gemm_i8_rq or, on a two-plane input, k_infer_gemm_i8_pl; k_infer_conv_i8; k_infer_gemm2_i8 — whose left operand may be two planes
// instead) or an Argmax that reads the int8 copy.
// q: the form of every tensor in this call (InferScratch::q), nb: the samples of the chunk, no_mfma: DP_INFER_NO_MFMA. infer_launch dispatches
// on it and infer_needs_int64 elides by it: what is launched and what is left unwritten cannot drift apart. Every other reader (Add2, LayerNorm,
// GELU, Softmax, Requant, ReLU, MaxPool, Embeddings, a 64-bit product) reads the int64 form: false.
inline bool infer_reads_int8_only(const InferProgram& p, const InferOp& o, int t, const std::vector<char>& q, size_t nb, bool no_mfma) {
  if (t < 0 || (t != o.in0 && t != o.in1)) return false;
  switch (o.kind) {
    case IO_GEMM: return !no_mfma && t == o.in0 && (q[(size_t)o.in0] == IQ_YES || q[(size_t)o.in0] == IQ_PLANES) && !p.consts[(size_t)o.w].w8.empty();
    case IO_CONV: return !no_mfma && t == o.in0 && q[(size_t)o.in0] == IQ_YES && !p.consts[(size_t)o.w].w8.empty();
    case IO_GEMM2: return !no_mfma && (o.d[0] & IG2_OK) && (q[(size_t)o.in0] == IQ_YES || q[(size_t)o.in0] == IQ_PLANES) && q[(size_t)o.in1] == IQ_YES && infer_gemm2_tiles(o.g, nb) <= 0x7fffffffu;
    case IO_ARGMAX: return t == o.in0 && q[(size_t)o.in0] == IQ_YES;
    default: return false;
  }
}
// whether tensor t must exist as int64 in this call: it is a model output, or some op reads more than its int8 form (when in doubt: yes)
inline bool infer_needs_int64(const InferProgram& p, int t, const std::vector<char>& q, size_t nb, bool no_mfma) {
  if (std::find(p.outputs.begin(), p.outputs.end(), t) != p.outputs.end()) return true;
  for (const InferOp& o : p.ops) if ((o.in0 == t || o.in1 == t) && !infer_reads_int8_only(p, o, t, q, nb, no_mfma)) return true;
  return false;
}
// The form k_infer_gemm2_i8_rq takes for the chain at IO_GEMM2 o in this call: 0 none (today's launches), 1 SM = false, 2 SM = true. The same
// per-call conditions as k_infer_gemm2_i8 (infer_reads_int8_only: the right operand has its int8 form, the tiles fit, no DP_INFER_NO_MFMA); the
// launch of the product and the skipped launch of the Softmax (infer_launch) both ask here, so they cannot drift apart
inline int infer_gemm2_rq_form(const InferProgram& p, const InferOp& o, const std::vector<char>& q, size_t nb, bool no_mfma) {
  if (o.kind != IO_GEMM2 || !o.nfused || !infer_reads_int8_only(p, o, o.in0, q, nb, no_mfma)) return 0;
  return (o.d[1] & IG2_SM) ? 2 : q[(size_t)o.in0] == IQ_YES ? 1 : 0;
}
// The chains k_infer_gemm_i8_rq serves in one launch, marked on the finished program (the last step of infer_plan): an IO_GEMM whose constant has
// an int8 copy and whose output has exactly one reader, an IO_REQUANT with shift >= 1, and is no model output; and behind that, where the
// Requant's output likewise has exactly one reader, an IO_RELU, and is no model output, the ReLU too. The absorbed ops run at the head's place
// in the order of the ops, so no op in between may be one that refuses data under another class (Embeddings, GELU, LayerNorm, Softmax): the
// status word holds the class of the FIRST op that refused a sample. Whether the head's input has its int8 form, and whether the chain's last
// tensor still needs its int64 form, is known per call only (infer_launch).
// The chains k_infer_conv_i8_rq serves, under the same rules (InferOp::fused): an IO_CONV that has its int8 image, its Requant with shift >= 1,
// then optionally a ReLU, then optionally — behind the ReLU or straight behind the Requant — a MaxPool. The MaxPool is absorbed only where a
// strip of IC_TP pixels holds whole pairs of rows (nw <= 64 and a divisor of IC_TP) and its (c, h, w) are the conv's (kw, nw, nw); otherwise the
// chain ends in front of it and k_infer_maxpool runs.
// The chains k_infer_gemm2_i8_rq serves, under the same rules: an IO_GEMM2 that infer_gemm2_plan has a form for and its Requant with shift >= 1
// (fused[0]), where the left operand has an int8 copy (IQ_YES, or IQ_IF_INPUTS: per call) — SM = false —; or where the left operand is the
// output of an IO_SOFTMAX of the two-plane kind (IQ_PLANES) that nothing else reads, that is no model output and that the product reads in the
// Softmax's own layout (g.C, g.R, g.K = its C, R, K; sAm = 1, sAr = K, sAc = R K) — SM = true: the Softmax (d[2]; its d[5] points back) is made
// on the way into LDS and neither the probabilities nor their planes are written. The Softmax's shift step stays where the Softmax is, and the
// fused launch runs at the product's place. A product on planes in any other layout, or on planes with another reader, keeps its launches.
// (The 16-bit image of the Softmax's table — every entry is within 0..16383 — becomes the w8 of the table's constant: little-endian pairs.)
inline int64_t infer_softmax_masked(const InferProgram& p, const InferOp& sm) {
  size_t idx = 0;
  return infer_softmax_index(infer_softmax_neg_inf(sm.right), sm.bits, (unsigned)sm.d[3], (unsigned)sm.d[4], &idx) ? p.consts[(size_t)sm.table].data()[idx] : 0;
}
inline void infer_fuse_plan(InferProgram& p) {
  const size_t nt = p.tensors.size(), no = p.ops.size();
  std::vector<int> readers(nt, 0), reader(nt, -1);
  for (size_t i = 0; i < no; i++) for (int t : {p.ops[i].in0, p.ops[i].in1}) if (t >= 0) { readers[(size_t)t]++; reader[(size_t)t] = (int)i; }
  for (int t : p.outputs) readers[(size_t)t] += 2;  // (a model output is never a tensor with ONE reader)
  // the only reader of tensor t, when it is an op of `kind` behind op `from` with no refusing op of another class between the two; else -1
  auto sole = [&](int t, int kind, size_t from) {
    const int j = readers[(size_t)t] == 1 ? reader[(size_t)t] : -1;
    if (j < 0 || (size_t)j <= from || p.ops[(size_t)j].kind != kind || p.ops[(size_t)j].in0 != t) return -1;
    for (size_t k = from + 1; k < (size_t)j; k++) { const int kk = p.ops[k].kind; if (kk == IO_EMBED || kk == IO_GELU || kk == IO_LAYERNORM || kk == IO_SOFTMAX) return -1; }
    return j;
  };
  for (size_t i = 0; i < no; i++) {
    InferOp& o = p.ops[i];
    if (o.kind == IO_CONV && o.d[7]) {  // (o.d[7]: the conv has its int8 image)
      const int rq = sole(o.out, IO_REQUANT, i);
      if (rq < 0 || p.ops[(size_t)rq].shift < 1) continue;
      o.fused[o.nfused++] = rq;
      const int rl = sole(p.ops[(size_t)rq].out, IO_RELU, i);
      if (rl >= 0) o.fused[o.nfused++] = rl;
      const int mp = sole(p.ops[(size_t)(rl < 0 ? rq : rl)].out, IO_MAXPOOL, i);
      const size_t kw = o.d[0], nw = o.d[3];
      if (mp >= 0 && nw <= 64 && IC_TP % nw == 0 && p.ops[(size_t)mp].d[0] == kw && p.ops[(size_t)mp].d[1] == nw && p.ops[(size_t)mp].d[2] == nw) o.fused[o.nfused++] = mp;
      continue;
    }
    if (o.kind == IO_GEMM2 && (o.d[0] & IG2_OK)) {
      const int rq = sole(o.out, IO_REQUANT, i), qa = p.tensors[(size_t)o.in0].q;
      if (rq < 0 || p.ops[(size_t)rq].shift < 1) continue;
      const InferGemmShape& g = o.g;
      const size_t lenO = p.tensors[(size_t)o.out].len;
      size_t fl = g.sOn == 1 && g.N % 16 == 0 && g.sOr % 16 == 0 && (g.C == 1 || g.sOc % 16 == 0) && lenO % 16 == 0 ? IG2_OW : 0;
      if (qa == IQ_PLANES) {
        int si = -1;
        for (size_t k = 0; k < i; k++) if (p.ops[k].out == o.in0) si = (int)k;
        if (si < 0 || p.ops[(size_t)si].kind != IO_SOFTMAX || sole(o.in0, IO_GEMM2, (size_t)si) != (int)i) continue;
        InferOp& sm = p.ops[(size_t)si];
        if (g.C != sm.d[0] || g.R != sm.d[1] || g.K != sm.d[2] || g.sAm != 1 || g.sAr != g.K || g.sAc != g.R * g.K) continue;
        const int64_t masked = infer_softmax_masked(p, sm);
        fl |= IG2_SM | (infer_gemm2_rq_table_lds(sm.bits) ? IG2_SM_LDS : 0) | (masked == 0 ? IG2_SM_SKIP : 0);
        InferConst& tc = p.consts[(size_t)sm.table];
        if (tc.w8.empty()) { tc.w8.resize(tc.n * 2); for (size_t j = 0; j < tc.n; j++) { tc.w8[2 * j] = (int8_t)(tc.own[j] & 255); tc.w8[2 * j + 1] = (int8_t)(tc.own[j] >> 8); } }
        sm.d[5] = i + 1; o.d[2] = (size_t)si;
      } else if (qa != IQ_YES && qa != IQ_IF_INPUTS) continue;
      o.fused[o.nfused++] = rq; o.d[1] = fl;
      continue;
    }
    if (o.kind != IO_GEMM || p.consts[(size_t)o.w].w8.empty()) continue;
    const int rq = sole(o.out, IO_REQUANT, i);
    if (rq < 0 || p.ops[(size_t)rq].shift < 1) continue;
    const int rl = sole(p.ops[(size_t)rq].out, IO_RELU, i);
    o.d[0] = rl < 0 ? 1 : 2; o.d[1] = (size_t)rq; o.d[2] = rl < 0 ? 0 : (size_t)rl;
  }
}
// Static value ranges, on the finished program (in front of infer_fuse_plan): every tensor gets an interval [lo, hi] that holds for ANY input
// data, refused samples included (what a refusing kernel writes for a refused element is named at each rule), or stays unknown:
//   Requant: -127..127 (the clamp); ReLU: its input's, clamped at 0; MaxPool: its input's; GELU: min..max of its table with 0 (a refused
//   element); Embeddings: min..max of its table (a bad token reads row 0); Softmax: min..max of its table with 0 (the index is masked);
//   IO_ADDC: left * [x] + right * [min w, max w] over the words read; IO_ADD2: left * [x] + right * [y];
//   model inputs, products, convolutions, LayerNorm, Argmax: unknown.
// The arithmetic is checked int64: an overflow makes the interval unknown (the device's sums wrap there). A tensor gets a NEW form only when it
// has none (IQ_NO) and some IO_GEMM whose constant has an int8 copy reads it as in0: IQ_YES within -128..127, IQ_PLANES within -16384..16383,
// none when the interval is unknown or wider. ReLU and MaxPool write an int8 copy and no planes (infer_q_through): their outputs get IQ_YES or
// nothing. Every other tensor, and with it the scratch layout and the launches of every program without such a product, stays as it is.
struct InferRange { bool known = false; int64_t lo = 0, hi = 0; };
inline InferRange infer_range_axpy(int64_t left, InferRange x, int64_t right, InferRange y) {
  InferRange r;
  if (!x.known || !y.known) return r;
  int64_t a[2], b[2], lo, hi;
  if (__builtin_mul_overflow(left, x.lo, &a[0]) || __builtin_mul_overflow(left, x.hi, &a[1]) || __builtin_mul_overflow(right, y.lo, &b[0]) || __builtin_mul_overflow(right, y.hi, &b[1])) return r;
  if (__builtin_add_overflow(std::min(a[0], a[1]), std::min(b[0], b[1]), &lo) || __builtin_add_overflow(std::max(a[0], a[1]), std::max(b[0], b[1]), &hi)) return r;
  r.known = true; r.lo = lo; r.hi = hi;
  return r;
}
inline std::vector<InferRange> infer_ranges(const InferProgram& p) {
  std::vector<InferRange> rg(p.tensors.size());
  auto span = [](const int64_t* w, size_t n, bool with_zero) {
    InferRange r;
    if (!w || !n) return r;
    r.known = true; r.lo = r.hi = with_zero ? 0 : w[0];
    for (size_t i = 0; i < n; i++) { r.lo = std::min(r.lo, w[i]); r.hi = std::max(r.hi, w[i]); }
    return r;
  };
  for (const InferOp& o : p.ops) {  // (in the order of the ops: every input is written before it is read)
    const InferRange x = o.in0 >= 0 ? rg[(size_t)o.in0] : InferRange();
    InferRange r;
    switch (o.kind) {
      case IO_REQUANT: r.known = true; r.lo = -127; r.hi = 127; break;
      case IO_RELU: r = x; r.lo = std::max<int64_t>(r.lo, 0); r.hi = std::max<int64_t>(r.hi, 0); break;
      case IO_MAXPOOL: r = x; break;
      case IO_GELU: case IO_SOFTMAX: r = span(p.consts[(size_t)o.table].data(), p.consts[(size_t)o.table].n, true); break;
      case IO_EMBED: r = span(p.consts[(size_t)o.w].data(), p.consts[(size_t)o.w].n, false); break;
      case IO_ADDC: r = infer_range_axpy(o.left, x, o.right, span(p.consts[(size_t)o.w].data(), std::min(p.consts[(size_t)o.w].n, p.tensors[(size_t)o.out].len), false)); break;
      case IO_ADD2: r = infer_range_axpy(o.left, x, o.right, rg[(size_t)o.in1]); break;
      default: break;
    }
    rg[(size_t)o.out] = r;
  }
  return rg;
}
inline void infer_range_plan(InferProgram& p) {
  const std::vector<InferRange> rg = infer_ranges(p);
  std::vector<int> producer(p.tensors.size(), -1);
  for (const InferOp& o : p.ops) producer[(size_t)o.out] = o.kind;
  for (const InferOp& o : p.ops) {
    if (o.kind != IO_GEMM || p.consts[(size_t)o.w].w8.empty()) continue;
    InferTensor& t = p.tensors[(size_t)o.in0];
    const InferRange& r = rg[(size_t)o.in0];
    const int k = producer[(size_t)o.in0];
    if (t.q != IQ_NO || !r.known) continue;
    const bool copy = k == IO_RELU || k == IO_MAXPOOL, planes = k == IO_GELU || k == IO_EMBED || k == IO_ADDC || k == IO_ADD2;  // (who writes which form)
    if ((copy || planes) && r.lo >= -128 && r.hi <= 127) t.q = IQ_YES;
    else if (planes && r.lo >= -16384 && r.hi <= 16383) t.q = IQ_PLANES;
  }
}
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
// The int8 image of a conv's filter, the channel-side operand of k_infer_conv_i8. The filter is [kw][kx][rn][rn] (rn = real_nw, the padded
// kernel side) and mostly padding: ra = the smallest number of leading filter rows that holds every non-zero weight of every filter of the
// layer (at least 1). The image is [kw][K]: k = (j * ra + a) * rn + c for input channel j, filter row a < ra and column c < rn — c keeps the
// padded rn, so rn consecutive k are rn consecutive input bytes —, zero padded from kx * ra * rn up to K, a multiple of the 32 of an MFMA
// step; at rn = 1 (ra = 1) simply k = j. No image (w8 empty, ra = K = 0) unless rn is 1, 2, 4, 8 or 16, nw a multiple of 4 (whole words of a plane are staged), every weight within
// -128..127, K * 128 * 128 < 2^31 (the 32-bit accumulator is exact) and the kernel's LDS fits (infer_conv_lds): a pointwise layer always does; where
// the kx spans of rn >= 2 fit IC_LDS_MAX the layer takes the whole-span form (jc = 0), otherwise the channel-sliced one where infer_conv_slice
// has a jc for it; otherwise (a very wide plane) the op stays on k_infer_conv.
struct InferConvImage { size_t ra = 0, K = 0; unsigned jc = 0; std::vector<int8_t> w8; };
inline InferConvImage infer_conv_pack(const LayerSpec& l) {
  InferConvImage im;
  const size_t rn = l.real_nw, per = rn * rn, nf = l.kw * l.kx;
  if ((rn != 1 && rn != 2 && rn != 4 && rn != 8 && rn != 16) || l.nw % 4 || l.nw > 4096 || l.weights.size() != nf * per) return im;
  size_t ra = 1;
  for (size_t i = 0; i < nf * per; i++) {
    if (l.weights[i] < -128 || l.weights[i] > 127) return im;
    if (l.weights[i]) ra = std::max(ra, i % per / rn + 1);
  }
  const size_t K = (l.kx * ra * rn + 31) & ~size_t(31);
  if (!((double)K * 128.0 * 128.0 < 2147483648.0)) return im;
  unsigned jc = 0;
  if (infer_conv_lds(l.kx, (unsigned)l.nw, (unsigned)ra, (unsigned)rn, (unsigned)K) > IC_LDS_MAX) {
    jc = infer_conv_slice((unsigned)l.kx, (unsigned)l.nw, (unsigned)ra, (unsigned)rn);
    if (!jc || infer_conv_lds(l.kx, (unsigned)l.nw, (unsigned)ra, (unsigned)rn, (unsigned)K, jc) > IC_LDS_MAX) return im;
  }
  im.ra = ra; im.K = K; im.jc = jc; im.w8.assign(l.kw * K, 0);
  for (size_t f = 0; f < nf; f++) for (size_t a = 0; a < ra; a++) for (size_t c = 0; c < rn; c++)
    im.w8[f / l.kx * K + (f % l.kx * ra + a) * rn + c] = (int8_t)l.weights[(f * rn + a) * rn + c];
  return im;
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
    o.d[0] = infer_gemm2_plan(o.g, p.tensors[(size_t)a].len, p.tensors[(size_t)b].len);
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
    // the output is an entry of the table or zero, whatever the data (the index is masked): two planes when every entry fits them
    const std::vector<int64_t>& tab = p.consts[(size_t)o.table].own;
    o.out = new_tensor(C * R * K, std::all_of(tab.begin(), tab.end(), [](int64_t v) { return v >= 0 && v <= 16383; }) ? IQ_PLANES : IQ_NO);
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
      o.d[0] = infer_gemm2_plan(o.g, alen, blen);
      o.out = new_tensor(o.g.C * o.g.R * o.g.N, IQ_NO);
      p.ops.push_back(o); slot[id] = {o.out};
      continue;
    }
    if (l.kind == L_REQUANT) {
      o.kind = IO_REQUANT; o.left = l.fixed_point_multiplier; o.shift = l.shift(); o.bits = l.intermediate_bit_size;
      o.out = new_tensor(alen, IQ_YES);
    } else if (l.kind == L_RELU) { o.kind = IO_RELU; o.out = new_tensor(alen, infer_q_through(p.tensors[(size_t)a].q)); }
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
      o.kind = IO_MAXPOOL; o.d[0] = l.pin[0]; o.d[1] = l.pin[1]; o.d[2] = l.pin[2]; o.out = new_tensor(alen / 4, infer_q_through(p.tensors[(size_t)a].q));
    } else if (l.kind == L_CONV) {
      DP_REQUIRE(alen == l.kx * l.nw * l.nw, DP_ERR_SHAPE, "conv: input size mismatch");
      o.kind = IO_CONV; o.w = new_const(l.weights.data(), l.weights.size()); o.bias = new_const(l.bias.data(), l.bias.size());
      o.d[0] = l.kw; o.d[1] = l.kx; o.d[2] = l.real_nw; o.d[3] = l.nw; o.d[4] = l.unp_out[0]; o.d[5] = l.unp_out[1]; o.d[6] = l.unp_out[2];
      InferConvImage im = infer_conv_pack(l);
      o.d[7] = im.ra; o.g.K = im.K; o.jc = im.jc; p.consts[(size_t)o.w].w8 = std::move(im.w8);
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
  infer_range_plan(p);
  infer_fuse_plan(p);
  return p;
}
#endif

}  // namespace dp
