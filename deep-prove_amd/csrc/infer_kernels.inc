// Kernels and the batch runner of dp_model_infer (infer.h). Included by hip_dev.hip after HipDev; not part of kernels.inc (the SIMT-emulator
// build of tests/ cuts its kernels from there). Activations are [batch][tensor] int64, with an int8 copy next to every tensor whose values are
// known to lie within -128..127 (what a Requant writes, and what ReLU / MaxPool make of it): the int8 copies are the operands of k_infer_gemm_i8,
// k_infer_conv_i8 and k_infer_gemm2_i8. The probabilities of a Softmax (0..4096) have two int8 planes instead, the left operand of k_infer_gemm2_i8;
// so has a tensor the planner has bounded within -16384..16383 (infer_range_plan: GELU and Embeddings outputs and sums of such), the left operand of k_infer_gemm_i8_pl.
// Bad data (a Requant input beyond its bit size, a token outside the vocabulary, ...) refuses its sample: the chunk has one status word per
// sample, which the five kernels that can refuse data set with a vector atomic to the class (INFER_BAD_* of infer.h) of the first op that refused
// the sample; the host reads the words with the outputs. Ops run in stream order and the word only ever goes from zero to a class
// (compare-and-swap), so whatever later ops make of a refused sample's values cannot change it. Those values travel on; the guards that keep
// every kernel inside its tables and buffers on such data are named at each kernel. What a refused sample means for the call (dp_model_infer_ex:
// the call fails; dp_model_infer_checked: the input is refused) is decided on the host, in hip_infer_run. Every launch is finite; nothing here
// waits for the host. A Softmax (IO_SOFTMAX) splits the chunk's stream in two: the host reads the status words and the Softmax input, computes
// one shift per row of every sample not refused so far (InferProgram::shifts) and uploads words and shifts.

typedef int infer_v4i __attribute__((ext_vector_type(4)));
typedef int infer_v16i __attribute__((ext_vector_type(16)));
constexpr int IG_TM = 64, IG_TN = 64, IG_TK = 64, IG_LD = IG_TK + 16;  // tile of a workgroup (4 waves, 32 x 32 each); LDS row pitch in bytes

// Sample `s` is refused with class `cls` unless an earlier op (or an earlier wave of this one: same class) refused it. The plain
// load keeps the atomics of a sample that is bad everywhere to the few waves that run before the first of them lands
__device__ __forceinline__ void infer_refuse(unsigned* status, size_t s, unsigned cls) {
  if (__hip_atomic_load(status + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicCAS(status + s, 0u, cls);
}
// What an element-wise kernel does with `bad` (element i of a tensor of `per` words per sample; every lane of the wave that has an element calls
// it, in converged control flow): one wave-wide vote — nothing more on good data — and then one atomic per run of bad lanes and sample, from
// the first lane of the run (a wave of 64 consecutive elements can straddle samples)
__device__ __forceinline__ void infer_flag(bool bad, size_t i, size_t per, unsigned* status, unsigned cls) {
  const unsigned long long m = __ballot(bad);
  if (!m) return;
  const unsigned lane = threadIdx.x & 63;
  if (bad && (lane == 0 || !((m >> (lane - 1)) & 1) || i % per == 0)) infer_refuse(status, i / per, cls);
}
// The int8 forms of element i of a tensor whose values the planner has bounded (infer_range_plan, the Softmax table scan), beside its int64 form:
// o8 — the int8 copy (every value within -128..127) — or the two planes lo = v & 127 (0..127) and hi = v >> 7 (arithmetic: -128..127), so that
// v = 128 * hi + lo exactly for every v of -16384..16383; null pointers: the tensor has no such form in this call
__device__ __forceinline__ void infer_put_forms(int64_t v, size_t i, int8_t* __restrict__ o8, int8_t* __restrict__ lo, int8_t* __restrict__ hi) {
  if (o8) o8[i] = (int8_t)v;
  if (lo) { lo[i] = (int8_t)(v & 127); hi[i] = (int8_t)(v >> 7); }
}
// 16 consecutive int8 of row `row` of X[rows][K] from column k on, zeros outside the matrix. K % 16 == 0: one aligned 16-byte load
__device__ __forceinline__ infer_v4i infer_ld16(const int8_t* __restrict__ X, size_t rows, size_t K, size_t row, size_t k, bool k16) {
  infer_v4i v = {0, 0, 0, 0};
  if (row >= rows || k >= K) return v;
  if (k16) return *(const infer_v4i*)(X + row * K + k);
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; j++) if (k + j < K) w[j >> 2] |= (unsigned)(uint8_t)X[row * K + k + j] << (8 * (j & 3));
  v[0] = (int)w[0]; v[1] = (int)w[1]; v[2] = (int)w[2]; v[3] = (int)w[3];
  return v;
}
// C[M][N] (int64) = A[M][K] (int8) * Bt[N][K]^T (int8) + bias[N], exact: v_mfma_i32_32x32x32_i8 accumulates in 32 bits and the caller has checked
// K * 128 * 128 < 2^31. Operands are staged through LDS in K slices of 64; rows / columns / K beyond the matrices are zero-filled in registers
// before they reach LDS, nothing is read past a buffer. Lane l of a wave holds 16 consecutive k (16 * (l >> 5) ...) of row l & 31 of A and of
// column l & 31 of B: A and B fragments are cut from LDS by the SAME (lane half, byte) -> k rule, so the products pair up whatever order the
// instruction gives the 32 k of a step. D: column = l & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5).
__global__ __launch_bounds__(256) void k_infer_gemm_i8(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, const int64_t* __restrict__ bias, int64_t* __restrict__ C, size_t M, size_t K, size_t N) {
  __shared__ __attribute__((aligned(16))) int8_t As[IG_TM * IG_LD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[IG_TN * IG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t m0 = (size_t)blockIdx.x * IG_TM, n0 = (size_t)blockIdx.y * IG_TN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = tid >> 2, lc = (tid & 3) * 16;  // the 16 bytes of the slice this thread stages: tile row, byte column
  const bool k16 = (K & 15) == 0;
  infer_v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  for (size_t k0 = 0; k0 < K; k0 += IG_TK) {
    const infer_v4i a = infer_ld16(A, M, K, m0 + lr, k0 + lc, k16), b = infer_ld16(Bt, N, K, n0 + lr, k0 + lc, k16);
    __syncthreads();  // (the fragments of the slice before have been read)
    *(infer_v4i*)&As[lr * IG_LD + lc] = a;
    *(infer_v4i*)&Bs[lr * IG_LD + lc] = b;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < IG_TK / 32; s++) {
      const infer_v4i fa = *(const infer_v4i*)&As[(wm + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16];
      const infer_v4i fb = *(const infer_v4i*)&Bs[(wn + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16];
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
    }
  }
  const size_t col = n0 + wn + (lane & 31);
  if (col >= N) return;
  const int64_t bv = bias ? bias[col] : 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const size_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M) C[row * N + col] = (int64_t)acc[r] + bv;
  }
}
// the general product in 64-bit multiply-adds with the host's wrap-around (unsigned arithmetic): one output element per thread, n fastest.
// B is a constant (lenB = 0) or a tensor of the batch
__global__ __launch_bounds__(256) void k_infer_gemm_i64(const int64_t* __restrict__ A, size_t lenA, const int64_t* __restrict__ B, size_t lenB, const int64_t* __restrict__ bias,
                                                        int64_t* __restrict__ O, size_t lenO, size_t batch, InferGemmShape g) {
  const size_t per = g.C * g.R * g.N;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * per) return;
  const size_t b = i / per, e = i % per, n = e % g.N, r = (e / g.N) % g.R, c = e / (g.N * g.R);
  const int64_t* a = A + b * lenA + c * g.sAc + r * g.sAr;
  const int64_t* w = B + b * lenB + c * g.sBc + n * g.sBn;
  uint64_t acc = 0;
  for (size_t k = 0; k < g.K; k++) acc += (uint64_t)a[k * g.sAm] * (uint64_t)w[k * g.sBm];
  if (bias) acc += (uint64_t)bias[n];
  O[b * lenO + c * g.sOc + r * g.sOr + n * g.sOn] = (int64_t)acc;
}
// One thread's 16 bytes of a 64 x IG_TK operand slice of k_infer_gemm2_i8, as they will lie in LDS ([tile row][k], k contiguous). X: the int8
// matrix of one (sample, concat index), element (row, k) at X[row * sRow + k * sK] for row < rows and k < K; exactly one of the strides is 1.
// sK == 1: thread t holds k0 + 16 * (t & 3) ... + 15 of tile row t >> 2 — one 16-byte load when `wide`, else byte by byte.
// sRow == 1: thread t reads rows 4 * (t & 15) ... + 3 (one word when `wide`, else byte by byte) at each of k0 + 4 * (t >> 4) ... + 3, along the
// contiguous axis, and transposes the 4 x 4 bytes in registers: word i of the result is row 4 * (t & 15) + i, bytes k ... k + 3.
// Rows and k beyond the matrix are zeros and are not read; `wide` (infer_gemm2_plan) says the load is aligned and inside the matrix whenever its
// first byte is.
__device__ __forceinline__ infer_v4i infer_g2_load(const int8_t* __restrict__ X, size_t rows, size_t K, size_t sRow, size_t sK, size_t row0, size_t k0, bool wide, int tid) {
  infer_v4i v = {0, 0, 0, 0};
  if (sK == 1) {
    const size_t row = row0 + (size_t)(tid >> 2), k = k0 + (size_t)(tid & 3) * 16;
    if (row >= rows || k >= K) return v;
    const int8_t* p = X + row * sRow + k;
    if (wide) return *(const infer_v4i*)p;
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) if (k + j < K) w[j >> 2] |= (unsigned)(uint8_t)p[j] << (8 * (j & 3));
    v[0] = (int)w[0]; v[1] = (int)w[1]; v[2] = (int)w[2]; v[3] = (int)w[3];
    return v;
  }
  const size_t row = row0 + (size_t)(tid & 15) * 4, k = k0 + (size_t)(tid >> 4) * 4;
  if (row >= rows) return v;
  unsigned w[4] = {0, 0, 0, 0};  // w[j]: rows row ... row + 3 at k + j
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (k + j >= K) continue;
    const int8_t* p = X + (k + j) * sK + row;
    if (wide) w[j] = *(const unsigned*)p;
    else for (int i = 0; i < 4; i++) if (row + i < rows) w[j] |= (unsigned)(uint8_t)p[i] << (8 * i);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) v[i] = (int)(((w[0] >> (8 * i)) & 0xffu) | (((w[1] >> (8 * i)) & 0xffu) << 8) | (((w[2] >> (8 * i)) & 0xffu) << 16) | (((w[3] >> (8 * i)) & 0xffu) << 24));
  return v;
}
__device__ __forceinline__ void infer_g2_store(int8_t* S, infer_v4i v, bool k_major, int tid) {
  if (k_major) { *(infer_v4i*)&S[(tid >> 2) * IG_LD + (tid & 3) * 16] = v; return; }
#pragma unroll
  for (int i = 0; i < 4; i++) *(int*)&S[((tid & 15) * 4 + i) * IG_LD + (tid >> 4) * 4] = v[i];
}
// The product of two tensors of the batch on the i8 MFMA (IO_GEMM2: MatMul2, ConcatMatMul, Q K^T and probabilities x V of an Mha node), exact:
// out[b][c*sOc + r*sOr + n*sOn] = sum_m A[b][c*sAc + r*sAr + m*sAm] * B[b][c*sBc + m*sBm + n*sBn], A and B the int8 copies of the two tensors
// (lenA, lenB, lenO: words per sample), accumulated in 32 bits (infer_gemm2_plan has checked K * 128 * 128 < 2^31) and stored as int64 at any
// output strides. The problems are many and small, so a workgroup (4 waves, one 32 x 32 accumulator each) owns one IG_TM x IG_TN tile of ONE
// (sample, concat index): blockIdx.x = ((b * C + c) * tiles of R + tile of r) * tiles of N + tile of n, and a tile never crosses either. Each
// operand goes through LDS as [tile row][k] in K slices of IG_TK, whatever its layout in memory: infer_g2_load reads along the operand's
// contiguous axis (m, or r / n with a 4 x 4 byte transposition in registers) and zero-fills beyond R, N and K in registers, nothing is read past
// a matrix. Fragments are then 16 aligned bytes along k, and lane l holds k 16 * (l >> 5) ... of row l & 31 of A and of column l & 31 of B: both
// follow the SAME (lane half, byte) -> k rule, as in k_infer_gemm_i8. D: column = l & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5).
// PL: A is a two-plane tensor (values 0..16383: A = lo, A2 = hi = v >> 7, both 0..127): two accumulators over the same B fragment, the result
// (int64)acc_hi * 128 + acc_lo; each plane keeps the accumulator bound. A wave whose 32 x 32 block lies outside R x N multiplies and stores nothing.
template <bool PL> __global__ __launch_bounds__(256) void k_infer_gemm2_i8(const int8_t* __restrict__ A, const int8_t* __restrict__ A2, size_t lenA, const int8_t* __restrict__ B, size_t lenB,
                                                                           int64_t* __restrict__ O, size_t lenO, InferGemmShape g, unsigned tr, unsigned tn, unsigned flags) {
  __shared__ __attribute__((aligned(16))) int8_t As[(PL ? 2 : 1) * IG_TM * IG_LD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[IG_TN * IG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned t = blockIdx.x;
  const size_t n0 = (size_t)(t % tn) * IG_TN; t /= tn;
  const size_t r0 = (size_t)(t % tr) * IG_TM; t /= tr;
  const size_t c = t % (unsigned)g.C, b = t / (unsigned)g.C;
  const size_t offA = b * lenA + c * g.sAc;
  const int8_t* Bm = B + b * lenB + c * g.sBc;
  const bool a_k = !(flags & IG2_AT), b_k = !(flags & IG2_BT), a_w = flags & IG2_AW, b_w = flags & IG2_BW;
  const size_t sAr = a_k ? g.sAr : 1, sAm = a_k ? 1 : g.sAm, sBn = b_k ? g.sBn : 1, sBm = b_k ? 1 : g.sBm;  // (the unit stride as a constant)
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool live = r0 + wm < g.R && n0 + wn < g.N;  // (uniform in the wave)
  infer_v16i acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = acc2[r] = 0;
  for (size_t k0 = 0; k0 < g.K; k0 += IG_TK) {
    const infer_v4i a = infer_g2_load(A + offA, g.R, g.K, sAr, sAm, r0, k0, a_w, tid), bb = infer_g2_load(Bm, g.N, g.K, sBn, sBm, n0, k0, b_w, tid);
    infer_v4i a2 = {0, 0, 0, 0};
    if (PL) a2 = infer_g2_load(A2 + offA, g.R, g.K, sAr, sAm, r0, k0, a_w, tid);
    __syncthreads();  // (the fragments of the slice before have been read)
    infer_g2_store(As, a, a_k, tid);
    if (PL) infer_g2_store(As + IG_TM * IG_LD, a2, a_k, tid);
    infer_g2_store(Bs, bb, b_k, tid);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int s = 0; s < IG_TK / 32; s++) {
        const int at = (wm + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16;
        const infer_v4i fb = *(const infer_v4i*)&Bs[(wn + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&As[at], fb, acc, 0, 0, 0);
        if (PL) acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&As[IG_TM * IG_LD + at], fb, acc2, 0, 0, 0);
      }
    }
  }
  const size_t col = n0 + wn + (lane & 31);
  if (!live || col >= g.N) return;
  int64_t* op = O + b * lenO + c * g.sOc + col * g.sOn;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const size_t row = r0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < g.R) op[row * g.sOr] = PL ? (int64_t)acc2[r] * 128 + acc[r] : (int64_t)acc[r];
  }
}
// Requant::apply: (v * mult + 2^(sh-1)) >> sh clamped to +-127; |v| > 2^bits refuses the sample, as run_model refuses the input (per = words per
// sample). A refused sample's output is clamped like any other: its int8 copy stays a valid operand of k_infer_gemm_i8
__global__ __launch_bounds__(256) void k_infer_requant(const int64_t* __restrict__ x, int64_t* __restrict__ o, int8_t* __restrict__ o8, size_t n, int64_t mult, unsigned sh, unsigned bits,
                                                       unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = x[i];
  const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
  infer_flag(mag > (uint64_t(1) << bits), i, per, status, INFER_BAD_REQUANT);
  int64_t y = (int64_t)((uint64_t)v * (uint64_t)mult + (uint64_t(1) << (sh - 1))) >> sh;
  y = y < -127 ? -127 : y > 127 ? 127 : y;
  o[i] = y;
  if (o8) o8[i] = (int8_t)y;
}
__global__ __launch_bounds__(256) void k_infer_relu(const int64_t* __restrict__ x, int64_t* __restrict__ o, int8_t* __restrict__ o8, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = x[i] < 0 ? 0 : x[i];
  o[i] = v;
  if (o8) o8[i] = (int8_t)v;
}
// A Dense / MatMul / QKV product with the Requant behind it (and the ReLU behind that: RELU) in ONE launch: C = A[M][K] (int8) * Bt[N][K]^T (int8)
// + bias[N] on v_mfma_i32_32x32x32_i8, exact under the rule of weight_const (K * 128 * 128 < 2^31), then in registers what k_infer_requant does,
// letter for letter: |v| > 2^bits refuses the sample, (v * mult + 2^(sh-1)) >> sh with the multiply and add in unsigned 64-bit arithmetic and an
// arithmetic shift, clamp to +-127; then max(., 0). O8 — the int8 copy of the chain's LAST tensor — is always written, its int64 form O64 only
// under W64 (infer_needs_int64); the int64 product and the Requant's tensor under a ReLU are never written. 1 byte per element instead of 42.
// Staging: the operands go through LDS in K slices of RQ_TK = 128 (four MFMA per wave between two barriers; k_infer_gemm_i8: two). A thread
//   stages 2 x 16 bytes of each operand and holds the NEXT slice's 64 bytes in registers: their global loads are issued right behind the
//   barrier that publishes the current slice and are in flight while it is multiplied. One LDS buffer, not two: the second costs as much LDS
//   as the registers cost nothing (below), and the store of a prefetched slice is 4 ds_write_b128 per thread. MFMA steps beyond K are skipped.
// Tile: 64 x 64 per workgroup of 4 waves (32 x 32 each), as k_infer_gemm_i8. The shapes that matter are M = batch x rows in the thousands with
//   N = 256 .. 1024 (the transformer layer at 320 inputs: M * N / 4096 = a few hundred tiles for 256 CUs) and N = 3 .. 10 (the last Dense of
//   Dense-4M and CNN-264k: one column tile). A 128-row tile would halve the traffic of Bt but leave half the CUs without a workgroup on the
//   former and change nothing on the latter; 64 x 64 keeps 16 accumulator registers and 18 KB of LDS, so several workgroups share a CU and one's
//   epilogue and prefetch latency hide under another's MFMA.
// Epilogue: lane l holds one column and 16 rows of D (column = l & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)). The requantised tile goes
//   through LDS as [64][RQ_LDC] bytes — the operand buffers are free behind a barrier after the last slice — and leaves row-contiguous: O8 in
//   16-byte vectors where N % 16 == 0 (the int8 copy of a tensor starts 256-aligned, its row pitch is N, a column tile starts at a multiple of
//   64), bytes otherwise; O64 in 16-byte pairs where N is even, words otherwise, consecutive lanes at consecutive addresses.
// Refusal: row `row` belongs to sample row / R (R = o.g.R; M = samples x R). A lane ORs its 16 tests into a mask; ONE ballot per wave decides,
//   and only a wave with a bad element walks its masks to infer_refuse (INFER_BAD_REQUANT). Rows >= M, columns >= N and k >= K are zero-filled
//   in registers before they reach LDS (infer_ld16; nothing is read past a matrix) and are never tested, stored or flagged. A refused sample's
//   output is clamped like any other: its int8 copy stays a valid operand (the invariant of k_infer_requant).
// Fragments: as k_infer_gemm_i8 — lane l holds 16 consecutive k (16 * (l >> 5) ...) of row l & 31 of A and of column l & 31 of B, the SAME rule.
constexpr int RQ_TK = 128, RQ_LD = RQ_TK + 16, RQ_LDC = IG_TN + 16;  // K slice, LDS row pitch of the operands and of the result tile, in bytes
typedef long long infer_v2l __attribute__((ext_vector_type(2)));
template <bool RELU, bool W64> __global__ __launch_bounds__(256) void k_infer_gemm_i8_rq(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, const int64_t* __restrict__ bias, int8_t* __restrict__ O8,
                                                                                      int64_t* __restrict__ O64, size_t M, size_t K, size_t N, int64_t mult, unsigned sh, unsigned bits, unsigned* status, size_t R) {
  __shared__ __attribute__((aligned(16))) int8_t lds[(IG_TM + IG_TN) * RQ_LD];
  int8_t* As = lds; int8_t* Bs = lds + IG_TM * RQ_LD; int8_t* Cs = lds;  // (Cs: [IG_TM][RQ_LDC], after the last slice)
  static_assert(IG_TM * RQ_LDC <= (IG_TM + IG_TN) * RQ_LD && IG_TM == 64 && IG_TN == 64, "the result tile lies in the operand buffers");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t m0 = (size_t)blockIdx.x * IG_TM, n0 = (size_t)blockIdx.y * IG_TN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = tid >> 3, lc = (tid & 7) * 16;  // the bytes of a slice this thread stages: tile rows lr and lr + 32, byte column lc
  const bool k16 = (K & 15) == 0;
  infer_v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  infer_v4i a0 = infer_ld16(A, M, K, m0 + lr, lc, k16), a1 = infer_ld16(A, M, K, m0 + lr + 32, lc, k16);
  infer_v4i b0 = infer_ld16(Bt, N, K, n0 + lr, lc, k16), b1 = infer_ld16(Bt, N, K, n0 + lr + 32, lc, k16);
  for (size_t k0 = 0; k0 < K; k0 += RQ_TK) {
    __syncthreads();  // (the fragments of the slice before have been read)
    *(infer_v4i*)&As[lr * RQ_LD + lc] = a0; *(infer_v4i*)&As[(lr + 32) * RQ_LD + lc] = a1;
    *(infer_v4i*)&Bs[lr * RQ_LD + lc] = b0; *(infer_v4i*)&Bs[(lr + 32) * RQ_LD + lc] = b1;
    __syncthreads();
    const size_t kn = k0 + RQ_TK + lc;  // the next slice: zeros, and no load, at kn >= K
    a0 = infer_ld16(A, M, K, m0 + lr, kn, k16); a1 = infer_ld16(A, M, K, m0 + lr + 32, kn, k16);
    b0 = infer_ld16(Bt, N, K, n0 + lr, kn, k16); b1 = infer_ld16(Bt, N, K, n0 + lr + 32, kn, k16);
#pragma unroll
    for (int s = 0; s < RQ_TK / 32; s++) {
      if (k0 + s * 32 < K) {  // (uniform)
        const infer_v4i fa = *(const infer_v4i*)&As[(wm + (lane & 31)) * RQ_LD + s * 32 + (lane >> 5) * 16];
        const infer_v4i fb = *(const infer_v4i*)&Bs[(wn + (lane & 31)) * RQ_LD + s * 32 + (lane >> 5) * 16];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
      }
    }
  }
  __syncthreads();  // (every wave has read its last fragments: the operand buffers become the result tile)
  const size_t col = n0 + wn + (lane & 31);
  const uint64_t bv = bias && col < N ? (uint64_t)bias[col] : 0, lim = uint64_t(1) << bits;
  unsigned bad = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int tr = wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int64_t v = (int64_t)((uint64_t)(int64_t)acc[r] + bv);
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (mag > lim && m0 + tr < M && col < N) bad |= 1u << r;
    int64_t y = (int64_t)((uint64_t)v * (uint64_t)mult + (uint64_t(1) << (sh - 1))) >> sh;
    y = y < -127 ? -127 : y > 127 ? 127 : y;
    if (RELU) y = y < 0 ? 0 : y;
    Cs[tr * RQ_LDC + wn + (lane & 31)] = (int8_t)y;
  }
  if (__ballot(bad != 0)) {
#pragma unroll
    for (int r = 0; r < 16; r++) if ((bad >> r) & 1) infer_refuse(status, (m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) / R, INFER_BAD_REQUANT);
  }
  __syncthreads();
  if ((N & 15) == 0) {  // one 16-byte vector of a row per thread
    const size_t row = m0 + (tid >> 2), c = n0 + (tid & 3) * 16;
    if (row < M && c < N) *(infer_v4i*)(O8 + row * N + c) = *(const infer_v4i*)&Cs[(tid >> 2) * RQ_LDC + (tid & 3) * 16];
  } else {
    for (int i = tid; i < IG_TM * IG_TN; i += 256) {
      const size_t row = m0 + (i >> 6), c = n0 + (i & 63);
      if (row < M && c < N) O8[row * N + c] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
    }
  }
  if (!W64) return;
  if ((N & 1) == 0) {  // (the int64 form of a tensor starts 256-aligned: an even column of any row is 16-aligned)
    for (int i = tid; i < IG_TM * IG_TN / 2; i += 256) {
      const size_t row = m0 + (i >> 5), c = n0 + (i & 31) * 2;
      const int8_t* y = &Cs[(i >> 5) * RQ_LDC + (i & 31) * 2];
      if (row < M && c < N) { infer_v2l v; v[0] = y[0]; v[1] = y[1]; *(infer_v2l*)(O64 + row * N + c) = v; }
    }
  } else {
    for (int i = tid; i < IG_TM * IG_TN; i += 256) {
      const size_t row = m0 + (i >> 6), c = n0 + (i & 63);
      if (row < M && c < N) O64[row * N + c] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
    }
  }
}
// The constant product on a TWO-PLANE left operand (IQ_PLANES: values within -16384..16383 as lo = v & 127 and hi = v >> 7, v = 128 * hi + lo):
// C = (128 * Ahi + Alo)[M][K] * Bt[N][K]^T + bias[N], exact — each plane is an int8 matrix, so each of the two 32-bit accumulators keeps the
// bound K * 128 * 128 < 2^31 of weight_const, and v = 128 * (int64)acc_hi + acc_lo + bias is formed in 64 bits. Served in both shapes of the
// launcher: RQ = false is the contract of k_infer_gemm_i8 (the int64 result to O64), RQ = true that of k_infer_gemm_i8_rq (bias + Requant
// (+ ReLU: RELU), O8 always, O64 under W64, refusal through infer_refuse with INFER_BAD_REQUANT), its epilogue letter for letter on v.
// One launch, not one per plane: a workgroup (4 waves, 64 x 64 tile, 32 x 32 per wave) stages BOTH planes of its A slice and ONE Bt slice through
//   LDS; a wave holds two accumulators and issues two v_mfma_i32_32x32x32_i8 per Bt fragment — three LDS fragment reads per two MFMA where the
//   one-plane kernels do two per MFMA, and Bt (the operand every row tile re-reads) crosses global memory and LDS once, not twice.
// Staging: K slices of PL_TK = 128 at row pitch PL_LD, the NEXT slice's 6 x 16 bytes per thread prefetched into registers right behind the
//   barrier that publishes the current one (k_infer_gemm_i8_rq's scheme with a third operand). LDS: (2 * 64 + 64) * 144 = 27648 bytes, five
//   workgroups per CU; a slice of 64 would double the barriers per MFMA for an LDS the 32 accumulator registers do not let more waves use.
//   The result tile of the fused shape lies in the operand buffers behind a barrier, [64][RQ_LDC] bytes.
// Fragments: as k_infer_gemm_i8 — lane l holds 16 consecutive k (16 * (l >> 5) ...) of row l & 31 of both planes of A and of column l & 31 of B,
//   the SAME (lane half, byte) -> k rule for the three. Rows >= M, columns >= N and k >= K are zero-filled in registers before they reach LDS
//   (infer_ld16; nothing is read past a matrix) and are never tested, stored or flagged; MFMA steps beyond K are skipped.
constexpr int PL_TK = 128, PL_LD = PL_TK + 16;
template <bool RQ, bool RELU, bool W64> __global__ __launch_bounds__(256) void k_infer_gemm_i8_pl(const int8_t* __restrict__ Alo, const int8_t* __restrict__ Ahi, const int8_t* __restrict__ Bt, const int64_t* __restrict__ bias,
                                                                                               int8_t* __restrict__ O8, int64_t* __restrict__ O64, size_t M, size_t K, size_t N, int64_t mult, unsigned sh, unsigned bits,
                                                                                               unsigned* status, size_t R) {
  __shared__ __attribute__((aligned(16))) int8_t lds[(2 * IG_TM + IG_TN) * PL_LD];
  int8_t* Al = lds; int8_t* Ah = lds + IG_TM * PL_LD; int8_t* Bs = lds + 2 * IG_TM * PL_LD; int8_t* Cs = lds;  // (Cs: [IG_TM][RQ_LDC], after the last slice)
  static_assert(IG_TM * RQ_LDC <= (2 * IG_TM + IG_TN) * PL_LD && IG_TM == 64 && IG_TN == 64 && PL_TK % 32 == 0, "the result tile lies in the operand buffers");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t m0 = (size_t)blockIdx.x * IG_TM, n0 = (size_t)blockIdx.y * IG_TN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = tid >> 3, lc = (tid & 7) * 16;  // the bytes of a slice this thread stages: tile rows lr and lr + 32, byte column lc
  const bool k16 = (K & 15) == 0;
  infer_v16i acc, acc2;  // lo plane, hi plane
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = acc2[r] = 0;
  infer_v4i l0 = infer_ld16(Alo, M, K, m0 + lr, lc, k16), l1 = infer_ld16(Alo, M, K, m0 + lr + 32, lc, k16);
  infer_v4i h0 = infer_ld16(Ahi, M, K, m0 + lr, lc, k16), h1 = infer_ld16(Ahi, M, K, m0 + lr + 32, lc, k16);
  infer_v4i b0 = infer_ld16(Bt, N, K, n0 + lr, lc, k16), b1 = infer_ld16(Bt, N, K, n0 + lr + 32, lc, k16);
  for (size_t k0 = 0; k0 < K; k0 += PL_TK) {
    __syncthreads();  // (the fragments of the slice before have been read)
    *(infer_v4i*)&Al[lr * PL_LD + lc] = l0; *(infer_v4i*)&Al[(lr + 32) * PL_LD + lc] = l1;
    *(infer_v4i*)&Ah[lr * PL_LD + lc] = h0; *(infer_v4i*)&Ah[(lr + 32) * PL_LD + lc] = h1;
    *(infer_v4i*)&Bs[lr * PL_LD + lc] = b0; *(infer_v4i*)&Bs[(lr + 32) * PL_LD + lc] = b1;
    __syncthreads();
    const size_t kn = k0 + PL_TK + lc;  // the next slice: zeros, and no load, at kn >= K
    l0 = infer_ld16(Alo, M, K, m0 + lr, kn, k16); l1 = infer_ld16(Alo, M, K, m0 + lr + 32, kn, k16);
    h0 = infer_ld16(Ahi, M, K, m0 + lr, kn, k16); h1 = infer_ld16(Ahi, M, K, m0 + lr + 32, kn, k16);
    b0 = infer_ld16(Bt, N, K, n0 + lr, kn, k16); b1 = infer_ld16(Bt, N, K, n0 + lr + 32, kn, k16);
#pragma unroll
    for (int s = 0; s < PL_TK / 32; s++) {
      if (k0 + s * 32 < K) {  // (uniform)
        const int at = (wm + (lane & 31)) * PL_LD + s * 32 + (lane >> 5) * 16;
        const infer_v4i fb = *(const infer_v4i*)&Bs[(wn + (lane & 31)) * PL_LD + s * 32 + (lane >> 5) * 16];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&Al[at], fb, acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&Ah[at], fb, acc2, 0, 0, 0);
      }
    }
  }
  const size_t col = n0 + wn + (lane & 31);
  const uint64_t bv = bias && col < N ? (uint64_t)bias[col] : 0;
  if (!RQ) {  // the contract of k_infer_gemm_i8
    if (col >= N) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const size_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row < M) O64[row * N + col] = (int64_t)((uint64_t)((int64_t)acc2[r] * 128 + (int64_t)acc[r]) + bv);
    }
    return;
  }
  __syncthreads();  // (every wave has read its last fragments: the operand buffers become the result tile)
  const uint64_t lim = uint64_t(1) << bits;
  unsigned bad = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int tr = wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int64_t v = (int64_t)((uint64_t)((int64_t)acc2[r] * 128 + (int64_t)acc[r]) + bv);
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (mag > lim && m0 + tr < M && col < N) bad |= 1u << r;
    int64_t y = (int64_t)((uint64_t)v * (uint64_t)mult + (uint64_t(1) << (sh - 1))) >> sh;
    y = y < -127 ? -127 : y > 127 ? 127 : y;
    if (RELU) y = y < 0 ? 0 : y;
    Cs[tr * RQ_LDC + wn + (lane & 31)] = (int8_t)y;
  }
  if (__ballot(bad != 0)) {
#pragma unroll
    for (int r = 0; r < 16; r++) if ((bad >> r) & 1) infer_refuse(status, (m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) / R, INFER_BAD_REQUANT);
  }
  __syncthreads();
  if ((N & 15) == 0) {  // one 16-byte vector of a row per thread
    const size_t row = m0 + (tid >> 2), c = n0 + (tid & 3) * 16;
    if (row < M && c < N) *(infer_v4i*)(O8 + row * N + c) = *(const infer_v4i*)&Cs[(tid >> 2) * RQ_LDC + (tid & 3) * 16];
  } else {
    for (int i = tid; i < IG_TM * IG_TN; i += 256) {
      const size_t row = m0 + (i >> 6), c = n0 + (i & 63);
      if (row < M && c < N) O8[row * N + c] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
    }
  }
  if (!W64) return;
  if ((N & 1) == 0) {  // (the int64 form of a tensor starts 256-aligned: an even column of any row is 16-aligned)
    for (int i = tid; i < IG_TM * IG_TN / 2; i += 256) {
      const size_t row = m0 + (i >> 5), c = n0 + (i & 31) * 2;
      const int8_t* y = &Cs[(i >> 5) * RQ_LDC + (i & 31) * 2];
      if (row < M && c < N) { infer_v2l v; v[0] = y[0]; v[1] = y[1]; *(infer_v2l*)(O64 + row * N + c) = v; }
    }
  } else {
    for (int i = tid; i < IG_TM * IG_TN; i += 256) {
      const size_t row = m0 + (i >> 6), c = n0 + (i & 63);
      if (row < M && c < N) O64[row * N + c] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
    }
  }
}
// Add with a static operand / Positional::Learned: left * x + right * w[i mod len] (w: the operand, or the first rows of the table).
// o8 / lo, hi (here and in k_infer_add2, k_infer_embed, k_infer_gelu): the int8 forms of the output, infer_put_forms
__global__ __launch_bounds__(256) void k_infer_addc(const int64_t* __restrict__ x, const int64_t* __restrict__ w, int64_t* __restrict__ o, int8_t* __restrict__ o8, int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                    size_t n, size_t len, int64_t left, int64_t right) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = (int64_t)((uint64_t)left * (uint64_t)x[i] + (uint64_t)right * (uint64_t)w[i % len]);
  o[i] = v;
  infer_put_forms(v, i, o8, lo, hi);
}
__global__ __launch_bounds__(256) void k_infer_add2(const int64_t* __restrict__ x, const int64_t* __restrict__ y, int64_t* __restrict__ o, int8_t* __restrict__ o8, int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                    size_t n, int64_t left, int64_t right) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = (int64_t)((uint64_t)left * (uint64_t)x[i] + (uint64_t)right * (uint64_t)y[i]);
  o[i] = v;
  infer_put_forms(v, i, o8, lo, hi);
}
// Embeddings: row tok[t] of the [vocab][emb] table for every token; a token outside the vocabulary refuses the sample (per = output words per
// sample) and reads row 0: the table is never read outside its rows, whatever the token
__global__ __launch_bounds__(256) void k_infer_embed(const int64_t* __restrict__ tok, const int64_t* __restrict__ table, int64_t* __restrict__ o, int8_t* __restrict__ o8, int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                     size_t n, size_t vocab, size_t emb, unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t t = tok[i / emb];
  const bool bad = t < 0 || (uint64_t)t >= vocab;
  infer_flag(bad, i, per, status, INFER_BAD_TOKEN);
  if (bad) t = 0;
  const int64_t v = table[(size_t)t * emb + i % emb];
  o[i] = v;
  infer_put_forms(v, i, o8, lo, hi);
}
// MaxPool 2 x 2, stride 2, on [batch][c][h][w]
__global__ __launch_bounds__(256) void k_infer_maxpool(const int64_t* __restrict__ x, int64_t* __restrict__ o, int8_t* __restrict__ o8, size_t n, size_t h, size_t w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t ow = w / 2, oh = h / 2, j = i % ow, r = (i / ow) % oh, plane = i / (ow * oh);  // plane = b * c + channel
  const int64_t* p = x + plane * h * w + 2 * r * w + 2 * j;
  const int64_t a = p[0] > p[1] ? p[0] : p[1], b = p[w] > p[w + 1] ? p[w] : p[w + 1], v = a > b ? a : b;
  o[i] = v;
  if (o8) o8[i] = (int8_t)v;
}
// Convolution::op on the padded tensors: the correlation the host's FFT product computes — on the FLAT index of a channel plane (offset a * nw + b,
// terms that leave the plane dropped) —, + bias, then clear_garbage (zero outside the unpadded output shape). One output element per thread.
__global__ __launch_bounds__(256) void k_infer_conv(const int64_t* __restrict__ x, const int64_t* __restrict__ f, const int64_t* __restrict__ bias, int64_t* __restrict__ o, size_t n,
                                                    size_t kw, size_t kx, size_t rn, size_t nw, size_t u0, size_t u1, size_t u2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t nn = nw * nw, p = i % nn, ch = (i / nn) % kw, b = i / (nn * kw), yy = p / nw, xx = p % nw;
  if (!(ch < u0 && yy < u1 && xx < u2)) { o[i] = 0; return; }
  uint64_t acc = (uint64_t)bias[ch];
  for (size_t j = 0; j < kx; j++) {
    const int64_t* xp = x + (b * kx + j) * nn;
    const int64_t* fp = f + (ch * kx + j) * rn * rn;
    for (size_t a = 0; a < rn; a++) for (size_t c = 0; c < rn; c++) { const size_t q = p + a * nw + c; if (q < nn) acc += (uint64_t)xp[q] * (uint64_t)fp[a * rn + c]; }
  }
  o[i] = (int64_t)acc;
}
// The pixel-side fragment of k_infer_conv_i8: the lane's 16 consecutive k are 16 / RN filter rows of RN columns, and the RN inputs under row
// q are RN consecutive bytes of the staged span, from byte 4 * (tab[q] + wl) + sh on (wl, sh: the lane's pixel of the strip, as a word and the
// byte within it). They are cut from whole aligned LDS words with v_alignbyte_b32, whatever sh is. RN == 2: eight rows of two bytes, two rows
// packed per register with v_perm_b32; RN == 16: one row, five words, four cuts
template <int RN> __device__ __forceinline__ infer_v4i infer_conv_frag(const unsigned* xs, const unsigned* tab, unsigned q, unsigned wl, unsigned sh) {
  infer_v4i v;
  if (RN == 2) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const unsigned* w0 = xs + tab[q + 2 * r] + wl;
      const unsigned* w1 = xs + tab[q + 2 * r + 1] + wl;
      v[r] = (int)__builtin_amdgcn_perm(__builtin_amdgcn_alignbyte(w1[1], w1[0], sh), __builtin_amdgcn_alignbyte(w0[1], w0[0], sh), 0x05040100u);
    }
    return v;
  }
  if (RN == 16) {
    const unsigned* w = xs + tab[q] + wl;
    unsigned lo = w[0];
#pragma unroll
    for (int i = 0; i < 4; i++) { const unsigned hi = w[i + 1]; v[i] = (int)__builtin_amdgcn_alignbyte(hi, lo, sh); lo = hi; }
    return v;
  }
#pragma unroll
  for (int r = 0; r < 16 / RN; r++) {
    const unsigned* w = xs + tab[q + r] + wl;
    if (RN == 4) v[r] = (int)__builtin_amdgcn_alignbyte(w[1], w[0], sh);
    else { const unsigned w1 = w[1]; v[2 * r] = (int)__builtin_amdgcn_alignbyte(w1, w[0], sh); v[2 * r + 1] = (int)__builtin_amdgcn_alignbyte(w[2], w1, sh); }
  }
  return v;
}
// The staging and the MFMA loop of a live workgroup of k_infer_conv_i8 / k_infer_conv_i8_rq (described at the former): the row table and the kx
// spans go to LDS once, the filter tile in K slices of IC_TK; acc += the 32 channels x 32 pixels of the wave. Called by every thread of the
// workgroup (it holds barriers); the last fragments of As may still be read by another wave when it returns
template <int RN> __device__ __forceinline__ void infer_conv_tile(infer_v16i& acc, const int8_t* __restrict__ x, const int8_t* __restrict__ f, int8_t* As, unsigned* tab, unsigned* xs, unsigned b, unsigned p0,
                                                                  unsigned ch0, unsigned tid, unsigned half, unsigned l31, unsigned pl, bool wave_live, unsigned kw, unsigned kx, unsigned ra, unsigned K,
                                                                  unsigned nw) {
  const unsigned nn = nw * nw, pw = infer_conv_pitch(nw, ra, RN) / 4;  // (the pitch of a span in words)
  for (unsigned q = tid; q < K / RN; q += 256) tab[q] = q < kx * ra ? q / ra * pw + q % ra * (nw / 4) : 0;
  for (unsigned i = tid; i < kx * pw; i += 256) {
    const unsigned j = i / pw, at = p0 + 4 * (i % pw);
    xs[i] = at < nn ? *(const unsigned*)(x + ((size_t)b * kx + j) * nn + at) : 0u;
  }
  const unsigned lr = tid >> 3, lc = (tid & 7) * 16;  // the 16 bytes of the filter slice this thread stages: tile row, byte column
  for (unsigned k0 = 0; k0 < K; k0 += IC_TK) {
    infer_v4i a = {0, 0, 0, 0};
    if (ch0 + lr < kw && k0 + lc < K) a = *(const infer_v4i*)(f + (size_t)(ch0 + lr) * K + k0 + lc);
    __syncthreads();  // (the fragments of the slice before have been read)
    *(infer_v4i*)&As[lr * IC_LDA + lc] = a;
    __syncthreads();  // (the first one: the spans and the table are in LDS, too)
    if (wave_live) {
#pragma unroll
      for (unsigned s = 0; s < IC_TK / 32; s++) {
        if (k0 + s * 32 < K) {
          const infer_v4i fa = *(const infer_v4i*)&As[l31 * IC_LDA + s * 32 + half * 16];
          const infer_v4i fb = infer_conv_frag<RN>(xs, tab, (k0 + s * 32 + half * 16) / RN, pl >> 2, pl & 3);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        }
      }
    }
  }
}
// infer_conv_tile for a pointwise layer (RN == 1: k = j, K = kx rounded up to 32): out[b][ch][p] = sum over j of f[ch][j] * x[b][j][p] is a GEMM whose
// tensor operand is contiguous along the PIXELS, so there are no spans and no row table (infer_conv_tab_words(K, 1) == 0): BOTH operands go through
// LDS in K slices of IC_TK = 128 input channels, the filter tile into As as before, the inputs into Xs = [IC_TP pixels][IC_TK k] at row pitch
// IC_LDA = 144 bytes, right behind As: IC_TC * IC_LDA + IC_TP * IC_LDA = 23040 bytes whatever kx is (infer_conv_lds).
// Staging the inputs: a slice is 32 pixel quads x 32 channel quads of 4 x 4 bytes, four per thread. A wave takes 16 consecutive pixel quads (lanes
// 0..15: 64 consecutive bytes of one channel's plane per load) x 4 consecutive channel quads; a thread loads the aligned word of its 4 pixels from
// each of 4 consecutive channels, transposes the 4 x 4 bytes in registers (v_perm_b32, 8 per quad) and writes four words of 4 channels x 1 pixel
// to Xs[pixel][4 cq ...]. Channels >= kx (the K padding and the rest of the last slice) and pixels >= nn are zeros in registers and are not read
// from memory, filter rows >= kw and columns >= K likewise: nn is a multiple of 4 (infer_conv_pack), so a word at pixel 4 pq < nn of channel
// j < kx of sample b < batch lies within x, and a 16-byte read of f at row < kw, column < K (a multiple of 32) within the image.
// Banks: a row of 36 words. The fragment of a lane is ONE 16-byte read at word 36 * pixel + 8 s + 4 half; over 16 consecutive pixels 36 p mod 64
// = 4 * (9 p mod 16) takes 16 different values: each quarter wave covers the 64 banks once. The transposed store of pixel 4 pq + i, channel quad
// cq is word 36 * (4 pq + i) + cq = 16 pq + 36 i + cq (mod 64): with the same i in every lane the 16 pixel quads of a wave would share 4 banks.
// So lane rotates its words by r = (pq >> 2) & 3 bytes (v_alignbyte_b32) before the transposition and its t-th store is pixel i = (t + r) & 3:
// 16 (pq & 3) + 36 ((t + r) & 3) takes 16 values, all multiples of 4, and the 4 channel quads of the wave fill the words between them — the 64
// lanes of a store hit 64 different banks. No prefetch into registers: the 16 words of the next slice would have to live across the MFMA steps;
// the loads are issued in front of the barrier instead, while other waves still multiply the slice before.
template <> __device__ __forceinline__ void infer_conv_tile<1>(infer_v16i& acc, const int8_t* __restrict__ x, const int8_t* __restrict__ f, int8_t* As, unsigned*, unsigned* xs, unsigned b, unsigned p0,
                                                                unsigned ch0, unsigned tid, unsigned half, unsigned l31, unsigned pl, bool wave_live, unsigned kw, unsigned kx, unsigned, unsigned K,
                                                                unsigned nw) {
  int8_t* Xs = (int8_t*)xs;
  const unsigned nn = nw * nw;
  const unsigned lr = tid >> 3, lc = (tid & 7) * 16;                            // the 16 bytes of the filter slice this thread stages: tile row, byte column
  const unsigned pq = (tid & 15) | ((tid >> 2) & 16), cq0 = ((tid >> 4) & 3) | ((tid >> 5) & 4);  // its pixel quad (0..31) and the first of its four channel quads (cq0 + 8 u)
  const unsigned rot = (pq >> 2) & 3;
  const bool px = p0 + 4 * pq < nn;
  const int8_t* xp = x + (size_t)b * kx * nn + p0 + 4 * pq;
  for (unsigned k0 = 0; k0 < K; k0 += IC_TK) {
    infer_v4i a = {0, 0, 0, 0};
    if (ch0 + lr < kw && k0 + lc < K) a = *(const infer_v4i*)(f + (size_t)(ch0 + lr) * K + k0 + lc);
    unsigned w[4][4];  // w[u][i]: the 4 pixels of channel k0 + 4 * (cq0 + 8 u) + i
#pragma unroll
    for (int u = 0; u < 4; u++) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const unsigned j = k0 + 4 * (cq0 + 8 * u) + i;
        w[u][i] = px && j < kx ? *(const unsigned*)(xp + (size_t)j * nn) : 0u;
      }
    }
    __syncthreads();  // (the fragments of the slice before have been read)
    *(infer_v4i*)&As[lr * IC_LDA + lc] = a;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      unsigned r[4];
#pragma unroll
      for (int i = 0; i < 4; i++) r[i] = __builtin_amdgcn_alignbyte(w[u][i], w[u][i], rot);  // byte t = pixel (t + rot) & 3
      const unsigned lo01 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);
      const unsigned lo23 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
      const unsigned t4[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u), __builtin_amdgcn_perm(hi23, hi01, 0x05040100u),
                              __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};  // t4[t]: channels i = 0..3 (byte i) of pixel (t + rot) & 3
#pragma unroll
      for (unsigned t = 0; t < 4; t++) *(unsigned*)&Xs[(4 * pq + ((t + rot) & 3)) * IC_LDA + 4 * (cq0 + 8 * u)] = t4[t];
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll
      for (unsigned s = 0; s < IC_TK / 32; s++) {
        if (k0 + s * 32 < K) {
          const infer_v4i fa = *(const infer_v4i*)&As[l31 * IC_LDA + s * 32 + half * 16];
          const infer_v4i fb = *(const infer_v4i*)&Xs[pl * IC_LDA + s * 32 + half * 16];
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        }
      }
    }
  }
}
// infer_conv_tile in channel slices (RN >= 2), for the layers whose kx spans do not fit the LDS (infer_conv_pack): the same products in the same
// order of k, but the input channels go through LDS jc = infer_conv_slice(kx, nw, ra, RN) at a time — jc * ra * RN consecutive k of the image, a
// whole number of filter K slices, and K = kx * ra * RN has no padding. LDS behind As: the row table of ONE slice, jc * ra words (tab[q] = q / ra *
// pw + q % ra * (nw / 4) does not depend on the slice: written once), then two span buffers of jc * pw words each, rounded up to whole rounds of 256
// words (infer_conv_lds with jc).
// Staging: a slice is jc * pw <= 4096 words = nt <= 16 rounds of the workgroup, and a thread owns words tid + 256 t, t < nt, of every slice:
// where[t] = the word's byte offset from the slice's first span in x, worked out once (no division in the loop; jc <= 64 and nn <= 2^24 keep it
// below 2^31), and keep[t] = all ones. A word past the slice (the padding of the last round, which no fragment reads) or at a pixel >= nn (which
// must be zero) has keep[t] = 0 and reads the strip's first word in the slice's first channel instead: every lane loads, ANDs and stores in every
// round, so no lane mask lives across the slice loop (sixteen of them would not fit the scalar registers; keep is opaque to the compiler for that
// reason), and t < nt is a scalar test. The loads of slice s + 1 are issued in front of the MFMA steps of slice s into 16 registers, which live
// across the steps, and are stored into the other buffer behind them. The hand-over has no barrier of its own: a wave stores slice s + 1 after the barriers
// of the LAST filter slice of slice s, which every wave passes only behind its last fragment of slice s - 1 — the buffer's readers are done —, and
// the two barriers of the first filter slice of slice s + 1 lie between these stores and the first fragment cut from them. Within a slice the
// filter tile goes through As in K slices of IC_TK exactly as in infer_conv_tile; the fragment rule is infer_conv_frag on the slice's own q.
// In bounds: word t of a slice is channel s * jc + i / pw < kx (i < jc * pw, s < kx / jc, kx a multiple of jc) at pixel p0 + 4 * (i % pw) < nn
// (checked; words at or beyond nn are zeros in registers and are not read: their lanes read offset 0, pixel p0 < nn of channel s * jc): a whole
// aligned word of x, as nn is a multiple of 4. A store of round t < nt lands at word tid + 256 t < 256 nt of the slice's own buffer. The 16-byte reads
// of f lie at row < kw and column s * ks + k0 + lc + 15 < K. LDS: table and buffers as sized by infer_conv_lds; a fragment reads tab[q .. q + 16 /
// RN) with q + 16 / RN <= jc * ra (ks is a multiple of 128) and span words within one pitch of its row's span, as in the whole-span form.
template <int RN> __device__ __forceinline__ void infer_conv_tile_sl(infer_v16i& acc, const int8_t* __restrict__ x, const int8_t* __restrict__ f, int8_t* As, unsigned* tab, unsigned b, unsigned p0,
                                                                     unsigned ch0, unsigned tid, unsigned half, unsigned l31, unsigned pl, bool wave_live, unsigned kw, unsigned kx, unsigned ra, unsigned K,
                                                                     unsigned nw) {
  const unsigned nn = nw * nw, pw = infer_conv_pitch(nw, ra, RN) / 4;  // (the pitch of a span in words)
  const unsigned jc = infer_conv_slice(kx, nw, ra, RN), sw = jc * pw, ks = jc * ra * RN;  // per slice: channels, span words, k
  unsigned* xs = tab + infer_conv_tab_words(ks, RN);
  for (unsigned q = tid; q < jc * ra; q += 256) tab[q] = q / ra * pw + q % ra * (nw / 4);
  const unsigned nt = (sw + 255) / 256, bw = 256 * nt;  // the rounds of a slice, the words of a span buffer
  unsigned where[16], keep[16], w[16];
#pragma unroll
  for (unsigned t = 0; t < 16; t++) {
    const unsigned i = tid + 256 * t, at = 4 * (i % pw);
    const bool in = i < sw && p0 + at < nn;
    where[t] = in ? i / pw * nn + at : 0u;
    keep[t] = in ? 0xffffffffu : 0u;
    asm volatile("" : "+v"(keep[t]));
  }
  const int8_t* xp = x + (size_t)b * kx * nn + p0;  // the strip's first pixel in channel 0; a slice further on: + jc * nn
#pragma unroll
  for (unsigned t = 0; t < 16; t++) if (t < nt) w[t] = *(const unsigned*)(xp + where[t]) & keep[t];
#pragma unroll
  for (unsigned t = 0; t < 16; t++) if (t < nt) xs[tid + 256 * t] = w[t];
  const unsigned lr = tid >> 3, lc = (tid & 7) * 16;  // the 16 bytes of the filter slice this thread stages: tile row, byte column
  const int8_t* fp = f + (size_t)(ch0 + lr) * K + lc;
  for (unsigned s = 0, kb = 0; kb < K; s++, kb += ks) {
    const unsigned* cur = xs + (s & 1) * bw;
    const bool more = kb + ks < K;
    if (more) {
      xp += (size_t)jc * nn;
#pragma unroll
      for (unsigned t = 0; t < 16; t++) if (t < nt) w[t] = *(const unsigned*)(xp + where[t]) & keep[t];
    }
    for (unsigned k0 = 0; k0 < ks; k0 += IC_TK) {
      infer_v4i a = {0, 0, 0, 0};
      if (ch0 + lr < kw) a = *(const infer_v4i*)(fp + kb + k0);
      __syncthreads();  // (the fragments of the slice before have been read)
      *(infer_v4i*)&As[lr * IC_LDA + lc] = a;
      __syncthreads();  // (the first one of a span slice: its spans are in LDS, too; the very first: the table)
      if (wave_live) {
#pragma unroll
        for (unsigned u = 0; u < IC_TK / 32; u++) {
          const infer_v4i fa = *(const infer_v4i*)&As[l31 * IC_LDA + u * 32 + half * 16];
          const infer_v4i fb = infer_conv_frag<RN>(cur, tab, (k0 + u * 32 + half * 16) / RN, pl >> 2, pl & 3);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        }
      }
    }
    if (more) {
      unsigned* nxt = xs + ((s + 1) & 1) * bw;
#pragma unroll
      for (unsigned t = 0; t < 16; t++) if (t < nt) nxt[tid + 256 * t] = w[t];
    }
  }
}
// k_infer_conv on the i8 MFMA, exact: out[b][ch][p] = bias[ch] + sum over (j, a, c) of x[b][j][p + a * nw + c] * f[ch][j][a][c] on the flat plane
// index p < nn = nw * nw, then clear_garbage. x: the int8 copy of the input, [batch][kx][nn]; f: the packed filter image [kw][K] of
// infer_conv_pack, k = (j * ra + a) * RN + c (RN = the padded kernel side, 2, 4, 8 or 16; RN = 1: infer_conv_tile<1> above; K a multiple of 32 with K * 128 * 128 < 2^31).
// A workgroup (4 waves) owns IC_TC = 32 output channels (blockIdx.y) of one strip of IC_TP = 128 consecutive pixels of one sample's plane
// (blockIdx.x = sample * strips + strip: a strip never crosses a sample), a wave 32 channels x 32 pixels: one accumulator of
// v_mfma_i32_32x32x32_i8 with the channels as its first operand and the pixels as its second, so that the D column — the lane — is the pixel and
// every store of a register is 32 consecutive words of [b][ch][nn]. D row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// The im2col operand is never formed: the inputs of channel j the strip can touch are ONE span of the plane, IC_TP + (ra - 1) * nw + RN - 1
// bytes from the strip's first pixel on. The kx spans are staged in LDS once (whole aligned words; words beyond the end of the plane are zeros
// and are not read from memory: a term that leaves the plane is dropped, as in k_infer_conv), with a table of where the input bytes of every
// filter row of the packed K start (rows of the K padding point at the first span: their weights are zero). The filter tile goes through LDS
// in K slices of IC_TK = 128, zero beyond kw and K. Lane l of a wave holds 16 consecutive k (k0 + 16 * (l >> 5) ...) of channel l & 31 and of
// pixel l & 31: both fragments follow the SAME (lane half, byte) -> k rule, byte t of the lane is k0 + 16 * (l >> 5) + t, so the products pair up
// whatever order the instruction gives the 32 k of a step.
// Every term that leaves the plane or wraps into the next row belongs to an output clear_garbage zeroes, so a workgroup whose channels are all
// >= u0 or whose rows are all >= u1 stages nothing and stores zeros, and so does such a wave of a live workgroup. In bounds: sample < batch
// (the grid), word reads of x below nn, 16-byte reads of f below row kw and column K, LDS reads within a span (infer_conv_pitch), stores at
// ch < kw and p < nn. SL: the spans go through LDS in channel slices (infer_conv_tile_sl, for the layers whose kx spans do not fit); grid, fragments,
// stores and the short cuts of dead tiles and waves are the same.
template <int RN, bool SL = false> __global__ __launch_bounds__(256) void k_infer_conv_i8(const int8_t* __restrict__ x, const int8_t* __restrict__ f, const int64_t* __restrict__ bias, int64_t* __restrict__ o,
                                                                          unsigned strips, unsigned kw, unsigned kx, unsigned ra, unsigned K, unsigned nw, unsigned u0, unsigned u1, unsigned u2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ic_lds[];
  int8_t* As = (int8_t*)ic_lds;
  unsigned* tab = (unsigned*)(ic_lds + IC_TC * IC_LDA);
  unsigned* xs = tab + infer_conv_tab_words(K, RN);
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const unsigned nn = nw * nw;
  const unsigned b = blockIdx.x / strips, p0 = (blockIdx.x % strips) * IC_TP, ch0 = blockIdx.y * IC_TC;
  const unsigned pl = wave * 32 + l31, p = p0 + pl;
  const bool tile_live = ch0 < u0 && p0 / nw < u1;                                         // (uniform in the workgroup)
  const bool wave_live = tile_live && p0 + wave * 32 < nn && (p0 + wave * 32) / nw < u1;  // (uniform in the wave)
  infer_v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  if (tile_live) {
    if constexpr (SL) infer_conv_tile_sl<RN>(acc, x, f, As, tab, b, p0, ch0, tid, half, l31, pl, wave_live, kw, kx, ra, K, nw);
    else infer_conv_tile<RN>(acc, x, f, As, tab, xs, b, p0, ch0, tid, half, l31, pl, wave_live, kw, kx, ra, K, nw);
  }
  if (p >= nn) return;
  const bool keep = wave_live && p / nw < u1 && p % nw < u2;
  int64_t* op = o + (size_t)b * kw * nn + p;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const unsigned ch = ch0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (ch < kw) op[(size_t)ch * nn] = keep && ch < u0 ? (int64_t)acc[r] + bias[ch] : (int64_t)0;
  }
}
// MaxPool 2 x 2 stride 2 (k_infer_maxpool's rule) on one channel row of the result tile of k_infer_conv_i8_rq: `row` holds whole pairs of rows of
// a plane of side nw. infer_pool1: pooled pixel j of the strip. infer_pool4: the four pooled pixels j .. j + 3, byte t = pixel j + t, for
// j % 4 == 0 and nw % 8 == 0 — they share a pooled row and their 2 x 8 tile bytes are two aligned 8-byte words (the tile's pitch is a multiple of 16)
__device__ __forceinline__ int infer_pool1(const int8_t* row, unsigned j, unsigned nw) {
  const int8_t* q = row + 2 * (j / (nw / 2)) * nw + 2 * (j % (nw / 2));
  const int a = q[0] > q[1] ? q[0] : q[1], b = q[nw] > q[nw + 1] ? q[nw] : q[nw + 1];
  return a > b ? a : b;
}
__device__ __forceinline__ unsigned infer_pool4(const int8_t* row, unsigned j, unsigned nw) {
  const unsigned at = 2 * (j / (nw / 2)) * nw + 2 * (j % (nw / 2));
  const uint2 a = *(const uint2*)(row + at), b = *(const uint2*)(row + at + nw);
  unsigned w = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const unsigned ua = t < 2 ? a.x : a.y, ub = t < 2 ? b.x : b.y, s = 16 * (t & 1);
    const int m0 = (int8_t)(ua >> s), m1 = (int8_t)(ua >> (s + 8)), m2 = (int8_t)(ub >> s), m3 = (int8_t)(ub >> (s + 8));
    const int ma = m0 > m1 ? m0 : m1, mb = m2 > m3 ? m2 : m3;
    w |= (unsigned)((ma > mb ? ma : mb) & 255) << (8 * t);
  }
  return w;
}
// A convolution with the Requant behind it, a ReLU behind that (RELU) and a MaxPool behind either (POOL) in ONE launch (infer_fuse_plan): the
// staging and the MFMA loop of k_infer_conv_i8 (infer_conv_tile: same grid, same LDS, a workgroup of 4 waves owns IC_TC = 32 channels x IC_TP = 128
// consecutive pixels of the plane of sample blockIdx.x / strips; lane = pixel, register r of a lane = channel (r & 3) + 8 * (r >> 2) +
// 4 * (lane >> 5)), then in registers, per element:
//   v = keep && ch < u0 ? acc + bias[ch] : 0 — what k_infer_conv_i8 stores: clear_garbage first, a cleared element is 0 —, then what
//   k_infer_requant does, letter for letter (the epilogue of k_infer_gemm_i8_rq): |v| > 2^bits refuses the sample, (v * mult + 2^(sh-1)) >> sh with
//   the multiply and add in unsigned 64-bit arithmetic and an arithmetic shift, clamp to +-127; then max(., 0) under RELU.
// Refusal: a workgroup holds one sample. A lane ORs its 16 tests into a mask; ONE ballot per wave decides, and only the lanes of a wave with a bad
//   element call infer_refuse (INFER_BAD_REQUANT). Elements at ch >= kw or p >= nn are never tested, stored or flagged.
// Result tile: the int8 values go to LDS as [32 channels][128 pixels] at row pitch IC_LDA, into the filter-slice buffer As — IC_TC * IC_LDA bytes,
//   exactly this tile, free behind one barrier after the last slice. A dead workgroup (all channels >= u0 or all rows >= u1) stages nothing and
//   its tile is zeros, as are the pixels >= nn of a plane shorter than a strip. After a second barrier every thread reads what others wrote:
//   no POOL: O8[b][ch][nn] leaves as 16-byte vectors along the pixels, 8 per channel row, one per thread (the int8 copy of a tensor starts
//     256-aligned, p0 is a multiple of 128 and nn of 16: a vector at p0 + 16 i < nn is aligned and ends within the plane);
//   POOL: the strip is 128 / nw whole rows from an even row on, or the whole plane (nn < 128) — whole pairs of rows for every nw the planner
//     admits —, min(128, nn) / 4 pooled pixels per channel, contiguous in O8[b][ch][nn / 4] from p0 / 4 on: 16-byte vectors (infer_pool4) where
//     that count is a multiple of 16 (then nw % 8 == 0), bytes otherwise. The max runs over requantised, ReLU'd, cleared values: the integers of
//     the three separate kernels. Neither the conv's tensor nor the Requant's or the ReLU's is written;
//   W64: the int64 form of the chain's LAST tensor (infer_needs_int64) from the same tile, sign-extended, in 16-byte pairs (an even element of
//     a channel row is 16-aligned: the int64 form starts 256-aligned and nn, nn / 4, p0 and p0 / 4 are even).
// In bounds: as k_infer_conv_i8 for the loads; bias[ch] at ch < u0 <= kw; LDS within the tile (rows < 32, pixels < 128; a pooled pixel j <
//   min(128, nn) / 4 reads rows 2 pr and 2 pr + 1 < min(128, nn) / nw); stores at ch < kw and p < nn (pooled: p0 / 4 + j < nn / 4).
template <int RN, bool RELU, bool POOL, bool W64, bool SL = false> __global__ __launch_bounds__(256) void k_infer_conv_i8_rq(const int8_t* __restrict__ x, const int8_t* __restrict__ f, const int64_t* __restrict__ bias,
    int8_t* __restrict__ O8, int64_t* __restrict__ O64, unsigned strips, unsigned kw, unsigned kx, unsigned ra, unsigned K, unsigned nw, unsigned u0, unsigned u1, unsigned u2, int64_t mult, unsigned sh,
    unsigned bits, unsigned* status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ic_lds[];
  int8_t* As = (int8_t*)ic_lds;
  unsigned* tab = (unsigned*)(ic_lds + IC_TC * IC_LDA);
  unsigned* xs = tab + infer_conv_tab_words(K, RN);
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const unsigned nn = nw * nw;
  const unsigned b = blockIdx.x / strips, p0 = (blockIdx.x % strips) * IC_TP, ch0 = blockIdx.y * IC_TC;
  const unsigned pl = wave * 32 + l31, p = p0 + pl;
  const bool tile_live = ch0 < u0 && p0 / nw < u1;                                         // (uniform in the workgroup)
  const bool wave_live = tile_live && p0 + wave * 32 < nn && (p0 + wave * 32) / nw < u1;  // (uniform in the wave)
  infer_v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  if (tile_live) {
    if constexpr (SL) infer_conv_tile_sl<RN>(acc, x, f, As, tab, b, p0, ch0, tid, half, l31, pl, wave_live, kw, kx, ra, K, nw);
    else infer_conv_tile<RN>(acc, x, f, As, tab, xs, b, p0, ch0, tid, half, l31, pl, wave_live, kw, kx, ra, K, nw);
  }
  __syncthreads();  // (every wave has read its last fragments: the filter-slice buffer becomes the result tile)
  const bool keep = wave_live && p < nn && p / nw < u1 && p % nw < u2;
  const uint64_t lim = uint64_t(1) << bits;
  unsigned bad = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const unsigned tc = (r & 3) + 8 * (r >> 2) + 4 * half, ch = ch0 + tc;
    const int64_t v = keep && ch < u0 ? (int64_t)((uint64_t)(int64_t)acc[r] + (uint64_t)bias[ch]) : (int64_t)0;
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (mag > lim && ch < kw && p < nn) bad |= 1u << r;
    int64_t y = (int64_t)((uint64_t)v * (uint64_t)mult + (uint64_t(1) << (sh - 1))) >> sh;
    y = y < -127 ? -127 : y > 127 ? 127 : y;
    if (RELU) y = y < 0 ? 0 : y;
    As[tc * IC_LDA + pl] = (int8_t)y;
  }
  if (__ballot(bad != 0)) { if (bad) infer_refuse(status, b, INFER_BAD_REQUANT); }
  __syncthreads();
  const unsigned live = nn - p0 < IC_TP ? nn - p0 : IC_TP;  // the pixels of the strip within the plane (a multiple of 16)
  if (!POOL) {
    const unsigned tc = tid >> 3, at = (tid & 7) * 16, ch = ch0 + tc;
    if (ch < kw && at < live) *(infer_v4i*)(O8 + ((size_t)b * kw + ch) * nn + p0 + at) = *(const infer_v4i*)&As[tc * IC_LDA + at];
    if (W64) {
      for (unsigned i = tid; i < IC_TC * IC_TP / 2; i += 256) {
        const unsigned c = i >> 6, e = (i & 63) * 2;
        const int8_t* y = &As[c * IC_LDA + e];
        if (ch0 + c < kw && e < live) { infer_v2l v; v[0] = y[0]; v[1] = y[1]; *(infer_v2l*)(O64 + ((size_t)b * kw + ch0 + c) * nn + p0 + e) = v; }
      }
    }
  } else {
    const unsigned np = live / 4, pn = nn / 4, pp0 = p0 / 4;  // pooled pixels: of the strip, of a plane, in front of the strip
    if ((np & 15) == 0) {
      const unsigned c = tid / (np / 16), j = tid % (np / 16) * 16;
      if (c < IC_TC && ch0 + c < kw) {
        infer_v4i v;
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = (int)infer_pool4(&As[c * IC_LDA], j + 4 * t, nw);
        *(infer_v4i*)(O8 + ((size_t)b * kw + ch0 + c) * pn + pp0 + j) = v;
      }
    } else {
      for (unsigned i = tid; i < IC_TC * np; i += 256) {
        const unsigned c = i / np, j = i % np;
        if (ch0 + c < kw) O8[((size_t)b * kw + ch0 + c) * pn + pp0 + j] = (int8_t)infer_pool1(&As[c * IC_LDA], j, nw);
      }
    }
    if (W64) {
      for (unsigned i = tid; i < IC_TC * np / 2; i += 256) {
        const unsigned c = i / (np / 2), j = i % (np / 2) * 2;
        if (ch0 + c < kw) { infer_v2l v; v[0] = infer_pool1(&As[c * IC_LDA], j, nw); v[1] = infer_pool1(&As[c * IC_LDA], j + 1, nw); *(infer_v2l*)(O64 + ((size_t)b * kw + ch0 + c) * pn + pp0 + j) = v; }
      }
    }
  }
}
// Activation::Gelu (gelu_op): table[v * mult + max], the table's rows being -max .. max - 1. |v| > 2^20 or a scaled value outside the table
// refuses the sample (per = words per sample) and nothing is read: the same test guards the table against the values of a sample refused earlier.
// The zero of a refused element goes to the int8 forms like any table entry (the planner's interval of the tensor includes 0)
__global__ __launch_bounds__(256) void k_infer_gelu(const int64_t* __restrict__ x, const int64_t* __restrict__ table, int64_t* __restrict__ o, int8_t* __restrict__ o8, int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                    size_t n, int64_t mult, int64_t mx, unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = x[i], lim = int64_t(1) << 20;
  const int64_t scaled = (int64_t)((uint64_t)v * (uint64_t)mult);  // (|v| <= 2^20 and mult <= 2^12 once the first check holds)
  const bool bad = v < -lim || v > lim || scaled < -mx || scaled >= mx;
  infer_flag(bad, i, per, status, INFER_BAD_GELU);
  const int64_t y = bad ? 0 : table[scaled + mx];
  o[i] = y;
  infer_put_forms(y, i, o8, lo, hi);
}
__device__ __forceinline__ uint64_t infer_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
  return v;
}
// LayerNorm::evaluate (layernorm_op): one wave per row of fd elements (a power of two; lanes beyond a short row add zeros). 64-bit wrap-around
// arithmetic as on the host: full = N mult sum(x^2) - mult sum(x)^2, in = full >> rcb (arithmetic), out = gamma (N x - sum) lut[in + 2^14] + beta.
// |x| > 2^20 anywhere in the row (INFER_BAD_LAYERNORM), or else `in` outside the table (INFER_BAD_LAYERNORM_TABLE: the host has a message of its
// own for it), refuses the sample and the row is written as zeros (the table is not read: the test on `in` is the guard for the rows of a
// sample refused earlier, too). Lane 0 refuses the sample of the row (per = rows per sample; a wave never straddles samples here, the vote is
// the __any below); where rows of one sample disagree the input class stands, whichever wave came first
__global__ __launch_bounds__(256) void k_infer_layernorm(const int64_t* __restrict__ x, const int64_t* __restrict__ gamma, const int64_t* __restrict__ beta, const int64_t* __restrict__ lut,
                                                         int64_t* __restrict__ o, size_t rows, size_t fd, int64_t nn, int64_t mult, unsigned rcb, unsigned* status, size_t per) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  const int64_t* xr = x + row * fd;
  const int64_t lim = int64_t(1) << 20, tmax = int64_t(1) << 14;
  uint64_t sq = 0, sum = 0; bool bad = false;
  for (size_t i = lane; i < fd; i += 64) { const int64_t v = xr[i]; bad = bad || v < -lim || v > lim; sq += (uint64_t)v * (uint64_t)v; sum += (uint64_t)v; }
  sq = infer_wave_sum(sq); sum = infer_wave_sum(sum);
  unsigned cls = __any(bad) ? INFER_BAD_LAYERNORM : INFER_OK;
  const uint64_t n = (uint64_t)nn, m = (uint64_t)mult;
  const int64_t in = (int64_t)(n * m * sq - m * sum * sum) >> rcb;
  if (!cls && (in < -tmax || in >= tmax)) cls = INFER_BAD_LAYERNORM_TABLE;
  if (cls) {
    if (lane == 0) { infer_refuse(status, row / per, cls); if (cls == INFER_BAD_LAYERNORM) atomicCAS(status + row / per, INFER_BAD_LAYERNORM_TABLE, INFER_BAD_LAYERNORM); }
    for (size_t i = lane; i < fd; i += 64) o[row * fd + i] = 0;
    return;
  }
  const uint64_t inv = (uint64_t)lut[in + tmax];
  for (size_t i = lane; i < fd; i += 64) o[row * fd + i] = (int64_t)((uint64_t)gamma[i] * (n * (uint64_t)xr[i] - sum) * inv + (uint64_t)beta[i]);
}
// Softmax::evaluate (softmax_op) after the shifts: element j of row i (rows of K words; i counts samples x C x R) is kept when j <= i mod R.
// |masked| = low byte | high byte | exponential table index (tv bits) | zero chunks (zc groups of zv bits): table[index], times (chunk == 0) for
// every group. |x| > 2^24 refuses the sample (per = words per sample; the index is masked: nothing is read outside the table, for any x and any
// shift): the host's shift step has already refused such a sample, or found it refused and given it zero shifts — the test here then leaves
// its word as it is. lo, hi: the two planes of a two-plane output (IQ_PLANES; null: none), the left operand of k_infer_gemm2_i8
__global__ __launch_bounds__(256) void k_infer_softmax(const int64_t* __restrict__ x, const int64_t* __restrict__ shift, const int64_t* __restrict__ table, int64_t* __restrict__ o, int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                       size_t n, size_t R, size_t K, int64_t scalar, int64_t neg_inf, unsigned tv, unsigned zc, unsigned zv, unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t row = i / K, j = i % K;
  const int64_t v = x[i], lim = int64_t(1) << 24;
  infer_flag(v < -lim || v > lim, i, per, status, INFER_BAD_SOFTMAX);
  const int64_t masked = j <= row % R ? (int64_t)((uint64_t)v * (uint64_t)scalar + (uint64_t)shift[row]) : neg_inf;
  size_t idx;
  const bool keep = infer_softmax_index(masked, tv, zc, zv, &idx);  // (the one place of this arithmetic: k_infer_gemm2_i8_rq and the planner call it too)
  const int64_t acc = keep ? table[idx] : 0;
  o[i] = acc;
  infer_put_forms(acc, i, nullptr, lo, hi);  // (the planner has seen every table entry within 0..16383)
}
// The product of two tensors of the batch with the Requant behind it — and, under SM, the Softmax in front of it — in ONE launch (infer_fuse_plan;
// Q K^T -> Requant and Softmax -> probabilities x V -> Requant of an attention block). The work split is k_infer_gemm2_i8's: a workgroup of 4 waves
// owns one 64 x 64 tile of ONE (sample, concat index), blockIdx.x = ((b * C + c) * tiles of R + tile of r) * tiles of N + tile of n; a wave holds
// one 32 x 32 accumulator on v_mfma_i32_32x32x32_i8 (SM: two, the lo and hi planes over the same B fragment), and a wave whose block lies outside
// R x N multiplies nothing. flags = InferOp::d[0] | d[1] (IG2_*).
// Staging: K slices of IG_TK through LDS at pitch IG_LD; the NEXT slice is loaded into registers right behind the barrier that publishes the
//   current one (k_infer_gemm_i8_rq's scheme) and is in flight while the current one is multiplied.
//   SM = false: both operands are int8 copies, read by infer_g2_load in every layout of infer_gemm2_plan.
//   SM = true: the left operand is MADE on the way into LDS. Thread t holds 16 consecutive int64 scores of tile row t >> 2 (k = k0 + 16 * (t & 3)
//   ...; eight 16-byte loads where K % 16 == 0, words inside the row otherwise) and the row's shift, and applies k_infer_softmax's arithmetic
//   through the same function: mask j <= row % R (the row of the Softmax is (b * C + c) * R + r: row % R = r), x * scalar + shift in unsigned 64-bit, the absolute
//   value, >> 16, the table index masked to tv bits, the zero chunks (infer_softmax_index). Each value v (0..16383) is split into lo = v & 127 and
//   hi = v >> 7; 16 bytes of each go to LDS in two 16-byte stores. Neither the int64 probabilities nor their planes exist in memory. Scores beyond
//   R or K are not read and stand as zeros: whatever the table makes of them meets a zero of B (k >= K) or a row that is never stored (r >= R).
//   The exponential table is read as 16-bit entries (every entry is within 0..16383): IG2_SM_LDS — the planner's decision, infer_gemm2_rq_table_lds —
//   stages all 2^tv of them in dynamic LDS once per workgroup, otherwise they are gathered from the 16-bit image in global memory.
// Causal skip (IG2_SM_SKIP: the planner has evaluated the value of a masked element, neg_inf through the table and the zero chunks, and found 0):
//   a slice with k0 > r0 + 63 lies wholly above the diagonal of the tile's rows; the loop ends in front of it, loads included.
// Epilogue: v = (int64)acc_hi * 128 + acc_lo (SM) or (int64)acc, then k_infer_requant's arithmetic letter for letter: |v| > 2^bits refuses the
//   sample, (v * mult + 2^(sh-1)) >> sh in unsigned 64-bit with an arithmetic shift, clamp to +-127. One ballot per wave; only a wave with a bad
//   element calls infer_refuse (the tile belongs to ONE sample). Rows >= R and columns >= N are never tested, stored or flagged. The int8 tile goes
//   through LDS (the operand buffers are free behind a barrier after the last slice) and leaves at the output strides sOc, sOr, sOn — the result
//   permutation of a ConcatMatMul included —, in 16-byte vectors along n under IG2_OW, bytes otherwise; the int64 form only under W64
//   (infer_needs_int64). A refused sample's output is clamped like any other.
// Refusal order: the Softmax's range test (|x| > 2^24) is DROPPED here. The host's shift step in front of this launch has applied it to every
//   sample not refused before (infer_softmax_shifts: the status word is set, the shifts are zero), so when this kernel runs the word of such a
//   sample already holds INFER_BAD_SOFTMAX or an earlier class, and the Requant refusal below — a compare-and-swap from zero — cannot replace it:
//   the status word still names the FIRST node that refused the sample.
struct InferSmArgs { const int64_t* x; const int64_t* shift; const uint16_t* tab; size_t lenX, lenS; int64_t scalar, neg_inf; unsigned tv, zc, zv; };
template <bool SM, bool W64> __global__ __launch_bounds__(256) void k_infer_gemm2_i8_rq(const int8_t* __restrict__ A, size_t lenA, InferSmArgs sm, const int8_t* __restrict__ B, size_t lenB, int8_t* __restrict__ O8,
                                                                                       int64_t* __restrict__ O64, size_t lenO, InferGemmShape g, unsigned tr, unsigned tn, unsigned flags, int64_t mult, unsigned sh,
                                                                                       unsigned bits, unsigned* status) {
  constexpr int PLANE = IG_TM * IG_LD;
  __shared__ __attribute__((aligned(16))) int8_t lds[(SM ? 3 : 2) * PLANE];
  extern __shared__ __attribute__((aligned(16))) uint16_t infer_sm_tab[];  // (IG2_SM_LDS: 2^tv entries)
  static_assert(IG_TM * RQ_LDC <= 2 * PLANE && 3 * PLANE == (int)IG2_RQ_OPERANDS && IG_TM == 64 && IG_TN == 64 && IG_TK == 64, "the result tile lies in the operand buffers; a thread stages 16 k of one row");
  int8_t* As = lds; int8_t* Bs = lds + (SM ? 2 : 1) * PLANE; int8_t* Cs = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned t = blockIdx.x;
  const size_t n0 = (size_t)(t % tn) * IG_TN; t /= tn;
  const size_t r0 = (size_t)(t % tr) * IG_TM; t /= tr;
  const size_t c = t % (unsigned)g.C, b = t / (unsigned)g.C;
  const int8_t* Am = SM ? nullptr : A + b * lenA + c * g.sAc;
  const int8_t* Bm = B + b * lenB + c * g.sBc;
  const bool a_k = !(flags & IG2_AT), b_k = !(flags & IG2_BT), a_w = flags & IG2_AW, b_w = flags & IG2_BW, tab_lds = flags & IG2_SM_LDS;
  const size_t sAr = a_k ? g.sAr : 1, sAm = a_k ? 1 : g.sAm, sBn = b_k ? g.sBn : 1, sBm = b_k ? 1 : g.sBm;  // (the unit stride as a constant)
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool live = r0 + wm < g.R && n0 + wn < g.N;  // (uniform in the wave)
  const size_t kend = SM && (flags & IG2_SM_SKIP) && r0 + IG_TM < g.K ? r0 + IG_TM : g.K;
  // SM: this thread's row of scores and its shift
  const size_t srow = r0 + (size_t)(tid >> 2), sk = (size_t)(tid & 3) * 16;
  const bool row_in = SM && srow < g.R, k16 = (g.K & 15) == 0;
  const int64_t* xr = SM ? sm.x + b * sm.lenX + (c * g.R + (row_in ? srow : 0)) * g.K : nullptr;
  const int64_t shift = row_in ? sm.shift[b * sm.lenS + c * g.R + srow] : 0;
  if (SM && tab_lds) {  // 2^tv 16-bit entries, tv >= 3: whole 16-byte vectors (published by the first barrier of the loop below... and one here)
    const unsigned nv = (2u << sm.tv) >> 4;
    for (unsigned i = (unsigned)tid; i < nv; i += 256) ((infer_v4i*)infer_sm_tab)[i] = ((const infer_v4i*)sm.tab)[i];
    __syncthreads();
  }
  infer_v16i acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = acc2[r] = 0;
  infer_v4i a = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, bb;
  int64_t raw[16];
  auto fetch = [&](size_t k0) {  // the slice at k0 into registers: zeros, and no load, beyond the matrices
    bb = infer_g2_load(Bm, g.N, g.K, sBn, sBm, n0, k0, b_w, tid);
    if (!SM) { a = infer_g2_load(Am, g.R, g.K, sAr, sAm, r0, k0, a_w, tid); return; }
    const size_t k = k0 + sk;
#pragma unroll
    for (int j = 0; j < 16; j++) raw[j] = 0;
    if (!row_in || k >= g.K) return;
    if (k16) {
#pragma unroll
      for (int j = 0; j < 8; j++) { const infer_v2l v = *(const infer_v2l*)(xr + k + 2 * j); raw[2 * j] = v[0]; raw[2 * j + 1] = v[1]; }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) if (k + j < g.K) raw[j] = xr[k + j];
    }
  };
  auto make = [&](size_t k0, const uint16_t* tab) {  // raw -> the 16 bytes of each plane
    const size_t k = k0 + sk;
    unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t masked = k + j <= srow ? (int64_t)((uint64_t)raw[j] * (uint64_t)sm.scalar + (uint64_t)shift) : sm.neg_inf;
      size_t idx;
      const bool keep = infer_softmax_index(masked, sm.tv, sm.zc, sm.zv, &idx);
      const unsigned v = keep ? (unsigned)tab[idx] : 0u;
      lo[j >> 2] |= (v & 127u) << (8 * (j & 3)); hi[j >> 2] |= (v >> 7) << (8 * (j & 3));
    }
    a[0] = (int)lo[0]; a[1] = (int)lo[1]; a[2] = (int)lo[2]; a[3] = (int)lo[3];
    a2[0] = (int)hi[0]; a2[1] = (int)hi[1]; a2[2] = (int)hi[2]; a2[3] = (int)hi[3];
  };
  fetch(0);
  for (size_t k0 = 0; k0 < kend; k0 += IG_TK) {
    if (SM) { if (tab_lds) make(k0, infer_sm_tab); else make(k0, sm.tab); }
    __syncthreads();  // (the fragments of the slice before have been read)
    infer_g2_store(As, a, SM || a_k, tid);
    if (SM) infer_g2_store(As + PLANE, a2, true, tid);
    infer_g2_store(Bs, bb, b_k, tid);
    __syncthreads();
    if (k0 + IG_TK < kend) fetch(k0 + IG_TK);
    if (live) {
#pragma unroll
      for (int s = 0; s < IG_TK / 32; s++) {
        if (k0 + s * 32 < g.K) {  // (uniform)
          const int at = (wm + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16;
          const infer_v4i fb = *(const infer_v4i*)&Bs[(wn + (lane & 31)) * IG_LD + s * 32 + (lane >> 5) * 16];
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&As[at], fb, acc, 0, 0, 0);
          if (SM) acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const infer_v4i*)&As[PLANE + at], fb, acc2, 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();  // (every wave has read its last fragments: the operand buffers become the result tile)
  const size_t col = n0 + wn + (lane & 31);
  const uint64_t lim = uint64_t(1) << bits;
  unsigned bad = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int trow = wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int64_t v = SM ? (int64_t)acc2[r] * 128 + acc[r] : (int64_t)acc[r];
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (mag > lim && r0 + trow < g.R && col < g.N) bad |= 1u << r;
    int64_t y = (int64_t)((uint64_t)v * (uint64_t)mult + (uint64_t(1) << (sh - 1))) >> sh;
    y = y < -127 ? -127 : y > 127 ? 127 : y;
    Cs[trow * RQ_LDC + wn + (lane & 31)] = (int8_t)y;
  }
  if (__ballot(bad != 0) && bad) infer_refuse(status, b, INFER_BAD_REQUANT);
  __syncthreads();
  const size_t obase = b * lenO + c * g.sOc;
  if (flags & IG2_OW) {  // one 16-byte vector of a row per thread
    const size_t row = r0 + (tid >> 2), cc = n0 + (tid & 3) * 16;
    if (row < g.R && cc < g.N) *(infer_v4i*)(O8 + obase + row * g.sOr + cc) = *(const infer_v4i*)&Cs[(tid >> 2) * RQ_LDC + (tid & 3) * 16];
  } else {
    for (int i = tid; i < IG_TM * IG_TN; i += 256) {
      const size_t row = r0 + (i >> 6), cc = n0 + (i & 63);
      if (row < g.R && cc < g.N) O8[obase + row * g.sOr + cc * g.sOn] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
    }
  }
  if (!W64) return;
  for (int i = tid; i < IG_TM * IG_TN; i += 256) {
    const size_t row = r0 + (i >> 6), cc = n0 + (i & 63);
    if (row < g.R && cc < g.N) O64[obase + row * g.sOr + cc * g.sOn] = Cs[(i >> 6) * RQ_LDC + (i & 63)];
  }
}
// Logits::Argmax (argmax_rows): one wave per row of K words (rows counts samples x rows of a sample); lanes stride over the row and keep (value,
// index) under "greater, or equal at a smaller index"; the pairs are reduced across the wave by the same rule, so the result is the FIRST maximum
// whatever the order of the reduction. Every lane holds a pair: K >= 1, and a lane without an element holds (INT64_MIN, K), which loses against
// every element. Reads the int8 copy of the input where it has one (the output of a Requant), else the int64 form. No refusal class: any data has an argmax.
__global__ __launch_bounds__(256) void k_infer_argmax(const int64_t* __restrict__ x64, const int8_t* __restrict__ x8, int64_t* __restrict__ o, size_t rows, size_t K) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  long long best = INT64_MIN; unsigned long long at = K;
  for (size_t j = lane; j < K; j += 64) {  // (ascending j: a later equal value never replaces an earlier one)
    const long long v = x8 ? (long long)x8[row * K + j] : (long long)x64[row * K + j];
    if (v > best || at == K) { best = v; at = j; }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const long long ov = __shfl_xor(best, d, 64); const unsigned long long oa = __shfl_xor(at, d, 64);
    if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
  }
  if (lane == 0) o[row] = (int64_t)at;
}
// model input tensor `off .. off + len` of every sample, from the uploaded block (int8 when the host found every word within -128..127, else int64)
__global__ __launch_bounds__(256) void k_infer_load(const int64_t* __restrict__ s64, const int8_t* __restrict__ s8, size_t stride, size_t off, size_t len, int64_t* __restrict__ o, int8_t* __restrict__ o8, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t src = (i / len) * stride + off + i % len;
  const int64_t v = s8 ? (int64_t)s8[src] : s64[src];
  o[i] = v;
  if (o8) o8[i] = (int8_t)v;
}
__global__ __launch_bounds__(256) void k_infer_store(const int64_t* __restrict__ x, size_t len, int64_t* __restrict__ dst, size_t stride, size_t off, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[(i / len) * stride + off + i % len] = x[i];
}
// Tap mode: the trace rows of the chunk. Tap blockIdx.y (uniform per workgroup: the descriptor is read once, in scalar registers) is tensor `src`,
// [sample][len] words, and goes to words off .. off + len of every sample's row of the sample-major image [sample][row_words]. The workgroups of
// a tap stride over its nb * len words: reads are consecutive throughout, writes consecutive within runs of len. A copy of 16 bytes per word
// (8 read, 8 written), plain vector loads and stores; any len and off (odd ones, len below or no multiple of the wave). 32-bit index arithmetic
// when the tap's words of the chunk can be counted in 31 bits. In bounds: j < nb * len (the tensor's words of the chunk), s < nb and
// off + e < row_words (the planner's layout: off + len <= row_words)
struct InferTapDesc { const int64_t* src; unsigned long long len, off; };
__global__ __launch_bounds__(256) void k_infer_tap_pack(const InferTapDesc* __restrict__ taps, int64_t* __restrict__ img, size_t row_words, size_t nb) {
  const InferTapDesc t = taps[blockIdx.y];
  const size_t n = nb * t.len, step = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t* dst = img + t.off;
  if (n <= 0x7fffffffu - step) {
    const unsigned len = (unsigned)t.len, n32 = (unsigned)n, st32 = (unsigned)step;
    for (unsigned j = (unsigned)i0; j < n32; j += st32) { const unsigned s = j / len, e = j - s * len; dst[(size_t)s * row_words + e] = t.src[j]; }
  } else {
    for (size_t j = i0; j < n; j += step) { const size_t s = j / t.len, e = j - s * t.len; dst[s * row_words + e] = t.src[j]; }
  }
}
// Decode: the next token of every sample of the chunk, after the ops of a step (decode_step of infer.h, the function the host loop calls). One
// thread per sample. out: the Logits tensor [nb][seq] of this step's inference; tokens: the int64 input block of the chunk [nb][seq], which the
// next step's k_infer_load reads; length, stop, limit: one word per sample; status: the chunk's status words, only read here. A sample whose stop
// is set is left alone, one whose status word is set becomes REFUSED and keeps its tokens. Plain loads and stores in stream order, no atomics.
// In bounds: i < nb; out is read at length - 1 and tokens written at length only once 1 <= length < seq holds (decode_limit).
__global__ __launch_bounds__(256) void k_infer_next_token(const int64_t* __restrict__ out, int64_t* __restrict__ tokens, unsigned* __restrict__ length, unsigned* __restrict__ stop,
                                                          const unsigned* __restrict__ limit, const unsigned* __restrict__ status, size_t nb, unsigned seq, int64_t eos) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  uint32_t len = length[i], st = stop[i];
  if (st) return;
  decode_step(len, st, limit[i], seq, eos, status[i], out + i * seq, tokens + i * seq);
  length[i] = len; stop[i] = st;
}

struct InferDeviceState {
  int device = 0;
  std::vector<int64_t*> c64; std::vector<int8_t*> c8;
  ~InferDeviceState() { (void)hipSetDevice(device); for (int64_t* p : c64) if (p) (void)hipFree(p); for (int8_t* p : c8) if (p) (void)hipFree(p); }
};
InferDeviceState* hip_infer_state_new(int device) { InferDeviceState* s = new InferDeviceState(); s->device = device; return s; }
void hip_infer_state_free(InferDeviceState* s) { delete s; }
// constants: on the device from the first launch that reads them on (freed with the model)
static const int64_t* infer_const64(const InferProgram& p, InferDeviceState* st, int c) {
  if (c < 0) return nullptr;
  if (!st->c64[(size_t)c]) { int64_t* dp_ = nullptr; HIP_CHECK(hipMalloc((void**)&dp_, std::max<size_t>(p.consts[(size_t)c].n, 1) * 8)); st->c64[(size_t)c] = dp_; HIP_CHECK(hipMemcpy(dp_, p.consts[(size_t)c].data(), p.consts[(size_t)c].n * 8, hipMemcpyHostToDevice)); }
  return st->c64[(size_t)c];
}
static const int8_t* infer_const8(const InferProgram& p, InferDeviceState* st, int c) {
  if (!st->c8[(size_t)c]) { int8_t* dp_ = nullptr; HIP_CHECK(hipMalloc((void**)&dp_, p.consts[(size_t)c].w8.size())); st->c8[(size_t)c] = dp_; HIP_CHECK(hipMemcpy(dp_, p.consts[(size_t)c].w8.data(), p.consts[(size_t)c].w8.size(), hipMemcpyHostToDevice)); }
  return st->c8[(size_t)c];
}

// The scratch of one chunk (outside the arenas, released before the call returns): [tensors, int64 | int8][input block][output block][one status
// word per sample]; and the pinned block of the host side: the input block on its way up, the output block with the status words behind it on
// its way down and, at the shift step of a Softmax, [its input of the chunk][the status words][the shifts]. Tap mode alone appends [the tap
// descriptors][the image of the chunk's trace rows] to the device block and the image's twin, behind the output block, to the pinned one
struct InferScratch {
  bool in_q = true;     // model inputs within -128..127 (checked on the host, for the whole call): they travel as int8 and count as quantised tensors
  std::vector<char> q;  // tensor t in this call: IQ_NO, IQ_YES (an int8 copy) or IQ_PLANES (two planes and NO int8 copy)
  std::vector<size_t> off64, off8, off8hi;
  size_t chunk = 1, off_in = 0, off_out = 0, off_stat = 0, total = 0, sm_in = 0, sm_stat = 0, pinned_bytes = 0;
  size_t off_taps = 0, off_img = 0, pin_img = 0;  // (tap mode)
  char* dev = nullptr; char* pinned = nullptr;
  int64_t* T64(int t) const { return (int64_t*)(dev + off64[(size_t)t]); }
  int8_t* T8(int t) const { return q[(size_t)t] == IQ_YES ? (int8_t*)(dev + off8[(size_t)t]) : (int8_t*)nullptr; }
  int8_t* TP(int t, int plane) const { return q[(size_t)t] == IQ_PLANES ? (int8_t*)(dev + (plane ? off8hi : off8)[(size_t)t]) : (int8_t*)nullptr; }
  unsigned* status() const { return (unsigned*)(dev + off_stat); }
  uint32_t* sm_status() const { return (uint32_t*)(pinned + sm_in); }
};
// (inputs null: the input block is int64 whatever it will hold — decode rewrites it on the device)
static InferScratch infer_layout(const InferProgram& p, const int64_t* inputs, size_t ninputs, bool taps) {
  const char* mbs = getenv("DP_INFER_SCRATCH_MB");
  const size_t scratch_cap = (mbs && atoll(mbs) > 0 ? (size_t)atoll(mbs) : size_t(1024)) << 20, nt = p.tensors.size();
  InferScratch m;
  if (!inputs) m.in_q = false;
  for (size_t i = 0, n = ninputs * p.input_len; i < n && m.in_q; i++) m.in_q = inputs[i] >= -128 && inputs[i] <= 127;
  m.q.resize(nt); m.off64.resize(nt); m.off8.resize(nt); m.off8hi.resize(nt);
  size_t per_sample = 0;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  for (size_t t = 0; t < nt; t++) { const int q = p.tensors[t].q; m.q[t] = (char)(q == IQ_IF_INPUTS ? (m.in_q ? IQ_YES : IQ_NO) : q); per_sample += p.tensors[t].len * (m.q[t] == IQ_PLANES ? 10 : m.q[t] ? 9 : 8); }
  per_sample += p.input_len * (m.in_q ? 1 : 8) + p.output_len * 8;
  if (taps) per_sample += p.row_words * 16;  // (the image and its pinned twin)
  const size_t chunk = m.chunk = std::max<size_t>(1, std::min(ninputs, scratch_cap / std::max<size_t>(per_sample, 1)));
  for (size_t t = 0; t < nt; t++) { m.off64[t] = m.total; m.total += up(chunk * p.tensors[t].len * 8); m.off8[t] = m.total; if (m.q[t]) m.total += up(chunk * p.tensors[t].len); m.off8hi[t] = m.total; if (m.q[t] == IQ_PLANES) m.total += up(chunk * p.tensors[t].len); }
  const size_t in_bytes = chunk * p.input_len * (m.in_q ? 1 : 8), out_bytes = chunk * p.output_len * 8 + chunk * 4;
  m.off_in = m.total; m.total += up(in_bytes);
  m.off_out = m.total; m.off_stat = m.off_out + chunk * p.output_len * 8; m.total += up(out_bytes);
  size_t sm_sh = 0;
  for (const InferOp& o : p.ops) if (o.kind == IO_SOFTMAX) { m.sm_in = std::max(m.sm_in, up(chunk * p.tensors[(size_t)o.in0].len * 8)); sm_sh = std::max(sm_sh, chunk * p.tensors[(size_t)o.in1].len * 8); }
  m.sm_stat = up(chunk * 4);
  m.pinned_bytes = std::max(std::max(in_bytes, out_bytes), m.sm_in + m.sm_stat + sm_sh);
  if (taps) {
    m.off_taps = m.total; m.total += up(p.taps.size() * sizeof(InferTapDesc));
    m.off_img = m.total; m.total += up(chunk * p.row_words * 8);
    m.pin_img = up(out_bytes); m.pinned_bytes = std::max(std::max(m.pinned_bytes, m.pin_img + chunk * p.row_words * 8), p.taps.size() * sizeof(InferTapDesc));
  }
  return m;
}
// The one table of what the host says of refused data: the message of a class (infer.h), and the order in which a plain call that met several
// classes in a chunk names one
static const char* const INFER_REFUSAL[] = {nullptr, "requant: value exceeds intermediate bit size", "embeddings: token outside the vocabulary", "gelu: input out of range", "layernorm: input out of range",
                                            "softmax: input out of range", "layernorm: the inverse square root input leaves its table"};
static uint32_t infer_first_class(const uint32_t* hs, size_t nb) {
  for (uint32_t cls : {INFER_BAD_REQUANT, INFER_BAD_TOKEN, INFER_BAD_GELU, INFER_BAD_LAYERNORM, INFER_BAD_LAYERNORM_TABLE, INFER_BAD_SOFTMAX}) if (std::find(hs, hs + nb, cls) != hs + nb) return cls;
  return INFER_OK;
}
static dim3 infer_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
// one op for the nb samples of the chunk: one launch. launches (INFER_COUNTS words): by kind the ops served, [IO_KINDS + 2]: the launches of
// k_infer_gemm_i8 and k_infer_gemm_i8_rq, [IO_KINDS + 3]: those of k_infer_conv_i8, [IO_KINDS + 4]: those of k_infer_gemm2_i8 (all counted
// under their kind as well), [IO_KINDS + 5]: those of k_infer_gemm_i8_rq, [IO_KINDS + 6]: the ops it absorbed — served, and counted under
// their kinds, without a launch of their own —, [IO_KINDS + 7]: the launches of k_infer_conv_i8_rq (counted under [IO_KINDS + 3] as well; the ops
// it absorbed under [IO_KINDS + 6]), [IO_KINDS + 8]: the launches of k_infer_gemm2_i8_rq (counted under IO_GEMM2 and [IO_KINDS + 4] as well; its
// Requant and, under SM, the Softmax it serves under [IO_KINDS + 6]). fuse: the head of a chain (infer_fuse_plan) whose input has its int8 form in this call takes
// k_infer_gemm_i8_rq / k_infer_conv_i8_rq; the result is the number of ops absorbed (IO_GEMM: o.d[1], o.d[2], IO_CONV: o.fused — the caller skips
// them; IO_GEMM2: o.fused[0], the Softmax of an SM chain has skipped its own launch), 0 for every other launch.
constexpr size_t INFER_COUNTS = IO_KINDS + 9;
static size_t infer_launch(const InferProgram& p, const InferOp& o, const InferScratch& m, InferDeviceState* st, hipStream_t s, size_t nb, size_t* launches, bool fuse) {
  static const bool no_mfma = getenv("DP_INFER_NO_MFMA") && atoi(getenv("DP_INFER_NO_MFMA"));
  const bool i8 = infer_reads_int8_only(p, o, o.in0, m.q, nb, no_mfma);  // (the one predicate: also what infer_needs_int64 elides by)
  auto c64 = [&](int c) { return infer_const64(p, st, c); };
  const size_t len = p.tensors[(size_t)o.out].len, n = nb * len;
  launches[o.kind]++;
  switch (o.kind) {
    case IO_GEMM:
      if (i8) {
        const size_t M = nb * o.g.R;
        const dim3 grid((unsigned)((M + IG_TM - 1) / IG_TM), (unsigned)((o.g.N + IG_TN - 1) / IG_TN));
        const bool pl = m.q[(size_t)o.in0] == IQ_PLANES;  // a two-plane input: k_infer_gemm_i8_pl in either shape, counted as the one-plane launches are
        launches[IO_KINDS + 2]++;
        if (fuse && o.d[0]) {
          const InferOp& rq = p.ops[o.d[1]];
          const bool relu = o.d[0] == 2;
          const int last = relu ? p.ops[o.d[2]].out : rq.out;
          int64_t* o64 = infer_needs_int64(p, last, m.q, nb, no_mfma) ? m.T64(last) : nullptr;
          auto go = [&](auto kern) { kern<<<grid, 256, 0, s>>>(m.T8(o.in0), infer_const8(p, st, o.w), c64(o.bias), m.T8(last), o64, M, o.g.K, o.g.N, rq.left, rq.shift, rq.bits, m.status(), o.g.R); };
          auto go_pl = [&](auto kern) { kern<<<grid, 256, 0, s>>>(m.TP(o.in0, 0), m.TP(o.in0, 1), infer_const8(p, st, o.w), c64(o.bias), m.T8(last), o64, M, o.g.K, o.g.N, rq.left, rq.shift, rq.bits, m.status(), o.g.R); };
          if (pl) {
            if (relu) { if (o64) go_pl(k_infer_gemm_i8_pl<true, true, true>); else go_pl(k_infer_gemm_i8_pl<true, true, false>); }
            else { if (o64) go_pl(k_infer_gemm_i8_pl<true, false, true>); else go_pl(k_infer_gemm_i8_pl<true, false, false>); }
          } else if (relu) { if (o64) go(k_infer_gemm_i8_rq<true, true>); else go(k_infer_gemm_i8_rq<true, false>); }
          else { if (o64) go(k_infer_gemm_i8_rq<false, true>); else go(k_infer_gemm_i8_rq<false, false>); }
          launches[IO_REQUANT]++; launches[IO_RELU] += relu; launches[IO_KINDS + 5]++; launches[IO_KINDS + 6] += o.d[0];
          return o.d[0];
        }
        if (pl) k_infer_gemm_i8_pl<false, false, true><<<grid, 256, 0, s>>>(m.TP(o.in0, 0), m.TP(o.in0, 1), infer_const8(p, st, o.w), c64(o.bias), nullptr, m.T64(o.out), M, o.g.K, o.g.N, 0, 1, 0, nullptr, o.g.R);
        else k_infer_gemm_i8<<<grid, 256, 0, s>>>(m.T8(o.in0), infer_const8(p, st, o.w), c64(o.bias), m.T64(o.out), M, o.g.K, o.g.N);
      } else k_infer_gemm_i64<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), p.tensors[(size_t)o.in0].len, c64(o.w), 0, c64(o.bias), m.T64(o.out), len, nb, o.g);
      break;
    case IO_GEMM2: {
      const size_t lenA = p.tensors[(size_t)o.in0].len, lenB = p.tensors[(size_t)o.in1].len;
      const size_t tr = (o.g.R + IG_TM - 1) / IG_TM, tn = (o.g.N + IG_TN - 1) / IG_TN, tiles = infer_gemm2_tiles(o.g, nb);
      static_assert(IG_TM == 64 && IG_TN == 64, "infer_gemm2_tiles counts 64 x 64 tiles");
      // the planner found a form for both operands (o.d[0]); i8: both have their int8 form in this call — only the LEFT one may be two planes
      if (const int form = fuse ? infer_gemm2_rq_form(p, o, m.q, nb, no_mfma) : 0) {  // the chain in one launch: o.fused[0] = its Requant; form 2: the Softmax o.d[2] as well
        const InferOp& rq = p.ops[(size_t)o.fused[0]];
        int64_t* o64 = infer_needs_int64(p, rq.out, m.q, nb, no_mfma) ? m.T64(rq.out) : nullptr;
        const unsigned flags = (unsigned)(o.d[0] | o.d[1]);
        InferSmArgs sa = {};
        size_t lds = 0;
        if (form == 2) {
          const InferOp& sm = p.ops[o.d[2]];
          sa = InferSmArgs{m.T64(sm.in0), m.T64(sm.in1), (const uint16_t*)infer_const8(p, st, sm.table), p.tensors[(size_t)sm.in0].len, p.tensors[(size_t)sm.in1].len, sm.left, infer_softmax_neg_inf(sm.right),
                           sm.bits, (unsigned)sm.d[3], (unsigned)sm.d[4]};
          DP_REQUIRE(!(flags & IG2_SM_LDS) || infer_gemm2_rq_table_lds(sm.bits), DP_ERR_ARG, "dp_model_infer: softmax table in LDS");
          lds = (flags & IG2_SM_LDS) ? size_t(2) << sm.bits : 0;
        }
        auto go = [&](auto kern) { kern<<<dim3((unsigned)tiles), 256, lds, s>>>(form == 2 ? nullptr : m.T8(o.in0), lenA, sa, m.T8(o.in1), lenB, m.T8(rq.out), o64, p.tensors[(size_t)rq.out].len, o.g, (unsigned)tr, (unsigned)tn, flags, rq.left, rq.shift, rq.bits, m.status()); };
        if (form == 2) { if (o64) go(k_infer_gemm2_i8_rq<true, true>); else go(k_infer_gemm2_i8_rq<true, false>); }
        else { if (o64) go(k_infer_gemm2_i8_rq<false, true>); else go(k_infer_gemm2_i8_rq<false, false>); }
        launches[IO_KINDS + 4]++; launches[IO_REQUANT]++; launches[IO_KINDS + 8]++; launches[IO_KINDS + 6] += 1 + (form == 2);
        return 1;
      }
      if (i8) {
        if (m.q[(size_t)o.in0] == IQ_PLANES) k_infer_gemm2_i8<true><<<dim3((unsigned)tiles), 256, 0, s>>>(m.TP(o.in0, 0), m.TP(o.in0, 1), lenA, m.T8(o.in1), lenB, m.T64(o.out), len, o.g, (unsigned)tr, (unsigned)tn, (unsigned)o.d[0]);
        else k_infer_gemm2_i8<false><<<dim3((unsigned)tiles), 256, 0, s>>>(m.T8(o.in0), nullptr, lenA, m.T8(o.in1), lenB, m.T64(o.out), len, o.g, (unsigned)tr, (unsigned)tn, (unsigned)o.d[0]);
        launches[IO_KINDS + 4]++;
      } else k_infer_gemm_i64<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), lenA, m.T64(o.in1), lenB, nullptr, m.T64(o.out), len, nb, o.g);
      break;
    }
    case IO_REQUANT: k_infer_requant<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n, o.left, o.shift, o.bits, m.status(), len); break;
    case IO_RELU: k_infer_relu<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n); break;
    case IO_ADDC: k_infer_addc<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), m.T64(o.out), m.T8(o.out), m.TP(o.out, 0), m.TP(o.out, 1), n, len, o.left, o.right); break;
    case IO_ADD2: k_infer_add2<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.in1), m.T64(o.out), m.T8(o.out), m.TP(o.out, 0), m.TP(o.out, 1), n, o.left, o.right); break;
    case IO_EMBED: k_infer_embed<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), m.T64(o.out), m.T8(o.out), m.TP(o.out, 0), m.TP(o.out, 1), n, o.d[0], o.d[1], m.status(), len); break;
    case IO_MAXPOOL: k_infer_maxpool<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n, o.d[1], o.d[2]); break;
    case IO_CONV:
      if (i8) {  // (the planner made the image: rn is 1, 2, 4, 8 or 16 and the LDS fits, whole spans or — o.jc — in channel slices)
        const unsigned kw = (unsigned)o.d[0], kx = (unsigned)o.d[1], rn = (unsigned)o.d[2], nw = (unsigned)o.d[3], ra = (unsigned)o.d[7], K = (unsigned)o.g.K;
        const unsigned strips = (nw * nw + IC_TP - 1) / IC_TP;
        const dim3 grid((unsigned)(nb * strips), (kw + IC_TC - 1) / IC_TC);
        const size_t lds = infer_conv_lds(kx, nw, ra, rn, K, o.jc);
        DP_REQUIRE(o.jc == (o.jc ? infer_conv_slice(kx, nw, ra, rn) : 0u), DP_ERR_ARG, "dp_model_infer: conv slices");  // (the kernel works jc out by the same rule)
        DP_REQUIRE(nb * strips <= 0x7fffffffu, DP_ERR_ARG, "dp_model_infer: conv grid");
        const int8_t* f8 = infer_const8(p, st, o.w);
        const unsigned u0 = (unsigned)o.d[4], u1 = (unsigned)o.d[5], u2 = (unsigned)o.d[6];
        auto by_side = [&](auto go) {  // the instantiation of the padded kernel side, whole spans or channel slices (rn >= 2 only)
          if (o.jc) switch (rn) {
            case 2: go(std::integral_constant<int, 2>(), std::true_type()); break;
            case 4: go(std::integral_constant<int, 4>(), std::true_type()); break;
            case 8: go(std::integral_constant<int, 8>(), std::true_type()); break;
            default: go(std::integral_constant<int, 16>(), std::true_type()); break;
          }
          else switch (rn) {
            case 1: go(std::integral_constant<int, 1>(), std::false_type()); break;
            case 2: go(std::integral_constant<int, 2>(), std::false_type()); break;
            case 4: go(std::integral_constant<int, 4>(), std::false_type()); break;
            case 8: go(std::integral_constant<int, 8>(), std::false_type()); break;
            default: go(std::integral_constant<int, 16>(), std::false_type()); break;
          }
        };
        launches[IO_KINDS + 3]++;
        if (fuse && o.nfused) {  // the chain in one launch: o.fused = its Requant, then a ReLU and / or a MaxPool
          const InferOp& rq = p.ops[(size_t)o.fused[0]];
          const InferOp& lo = p.ops[(size_t)o.fused[o.nfused - 1]];
          const bool relu = o.nfused >= 2 && p.ops[(size_t)o.fused[1]].kind == IO_RELU, pool = lo.kind == IO_MAXPOOL;
          int64_t* o64 = infer_needs_int64(p, lo.out, m.q, nb, no_mfma) ? m.T64(lo.out) : nullptr;
          auto go = [&](auto kern) { kern<<<grid, 256, lds, s>>>(m.T8(o.in0), f8, c64(o.bias), m.T8(lo.out), o64, strips, kw, kx, ra, K, nw, u0, u1, u2, rq.left, rq.shift, rq.bits, m.status()); };
          auto pick = [&](auto r, auto sl) {
            constexpr int RN = decltype(r)::value;
            constexpr bool SL = decltype(sl)::value;
            switch ((relu ? 1 : 0) | (pool ? 2 : 0) | (o64 ? 4 : 0)) {
              case 0: go(k_infer_conv_i8_rq<RN, false, false, false, SL>); break;
              case 1: go(k_infer_conv_i8_rq<RN, true, false, false, SL>); break;
              case 2: go(k_infer_conv_i8_rq<RN, false, true, false, SL>); break;
              case 3: go(k_infer_conv_i8_rq<RN, true, true, false, SL>); break;
              case 4: go(k_infer_conv_i8_rq<RN, false, false, true, SL>); break;
              case 5: go(k_infer_conv_i8_rq<RN, true, false, true, SL>); break;
              case 6: go(k_infer_conv_i8_rq<RN, false, true, true, SL>); break;
              default: go(k_infer_conv_i8_rq<RN, true, true, true, SL>); break;
            }
          };
          by_side(pick);
          launches[IO_REQUANT]++; launches[IO_RELU] += relu; launches[IO_MAXPOOL] += pool; launches[IO_KINDS + 7]++; launches[IO_KINDS + 6] += (size_t)o.nfused;
          return (size_t)o.nfused;
        }
        by_side([&](auto r, auto sl) { k_infer_conv_i8<decltype(r)::value, decltype(sl)::value><<<grid, 256, lds, s>>>(m.T8(o.in0), f8, c64(o.bias), m.T64(o.out), strips, kw, kx, ra, K, nw, u0, u1, u2); });
      } else k_infer_conv<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), c64(o.bias), m.T64(o.out), n, o.d[0], o.d[1], o.d[2], o.d[3], o.d[4], o.d[5], o.d[6]);
      break;
    case IO_GELU: k_infer_gelu<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.table), m.T64(o.out), m.T8(o.out), m.TP(o.out, 0), m.TP(o.out, 1), n, o.left, (int64_t)o.d[0], m.status(), len); break;
    case IO_LAYERNORM: {
      const size_t rows = n / o.d[0];
      k_infer_layernorm<<<infer_grid(rows * 64), 256, 0, s>>>(m.T64(o.in0), c64(o.w), c64(o.bias), c64(o.table), m.T64(o.out), rows, o.d[0], (int64_t)o.d[1], o.left, o.shift, m.status(), len / o.d[0]);
      break;
    }
    case IO_SOFTMAX:
      if (fuse && o.d[5] && infer_gemm2_rq_form(p, p.ops[o.d[5] - 1], m.q, nb, no_mfma) == 2) break;  // (served, after its shift step, by the k_infer_gemm2_i8_rq launch of its chain)
      k_infer_softmax<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.in1), c64(o.table), m.T64(o.out), m.TP(o.out, 0), m.TP(o.out, 1), n, o.d[1], o.d[2], o.left, -(((o.right >> 16) + 1) << 16), o.bits, (unsigned)o.d[3], (unsigned)o.d[4], m.status(), len); break;  // (after infer_shift_trip)
    case IO_ARGMAX: { const size_t rows = nb * o.d[0]; k_infer_argmax<<<infer_grid(rows * 64), 256, 0, s>>>(m.T64(o.in0), i8 ? m.T8(o.in0) : nullptr, m.T64(o.out), rows, o.d[1]); break; }
    default: throw DpError(DP_ERR_ARG, "dp_model_infer: unknown op");
  }
  return 0;
}
// The round trip in front of an IO_SOFTMAX: the shift of every row is made on the host, by the function the host inference calls. The status
// words come down with the Softmax input: the samples refused so far are skipped (their rows are not read), those the range check refuses here
// are marked, and the words go back to the device with the shifts. They are at m.sm_status() afterwards
static void infer_shift_trip(const InferProgram& p, const InferOp& o, const InferScratch& m, hipStream_t s, size_t nb) {
  const size_t nx = nb * p.tensors[(size_t)o.in0].len, nsh = nb * p.tensors[(size_t)o.in1].len;
  int64_t* shifts = (int64_t*)(m.pinned + m.sm_in + m.sm_stat);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(m.sm_status(), m.status(), nb * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(m.pinned, m.T64(o.in0), nx * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  p.shifts(o, (const int64_t*)m.pinned, nb, shifts, m.sm_status());
  HIP_CHECK(hipMemcpyAsync(m.status(), m.sm_status(), nb * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(m.T64(o.in1), shifts, nsh * 8, hipMemcpyHostToDevice, s));
}
// The program for the nb samples of the chunk whose input block is on the device: the loads of the model inputs, then every op in order, with
// the round trip in front of each IO_SOFTMAX (the only host synchronisation here: a program without one is enqueued and nothing waits).
// Plain mode (not checked): the class of the refused sample a shift step found, which ends the call; the later ops are not enqueued then
static uint32_t infer_enqueue(const InferProgram& p, const InferScratch& m, InferDeviceState* st, hipStream_t s, size_t nb, bool checked, size_t* launches, size_t& trips, double& trip_ms, bool taps = false) {
  static const bool no_fuse = getenv("DP_INFER_NO_FUSE") && atoi(getenv("DP_INFER_NO_FUSE"));
  const bool fuse = !no_fuse && !taps;  // (tap mode: every tensor is an entry of the trace row, nothing is elided)
  std::vector<char> absorbed(p.ops.size(), 0);
  size_t ioff = 0;
  for (int t : p.inputs) {
    const size_t len = p.tensors[(size_t)t].len, n = nb * len;
    k_infer_load<<<infer_grid(n), 256, 0, s>>>(m.in_q ? nullptr : (const int64_t*)(m.dev + m.off_in), m.in_q ? (const int8_t*)(m.dev + m.off_in) : nullptr, p.input_len, ioff, len, m.T64(t), m.T8(t), n);
    ioff += len; launches[IO_KINDS]++;
  }
  for (size_t i = 0; i < p.ops.size(); i++) {
    const InferOp& o = p.ops[i];
    if (absorbed[i]) continue;  // (a Requant / ReLU / MaxPool the fused launch of its chain's head has served)
    if (o.kind == IO_SOFTMAX) {
      const auto ts = std::chrono::steady_clock::now();
      infer_shift_trip(p, o, m, s, nb);
      trips++; trip_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
      if (!checked) if (const uint32_t cls = infer_first_class(m.sm_status(), nb)) return cls;
    }
    for (size_t k = infer_launch(p, o, m, st, s, nb, launches, fuse); k >= 1; k--) absorbed[o.kind == IO_GEMM ? o.d[k] : (size_t)o.fused[k - 1]] = 1;
  }
  return INFER_OK;
}
void hip_infer_run(Dev* d, const InferProgram& p, InferDeviceState* st, const int64_t* inputs, size_t ninputs, int64_t* outputs, size_t out_stride, double* wall_ms, uint32_t* reasons,
                   int64_t* rows, size_t row_stride) {
  HipDev* hd = static_cast<HipDev*>(d);
  hd->bind_thread(); hd->sync();
  hipStream_t s = hd->stream();
  static const bool log_line = getenv("DP_INFER_LOG") && atoi(getenv("DP_INFER_LOG"));
  const auto t0 = std::chrono::steady_clock::now();
  const bool taps = rows != nullptr;
  DP_REQUIRE(!taps || (row_stride >= p.row_words && p.taps.size() >= 1 && p.taps.size() <= 65535), DP_ERR_ARG, "dp_model_infer_trace: row buffer too small");
  InferScratch m = infer_layout(p, inputs, ninputs, taps);
  size_t tap_max = 0, tap_launches = 0;
  for (const InferTap& t : p.taps) tap_max = std::max(tap_max, t.len);
  hipEvent_t tap_ev[2] = {nullptr, nullptr};  // (DP_INFER_LOG in tap mode: the time of the chunks' k_infer_tap_pack launches)
  double tap_ms = 0;
  const size_t chunk = m.chunk, in_w = m.in_q ? 1 : 8;
  st->c64.resize(p.consts.size(), nullptr); st->c8.resize(p.consts.size(), nullptr);
  size_t launches[INFER_COUNTS] = {0}, nchunks = 0, trips = 0, nrefused = 0;
  double trip_ms = 0;
  uint32_t stop = INFER_OK;  // plain mode (no `reasons`): the class of the refused sample that ends the call
  auto cleanup = [&] {
    (void)hipStreamSynchronize(s); if (m.dev) (void)hipFree(m.dev); if (m.pinned) (void)hipHostFree(m.pinned); m.dev = m.pinned = nullptr;
    for (hipEvent_t& e : tap_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  };
  try {
    HIP_CHECK(hipMalloc((void**)&m.dev, m.total));
    HIP_CHECK(hipHostMalloc((void**)&m.pinned, m.pinned_bytes, hipHostMallocDefault));
    int64_t* dout = (int64_t*)(m.dev + m.off_out);
    if (taps) {  // the descriptors: made in the pinned block, uploaded once per call (the copy has landed before the block is written again)
      InferTapDesc* h = (InferTapDesc*)m.pinned;
      DP_REQUIRE(p.taps.size() * sizeof(InferTapDesc) <= m.pinned_bytes, DP_ERR_ARG, "dp_model_infer_trace: tap descriptors");
      for (size_t k = 0; k < p.taps.size(); k++) h[k] = InferTapDesc{m.T64(p.taps[k].tensor), p.taps[k].len, p.taps[k].off};
      HIP_CHECK(hipMemcpyAsync(m.dev + m.off_taps, h, p.taps.size() * sizeof(InferTapDesc), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (log_line) for (hipEvent_t& e : tap_ev) HIP_CHECK(hipEventCreate(&e));
    }
    for (size_t b0 = 0; b0 < ninputs && !stop; b0 += chunk) {
      const size_t nb = std::min(chunk, ninputs - b0), nin = nb * p.input_len, nout = nb * p.output_len;
      nchunks++;
      if (m.in_q) { int8_t* h = (int8_t*)m.pinned; const int64_t* src = inputs + b0 * p.input_len; for (size_t i = 0; i < nin; i++) h[i] = (int8_t)src[i]; }
      else memcpy(m.pinned, inputs + b0 * p.input_len, nin * 8);
      HIP_CHECK(hipMemcpyAsync(m.dev + m.off_in, m.pinned, nin * in_w, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemsetAsync(m.status(), 0, nb * 4, s));
      if ((stop = infer_enqueue(p, m, st, s, nb, reasons != nullptr, launches, trips, trip_ms, taps))) break;
      size_t ooff = 0;
      for (int t : p.outputs) {
        const size_t len = p.tensors[(size_t)t].len, n = nb * len;
        k_infer_store<<<infer_grid(n), 256, 0, s>>>(m.T64(t), len, dout, p.output_len, ooff, n);
        ooff += len; launches[IO_KINDS + 1]++;
      }
      if (taps) {
        const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((nb * tap_max + 255) / 256, 1024));
        if (tap_ev[0]) HIP_CHECK(hipEventRecord(tap_ev[0], s));
        k_infer_tap_pack<<<dim3(gx, (unsigned)p.taps.size()), 256, 0, s>>>((const InferTapDesc*)(m.dev + m.off_taps), (int64_t*)(m.dev + m.off_img), p.row_words, nb);
        if (tap_ev[1]) HIP_CHECK(hipEventRecord(tap_ev[1], s));
        tap_launches++;
      }
      HIP_CHECK(hipGetLastError());
      if (taps) HIP_CHECK(hipMemcpyAsync(m.pinned + m.pin_img, m.dev + m.off_img, nb * p.row_words * 8, hipMemcpyDeviceToHost, s));
      // the outputs and the status words behind them: one copy (a partial last chunk: the words are fetched on their own)
      if (nb == chunk) HIP_CHECK(hipMemcpyAsync(m.pinned, dout, nout * 8 + nb * 4, hipMemcpyDeviceToHost, s));
      else { HIP_CHECK(hipMemcpyAsync(m.pinned, dout, nout * 8, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(m.pinned + nout * 8, m.status(), nb * 4, hipMemcpyDeviceToHost, s)); }
      HIP_CHECK(hipStreamSynchronize(s));
      const uint32_t* hs = (const uint32_t*)(m.pinned + nout * 8);
      if (tap_ev[1]) { float ems = 0; HIP_CHECK(hipEventElapsedTime(&ems, tap_ev[0], tap_ev[1])); tap_ms += ems; }
      if (!reasons && (stop = infer_first_class(hs, nb))) break;  // (none of the chunk's rows is copied out)
      for (size_t i = 0; i < nb; i++) {  // refused samples (checked mode): the public reason, and zeros for whatever the later kernels made of them
        const uint32_t cls = hs[i] == INFER_BAD_LAYERNORM_TABLE ? INFER_BAD_LAYERNORM : hs[i];
        if (reasons) reasons[b0 + i] = cls;
        if (cls) { memset(outputs + (b0 + i) * out_stride, 0, p.output_len * 8); nrefused++; }
        else memcpy(outputs + (b0 + i) * out_stride, m.pinned + i * p.output_len * 8, p.output_len * 8);
        if (taps && cls) memset(rows + (b0 + i) * row_stride, 0, p.row_words * 8);
        else if (taps) memcpy(rows + (b0 + i) * row_stride, m.pinned + m.pin_img + i * p.row_words * 8, p.row_words * 8);
      }
    }
  } catch (...) { cleanup(); throw; }
  cleanup();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (wall_ms) *wall_ms = ms;
  const size_t n_i8 = launches[IO_KINDS + 2] + launches[IO_KINDS + 4], n_i64 = launches[IO_GEMM] + launches[IO_GEMM2] - n_i8;
  if (log_line) fprintf(stderr, "[dp infer] gemm_i8 %zu gemm_i64 %zu gemm2_i8 %zu conv %zu conv_i8 %zu requant %zu relu %zu add %zu add2 %zu embed %zu maxpool %zu load %zu store %zu gelu %zu layernorm %zu softmax %zu argmax %zu fused %zu conv_rq %zu gemm2_rq %zu shift_trips %zu shift_ms %.3f; batch %zu in %zu chunks of %zu, scratch %.1f MB, inputs as %s, %.3f ms%s%s\n",
                   n_i8, n_i64, launches[IO_KINDS + 4], launches[IO_CONV], launches[IO_KINDS + 3], launches[IO_REQUANT], launches[IO_RELU], launches[IO_ADDC], launches[IO_ADD2], launches[IO_EMBED], launches[IO_MAXPOOL], launches[IO_KINDS], launches[IO_KINDS + 1], launches[IO_GELU], launches[IO_LAYERNORM], launches[IO_SOFTMAX], launches[IO_ARGMAX], launches[IO_KINDS + 5], launches[IO_KINDS + 7], launches[IO_KINDS + 8], trips, trip_ms,
                   ninputs, nchunks, chunk, (double)m.total / 1048576.0, m.in_q ? "int8" : "int64", ms,
                   taps ? ("; taps " + std::to_string(p.taps.size()) + " entries, " + std::to_string(p.row_words) + " words, pack_launches " + std::to_string(tap_launches) + " pack_ms " + std::to_string(tap_ms)).c_str() : "",
                   reasons ? ("; checked, refused " + std::to_string(nrefused)).c_str() : "");
  DP_REQUIRE(!stop, DP_ERR_ARG, INFER_REFUSAL[stop]);
}
// dp_model_decode: greedy generation for a batch of prompts, on the device from the upload of the prompts to the download of the completions.
// Per chunk (DP_INFER_SCRATCH_MB, as hip_infer_run): the token block [nb][seq] (the prompts, `pad` behind them; always int64: k_infer_next_token
// rewrites it) and the state (length, stop, limit per sample) go up once; then step after step is enqueued — the program (infer_enqueue: a
// decodable program holds no IO_SOFTMAX, so nothing in a step waits for the host), then k_infer_next_token. The number of steps is known in
// advance: the most tokens a sample of the chunk can still take. Every DECODE_POLL_STEPS steps the 4-byte stop words come down, and the chunk
// ends early when all are set. Then ONE more pass of the program over the final tokens gives the outputs (what a proof of tokens[i] carries),
// and outputs, tokens, lengths, stops and status words come down behind one synchronisation. The status words are never cleared between the
// steps: a refused sample stays refused (its stop is REFUSED and its tokens stay as they were), every other sample's word is zero. A sample the
// final pass refuses is REFUSED as well, with zeros for its outputs.
constexpr size_t DECODE_POLL_STEPS = 4;
void hip_infer_decode(Dev* d, const InferProgram& p, InferDeviceState* st, const int64_t* prompts, const uint32_t* prompt_len, size_t nprompts, uint32_t max_new, int64_t eos, int64_t pad,
                      int64_t* tokens, uint32_t* length, uint32_t* stop, uint32_t* reasons, int64_t* outputs, double* wall_ms) {
  HipDev* hd = static_cast<HipDev*>(d);
  hd->bind_thread(); hd->sync();
  hipStream_t s = hd->stream();
  static const bool timing = getenv("DP_TIMING") && atoi(getenv("DP_TIMING"));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t seq = p.input_len;
  DP_REQUIRE(seq >= 1 && seq < (size_t(1) << 31) && p.output_len == seq && p.inputs.size() == 1 && p.outputs.size() == 1, DP_ERR_ARG, "dp_model_decode: the program is not decodable");
  for (const InferOp& o : p.ops) DP_REQUIRE(o.kind != IO_SOFTMAX, DP_ERR_ARG, "dp_model_decode: the program holds a Softmax");
  InferScratch m = infer_layout(p, nullptr, nprompts, false);
  const size_t chunk = m.chunk;
  const auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  // the state of the chunk on the device: [length][stop][limit], chunk words each; the pinned block: [outputs][tokens][length][stop][status] on
  // the way down (the tokens and the three state arrays at the same places on the way up)
  const size_t tok_bytes = up(chunk * seq * 8), word_bytes = up(chunk * 4);
  char* dstate = nullptr; char* pin = nullptr;
  st->c64.resize(p.consts.size(), nullptr); st->c8.resize(p.consts.size(), nullptr);
  size_t launches[INFER_COUNTS] = {0}, nchunks = 0, nsteps = 0, nlaunch = 0, npolls = 0, trips = 0;
  double trip_ms = 0, final_ms = 0;
  auto cleanup = [&] {
    (void)hipStreamSynchronize(s);
    if (m.dev) (void)hipFree(m.dev); if (dstate) (void)hipFree(dstate); if (pin) (void)hipHostFree(pin);
    m.dev = nullptr; dstate = pin = nullptr;
  };
  try {
    HIP_CHECK(hipMalloc((void**)&m.dev, m.total));
    HIP_CHECK(hipMalloc((void**)&dstate, 3 * word_bytes));
    HIP_CHECK(hipHostMalloc((void**)&pin, 2 * tok_bytes + 3 * word_bytes, hipHostMallocDefault));
    int64_t* dtok = (int64_t*)(m.dev + m.off_in);
    unsigned* dlen = (unsigned*)dstate; unsigned* dstop = (unsigned*)(dstate + word_bytes); unsigned* dlim = (unsigned*)(dstate + 2 * word_bytes);
    int64_t* hout = (int64_t*)pin; int64_t* htok = (int64_t*)(pin + tok_bytes);
    uint32_t* hlen = (uint32_t*)(pin + 2 * tok_bytes); uint32_t* hstop = (uint32_t*)(pin + 2 * tok_bytes + word_bytes); uint32_t* hlim = (uint32_t*)(pin + 2 * tok_bytes + 2 * word_bytes);
    const int64_t* dout = m.T64(p.outputs[0]);  // (the Logits tensor, [nb][seq]: the layout of the output rows)
    for (size_t b0 = 0; b0 < nprompts; b0 += chunk) {
      const size_t nb = std::min(chunk, nprompts - b0);
      nchunks++;
      size_t steps = 0;  // the most tokens a sample of the chunk can take
      for (size_t i = 0; i < nb; i++) {
        const uint32_t pl = prompt_len[b0 + i], lim = (uint32_t)std::min<size_t>(seq, (size_t)pl + max_new);
        for (size_t j = 0; j < seq; j++) htok[i * seq + j] = j < pl ? prompts[(b0 + i) * seq + j] : pad;
        hlen[i] = pl; hlim[i] = lim; hstop[i] = decode_limit(pl, lim, (uint32_t)seq);
        steps = std::max<size_t>(steps, lim - pl);
      }
      HIP_CHECK(hipMemcpyAsync(dtok, htok, nb * seq * 8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(dlen, hlen, nb * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(dstop, hstop, nb * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(dlim, hlim, nb * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemsetAsync(m.status(), 0, nb * 4, s));
      for (size_t k = 0; k < steps; k++) {
        (void)infer_enqueue(p, m, st, s, nb, true, launches, trips, trip_ms);
        k_infer_next_token<<<infer_grid(nb), 256, 0, s>>>(dout, dtok, dlen, dstop, dlim, m.status(), nb, (unsigned)seq, eos);
        nsteps++; nlaunch++;
        if ((k + 1) % DECODE_POLL_STEPS == 0 && k + 1 < steps) {  // (the copy up of the state has landed long ago: hstop is free)
          HIP_CHECK(hipGetLastError());
          HIP_CHECK(hipMemcpyAsync(hstop, dstop, nb * 4, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          npolls++;
          if (std::find(hstop, hstop + nb, 0u) == hstop + nb) break;
        }
      }
      const auto tf = std::chrono::steady_clock::now();
      (void)infer_enqueue(p, m, st, s, nb, true, launches, trips, trip_ms);
      HIP_CHECK(hipGetLastError());
      uint32_t* hstat = hlim;  // (the limits are not needed again: the status words come down in their place)
      HIP_CHECK(hipMemcpyAsync(hout, dout, nb * seq * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(htok, dtok, nb * seq * 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(hlen, dlen, nb * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(hstop, dstop, nb * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(hstat, m.status(), nb * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      final_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count();
      for (size_t i = 0; i < nb; i++) {
        const uint32_t cls = hstat[i] == INFER_BAD_LAYERNORM_TABLE ? INFER_BAD_LAYERNORM : hstat[i];
        DP_REQUIRE(cls || hstop[i], DP_ERR_ARG, "dp_model_decode: a prompt is still decoding after its last step");
        memcpy(tokens + (b0 + i) * seq, htok + i * seq, seq * 8);
        length[b0 + i] = hlen[i]; stop[b0 + i] = cls ? DECODE_STOP_REFUSED : hstop[i]; reasons[b0 + i] = cls;
        if (outputs && cls) memset(outputs + (b0 + i) * seq, 0, seq * 8);
        else if (outputs) memcpy(outputs + (b0 + i) * seq, hout + i * seq, seq * 8);
      }
    }
  } catch (...) { cleanup(); throw; }
  cleanup();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (wall_ms) *wall_ms = ms;
  for (size_t k = 0; k < IO_KINDS + 2; k++) nlaunch += launches[k];  // (launches[IO_KINDS + 2] .. [+ 5] count the i8 forms of launches counted under IO_GEMM, IO_CONV and IO_GEMM2)
  nlaunch -= launches[IO_KINDS + 6];  // (ops a fused launch absorbed: served without a launch)
  if (timing) fprintf(stderr, "[dp decode] prompts %zu chunks %zu steps %zu launches %zu polls %zu final_ms %.3f\n", nprompts, nchunks, nsteps, nlaunch, npolls, final_ms);
}
