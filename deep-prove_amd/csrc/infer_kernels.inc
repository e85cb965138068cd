// Kernels and the batch runner of dp_model_infer (infer.h). Included by hip_dev.hip after HipDev; not part of kernels.inc (the SIMT-emulator
// build of tests/ cuts its kernels from there). Activations are [batch][tensor] int64, with an int8 copy next to every tensor whose values are
// known to lie within -128..127 (what a Requant writes, and what ReLU / MaxPool make of it): the int8 copies are the operands of k_infer_gemm_i8.
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
// Add with a static operand / Positional::Learned: left * x + right * w[i mod len] (w: the operand, or the first rows of the table)
__global__ __launch_bounds__(256) void k_infer_addc(const int64_t* __restrict__ x, const int64_t* __restrict__ w, int64_t* __restrict__ o, size_t n, size_t len, int64_t left, int64_t right) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = (int64_t)((uint64_t)left * (uint64_t)x[i] + (uint64_t)right * (uint64_t)w[i % len]);
}
__global__ __launch_bounds__(256) void k_infer_add2(const int64_t* __restrict__ x, const int64_t* __restrict__ y, int64_t* __restrict__ o, size_t n, int64_t left, int64_t right) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = (int64_t)((uint64_t)left * (uint64_t)x[i] + (uint64_t)right * (uint64_t)y[i]);
}
// Embeddings: row tok[t] of the [vocab][emb] table for every token; a token outside the vocabulary refuses the sample (per = output words per
// sample) and reads row 0: the table is never read outside its rows, whatever the token
__global__ __launch_bounds__(256) void k_infer_embed(const int64_t* __restrict__ tok, const int64_t* __restrict__ table, int64_t* __restrict__ o, size_t n, size_t vocab, size_t emb,
                                                     unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t t = tok[i / emb];
  const bool bad = t < 0 || (uint64_t)t >= vocab;
  infer_flag(bad, i, per, status, INFER_BAD_TOKEN);
  if (bad) t = 0;
  o[i] = table[(size_t)t * emb + i % emb];
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
// Activation::Gelu (gelu_op): table[v * mult + max], the table's rows being -max .. max - 1. |v| > 2^20 or a scaled value outside the table
// refuses the sample (per = words per sample) and nothing is read: the same test guards the table against the values of a sample refused earlier
__global__ __launch_bounds__(256) void k_infer_gelu(const int64_t* __restrict__ x, const int64_t* __restrict__ table, int64_t* __restrict__ o, size_t n, int64_t mult, int64_t mx,
                                                    unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = x[i], lim = int64_t(1) << 20;
  const int64_t scaled = (int64_t)((uint64_t)v * (uint64_t)mult);  // (|v| <= 2^20 and mult <= 2^12 once the first check holds)
  const bool bad = v < -lim || v > lim || scaled < -mx || scaled >= mx;
  infer_flag(bad, i, per, status, INFER_BAD_GELU);
  if (bad) { o[i] = 0; return; }
  o[i] = table[scaled + mx];
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
// its word as it is
__global__ __launch_bounds__(256) void k_infer_softmax(const int64_t* __restrict__ x, const int64_t* __restrict__ shift, const int64_t* __restrict__ table, int64_t* __restrict__ o, size_t n,
                                                       size_t R, size_t K, int64_t scalar, int64_t neg_inf, unsigned tv, unsigned zc, unsigned zv, unsigned* status, size_t per) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t row = i / K, j = i % K;
  const int64_t v = x[i], lim = int64_t(1) << 24;
  infer_flag(v < -lim || v > lim, i, per, status, INFER_BAD_SOFTMAX);
  const int64_t masked = j <= row % R ? (int64_t)((uint64_t)v * (uint64_t)scalar + (uint64_t)shift[row]) : neg_inf;
  int64_t r = masked < 0 ? (int64_t)(0 - (uint64_t)masked) : masked;
  r >>= 16;
  int64_t acc = table[r & ((int64_t(1) << tv) - 1)];
  r >>= tv;
  for (unsigned z = 0; z < zc; z++) { acc *= (r & ((int64_t(1) << zv) - 1)) == 0 ? 1 : 0; r >>= zv; }
  o[i] = acc;
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
  std::vector<char> q;  // tensor t has an int8 copy
  std::vector<size_t> off64, off8;
  size_t chunk = 1, off_in = 0, off_out = 0, off_stat = 0, total = 0, sm_in = 0, sm_stat = 0, pinned_bytes = 0;
  size_t off_taps = 0, off_img = 0, pin_img = 0;  // (tap mode)
  char* dev = nullptr; char* pinned = nullptr;
  int64_t* T64(int t) const { return (int64_t*)(dev + off64[(size_t)t]); }
  int8_t* T8(int t) const { return q[(size_t)t] ? (int8_t*)(dev + off8[(size_t)t]) : (int8_t*)nullptr; }
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
  m.q.resize(nt); m.off64.resize(nt); m.off8.resize(nt);
  size_t per_sample = 0;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  for (size_t t = 0; t < nt; t++) { m.q[t] = p.tensors[t].q == IQ_YES || (p.tensors[t].q == IQ_IF_INPUTS && m.in_q); per_sample += p.tensors[t].len * (m.q[t] ? 9 : 8); }
  per_sample += p.input_len * (m.in_q ? 1 : 8) + p.output_len * 8;
  if (taps) per_sample += p.row_words * 16;  // (the image and its pinned twin)
  const size_t chunk = m.chunk = std::max<size_t>(1, std::min(ninputs, scratch_cap / std::max<size_t>(per_sample, 1)));
  for (size_t t = 0; t < nt; t++) { m.off64[t] = m.total; m.total += up(chunk * p.tensors[t].len * 8); m.off8[t] = m.total; if (m.q[t]) m.total += up(chunk * p.tensors[t].len); }
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
// one op for the nb samples of the chunk: one launch. launches: by kind, [IO_KINDS + 2]: those of k_infer_gemm_i8
static void infer_launch(const InferProgram& p, const InferOp& o, const InferScratch& m, InferDeviceState* st, hipStream_t s, size_t nb, size_t* launches) {
  static const bool no_mfma = getenv("DP_INFER_NO_MFMA") && atoi(getenv("DP_INFER_NO_MFMA"));
  auto c64 = [&](int c) { return infer_const64(p, st, c); };
  const size_t len = p.tensors[(size_t)o.out].len, n = nb * len;
  launches[o.kind]++;
  switch (o.kind) {
    case IO_GEMM:
      if (!no_mfma && m.q[(size_t)o.in0] && !p.consts[(size_t)o.w].w8.empty()) {
        const size_t M = nb * o.g.R;
        k_infer_gemm_i8<<<dim3((unsigned)((M + IG_TM - 1) / IG_TM), (unsigned)((o.g.N + IG_TN - 1) / IG_TN)), 256, 0, s>>>(m.T8(o.in0), infer_const8(p, st, o.w), c64(o.bias), m.T64(o.out), M, o.g.K, o.g.N);
        launches[IO_KINDS + 2]++;
      } else k_infer_gemm_i64<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), p.tensors[(size_t)o.in0].len, c64(o.w), 0, c64(o.bias), m.T64(o.out), len, nb, o.g);
      break;
    case IO_GEMM2: k_infer_gemm_i64<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), p.tensors[(size_t)o.in0].len, m.T64(o.in1), p.tensors[(size_t)o.in1].len, nullptr, m.T64(o.out), len, nb, o.g); break;
    case IO_REQUANT: k_infer_requant<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n, o.left, o.shift, o.bits, m.status(), len); break;
    case IO_RELU: k_infer_relu<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n); break;
    case IO_ADDC: k_infer_addc<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), m.T64(o.out), n, len, o.left, o.right); break;
    case IO_ADD2: k_infer_add2<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.in1), m.T64(o.out), n, o.left, o.right); break;
    case IO_EMBED: k_infer_embed<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), m.T64(o.out), n, o.d[0], o.d[1], m.status(), len); break;
    case IO_MAXPOOL: k_infer_maxpool<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.out), m.T8(o.out), n, o.d[1], o.d[2]); break;
    case IO_CONV: k_infer_conv<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.w), c64(o.bias), m.T64(o.out), n, o.d[0], o.d[1], o.d[2], o.d[3], o.d[4], o.d[5], o.d[6]); break;
    case IO_GELU: k_infer_gelu<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), c64(o.table), m.T64(o.out), n, o.left, (int64_t)o.d[0], m.status(), len); break;
    case IO_LAYERNORM: {
      const size_t rows = n / o.d[0];
      k_infer_layernorm<<<infer_grid(rows * 64), 256, 0, s>>>(m.T64(o.in0), c64(o.w), c64(o.bias), c64(o.table), m.T64(o.out), rows, o.d[0], (int64_t)o.d[1], o.left, o.shift, m.status(), len / o.d[0]);
      break;
    }
    case IO_SOFTMAX: k_infer_softmax<<<infer_grid(n), 256, 0, s>>>(m.T64(o.in0), m.T64(o.in1), c64(o.table), m.T64(o.out), n, o.d[1], o.d[2], o.left, -(((o.right >> 16) + 1) << 16), o.bits, (unsigned)o.d[3], (unsigned)o.d[4], m.status(), len); break;  // (after infer_shift_trip)
    case IO_ARGMAX: { const size_t rows = nb * o.d[0]; k_infer_argmax<<<infer_grid(rows * 64), 256, 0, s>>>(m.T64(o.in0), m.T8(o.in0), m.T64(o.out), rows, o.d[1]); break; }
    default: throw DpError(DP_ERR_ARG, "dp_model_infer: unknown op");
  }
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
static uint32_t infer_enqueue(const InferProgram& p, const InferScratch& m, InferDeviceState* st, hipStream_t s, size_t nb, bool checked, size_t* launches, size_t& trips, double& trip_ms) {
  size_t ioff = 0;
  for (int t : p.inputs) {
    const size_t len = p.tensors[(size_t)t].len, n = nb * len;
    k_infer_load<<<infer_grid(n), 256, 0, s>>>(m.in_q ? nullptr : (const int64_t*)(m.dev + m.off_in), m.in_q ? (const int8_t*)(m.dev + m.off_in) : nullptr, p.input_len, ioff, len, m.T64(t), m.T8(t), n);
    ioff += len; launches[IO_KINDS]++;
  }
  for (const InferOp& o : p.ops) {
    if (o.kind == IO_SOFTMAX) {
      const auto ts = std::chrono::steady_clock::now();
      infer_shift_trip(p, o, m, s, nb);
      trips++; trip_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
      if (!checked) if (const uint32_t cls = infer_first_class(m.sm_status(), nb)) return cls;
    }
    infer_launch(p, o, m, st, s, nb, launches);
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
  size_t launches[IO_KINDS + 3] = {0}, nchunks = 0, trips = 0, nrefused = 0;
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
      if ((stop = infer_enqueue(p, m, st, s, nb, reasons != nullptr, launches, trips, trip_ms))) break;
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
  const size_t n_i8 = launches[IO_KINDS + 2], n_i64 = launches[IO_GEMM] + launches[IO_GEMM2] - n_i8;
  if (log_line) fprintf(stderr, "[dp infer] gemm_i8 %zu gemm_i64 %zu conv %zu requant %zu relu %zu add %zu add2 %zu embed %zu maxpool %zu load %zu store %zu gelu %zu layernorm %zu softmax %zu argmax %zu shift_trips %zu shift_ms %.3f; batch %zu in %zu chunks of %zu, scratch %.1f MB, inputs as %s, %.3f ms%s%s\n",
                   n_i8, n_i64, launches[IO_CONV], launches[IO_REQUANT], launches[IO_RELU], launches[IO_ADDC], launches[IO_ADD2], launches[IO_EMBED], launches[IO_MAXPOOL], launches[IO_KINDS], launches[IO_KINDS + 1], launches[IO_GELU], launches[IO_LAYERNORM], launches[IO_SOFTMAX], launches[IO_ARGMAX], trips, trip_ms,
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
  size_t launches[IO_KINDS + 3] = {0}, nchunks = 0, nsteps = 0, nlaunch = 0, npolls = 0, trips = 0;
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
  for (size_t k = 0; k < IO_KINDS + 2; k++) nlaunch += launches[k];  // (launches[IO_KINDS + 2] counts the i8 form of launches counted under IO_GEMM)
  if (timing) fprintf(stderr, "[dp decode] prompts %zu chunks %zu steps %zu launches %zu polls %zu final_ms %.3f\n", nprompts, nchunks, nsteps, nlaunch, npolls, final_ms);
}
