// DEVICE CODE of libdeepprove_hip.so: every kernel body (KBODY) of the deep-prove hot path, the field / Poseidon2 / sumcheck device
// helpers they share, and the two CP-dispatched entry forms kg<Body> / kc<Body>. Included by hip_dev.hip inside namespace dp: the
// bodies behind kg<Body> (one proof, own stream) and kc<Body> (a lock-step cohort).
// (Round 3's resident executor — the same bodies behind two persistent worker kernels, csrc/rx.hip — measured 10-20 % slower than the
// cohorts and was removed in round 4; DESIGN.md §6 "Verdict on the executor" keeps the numbers, git history the code.)
// tests/support/kernel_emul/extract.py cuts device functions out of this file for the CPU SIMT emulator.
__constant__ u64 c_rc[DP_POSEIDON2_RC_WORDS];
__constant__ unsigned long long c_poll_timeout_ticks = 2000000000ull;  // 20 s of the 100 MHz constant clock (DP_POLL_TIMEOUT_S)
__device__ __forceinline__ unsigned long long dp_realtime() { return __builtin_amdgcn_s_memrealtime(); }
__constant__ int c_poll_sleep = 1;
#ifdef DP_DIAG_SKIP_HASH  // diagnostic build only (DP_HIPCC_EXTRA=-DDP_DIAG_SKIP_HASH, DP_LIB_VARIANT): the one-node-per-lane Merkle layers xor instead of hashing — invalid proofs, the
#define DP_SKIP_HASH_ON() (true)   // same launches and memory traffic: what the batch rate would be if Poseidon2 cost nothing (tools/r06/call18.sh)
#else
#define DP_SKIP_HASH_ON() (false)
#endif

constexpr int TPB = 256;
constexpr int MAX_TABS = 32;
constexpr int MAX_TERMS = 48;
constexpr int MAX_PT = 32;

struct PointArg { Ext p[MAX_PT]; };

// ------------------------------------------------------------------------------------------------ launch forms
// Every kernel of this file is written once, as a device function (KBODY), and gets TWO entry points:
//   kg<Body>  one proof: the arguments arrive by value in the kernarg segment;
//   kc<Body>  a cohort of proofs in lock step: ONE launch serves every proof of the cohort, blockIdx.z selects the proof and
//             the workgroup fetches ITS arguments from a table of argument packs (one ArgPack per proof, written by the host
//             into a mapped ring; tools/argsrc.hip: uniform reads of such a table cost what kernarg reads cost).
// blockIdx.x / blockIdx.y keep their meaning inside the body in both forms. See `Cohort` below for the host side.
#define KBODY __device__ __forceinline__ void
// values a reduce-and-publish body keeps in LDS (the host checks nout against it, HipDev::reduce_max)
constexpr int REDUCE_LDS_VALUES = 1024;
// LDS of a body: a frame is a static __shared__ object, the dynamic part the launch's dynamic LDS
#define DP_LDS_FRAME(T, f) __shared__ T f
#define DP_LDS_DYN0(name) extern __shared__ __align__(16) unsigned char name[]
#define DP_LDS_DYN(name, T) extern __shared__ __align__(16) unsigned char name[]
// lanes of ONE wave hand data to each other through LDS: the hardware runs a wave's LDS operations in order, the compiler must not move them across this point
#define DP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
template <class... A> struct ArgPack;
template <> struct ArgPack<> {
  template <class F, class... B> __device__ __forceinline__ void call(F f, const B&... b) const { f(b...); }
};
template <class H, class... T> struct ArgPack<H, T...> {
  H h; ArgPack<T...> t;
  ArgPack() = default;
  ArgPack(const H& h_, const T&... t_) : h(h_), t(t_...) {}
  template <class F, class... B> __device__ __forceinline__ void call(F f, const B&... b) const { t.call(f, b..., h); }
};
// parameter list of a body with references stripped: what travels (a body takes its large argument structs by const
// reference so that both entry points read them in place — kernarg segment / pack table — instead of copying them to scratch)
template <class T> struct KArgs;
template <class... A> struct KArgs<void (*)(A...)> {};
// FLAGS select how a one-workgroup (latency-critical) body shares the chip:
//   KF_CLAIM  latency mode, ONE proof on the GPU: the workgroup claims the whole register file of its CU (16 waves x 128 VGPRs;
//             with the LDS reservation of the launch no wave of another kernel can share the CU);
//   KF_PRIO   throughput mode, hundreds of proofs in flight: NO reservation at all — 256 threads, no LDS beyond what the body
//             needs — and raised wave priority instead (s_setprio 3: the SIMD's arbiter issues these waves first, the
//             Poseidon2 waves of the Merkle layers fill the remaining issue slots). A workgroup that needs an EMPTY CU stalls
//             the workgroup dispatcher until one drains, and the chip idles meanwhile: tools/hol.hip — two streams of
//             whole-CU workgroups (16 CUs, 6 % of the chip) halve the throughput of 14 streams of wide kernels, the same
//             serial work in 256-thread workgroups costs 9 %.
enum { KF_NONE = 0, KF_CLAIM = 1, KF_PRIO = 2, KF_HASH = 4 };
// DP_HASH_VGPRS (compile time, 0 = off; A/B builds): the bulk one-node-per-lane hash body (KF_HASH) is compiled for 256-thread workgroups and made to OWN that many
// VGPRs per lane (it needs 70): 168 -> three hash waves per SIMD instead of seven. What a retiring hash workgroup frees is then a hole on all four SIMDs of its CU
// that a protocol tail (154-200 VGPRs; DP_TAIL_WPE = 3 compiles the KF_PRIO forms for <= 168) or a streaming workgroup fits into, instead of a 72-register
// hole that only the next hash workgroup can take (NOTES_NEXT_ROUND.md: "tails that need a smaller hole", approached from the other side).
#ifndef DP_HASH_VGPRS
#define DP_HASH_VGPRS 0
#endif
#ifndef DP_TAIL_WPE
#define DP_TAIL_WPE 1
#endif
#define DP_STR2(x) #x
#define DP_STR(x) DP_STR2(x)
// DP_BASE_PRIO (compile time, 0 .. 2; A/B builds): the wave priority of EVERY kernel without KF_PRIO — the small kernels between the wide ones (k_publish, k_download,
// k_classic_reduce: 15-40 us alone, 1-1.8 ms each in the cohort regime, profiles/r05_bench448_kernel_stats.csv) and the streaming kernels of the batch opening;
// the one-node-per-lane Poseidon2 bodies (dp_hash_prio) go back to 0, so that hash waves — always ready, never waiting for memory, the oldest on their SIMD —
// only take the issue slots nobody else wants (tools/r04/contend.hip: a priority-0 wave next to 8 hashing workgroups per CU is 550 x slower).
// Default 2 since round 6 (tools/r06/call22.sh, 12 waves of 448 Dense-4M proofs, alternating with the priority-0 build on one box, both with DP_WIDE_WG_CAP=256): 1 077 / 1 057
// against 976 / 998 proofs/s, 1 112 against 1 021 at 660 in flight, CNN-264k 720 against 657. (Round 6's first A/B, without the grid cap, had it inside the noise.)
#ifndef DP_BASE_PRIO
#define DP_BASE_PRIO 2
#endif
template <int FLAGS> __device__ __forceinline__ void kf_prologue() {
  if (FLAGS & KF_CLAIM) asm volatile("v_mov_b32 v127, 0" ::: "v127");
  if (FLAGS & KF_PRIO) __builtin_amdgcn_s_setprio(3);
  else if (DP_BASE_PRIO) __builtin_amdgcn_s_setprio(DP_BASE_PRIO);
#if DP_HASH_VGPRS
  if (FLAGS & KF_HASH) asm volatile("v_mov_b32 v" DP_STR(DP_HASH_TOUCH) ", 0" ::: "v" DP_STR(DP_HASH_TOUCH));
#endif
}
template <int FLAGS> constexpr int kf_min_waves() { return (FLAGS & KF_PRIO) ? DP_TAIL_WPE : 1; }
__device__ __forceinline__ void dp_hash_prio() { if (DP_BASE_PRIO) __builtin_amdgcn_s_setprio(0); }
template <auto Body, int MAXT, int FLAGS, class... A> __global__ void __launch_bounds__(MAXT, kf_min_waves<FLAGS>()) kg(A... a) { kf_prologue<FLAGS>(); Body(a...); }
#ifdef DP_WG_TIMES
// DIAGNOSTIC BUILD ONLY (DP_HIPCC_EXTRA=-DDP_WG_TIMES, tools/wg_times.py): every workgroup of k_logup_tail records when it entered and
// left, on which CU, and which merged launch it belonged to (the address of the launch's argument packs) — how much of a merged
// launch's duration is the spread between its fastest and its slowest member?
__shared__ unsigned long long s_dbg_launch;
__device__ unsigned long long g_wgt[4 * 65536];
__device__ unsigned g_wgt_n;
__device__ unsigned long long g_sponge_ticks, g_sponge_perms, g_member_ticks;  // k_logup_tail: time inside wc_duplex, permutations, entry -> exit
__device__ unsigned long long g_phase_ticks[16];  // k_logup_tail: sponge-free time of wave 0 by phase (DBG_PHASE below): 0 tree, 1 layer set-up, 2 passes, 3 message + challenge, 4 layer end, 5 column claims, 6 tail, 7 launches
__device__ __forceinline__ void dbg_sponge_record(unsigned long long t_in, unsigned long long sp, unsigned long long np) {
  atomicAdd(&g_sponge_ticks, sp); atomicAdd(&g_sponge_perms, np); atomicAdd(&g_member_ticks, dp_realtime() - t_in);
}
__device__ __forceinline__ void dbg_wg_record(unsigned long long t_in) {
  unsigned i = atomicAdd(&g_wgt_n, 1u);
  if (i >= 65536) return;
  unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID, all 32 bits
  unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11));  // HW_REG_XCC_ID, 4 bits
  g_wgt[4 * i] = t_in; g_wgt[4 * i + 1] = dp_realtime(); g_wgt[4 * i + 2] = s_dbg_launch;
  g_wgt[4 * i + 3] = (unsigned long long)hw | ((unsigned long long)xcc << 32) | ((unsigned long long)blockIdx.z << 40);
}
template <auto Body, int MAXT, int FLAGS, class... A> __global__ void __launch_bounds__(MAXT, kf_min_waves<FLAGS>()) kc(const ArgPack<A...>* __restrict__ packs) { kf_prologue<FLAGS>(); if (threadIdx.x == 0) s_dbg_launch = (unsigned long long)packs; packs[blockIdx.z].call(Body); }
#else
template <auto Body, int MAXT, int FLAGS, class... A> __global__ void __launch_bounds__(MAXT, kf_min_waves<FLAGS>()) kc(const ArgPack<A...>* __restrict__ packs) { kf_prologue<FLAGS>(); packs[blockIdx.z].call(Body); }
#endif

// ------------------------------------------------------------------------------------------------ reductions
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int d) {
  int lo = __shfl_down((int)(u32)v, d, 64);
  int hi = __shfl_down((int)(u32)(v >> 32), d, 64);
  return ((u64)(u32)hi << 32) | (u64)(u32)lo;
}
__device__ __forceinline__ Ext wave_reduce_ext(Ext v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Ext o = ex(shfl_down_u64(v.c0, d), shfl_down_u64(v.c1, d));
    v = ex_add(v, o);
  }
  return v;
}
// sum over the block; result valid in thread 0. `sm` must hold TPB/64 Ext values.
__device__ __forceinline__ Ext block_reduce_ext(Ext v, Ext* sm) {
  v = wave_reduce_ext(v);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  Ext r = ex_zero();
  if (threadIdx.x == 0) {
    r = sm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) r = ex_add(r, sm[i]);
  }
  return r;
}
__device__ __forceinline__ Ext ld_elem(const void* p, bool ext, size_t i) {
  if (ext) return ((const Ext*)p)[i];
  return ex_base(((const u64*)p)[i]);
}

// ------------------------------------------------------------------------------------------------ elementwise
KBODY k_copy_words(u64* dst, const u64* src, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
KBODY k_zero_words(u64* dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = 0;
}
KBODY k_fieldize(const int64_t* in, u64* out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = gl_from_i64(in[i]);
}
KBODY k_pow_table(u64* out, u64 base, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = gl_pow(base, i);
}
// K4: eq(x, pt) computed per index as a product over its bits (k ext multiplications per element, no log-k passes)
KBODY k_eq_table(Ext* out, const PointArg& pt, unsigned k, Ext scale, int acc, size_t n) {  // n > 2^k: the table repeats
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Ext v = scale;
    for (unsigned t = 0; t < k; t++) {
      Ext r = pt.p[t];
      v = ex_mul(v, ((i >> t) & 1) ? r : ex_sub(ex_one(), r));
    }
    out[i] = acc ? ex_add(out[i], v) : v;
  }
}
struct EvalArgs { const void* f[8]; int ext[8]; int nf; };
// out partial[block][f] = sum over the block's x of f(x) * eq(x, pt)
KBODY k_mle_eval_partial(const EvalArgs& a, const PointArg& pt, unsigned k, Ext* partial) {
  __shared__ Ext sm[TPB / 64];
  size_t n = size_t(1) << k;
  Ext acc[8];
#pragma unroll
  for (int f = 0; f < 8; f++) acc[f] = ex_zero();
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Ext e = ex_one();
    for (unsigned t = 0; t < k; t++) {
      Ext r = pt.p[t];
      e = ex_mul(e, ((i >> t) & 1) ? r : ex_sub(ex_one(), r));
    }
#pragma unroll
    for (int f = 0; f < 8; f++)
      if (f < a.nf) acc[f] = ex_add(acc[f], a.ext[f] ? ex_mul(e, ((const Ext*)a.f[f])[i]) : ex_mul_base(e, ((const u64*)a.f[f])[i]));
  }
#pragma unroll
  for (int f = 0; f < 8; f++) {
    if (f < a.nf) {
      Ext r = block_reduce_ext(acc[f], sm);
      if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 8 + f] = r;
    }
  }
}
// generic second stage: out[j] = sum_b partial[b*stride + j], one block per j
KBODY k_reduce_partials(const Ext* partial, size_t nblocks, size_t stride, Ext* out) {
  __shared__ Ext sm[TPB / 64];
  size_t j = blockIdx.x;
  Ext acc = ex_zero();
  for (size_t b = threadIdx.x; b < nblocks; b += blockDim.x) acc = ex_add(acc, partial[b * stride + j]);
  Ext r = block_reduce_ext(acc, sm);
  if (threadIdx.x == 0) out[j] = r;
}
// K2 one pass: partial[split][c] = sum over the split's rows of eq[r] * W[r*C + c]
KBODY k_fix_high_partial(const u64* W, const Ext* eq, size_t R, size_t C, size_t rows_per_split, Ext* partial) {
  size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= C) return;
  size_t r0 = blockIdx.y * rows_per_split, r1 = min(R, r0 + rows_per_split);
  Ext acc = ex_zero();
  for (size_t r = r0; r < r1; r++) acc = ex_add(acc, ex_mul_base(eq[r], W[r * C + c]));
  partial[(size_t)blockIdx.y * C + c] = acc;
}
// Dev::fix_low: out[r] = sum_c eq[c] * W[r][c] — one wave per row of a row-major base table, lanes stride along the row (coalesced);
// HBM-bound: the table is read once (8 R C bytes), eq (16 C bytes) stays in cache
KBODY k_fix_low(const u64* W, const Ext* eq, Ext* out, size_t R, size_t C) {
  const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < R; r += nwaves) {
    const u64* row = W + r * C;
    Ext acc = ex_zero();
    for (size_t c = lane; c < C; c += 64) acc = ex_add(acc, ex_mul_base(eq[c], row[c]));
    acc = wave_reduce_ext(acc);
    if (lane == 0) out[r] = acc;
  }
}
KBODY k_colsum(const Ext* partial, size_t nsplit, size_t C, Ext* out) {
  size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (c >= C) return;
  Ext acc = ex_zero();
  for (size_t s = 0; s < nsplit; s++) acc = ex_add(acc, partial[s * C + c]);
  out[c] = acc;
}

// ------------------------------------------------------------------------------------------------ sumcheck (K1, K3)
struct FoldArgs { const void* in[MAX_TABS]; Ext* out[MAX_TABS]; int ext[MAX_TABS]; size_t half[MAX_TABS]; };
// K1: out[i] = in[2i] + r (in[2i+1] - in[2i]); blockIdx.y selects the table
KBODY k_fold(const FoldArgs& a, Ext r) {
  int t = blockIdx.y;
  size_t h = a.half[t];
  const void* in = a.in[t];
  Ext* out = a.out[t];
  if (a.ext[t]) {
    const Ext* p = (const Ext*)in;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x) out[i] = ex_lerp(p[2 * i], p[2 * i + 1], r);
  } else {
    const u64* p = (const u64*)in;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x) out[i] = ex_lerp_base(p[2 * i], p[2 * i + 1], r);
  }
}
constexpr int SC_SLOTS = SC_MAXK + 1;  // evaluations at t = 0..k of a degree-k term, k <= SC_MAXK
// The round sums of ONE product term over the pairs start, start + stride, .. < npairs: acc[t] += prod_j (lo_j + t (hi_j - lo_j)).
// `L(j, b, lo, hi)` loads pair b of the j-th factor. Degrees 1..3 (every sumcheck of the Dense / logup / Basefold path)
// keep their hand-scheduled bodies; degrees 4 and 5 (the maxpool zero-check) walk t with forward differences.
// HI = false: degrees 1..3 only (every sumcheck of the Dense / logup / Basefold path); HI = true adds degrees 4 and 5 (the
// maxpool zero-check), walking t = 0..5 with forward differences. Kernels are instantiated for both so that the register
// needs of the high-degree body never weigh on the common case.
template <bool HI, class PairLoader>
__device__ __forceinline__ void sc_accumulate(int k, PairLoader L, size_t start, size_t stride, size_t npairs, Ext (&acc)[SC_SLOTS]) {
#pragma unroll
  for (int t = 0; t < SC_SLOTS; t++) acc[t] = ex_zero();
  if (k == 1) {
    for (size_t b = start; b < npairs; b += stride) { Ext a0, b0; L(0, b, a0, b0); acc[0] = ex_add(acc[0], a0); acc[1] = ex_add(acc[1], b0); }
  } else if (k == 2) {
    for (size_t b = start; b < npairs; b += stride) {
      Ext a0, b0, a1, b1; L(0, b, a0, b0); L(1, b, a1, b1);
      Ext c0 = ex_sub(ex_dbl(b0), a0), c1 = ex_sub(ex_dbl(b1), a1);  // value at t = 2
      acc[0] = ex_add(acc[0], ex_mul(a0, a1)); acc[1] = ex_add(acc[1], ex_mul(b0, b1)); acc[2] = ex_add(acc[2], ex_mul(c0, c1));
    }
  } else if (!HI || k == 3) {
    for (size_t b = start; b < npairs; b += stride) {
      Ext a0, b0, a1, b1, a2, b2; L(0, b, a0, b0); L(1, b, a1, b1); L(2, b, a2, b2);
      Ext d0 = ex_sub(b0, a0), d1 = ex_sub(b1, a1), d2 = ex_sub(b2, a2);
      Ext c0 = ex_add(b0, d0), c1 = ex_add(b1, d1), c2 = ex_add(b2, d2);  // t = 2
      Ext f0 = ex_add(c0, d0), f1 = ex_add(c1, d1), f2 = ex_add(c2, d2);  // t = 3
      acc[0] = ex_add(acc[0], ex_mul(ex_mul(a0, a1), a2)); acc[1] = ex_add(acc[1], ex_mul(ex_mul(b0, b1), b2));
      acc[2] = ex_add(acc[2], ex_mul(ex_mul(c0, c1), c2)); acc[3] = ex_add(acc[3], ex_mul(ex_mul(f0, f1), f2));
    }
  } else if (HI) {
    for (size_t b = start; b < npairs; b += stride) {
      Ext cur[SC_MAXK], d[SC_MAXK];
#pragma unroll
      for (int j = 0; j < SC_MAXK; j++) {
        if (j < k) { Ext lo, hi; L(j, b, lo, hi); cur[j] = lo; d[j] = ex_sub(hi, lo); }
        else { cur[j] = ex_one(); d[j] = ex_zero(); }
      }
#pragma unroll
      for (int t = 0; t < SC_SLOTS; t++) {
        Ext p = ex_mul(ex_mul(cur[0], cur[1]), ex_mul(cur[2], cur[3]));
        if (k == 5) p = ex_mul(p, cur[4]);
        acc[t] = ex_add(acc[t], p);
#pragma unroll
        for (int j = 0; j < SC_MAXK; j++) cur[j] = ex_add(cur[j], d[j]);
      }
    }
  }
}
// number of factor slots a kernel instantiation has to wire up
template <bool HI> struct ScW { static constexpr int K = HI ? SC_MAXK : 3; };
// pair loader over tables in global memory (natural order: pair b = elements 2b, 2b+1), base or extension per table
struct GlobalPairs {
  const void* p[SC_MAXK]; bool e[SC_MAXK];
  __device__ __forceinline__ void operator()(int j, size_t b, Ext& lo, Ext& hi) const { lo = ld_elem(p[j], e[j], 2 * b); hi = ld_elem(p[j], e[j], 2 * b + 1); }
};
// pair loader over LDS-resident tables kept in bit-reversed order: pair q = positions q, q + h
struct LdsPairs {
  const Ext* p[SC_MAXK]; size_t h;
  __device__ __forceinline__ void operator()(int j, size_t q, Ext& lo, Ext& hi) const { lo = p[j][q]; hi = p[j][q + h]; }
};
struct TermArgs { const void* tab[MAX_TABS]; int ext[MAX_TABS]; int k[MAX_TERMS]; int t[MAX_TERMS][SC_MAXK]; size_t npairs; };
// K3: partial[(term*gridDim.x + block)*SC_SLOTS + t] = sum over the block's pairs of prod_j (a_j + t d_j), t = 0..k
template <bool HI>
KBODY k_sc_terms(const TermArgs& a, Ext* partial) {
  __shared__ Ext sm[TPB / 64];
  int term = blockIdx.y;
  int k = a.k[term];
  Ext acc[SC_SLOTS];
  bool all_base = k <= 3;
  for (int j = 0; j < k; j++) all_base = all_base && !a.ext[a.t[term][j]];
  if (all_base) {
    // every factor is a base-field table (first round of a sumcheck over committed columns): stay in the base field,
    // as the reference macro does (sumcheck_macro/src/lib.rs:283-296), one 16-byte load per table and pair
    const void* p0 = a.tab[a.t[term][0]]; const void* p1 = a.tab[a.t[term][k > 1 ? 1 : 0]]; const void* p2 = a.tab[a.t[term][k > 2 ? 2 : 0]];
    // (round 6: the products are the any-representative multiplication of poseidon2_fast.h / gl64_gfx950.h — 12 VALU instructions instead of the canonical
    // gl_mul's 16 — and the running sums exact integers of 64 + 32 bits reduced once per thread (3 instead of 9): the 2^24-entry first round of BASELINE config 5
    // ran at 3.65 TB/s. Same field elements: what leaves the thread is canonical.)
    p2f::W s0 = p2f::w_of(0), s1 = p2f::w_of(0), s2 = p2f::w_of(0), s3 = p2f::w_of(0);
    auto step3 = [&](ulonglong2 x0, ulonglong2 x1, ulonglong2 x2) {
      u64 d0 = gl_sub(x0.y, x0.x), d1 = gl_sub(x1.y, x1.x), d2 = gl_sub(x2.y, x2.x);
      u64 c0 = gl_add(x0.y, d0), c1 = gl_add(x1.y, d1), c2 = gl_add(x2.y, d2);
      u64 g0 = gl_add(c0, d0), g1 = gl_add(c1, d1), g2 = gl_add(c2, d2);
      s0 = p2f::w_add64(s0, p2f::mul(p2f::mul(x0.x, x1.x), x2.x)); s1 = p2f::w_add64(s1, p2f::mul(p2f::mul(x0.y, x1.y), x2.y));
      s2 = p2f::w_add64(s2, p2f::mul(p2f::mul(c0, c1), c2)); s3 = p2f::w_add64(s3, p2f::mul(p2f::mul(g0, g1), g2));
    };
    const size_t gstride = (size_t)gridDim.x * blockDim.x;
    if (k == 3) {
      // two pairs per trip, their six 16-byte loads issued before the first product: the kernel is a stream of three tables with ~190 instructions per 48 bytes
      for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < a.npairs; b += 2 * gstride) {
        const size_t b2 = b + gstride < a.npairs ? b + gstride : b;
        const ulonglong2 x0 = ((const ulonglong2*)p0)[b], x1 = ((const ulonglong2*)p1)[b], x2 = ((const ulonglong2*)p2)[b];
        const ulonglong2 y0 = ((const ulonglong2*)p0)[b2], y1 = ((const ulonglong2*)p1)[b2], y2 = ((const ulonglong2*)p2)[b2];
        step3(x0, x1, x2);
        if (b2 != b) step3(y0, y1, y2);
      }
    } else
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < a.npairs; b += gstride) {
      ulonglong2 x0 = ((const ulonglong2*)p0)[b];
      if (k == 1) { s0 = p2f::w_add64(s0, x0.x); s1 = p2f::w_add64(s1, x0.y); }
      else if (k == 2) {
        ulonglong2 x1 = ((const ulonglong2*)p1)[b];
        u64 c0 = gl_sub(gl_dbl(x0.y), x0.x), c1 = gl_sub(gl_dbl(x1.y), x1.x);
        s0 = p2f::w_add64(s0, p2f::mul(x0.x, x1.x)); s1 = p2f::w_add64(s1, p2f::mul(x0.y, x1.y)); s2 = p2f::w_add64(s2, p2f::mul(c0, c1));
      }
    }
    acc[0] = ex_base(p2f::canon(p2f::w_reduce(s0))); acc[1] = ex_base(p2f::canon(p2f::w_reduce(s1))); acc[2] = ex_base(p2f::canon(p2f::w_reduce(s2))); acc[3] = ex_base(p2f::canon(p2f::w_reduce(s3)));
    acc[4] = ex_zero(); acc[5] = ex_zero();
  } else {
    GlobalPairs L;
#pragma unroll
    for (int j = 0; j < ScW<HI>::K; j++) { int ti = a.t[term][j < k ? j : 0]; L.p[j] = a.tab[ti]; L.e[j] = a.ext[ti]; }
    sc_accumulate<HI>(k, L, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, a.npairs, acc);
  }
  size_t base = ((size_t)term * gridDim.x + blockIdx.x) * SC_SLOTS;
#pragma unroll
  for (int t = 0; t < SC_SLOTS; t++) {
    if (t <= k) { Ext r = block_reduce_ext(acc[t], sm); if (threadIdx.x == 0) partial[base + t] = r; }
    else if (threadIdx.x == 0) partial[base + t] = ex_zero();
  }
}
// out[term*4 + t] = sum_b partial[(term*nblocks + b)*4 + t]; one block per (term, t)
KBODY k_reduce_terms(const Ext* partial, size_t nblocks, Ext* out) {
  __shared__ Ext sm[TPB / 64];
  size_t term = blockIdx.x >> 2, t = blockIdx.x & 3;
  Ext acc = ex_zero();
  for (size_t b = threadIdx.x; b < nblocks; b += blockDim.x) acc = ex_add(acc, partial[(term * nblocks + b) * 4 + t]);
  Ext r = block_reduce_ext(acc, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}
// K3' (SURVEY.md 2.3): fused fold + round sums for ONE product of K equally typed large tables. Each lane takes 4
// consecutive elements of every table (32 contiguous bytes for base tables, 64 for extension tables), folds them with r
// into 2 values, stores those (32 contiguous bytes) and immediately accumulates the next round's sums on that pair —
// every table byte is read once and every folded byte written once per round (the unfused path reads the folded
// table a second time). partial[block*4 + t] = sum over the block's pairs of prod_j (f0_j + t (f1_j - f0_j)).
// SKIP1: the caller knows the round's claimed sum s(0) + s(1), so the t = 1 products are not computed (slot 1 stays 0
// and the host sets s(1) = claim - s(0)): 2 of the 8 extension products per pair less.
// `counter` non-null: the last workgroup to finish adds up the block sums of all workgroups and publishes the four sums to the host itself — no k_reduce_publish
// launch between two rounds of a large sumcheck (the last-workgroup epilogue below).
__device__ void sc_publish_vals_fwd(Ext* result, const Ext* src, size_t stride, int n, unsigned long long* flag, unsigned long long seq, int lane);
// ---- the last-workgroup epilogue of the streaming round kernels (k_sc_fused, k_sc_terms2, k_sc_fused2, k_bf_msg, k_bf_fold_msg: sc_block_sums_finish; k_classic_fused_pub)
// Every workgroup stores its block sums, then takes a ticket; whoever draws the last one adds all block sums up, publishes the round's sums to the host and puts the
// ticket back to zero. The block sums must reach that workgroup — possibly on another XCD, behind another L2, and the per-XCD L2s are not coherent with each other.
//  * Written through, not fenced: an agent-scope release fence per workgroup writes the XCD's whole L2 back (the folded tables the kernel has just written), thousands of
//    times per launch — 7x slower than a second launch. Instead the few block sums are WRITTEN THROUGH every cache level (system-scope relaxed stores, the idiom of every
//    host publication of this file), thread 0 waits for their acknowledgement (gfx9 counts stores in vmcnt) and only then takes the ticket, a relaxed memory-side atomic.
//  * The last workgroup reads every block sum PAST its own L2 (system-scope relaxed loads): no acquire fence, no invalidation of the bulk data. This rests on how the
//    caches treat system-scope accesses, which the HIP memory model does not spell out (tests/test_gpu_sharded.py, the ticket test, says what is relied on).
//  * ONE ticket word per context is enough: the host waits for what such a kernel publishes before the context launches anything else, a context launches on one
//    stream (its own, or its cohort's, where every blockIdx.z brings its own ticket, result and flag), and the zero is written back before the kernel ends.
__device__ __forceinline__ void sc_store_through(Ext* p, Ext v) {
  __hip_atomic_store((u64*)p, v.c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __hip_atomic_store((u64*)p + 1, v.c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ bool sums_ticket_take(unsigned* counter) {  // after thread 0's sc_store_through calls; true in every thread of the workgroup that drew the last ticket
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  return s_last;
}
__device__ __forceinline__ Ext ld_through(const Ext* p) {
  return ex(__hip_atomic_load((const u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), __hip_atomic_load((const u64*)p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ void sums_ticket_return(unsigned* counter) {  // one thread, after the publication: the next launch of this context starts from zero
  __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// partial[NV * block + i] = the block's sum of vals[i]; `counter` non-null: the epilogue above, the NV sums published to `result` under `seq`
template <int NV>
__device__ __forceinline__ void sc_block_sums_finish(const Ext* vals, Ext* sm, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  const size_t base = (size_t)blockIdx.x * NV;
  if (counter) {
#pragma unroll
    for (int i = 0; i < NV; i++) { Ext v = block_reduce_ext(vals[i], sm); if (threadIdx.x == 0) sc_store_through(&partial[base + i], v); }
    __shared__ Ext res[NV];
    if (sums_ticket_take(counter)) {
      const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
      for (int i = wave; i < NV; i += nwaves) {
        Ext acc = ex_zero();
        for (unsigned b = lane; b < gridDim.x; b += 64) acc = ex_add(acc, ld_through(&partial[(size_t)b * NV + i]));
        acc = wave_reduce_ext(acc);
        if (lane == 0) res[i] = acc;
      }
      __syncthreads();
      if (wave == 0) sc_publish_vals_fwd(result, res, 1, NV, flag, seq, lane);
      if (threadIdx.x == 0) sums_ticket_return(counter);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NV; i++) { Ext v = block_reduce_ext(vals[i], sm); if (threadIdx.x == 0) partial[base + i] = v; }
}
// the round sums of one folded pair of K tables: acc_t += prod_j (f0_j + t (f1_j - f0_j)), t = 0 .. K (t = 1 left out with SKIP1), shared by k_sc_fused and k_sc_fused2
template <int K, bool SKIP1>
__device__ __forceinline__ void sc_prod_acc(const Ext (&f0)[K], const Ext (&f1)[K], lz::ExAcc& acc0, lz::ExAcc& acc1, lz::ExAcc& acc2, lz::ExAcc& acc3) {
  if (K == 1) { lz::acc_add(acc0, f0[0]); if (!SKIP1) lz::acc_add(acc1, f1[0]); }
  else if (K == 2) {
    Ext c0 = ex_sub(ex_dbl(f1[0]), f0[0]), c1 = ex_sub(ex_dbl(f1[1]), f0[1]);
    lz::acc_add(acc0, lz::ex_mul(f0[0], f0[1])); if (!SKIP1) lz::acc_add(acc1, lz::ex_mul(f1[0], f1[1])); lz::acc_add(acc2, lz::ex_mul(c0, c1));
  } else {
    Ext d0 = ex_sub(f1[0], f0[0]), d1 = ex_sub(f1[1], f0[1]), d2 = ex_sub(f1[2], f0[2]);
    Ext c0 = ex_add(f1[0], d0), c1 = ex_add(f1[1], d1), c2 = ex_add(f1[2], d2);
    Ext g0 = ex_add(c0, d0), g1 = ex_add(c1, d1), g2 = ex_add(c2, d2);
    lz::acc_add(acc0, lz::ex_mul(lz::ex_mul(f0[0], f0[1]), f0[2])); if (!SKIP1) lz::acc_add(acc1, lz::ex_mul(lz::ex_mul(f1[0], f1[1]), f1[2]));
    lz::acc_add(acc2, lz::ex_mul(lz::ex_mul(c0, c1), c2)); lz::acc_add(acc3, lz::ex_mul(lz::ex_mul(g0, g1), g2));
  }
}
template <int K, bool BASE, bool SKIP1>
KBODY k_sc_fused(const void* in0, const void* in1, const void* in2, Ext* out0, Ext* out1, Ext* out2,
                                                  size_t nquads, Ext r, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  const void* in[3] = {in0, in1, in2};
  Ext* out[3] = {out0, out1, out2};
  // The kernel is VALU-bound (93 % of the issue slots in its base-table round, profiles/r02_pmc_sq_sumcheck24.json), so the
  // field arithmetic is the lazy kind of gl64_lazy.h: folds as one fused multiply-add with a single reduction per limb,
  // extension products schoolbook with two reductions, running sums as exact integers reduced once per thread. What is STORED is
  // canonical (other kernels read the folded tables), what is multiplied is any representative.
  lz::ExAcc acc0 = lz::acc_zero(), acc1 = lz::acc_zero(), acc2 = lz::acc_zero(), acc3 = lz::acc_zero();
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquads; q += (size_t)gridDim.x * blockDim.x) {
    Ext f0[K], f1[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (BASE) {
        const ulonglong2* p = (const ulonglong2*)((const u64*)in[j] + 4 * q);
        ulonglong2 a = p[0], b = p[1];
        f0[j] = lz::ex_canon(lz::ex_fma_base(r, gl_sub(a.y, a.x), a.x));
        f1[j] = lz::ex_canon(lz::ex_fma_base(r, gl_sub(b.y, b.x), b.x));
      } else {
        const Ext* p = (const Ext*)in[j] + 4 * q;
        Ext e0 = p[0], e1 = p[1], e2 = p[2], e3 = p[3];
        f0[j] = lz::ex_canon(lz::ex_fma(r, ex_sub(e1, e0), e0));
        f1[j] = lz::ex_canon(lz::ex_fma(r, ex_sub(e3, e2), e2));
      }
      out[j][2 * q] = f0[j];
      out[j][2 * q + 1] = f1[j];
    }
    sc_prod_acc<K, SKIP1>(f0, f1, acc0, acc1, acc2, acc3);
  }
  Ext vals[4] = {lz::acc_value(acc0), lz::acc_value(acc1), lz::acc_value(acc2), lz::acc_value(acc3)};
  sc_block_sums_finish<4>(vals, sm, partial, counter, result, flag, seq);
}
// ---- the first TWO rounds of one product of K base-field tables in one pass, and both folds in one pass (round 6; Dev::sc_round, "grid2")
// Round 1 needs no challenge, and round 2's polynomial is a polynomial of degree K in the FIRST challenge: with f_j(X1, X2, x') the bilinear extension of a
// table's four neighbours (index 4 q + x1 + 2 x2),  A[u1][u2] = sum_q prod_j f_j(u1, u2, q)  over a 4 x 4 grid of points determines the polynomial Q(X1, X2) = sum_q prod_j f_j
// (degree K in each variable): the round-1 message is s1(t) = Q(t, 0) + Q(t, 1) at once and, after r1 exists, the round-2 message is s2(t) = Q(r1, t), both evaluated on the
// host — exact field arithmetic, the same field elements the two streaming rounds produce, i.e. the same proof bytes (prover.rs:498-585 is what is matched). The
// base tables are then read ONCE more: k_sc_fused2 folds both variables (f = e0 + r2 (e1 - e0), e = a + r1 (b - a)), writes tables a QUARTER as long and
// sums round 3. Against k_sc_terms + two k_sc_fused launches that is 1.0 instead of 1.8 GB of traffic at 3 x 2^24 entries and one host round trip less.
// The sixteen sums are base-field values; they travel as eight (c0, c1) pairs through the extension-field reductions (an extension addition is limb-wise).
// The grid is chip-sized (768 workgroups: three 140-register waves per SIMD, all resident at once) and every thread walks ~20 quads with the next quad's loads in
// flight while it multiplies (~600 VALU instructions per quad: 32 multiplications of 12, 36 subtractions, 16 wide sums): with 4096 workgroups of 4 quads per thread
// the eight block reductions cost a third of the work again and nothing covered the load latency — 199 us at 3 x 2^24 entries against 105 us for k_sc_terms.
template <int K>
KBODY k_sc_terms2(const void* in0, const void* in1, const void* in2, size_t nquads, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  const void* in[3] = {in0, in1, in2};
  p2f::W acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = p2f::w_of(0);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  ulonglong2 na[K], nb[K];
  if (q < nquads) {
#pragma unroll
    for (int j = 0; j < K; j++) { const ulonglong2* p = (const ulonglong2*)((const u64*)in[j] + 4 * q); na[j] = p[0]; nb[j] = p[1]; }
  }
  for (; q < nquads; q += stride) {
    // The grid is taken at the points {0, 1, oo, -1} of each variable ("oo": the leading coefficient, i.e. the product of the slopes): a row IS its values at 0 and 1, its
    // difference IS its slope, and -1 costs one more subtraction — 12 modular subtractions per table and quad where the points {0, 1, 2, 3} took 21 additions (a fifth of
    // the kernel's instructions). The host rebuilds each cubic from three values and its leading coefficient (hip_dev.hip, grid2_coeffs). pt[j][2 i + x2]: row x2 of table j at the i-th point of x1.
    u64 pt[K][8];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const ulonglong2 a = na[j], b = nb[j];
      const u64 d0 = gl_sub(a.y, a.x), d1 = gl_sub(b.y, b.x);
      pt[j][0] = a.x; pt[j][1] = b.x; pt[j][2] = a.y; pt[j][3] = b.y; pt[j][4] = d0; pt[j][5] = d1; pt[j][6] = gl_sub(a.x, d0); pt[j][7] = gl_sub(b.x, d1);
    }
    if (q + stride < nquads) {
#pragma unroll
      for (int j = 0; j < K; j++) { const ulonglong2* p = (const ulonglong2*)((const u64*)in[j] + 4 * (q + stride)); na[j] = p[0]; nb[j] = p[1]; }
    }
#pragma unroll
    for (int u1 = 0; u1 < 4; u1++) {
      u64 pr[4];
#pragma unroll
      for (int j = 0; j < K; j++) {
        const u64 c0 = pt[j][2 * u1], c1 = pt[j][2 * u1 + 1], e = gl_sub(c1, c0), m = gl_sub(c0, e);  // u2 = 0, 1, oo, -1
        if (j == 0) { pr[0] = c0; pr[1] = c1; pr[2] = e; pr[3] = m; }
        else { pr[0] = p2f::mul(pr[0], c0); pr[1] = p2f::mul(pr[1], c1); pr[2] = p2f::mul(pr[2], e); pr[3] = p2f::mul(pr[3], m); }
      }
#pragma unroll
      for (int u2 = 0; u2 < 4; u2++) acc[u1 * 4 + u2] = p2f::w_add64(acc[u1 * 4 + u2], pr[u2]);
    }
  }
  Ext vals[8];
#pragma unroll
  for (int i = 0; i < 8; i++) vals[i] = ex(p2f::canon(p2f::w_reduce(acc[2 * i])), p2f::canon(p2f::w_reduce(acc[2 * i + 1])));
  sc_block_sums_finish<8>(vals, sm, partial, counter, result, flag, seq);
}
// both folds of k_sc_terms2's two rounds and the sums of the round after: thread q turns 8 base entries of every table into 2 extension entries
template <int K, bool SKIP1>
KBODY k_sc_fused2(const void* in0, const void* in1, const void* in2, Ext* out0, Ext* out1, Ext* out2,
                  size_t nocts, Ext r1, Ext r2, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  const void* in[3] = {in0, in1, in2};
  Ext* out[3] = {out0, out1, out2};
  lz::ExAcc acc0 = lz::acc_zero(), acc1 = lz::acc_zero(), acc2 = lz::acc_zero(), acc3 = lz::acc_zero();
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nocts; q += (size_t)gridDim.x * blockDim.x) {
    Ext f0[K], f1[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const ulonglong2* p = (const ulonglong2*)((const u64*)in[j] + 8 * q);
      const ulonglong2 a = p[0], b = p[1], c = p[2], d = p[3];
      const Ext ea = lz::ex_canon(lz::ex_fma_base(r1, gl_sub(a.y, a.x), a.x)), eb = lz::ex_canon(lz::ex_fma_base(r1, gl_sub(b.y, b.x), b.x));
      const Ext ec = lz::ex_canon(lz::ex_fma_base(r1, gl_sub(c.y, c.x), c.x)), ed = lz::ex_canon(lz::ex_fma_base(r1, gl_sub(d.y, d.x), d.x));
      f0[j] = lz::ex_canon(lz::ex_fma(r2, ex_sub(eb, ea), ea));
      f1[j] = lz::ex_canon(lz::ex_fma(r2, ex_sub(ed, ec), ec));
      out[j][2 * q] = f0[j];
      out[j][2 * q + 1] = f1[j];
    }
    sc_prod_acc<K, SKIP1>(f0, f1, acc0, acc1, acc2, acc3);
  }
  Ext vals[4] = {lz::acc_value(acc0), lz::acc_value(acc1), lz::acc_value(acc2), lz::acc_value(acc3)};
  sc_block_sums_finish<4>(vals, sm, partial, counter, result, flag, seq);
}
// last fold of a sumcheck: every table has 2 elements; results go to one contiguous array
KBODY k_finish(const FoldArgs& a, Ext r, int ntabs, Ext* out) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntabs) return;
  Ext v;
  if (a.ext[t]) { const Ext* p = (const Ext*)a.in[t]; v = ex_lerp(p[0], p[1], r); }
  else { const u64* p = (const u64*)a.in[t]; v = ex_lerp_base(p[0], p[1], r); }
  out[t] = v;
}

// ------------------------------------------------------------------------------------------------ logup (K13)
struct ColsArg { const u64* col[16]; int n; };
KBODY k_logup_den(Ext* out, const ColsArg& cols, Ext c, Ext chi, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Ext acc = c, pw = ex_one();
    for (int j = 0; j < cols.n; j++) {
      acc = ex_add(acc, ex_mul_base(pw, cols.col[j][i]));
      pw = ex_mul(pw, chi);
    }
    out[i] = acc;
  }
}
// (n1/d1 + n2/d2) pairing index i with i + half;  num_mode: 0 = all numerators are -1, 1 = base numerators, 2 = ext
KBODY k_logup_layer(const void* num, int num_mode, const Ext* den, Ext* num_out, Ext* den_out, size_t half) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < half; i += (size_t)gridDim.x * blockDim.x) {
    Ext d1 = den[i], d2 = den[i + half];
    Ext nn;
    if (num_mode == 0) nn = ex_neg(ex_add(d1, d2));
    else if (num_mode == 1) { const u64* p = (const u64*)num; nn = ex_add(ex_mul_base(d2, p[i]), ex_mul_base(d1, p[i + half])); }
    else { const Ext* p = (const Ext*)num; nn = ex_add(ex_mul(p[i], d2), ex_mul(d1, p[i + half])); }
    num_out[i] = nn;
    den_out[i] = ex_mul(d1, d2);
  }
}

struct LogupTreeDesc { const u64* col[8]; int ncols; int num_mode; const void* num0; Ext* den_all; Ext* num_all; };
// K13 fused: denominators and every layer of the fractional-sum tree of one instance per workgroup (small tables).
// den_all: layer j at offset 2n - (2n >> j) (lengths n, n/2, .., 2); num_all: layer j >= 1 at offset n - (2n >> j).
// out[4*inst..] = [num_last[0], num_last[1], den_last[0], den_last[1]].
KBODY k_logup_tree(const LogupTreeDesc* d, size_t n, Ext c, Ext chi, Ext* out) {
  LogupTreeDesc t = d[blockIdx.x];
  int tid = threadIdx.x, nt = blockDim.x;
  Ext* den = t.den_all;
  for (size_t i = tid; i < n; i += nt) {
    Ext acc = c, pw = ex_one();
    for (int j = 0; j < t.ncols; j++) { acc = ex_add(acc, ex_mul_base(pw, t.col[j][i])); pw = ex_mul(pw, chi); }
    den[i] = acc;
  }
  __syncthreads();
  const void* num = t.num0;
  int mode = t.num_mode;
  size_t len = n, doff = 0, noff = 0;
  Ext* num_out = t.num_all;
  while (len > 2) {
    size_t half = len / 2;
    Ext* dcur = den + doff;
    Ext* dnext = den + doff + len;
    for (size_t i = tid; i < half; i += nt) {
      Ext d1 = dcur[i], d2 = dcur[i + half], nn;
      if (mode == 0) nn = ex_neg(ex_add(d1, d2));
      else if (mode == 1) { const u64* p = (const u64*)num; nn = ex_add(ex_mul_base(d2, p[i]), ex_mul_base(d1, p[i + half])); }
      else { const Ext* p = (const Ext*)num; nn = ex_add(ex_mul(p[i], d2), ex_mul(d1, p[i + half])); }
      num_out[noff + i] = nn;
      dnext[i] = ex_mul(d1, d2);
    }
    __syncthreads();
    num = (const void*)(num_out + noff); mode = 2;
    doff += len; noff += half; len = half;
  }
  if (tid < 4) {
    // len == 2 here: the last layer
    const Ext* nl = (const Ext*)num; const Ext* dl = den + doff;
    Ext v;
    if (tid < 2) { if (mode == 0) v = ex_neg(ex_one()); else if (mode == 1) v = ex_base(((const u64*)num)[tid]); else v = nl[tid]; }
    else v = dl[tid - 2];
    out[4 * blockIdx.x + tid] = v;
  }
}

// ------------------------------------------------------------------------------------------------ RS code / NTT (K5-K7)
template <bool EXT>
KBODY k_mobius_stage(void* data, size_t n, unsigned lg_half) {
  size_t half = size_t(1) << lg_half;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n / 2; b += (size_t)gridDim.x * blockDim.x) {
    size_t lo = ((b >> lg_half) << (lg_half + 1)) | (b & (half - 1));
    if (EXT) { Ext* p = (Ext*)data; p[lo + half] = ex_sub(p[lo + half], p[lo]); }
    else { u64* p = (u64*)data; p[lo + half] = gl_sub(p[lo + half], p[lo]); }
  }
}
// cw[2i] = cw[2i+1] = coeff[i] * shift^{bitrev_nv(i)}: bit-reversed, zero-padded, coset-scaled DIT input with the
// first (trivial, zero-tail) butterfly stage already applied (rs.rs:129-173 "r = 1")
template <bool EXT>
KBODY k_rs_prepare(const void* coeff, void* cw, const u64* pow7, unsigned nv, unsigned L) {
  size_t n = size_t(1) << nv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    size_t j = __brevll((unsigned long long)i) >> (64 - nv);
    u64 s = pow7[j << (L - nv)];
    if (EXT) { Ext v = ex_mul_base(((const Ext*)coeff)[i], s); ((Ext*)cw)[2 * i] = v; ((Ext*)cw)[2 * i + 1] = v; }
    else { u64 v = gl_mul(((const u64*)coeff)[i], s); ((u64*)cw)[2 * i] = v; ((u64*)cw)[2 * i + 1] = v; }
  }
}
// one radix-2 DIT stage; twiddle w_{2^(lg_half+1)}^j = tw[j << (L - lg_half)], tw[i] = w_{2^(L+1)}^i
template <bool EXT>
KBODY k_ntt_stage(void* data, size_t N, unsigned lg_half, const u64* tw, unsigned L) {
  size_t half = size_t(1) << lg_half;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < N / 2; b += (size_t)gridDim.x * blockDim.x) {
    size_t j = b & (half - 1);
    size_t lo = ((b >> lg_half) << (lg_half + 1)) | j;
    u64 w = tw[j << (L - lg_half)];
    if (EXT) { Ext* p = (Ext*)data; Ext t = ex_mul_base(p[lo + half], w), u = p[lo]; p[lo] = ex_add(u, t); p[lo + half] = ex_sub(u, t); }
    else { u64* p = (u64*)data; u64 t = gl_mul(p[lo + half], w), u = p[lo]; p[lo] = gl_add(u, t); p[lo + half] = gl_sub(u, t); }
  }
}
template <bool EXT>
KBODY k_bitrev(void* dst, const void* src, unsigned lg) {
  size_t n = size_t(1) << lg;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    size_t j = lg ? (__brevll((unsigned long long)i) >> (64 - lg)) : 0;
    if (EXT) ((Ext*)dst)[j] = ((const Ext*)src)[i]; else ((u64*)dst)[j] = ((const u64*)src)[i];
  }
}

// ------------------------------------------------------------------------------------------------ Merkle (K8)
// layer 0: digest = the two leaves verbatim (hash_or_noop on <= 4 base elements)
template <bool EXT>
KBODY k_merkle_leaves(const void* leaves, u64* nodes, size_t npairs) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npairs; i += (size_t)gridDim.x * blockDim.x) {
    u64 d0, d1, d2, d3;
    if (EXT) { Ext a = ((const Ext*)leaves)[2 * i], b = ((const Ext*)leaves)[2 * i + 1]; d0 = a.c0; d1 = a.c1; d2 = b.c0; d3 = b.c1; }
    else { d0 = ((const u64*)leaves)[2 * i]; d1 = ((const u64*)leaves)[2 * i + 1]; d2 = 0; d3 = 0; }
    u64* o = nodes + 4 * i;
    o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3;
  }
}
// the node hash of the one-node-per-lane Merkle kernels
__device__ __forceinline__ void merkle_compress(const u64* x, const u64* y, u64* o) {
  if (DP_SKIP_HASH_ON()) { for (int k = 0; k < 4; k++) o[k] = x[k] ^ y[k]; return; }
  p2f::compress(x, y, o, c_rc);  // poseidon2_fast.h: the same permutation with wide accumulation and any-representative words (1.33x, tools/p2bench.hip)
}
// one Poseidon2 compress (2 permutations) per lane; state held in 8 VGPR pairs, round constants in constant memory
KBODY k_merkle_layer(const u64* in, u64* out, size_t cnt) {
  if (cnt >= (size_t(1) << 15)) dp_hash_prio();  // (the bulk layers; a narrow layer is a link of its proof's chain like any small kernel)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) {
    const ulonglong2* p = (const ulonglong2*)(in + 8 * i);
    ulonglong2 x01 = p[0], x23 = p[1], y01 = p[2], y23 = p[3];
    u64 x[4] = {x01.x, x01.y, x23.x, x23.y}, y[4] = {y01.x, y01.y, y23.x, y23.y}, o[4];
    merkle_compress(x, y, o);
    ulonglong2* q = (ulonglong2*)(out + 4 * i);
    q[0] = make_ulonglong2(o[0], o[1]);
    q[1] = make_ulonglong2(o[2], o[3]);
  }
}

// The row hashes of MerkleTree::from_batch_leaves (merkle_tree.rs:261-329; util/hash.rs:32-41): several polynomials of one size share ONE
// tree whose leaf j is the row [cw_0[j], .., cw_{k-1}[j]]. Lane j writes hash_or_noop(row j) (poseidon_hash.rs:22-28: up to four base words
// are the digest themselves, zero padded; more go through the sponge: overwrite four lanes, permute, the digest is popped from the back)
// as the two extension "leaves" 2j, 2j+1 of `out`: the ordinary tree over `out` (k_merkle_leaves packs pairs, layers compress) then IS the
// batch tree from its first hashed layer up — hash_two_digests(hash(row 2i), hash(row 2i+1)) — so nothing else is specific to batches.
// Reads are coalesced per polynomial (consecutive lanes, consecutive elements). Not on the zkml path (dp_pcs_batch_commit only).
constexpr int BATCH_ROW_MAX = 32;
struct BatchRowPtrs { const u64* cw[BATCH_ROW_MAX]; };
template <bool EXT>
KBODY k_batch_row_hash(BatchRowPtrs a, int k, u64* out, size_t n) {
  constexpr int W = EXT ? 2 : 1;
  const int m = k * W;
  for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
    u64 s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c0 = 0; c0 < m; c0 += 4) {
#pragma unroll
      for (int i = 0; i < 4; i++) { const int t = c0 + i; if (t < m) s[i] = a.cw[t / W][W * j + t % W]; }
      if (m > 4) poseidon2_permute(s, c_rc);
    }
    u64* q = out + 4 * j;
    if (m > 4) { q[0] = s[3]; q[1] = s[2]; q[2] = s[1]; q[3] = s[0]; }
    else { q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; q[3] = s[3]; }
  }
}

// ------------------------------------------------------------------------------------------------ Basefold opening (K9-K12, K14)
struct PolyDesc { const void* f; const Ext* eq; Ext* fout; Ext* eqout; size_t n; int fext; int pad; };
// fold every (f, eq) pair of length > 1 by r; blockIdx.y = polynomial
KBODY k_classic_fold(const PolyDesc* d, Ext r) {
  PolyDesc p = d[blockIdx.y];
  if (p.n <= 1) return;
  size_t h = p.n / 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x) {
    p.eqout[i] = ex_lerp(p.eq[2 * i], p.eq[2 * i + 1], r);
    if (p.fext) p.fout[i] = ex_lerp(((const Ext*)p.f)[2 * i], ((const Ext*)p.f)[2 * i + 1], r);
    else p.fout[i] = ex_lerp_base(((const u64*)p.f)[2 * i], ((const u64*)p.f)[2 * i + 1], r);
  }
}
// the classic round kernels (k_classic_sums, k_classic_fused): entries 4 j .. 4 j + 3 of f, base or extension, folded by r into two
__device__ __forceinline__ void classic_fold_quad(const void* f, int fext, size_t j, Ext r, Ext& f0, Ext& f1) {
  if (fext) { const Ext* q = (const Ext*)f + 4 * j; f0 = ex_lerp(q[0], q[1], r); f1 = ex_lerp(q[2], q[3], r); }
  else { const u64* q = (const u64*)f + 4 * j; f0 = ex_lerp_base(q[0], q[1], r); f1 = ex_lerp_base(q[2], q[3], r); }
}
// c0 += sum f0 e0, c2 += sum (f1 - f0)(e1 - e0) over the pairs j = start, start + stride, .. < npairs of f and eq as they are stored
__device__ __forceinline__ void classic_pair_sums(const void* f, int fext, const Ext* eq, size_t start, size_t stride, size_t npairs, Ext& c0, Ext& c2) {
  for (size_t j = start; j < npairs; j += stride) {
    Ext l0 = eq[2 * j], l1 = eq[2 * j + 1];
    if (fext) {
      Ext r0 = ((const Ext*)f)[2 * j], r1 = ((const Ext*)f)[2 * j + 1];
      c0 = ex_add(c0, ex_mul(l0, r0));
      c2 = ex_add(c2, ex_mul(ex_sub(l1, l0), ex_sub(r1, r0)));
    } else {
      u64 r0 = ((const u64*)f)[2 * j], r1 = ((const u64*)f)[2 * j + 1];
      c0 = ex_add(c0, ex_mul_base(l0, r0));
      c2 = ex_add(c2, ex_mul_base(ex_sub(l1, l0), gl_sub(r1, r0)));
    }
  }
}
// partial[(poly*gridDim.x + block)*2 + {0,1}]: c0 = sum f0*e0, c2 = sum (f1-f0)(e1-e0)   (coeff.rs:236-345)
KBODY k_classic_sums(const PolyDesc* d, Ext* partial) {
  __shared__ Ext sm[TPB / 64];
  PolyDesc p = d[blockIdx.y];
  Ext c0 = ex_zero(), c2 = ex_zero();
  if (p.n == 1) {
    if (blockIdx.x == 0 && threadIdx.x == 0) c0 = ex_mul(ld_elem(p.f, p.fext, 0), p.eq[0]);
  } else classic_pair_sums(p.f, p.fext, p.eq, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, p.n / 2, c0, c2);
  size_t base = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
  Ext r;
  r = block_reduce_ext(c0, sm); if (threadIdx.x == 0) partial[base] = r;
  r = block_reduce_ext(c2, sm); if (threadIdx.x == 0) partial[base + 1] = r;
}
KBODY k_reduce_pairs(const Ext* partial, size_t nblocks, Ext* out) {
  __shared__ Ext sm[TPB / 64];
  size_t poly = blockIdx.x >> 1, t = blockIdx.x & 1;
  Ext acc = ex_zero();
  for (size_t b = threadIdx.x; b < nblocks; b += blockDim.x) acc = ex_add(acc, partial[(poly * nblocks + b) * 2 + t]);
  Ext r = block_reduce_ext(acc, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}
// K11: acc[j*rep + q] += x[j] * coeff
KBODY k_axpy_rep(Ext* acc, const void* x, int xext, Ext coeff, size_t n_acc, unsigned lg_rep) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_acc; i += (size_t)gridDim.x * blockDim.x) {
    size_t j = i >> lg_rep;
    Ext m = xext ? ex_mul(((const Ext*)x)[j], coeff) : ex_mul_base(coeff, ((const u64*)x)[j]);
    acc[i] = ex_add(acc[i], m);
  }
}
// The two [rows][K] columns of a Logits (argmax) step (Dev::logits_columns) in one pass over its input: diff[i] = max[row] - in[i] (what the range lookup
// reads; canonical, as gl_sub of canonical operands is) and onehot[i] = (column == idx[row]), K = 2^lg_k. 8 bytes read, 16 written per entry; the `rows`
// maxima / indices are read through the caches by the K lanes that share them.
KBODY k_logits_cols(const u64* __restrict__ in, const u64* __restrict__ mx, const u64* __restrict__ idx, u64* __restrict__ diff, u64* __restrict__ onehot, size_t n, unsigned lg_k) {
  const size_t kmask = (size_t(1) << lg_k) - 1;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i >> lg_k;
    diff[i] = gl_sub(mx[row], in[i]);
    onehot[i] = (i & kmask) == idx[row] ? 1 : 0;
  }
}
// K10 message on evaluation-form pairs: [sum a*ea, sum ((b-a)*ea + a*(eb-ea)), sum (b-a)(eb-ea)]
// partial[3 * block + {0,1,2}]; `counter` non-null: the last workgroup adds the blocks up and publishes the three sums itself (sc_block_sums_finish)
__device__ __forceinline__ void bf_msg_acc(Ext a, Ext a1, Ext ea, Ext e1, Ext* c) {
  Ext b = ex_sub(a1, a), eb = ex_sub(e1, ea);
  c[0] = ex_add(c[0], ex_mul(a, ea));
  c[1] = ex_add(c[1], ex_add(ex_mul(b, ea), ex_mul(a, eb)));
  c[2] = ex_add(c[2], ex_mul(b, eb));
}
KBODY k_bf_msg(const Ext* f, const Ext* eq, size_t npairs, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  Ext c[3] = {ex_zero(), ex_zero(), ex_zero()};
  for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < npairs; j += (size_t)gridDim.x * blockDim.x) bf_msg_acc(f[2 * j], f[2 * j + 1], eq[2 * j], eq[2 * j + 1], c);
  sc_block_sums_finish<3>(c, sm, partial, counter, result, flag, seq);
}
// One commit-phase round after the first in ONE pass (Dev::bf_round with a challenge): each lane takes four consecutive entries of f and of eq, folds them with
// ch into two (k_fold's formula: the stored tables are k_fold's word for word), stores those and adds the folded pair to k_bf_msg's sums — the folded
// tables are not read back for the message, and the last workgroup publishes it (no k_reduce_publish launch).
KBODY k_bf_fold_msg(const Ext* f, const Ext* eq, Ext* fout, Ext* eqout, size_t nquads, Ext ch, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  Ext c[3] = {ex_zero(), ex_zero(), ex_zero()};
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquads; q += (size_t)gridDim.x * blockDim.x) {
    const Ext* pf = f + 4 * q; const Ext* pe = eq + 4 * q;
    Ext a = ex_lerp(pf[0], pf[1], ch), a1 = ex_lerp(pf[2], pf[3], ch), ea = ex_lerp(pe[0], pe[1], ch), e1 = ex_lerp(pe[2], pe[3], ch);
    fout[2 * q] = a; fout[2 * q + 1] = a1; eqout[2 * q] = ea; eqout[2 * q + 1] = e1;
    bf_msg_acc(a, a1, ea, e1, c);
  }
  sc_block_sums_finish<3>(c, sm, partial, counter, result, flag, seq);
}
// K9: out[i] = y0 + (ch - x0)(y1 - y0) w,  x0 = gamma * w_{2^(level+1)}^{bitrev(i)},  w = -1/(2 x0)   (rs.rs:377-410)
KBODY k_fri_fold(const Ext* in, Ext* out, size_t nout, unsigned level, const u64* tw, unsigned L, u64 gamma, u64 neg_inv2gamma, Ext ch) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nout; i += (size_t)gridDim.x * blockDim.x) {
    size_t b = level ? (__brevll((unsigned long long)i) >> (64 - level)) : 0;
    u64 root = tw[b << (L - level)];
    u64 x0 = gl_mul(root, gamma);
    u64 rinv = b == 0 ? 1 : gl_neg(tw[((size_t(1) << level) - b) << (L - level)]);
    u64 w = gl_mul(neg_inv2gamma, rinv);
    Ext y0 = in[2 * i], y1 = in[2 * i + 1];
    Ext t = ex_mul(ex(gl_sub(ch.c0, x0), ch.c1), ex_sub(y1, y0));
    out[i] = ex_add(y0, ex_mul_base(t, w));
  }
}
struct GatherDesc { const void* leaves; const u64* nodes; size_t nleaves; size_t p0; size_t out_off; size_t path_off; int ext; int height; };  // pair words at out_off, path words at path_off
// K14: one wave per (query, tree): leaf pair then the sibling digests bottom-up
KBODY k_query_gather(const GatherDesc* d, size_t nd, u64* out) {
  const int lane = threadIdx.x & 63;
  const size_t wpb = blockDim.x >> 6;  // (the grid strides over the descriptors: a cohort's launch is capped, HipDev::grid_for)
  for (size_t q = blockIdx.x * wpb + (threadIdx.x >> 6); q < nd; q += (size_t)gridDim.x * wpb) {
    GatherDesc g = d[q];
    u64* o = out + g.out_off;
    u64* op = out + g.path_off;
    int nleafw = g.ext ? 4 : 2;
    if (lane < nleafw) o[lane] = ((const u64*)g.leaves)[g.p0 * (g.ext ? 2 : 1) + lane];
    int npath = g.height - 1;
    for (int w = lane; w < npath * 4; w += 64) {
      int l = w >> 2;
      size_t off = g.nleaves - (g.nleaves >> l);
      size_t idx = (g.p0 >> (l + 1)) ^ 1;
      op[w] = g.nodes[4 * (off + idx) + (w & 3)];
    }
  }
}

// K14b: the query section of a batch opening written as its stream words (Dev::query_section has the layout). spec (host-written, read-only): [nq] [ntrees] [#oracle]
// [#commitments] [words per query] [position of the #commitments word] [0] [0], the nq query indices, then five words per tree: leaves, nodes, nleaves,
// shift | ext << 8 | height << 16, offset of the tree's entry in a query's block. One wave per (query, tree), as in k_query_gather; the wave of a query's first tree
// also writes the block's three header words (and the very first the count): every word of the image is written by exactly one lane.
KBODY k_query_section(const u64* spec, u64* out) {
  const int lane = threadIdx.x & 63;
  const size_t wpb = blockDim.x >> 6;
  const size_t nq = spec[0], nt = spec[1], stride = spec[4];
  const u64* qidx = spec + 8;
  const u64* tr = qidx + nq;
  for (size_t q = blockIdx.x * wpb + (threadIdx.x >> 6); q < nq * nt; q += (size_t)gridDim.x * wpb) {
    const size_t qi = q / nt, k = q - qi * nt;
    const u64* t = tr + 5 * k;
    const u64 x = qidx[qi], meta = t[3];
    const unsigned shift = (unsigned)(meta & 0xff);
    const int ext = (int)((meta >> 8) & 1), height = (int)(meta >> 16);
    const size_t nleaves = t[2], p0 = (x >> shift) & ~size_t(1);
    const u64* nodes = (const u64*)t[1];
    u64* o = out + 1 + qi * stride;
    u64* e = o + t[4];
    const int nleafw = ext ? 4 : 2, npath = height - 1;
    if (lane < nleafw) e[1 + lane] = ((const u64*)t[0])[p0 * (ext ? 2 : 1) + lane];
    if (lane == 8) { e[0] = (u64)ext; e[1 + nleafw] = p0; e[2 + nleafw] = (u64)npath; }
    if (lane == 9 && k == 0) { o[0] = x; o[1] = spec[2]; o[spec[5]] = spec[3]; if (qi == 0) out[0] = nq; }
    u64* op = e + 3 + nleafw;
    for (int w = lane; w < npath * 4; w += 64) {
      int l = w >> 2;
      size_t off = nleaves - (nleaves >> l);
      size_t idx = (p0 >> (l + 1)) ^ 1;
      op[w] = nodes[4 * (off + idx) + (w & 3)];
    }
  }
}


// ---- relaxed system-scope publication helpers (see sc_publish below)
// A one-workgroup protocol kernel ASSEMBLES its message in LDS (MSG_PUT) and sends it to the host in one burst when it is complete (msg_flush): a store to
// host-mapped memory is acknowledged across PCIe, and whatever waits for outstanding memory operations next — a barrier, a fence, a flat access — stalls until
// the acknowledgement is back. Round 4's kernels published every round's message as they went: microseconds per Fiat-Shamir round once hundreds of proofs share
// the link, and the argument-pack reads of every other launch queued behind them (k_logup_tail alone: member 4.2 -> 2.4 ms, start skew of a merged launch
// 2.6 -> 0.55 ms, Dense-4M 450 -> 690 proofs/s on one box; profiles/r05_wgtimes_448_*).
#define MSG_PUT(p, v) (*(p) = (v))
__device__ __forceinline__ unsigned long long pub_mix(unsigned long long seq) { return seq * 0x9E3779B97F4A7C15ull + 0x7F4A7C159E3779B9ull; }
__device__ __forceinline__ void pub_store(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void msg_flush(u64* host, const u64* mb, size_t nwords, int lane) {  // one wave; the tag (the caller's) follows
  DP_WAVE_SYNC();
  for (size_t w = (size_t)lane; w < nwords; w += 64) pub_store(host + w, mb[w]);
}
// one wave: lane l owns words l, l+64, ...; returns (on lane 0) the payload checksum
__device__ __forceinline__ unsigned long long pub_wave_sum(unsigned long long local) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local += shfl_down_u64(local, d);
  return local;
}

// ------------------------------------------------------------------------------------------------ lane-parallel Poseidon2
// One permutation spread over 8 adjacent lanes (lane i holds state[i]): used where there are too few hashes to fill
// the machine with one-hash-per-lane (the top layers of every Merkle tree), cutting the serial latency of a compress
// from 2 x ~520 dependent multiplications to 2 x ~100.
__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  int lo = __shfl((int)(u32)v, src, 64);
  int hi = __shfl((int)(u32)(v >> 32), src, 64);
  return ((u64)(u32)hi << 32) | (u64)(u32)lo;
}
// DPP cross-lane moves (no LDS crossbar round trip): quad permutes and the 8-lane half-row mirror
template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
  int lo = __builtin_amdgcn_update_dpp(0, (int)(u32)v, CTRL, 0xF, 0xF, false);
  int hi = __builtin_amdgcn_update_dpp(0, (int)(u32)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((u64)(u32)hi << 32) | (u64)(u32)lo;
}
template <int CTRL> __device__ __forceinline__ u32 dpp_u32(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
constexpr int DPP_QUAD_ROT1 = 0x39;     // quad_perm [1,2,3,0]: lane j reads j+1 (mod 4)
constexpr int DPP_QUAD_ROT2 = 0x4E;     // quad_perm [2,3,0,1]: lane j reads j+2 == j^2
constexpr int DPP_QUAD_ROT3 = 0x93;     // quad_perm [3,0,1,2]: lane j reads j+3
constexpr int DPP_QUAD_XOR1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int DPP_QUAD_REV = 0x1B;      // quad_perm [3,2,1,0]
constexpr int DPP_HALF_MIRROR = 0x141;  // row_half_mirror: lane i reads 7-i within its group of 8
constexpr int DPP_QUAD_BCAST0 = 0x00;   // quad_perm [0,0,0,0]: every lane of a quad reads the quad's lane 0
// The 8-lane permutation, round-4 formulation. One wave on this dependent chain pays 4-5 cycles for EVERY instruction slot — VALU, SALU or s_nop wait
// state alike (profiles/r04_issue_rate_one_wave.txt) — so the permutation is built to minimise slots:
//  * multiplications are the hand-written gfx950 sequences of gl64_gfx950.h (12 VALU), their rare borrow deferred to one check per permutation;
//  * the linear layers never touch a carry flag (an SGPR carry costs two wait states on gfx950): a state word travels as three limbs of 22 / 22 / 20 bits
//    in 32-bit registers, sums of up to 21 words stay exact there, and every cross-lane move is fused into an add (v_add_u32 with a DPP operand);
//  * limbs return to 64 bits inside multiply-accumulates: join3_f (6 VALU) in front of an S-box, fma3_f (17 VALU) for the internal layer's d_i x_i + sum;
//  * the per-lane round constants of the 8 external rounds and the internal diagonal live in registers (P2lK), loaded once per kernel instead of once
//    per round from memory that is busy serving the rest of the chip.
// (Round 3's form: 64 + 32-bit accumulators with add / addc chains through DPP moves, 10.8 us per permutation with the new multiplication, 12.7 without.)
constexpr u32 L3_MASK = 0x3FFFFFu;
struct L3 { u32 a, b, c; };  // a + b 2^22 + c 2^44; the limbs of a SUM may exceed their width (they are added as plain 32-bit integers)
__device__ __forceinline__ L3 l3_split(u64 x) { L3 r; r.a = (u32)x & L3_MASK; r.b = (u32)(x >> 22) & L3_MASK; r.c = (u32)(x >> 44); return r; }
struct P2lK { u64 diag; L3 ext[8]; L3 tab; };  // this lane's internal diagonal entry, its constants of the 4 + 4 external rounds as limbs, and — lane r of `tab` — the limbs of internal constant r (fetched with v_readlane: no memory access inside a permutation)
__device__ __forceinline__ P2lK p2l_load(int lane) {
  P2lK k; const int i = lane & 7;
  k.diag = c_rc[86 + i];
#pragma unroll
  for (int r = 0; r < 4; r++) { k.ext[r] = l3_split(c_rc[r * 8 + i]); k.ext[4 + r] = l3_split(c_rc[54 + r * 8 + i]); }
  k.tab = l3_split(lane < 22 ? c_rc[32 + lane] : 0);  // (lane 22 = the zero added after the last internal round)
  return k;
}
// portable forms of the three multiply-accumulate blocks (host, CPU emulator, -DDP_NO_GFX950_ASM): same field elements
__device__ __forceinline__ u64 p2l_ref_join3(u32 A, u32 B, u32 C) {
  const unsigned __int128 v = (unsigned __int128)A + ((unsigned __int128)B << 22) + ((unsigned __int128)C << 44);
  return p2f::red128((u64)v, (u64)(v >> 64));
}
__device__ __forceinline__ u64 p2l_ref_fma3(u64 x, u64 d, u32 A, u32 B, u32 C) {
  const unsigned __int128 v = (unsigned __int128)x * d + (unsigned __int128)A + ((unsigned __int128)B << 22) + ((unsigned __int128)C << 44);  // d < p: below 2^128
  return p2f::red128((u64)v, (u64)(v >> 64));
}
template <bool FIX> __device__ __forceinline__ u64 p2l_mul(u64 a, u64 b, u64& flag, u64& pend) {
#ifdef DP_GFX950_ASM
  return gx::mul_f<FIX>(a, b, flag, pend);
#else
  (void)flag; (void)pend; return p2f::mul(a, b);
#endif
}
template <bool FIX> __device__ __forceinline__ u64 p2l_join3(L3 v, u64& flag, u64& pend) {
#ifdef DP_GFX950_ASM
  return gx::join3_f<FIX>(v.a, v.b, v.c, flag, pend);
#else
  (void)flag; (void)pend; return p2l_ref_join3(v.a, v.b, v.c);
#endif
}
template <bool FIX> __device__ __forceinline__ u64 p2l_fma3(u64 x, u64 d, L3 v, u64& flag, u64& pend) {
#ifdef DP_GFX950_ASM
  return gx::fma3_f<FIX>(x, d, v.a, v.b, v.c, flag, pend);
#else
  (void)flag; (void)pend; return p2l_ref_fma3(x, d, v.a, v.b, v.c);
#endif
}
template <bool FIX> __device__ __forceinline__ u64 p2l_sbox(u64 x, u64& flag, u64& pend) {
  const u64 x2 = p2l_mul<FIX>(x, x, flag, pend), x3 = p2l_mul<FIX>(x2, x, flag, pend), x4 = p2l_mul<FIX>(x2, x2, flag, pend);
  return p2l_mul<FIX>(x3, x4, flag, pend);
}
// external layer circ(2 M4, M4) on one limb: t_j = 2 v_j + 3 v_{j+1} + v_{j+2} + v_{j+3} = (quad sum) + v_j + 2 v_{j+1} inside the quad, out = 2 t + t(lane ^ 4).
// v < 2^22 -> out < 21 * 2^22. Eight instructions, no carries.
__device__ __forceinline__ u32 p2l_mds_limb(u32 v) {
  const u32 p = v + dpp_u32<DPP_QUAD_XOR1>(v);
  const u32 S = p + dpp_u32<DPP_QUAD_ROT2>(p);
  const u32 t = S + v + 2u * dpp_u32<DPP_QUAD_ROT1>(v);
  const u32 m = dpp_u32<DPP_HALF_MIRROR>(t);
  return 2u * t + dpp_u32<DPP_QUAD_REV>(m);  // lane i reads i ^ 4
}
__device__ __forceinline__ L3 p2l_mds(L3 v) { L3 r; r.a = p2l_mds_limb(v.a); r.b = p2l_mds_limb(v.b); r.c = p2l_mds_limb(v.c); return r; }
__device__ __forceinline__ u32 p2l_sum8_limb(u32 v) {
  const u32 p = v + dpp_u32<DPP_QUAD_XOR1>(v);
  const u32 q = p + dpp_u32<DPP_QUAD_ROT2>(p);
  return q + dpp_u32<DPP_HALF_MIRROR>(q);  // every lane of a quad holds the quad sum: any lane of the other quad will do
}
__device__ __forceinline__ L3 l3_add(L3 x, L3 y) { L3 r; r.a = x.a + y.a; r.b = x.b + y.b; r.c = x.c + y.c; return r; }
// the external layer of a 64-bit word plus this lane's round constant, limbs in / limbs out (device: one 28-instruction block, gl64_gfx950.h lin_full)
__device__ __forceinline__ L3 p2l_lin_full(u64 x, L3 rc) {
#ifdef DP_GFX950_ASM
  L3 r; gx::lin_full(x, rc.a, rc.b, rc.c, r.a, r.b, r.c); return r;
#else
  return l3_add(p2l_mds(l3_split(x)), rc);
#endif
}
__device__ __forceinline__ L3 p2l_lin_sum8(u64 x) {
#ifdef DP_GFX950_ASM
  L3 r; gx::lin_sum8(x, r.a, r.b, r.c); return r;
#else
  const L3 xl = l3_split(x); L3 r; r.a = p2l_sum8_limb(xl.a); r.b = p2l_sum8_limb(xl.b); r.c = p2l_sum8_limb(xl.c); return r;
#endif
}
// sum + (limbs of internal round constant r) on word 0 (lanes with one0 = 1), sum elsewhere: lane r of the table registers broadcast through SGPRs
// (v_readlane: no memory access inside a permutation), then one 24-bit multiply-add by the 0 / 1 lane flag per limb (the constants' limbs are 22 bits).
// One block: the SGPRs a v_readlane writes may be read by a VALU instruction two slots later at the earliest.
__device__ __forceinline__ L3 p2l_add_int_rc(const P2lK& k, int r, u32 one0, L3 sum) {
#ifdef DP_GFX950_ASM
  u32 sa, sb, sc;
  asm("v_readlane_b32 %[sa], %[ta], %[r]\n"
      "v_readlane_b32 %[sb], %[tb], %[r]\n"
      "v_readlane_b32 %[sc], %[tc], %[r]\n"
      "v_mad_u32_u24 %[a], %[one], %[sa], %[a]\n"
      "v_mad_u32_u24 %[b], %[one], %[sb], %[b]\n"
      "v_mad_u32_u24 %[c], %[one], %[sc], %[c]\n"
      : [a] "+v"(sum.a), [b] "+v"(sum.b), [c] "+v"(sum.c), [sa] "=&s"(sa), [sb] "=&s"(sb), [sc] "=&s"(sc)
      : [ta] "v"(k.tab.a), [tb] "v"(k.tab.b), [tc] "v"(k.tab.c), [one] "v"(one0), [r] "s"(r));
  return sum;
#else
  L3 o; o.a = sum.a + one0 * (u32)__builtin_amdgcn_readlane((int)k.tab.a, r); o.b = sum.b + one0 * (u32)__builtin_amdgcn_readlane((int)k.tab.b, r); o.c = sum.c + one0 * (u32)__builtin_amdgcn_readlane((int)k.tab.c, r);
  return o;
#endif
}
template <bool FIX> __device__ __forceinline__ u64 p2l_permute_impl(u64 s, int lane, const P2lK& k, u64& flag, u64& pend) {
  const u32 one0 = (lane & 7) == 0 ? 1u : 0u;  // word 0 of the state: the lane whose S-box counts in the internal rounds
  // external rounds: w = M_E s; 4 x { s = sbox(w + rc); w = M_E s } — the constant of the NEXT round is added as the layer is applied
  L3 w = p2l_lin_full(s, k.ext[0]);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    L3 nrc; if (r < 3) nrc = k.ext[r + 1]; else { L3 z; z.a = z.b = z.c = 0; nrc = p2l_add_int_rc(k, 0, one0, z); }  // into the internal rounds: word 0 carries the first internal constant
    w = p2l_lin_full(p2l_sbox<FIX>(p2l_join3<FIX>(w, flag, pend), flag, pend), nrc);
  }
  u64 y = p2l_join3<FIX>(w, flag, pend);
#pragma unroll 1
  for (int r = 0; r < 22; r++) {
    const u64 x7 = p2l_sbox<FIX>(y, flag, pend);  // (every lane computes, word 0's counts)
    const u64 x = one0 ? x7 : y;
    L3 sum = p2l_lin_sum8(x);
    sum = p2l_add_int_rc(k, r + 1, one0, sum);  // the next round's constant rides in word 0's addend (table lane 22 = 0 after the last round)
    y = p2l_fma3<FIX>(x, k.diag, sum, flag, pend);  // y_i = d_i x_i + sum (+ the next constant on word 0)
  }
  // terminal external rounds: 4 x { s = sbox(w + rc); w = M_E s }, the first on the state as it is
  w = l3_add(l3_split(y), k.ext[4]);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    L3 nrc; if (r < 3) nrc = k.ext[5 + r]; else { nrc.a = 0; nrc.b = 0; nrc.c = 0; }
    w = p2l_lin_full(p2l_sbox<FIX>(p2l_join3<FIX>(w, flag, pend), flag, pend), nrc);
  }
  return p2l_join3<FIX>(w, flag, pend);
}
__device__ __forceinline__ u64 p2l_permute(u64 s, int lane, const P2lK& k) {
  u64 flag = 0, pend = 0;
  u64 r = p2l_permute_impl<false>(s, lane, k, flag, pend);
#ifdef DP_GFX950_ASM
  if (flag | pend) r = p2l_permute_impl<true>(s, lane, k, flag, pend);  // a deferred borrow fired somewhere in the wave: once more with the exact forms
#endif
  return p2f::canon(r);  // canonical: the host resumes transcripts from these words
}
// in: 8 words (two digests), out: 4 words; executed by the 8 lanes of one group together
__device__ __forceinline__ void p2l_compress(const u64* in, u64* out, int lane, const P2lK& k) {
  int i = lane & 7;
  u64 s = i < 4 ? in[i] : 0;
  s = p2l_permute(s, lane, k);
  if (i < 4) s = in[4 + i];
  s = p2l_permute(s, lane, k);
  if (i < 4) out[3 - i] = s;
}
// one Merkle layer with 8 lanes per node: for layers too narrow to hide the latency of a one-lane compress
KBODY k_merkle_layer_lp(const u64* in, u64* out, size_t cnt) {
  size_t g = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 3;
  size_t stride = ((size_t)gridDim.x * blockDim.x) >> 3;
  if (DP_SKIP_HASH_ON()) { for (; g < cnt; g += stride) if ((threadIdx.x & 7) < 4) out[4 * g + (threadIdx.x & 7)] = in[8 * g + (threadIdx.x & 7)]; return; }
  const P2lK pk = p2l_load(threadIdx.x & 63);
  for (; g < cnt; g += stride) p2l_compress(in + 8 * g, out + 4 * g, threadIdx.x & 63, pk);
}
// verifier: one Merkle path per lane, from the leaf-pair digest up to the root (authenticate_merkle_path_root,
// mpcs/src/util/merkle_tree.rs:331-420). meta[3j..] = {index of the leaf pair, first digest of the path in `pool`, depth};
// bad[0] counts the paths that do not authenticate, bad[1] = the smallest index of one
KBODY k_merkle_paths(const u64* leaf, const u64* root, const u64* meta, const u64* pool, size_t n, unsigned long long* bad) {
  for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
    u64 h[4] = {leaf[4 * j], leaf[4 * j + 1], leaf[4 * j + 2], leaf[4 * j + 3]};
    u64 x = meta[3 * j];
    const u64* p = pool + 4 * meta[3 * j + 1];
    const unsigned depth = (unsigned)meta[3 * j + 2];
    for (unsigned l = 0; l < depth; l++) {
      u64 sib[4] = {p[4 * l], p[4 * l + 1], p[4 * l + 2], p[4 * l + 3]}, o[4];
      if (x & 1) p2f::compress(sib, h, o, c_rc); else p2f::compress(h, sib, o, c_rc);
      h[0] = o[0]; h[1] = o[1]; h[2] = o[2]; h[3] = o[3];
      x >>= 1;
    }
    if (h[0] != root[4 * j] || h[1] != root[4 * j + 1] || h[2] != root[4 * j + 2] || h[3] != root[4 * j + 3]) { atomicAdd(&bad[0], 1ull); atomicMin(&bad[1], (unsigned long long)j); }
  }
}
struct TailDesc { u64* nodes; size_t off; size_t cnt; };
// All Merkle layers above an already computed layer of `cnt` (<= 2048) digests, one workgroup per tree, no relaunch
// between layers. Wide layers hash one node per lane, narrow ones use the 8-lane permutation. roots[4*tree..] = root.
KBODY k_merkle_tail(const TailDesc* d, u64* roots, u64* host_result, unsigned long long* flag, unsigned long long seq) {
  TailDesc t = d[blockIdx.x];
  u64* nd = t.nodes;
  size_t off = t.off, cnt = t.cnt;
  int tid = threadIdx.x;
  const P2lK pk = p2l_load(tid & 63);
  while (cnt > 1) {
    size_t next = cnt / 2;
    const u64* in = nd + 4 * off;
    u64* out = nd + 4 * (off + cnt);
    if (next > blockDim.x) {  // very wide layer: one node per lane; otherwise 8 lanes per node (the DPP permutation is ~8x lower latency)
      for (size_t i = tid; i < next; i += blockDim.x) {
        u64 o[4];
        p2f::compress(in + 8 * i, in + 8 * i + 4, o, c_rc);
        out[4 * i] = o[0]; out[4 * i + 1] = o[1]; out[4 * i + 2] = o[2]; out[4 * i + 3] = o[3];
      }
    } else {
      for (size_t g = tid >> 3; g < next; g += (blockDim.x >> 3)) p2l_compress(in + 8 * g, out + 4 * g, tid & 63, pk);
    }
    __syncthreads();
    off += cnt; cnt = next;
  }
  if (tid < 4) roots[4 * blockIdx.x + tid] = nd[4 * off + tid];
  if (host_result && tid < 64) {  // single tree: publish the root (4 words) directly
    unsigned long long cs = 0;
    if (tid < 4) { u64 v = nd[4 * off + tid]; pub_store(host_result + tid, v); cs = (unsigned long long)(tid + 1) * v; }
    cs = pub_wave_sum(cs);
    if (tid == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
  }
}
struct SmallCommitDesc { const void* evals; void* cw; void* bh; u64* nodes; void* tmp; };
// layer 0 of many equally sized trees: blockIdx.y = tree
template <bool EXT>
KBODY k_merkle_leaves_many(const SmallCommitDesc* d, size_t npairs) {
  const void* leaves = d[blockIdx.y].cw;
  u64* nodes = d[blockIdx.y].nodes;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npairs; i += (size_t)gridDim.x * blockDim.x) {
    u64 d0, d1, d2, d3;
    if (EXT) { Ext a = ((const Ext*)leaves)[2 * i], b = ((const Ext*)leaves)[2 * i + 1]; d0 = a.c0; d1 = a.c1; d2 = b.c0; d3 = b.c1; }
    else { d0 = ((const u64*)leaves)[2 * i]; d1 = ((const u64*)leaves)[2 * i + 1]; d2 = 0; d3 = 0; }
    u64* o = nodes + 4 * i;
    o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3;
  }
}
template <bool EXT> struct ElemOps;
template <> struct ElemOps<false> {
  typedef u64 T;
  static __device__ __forceinline__ T sub(T a, T b) { return gl_sub(a, b); }
  static __device__ __forceinline__ T add(T a, T b) { return gl_add(a, b); }
  static __device__ __forceinline__ T mulb(T a, u64 b) { return gl_mul(a, b); }
};
template <> struct ElemOps<true> {
  typedef Ext T;
  static __device__ __forceinline__ T sub(T a, T b) { return ex_sub(a, b); }
  static __device__ __forceinline__ T add(T a, T b) { return ex_add(a, b); }
  static __device__ __forceinline__ T mulb(T a, u64 b) { return ex_mul_base(a, b); }
};
// Stages [s_lo, s_hi) of the Moebius transform (NTT = false: p[lo + half] -= p[lo]) or of the radix-2 DIT NTT (NTT = true:
// butterfly with w = tw[j << (L - s)], j = the index bits below s) in ONE launch, LDS-tiled: a tile is the 2^(s_hi - s_lo + lgc)
// elements whose index is (hi << s_hi) | (m << s_lo) | (lowblk << lgc) | c for all m < 2^(s_hi - s_lo), c < 2^lgc — the bits
// the stages act on (m) plus 2^lgc consecutive elements, so that global accesses stay 128-byte segments when the stride
// 2^s_lo is large; lgc <= s_lo, and with lgc == s_lo the tile is one contiguous block. Tiles partition the array, every stage of
// the range only pairs elements of one tile: a 2^20-coefficient polynomial takes 2 Moebius + 2 NTT passes instead of 20 + 20
// per-stage launches over HBM (K5 / K7; SURVEY.md §7 step 6). In LDS the element sits at (m << lgc) | c.
template <bool EXT, bool NTT>
KBODY k_butterfly_pass(void* data, unsigned s_lo, unsigned s_hi, unsigned lgc, const u64* tw, unsigned L) {
  DP_LDS_DYN0(lds_bp);
  typedef typename ElemOps<EXT>::T T;
  T* A = (T*)lds_bp;
  T* p = (T*)data;
  const unsigned span = s_hi - s_lo, lgt = span + lgc;
  const size_t tile = blockIdx.x;
  const size_t nlowblk = size_t(1) << (s_lo - lgc);           // tiles per value of the high bits
  const size_t hi = tile >> (s_lo - lgc), lowblk = tile & (nlowblk - 1);
  const size_t base = (hi << s_hi) | (lowblk << lgc);
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t telems = size_t(1) << lgt;
  for (size_t q = tid; q < telems; q += nt) { size_t m = q >> lgc, c = q & ((size_t(1) << lgc) - 1); A[q] = p[base | (m << s_lo) | c]; }
  __syncthreads();
  for (unsigned s = s_lo; s < s_hi; s++) {
    const unsigned b = s - s_lo;                               // the bit of m this stage pairs
    for (size_t q = tid; q < telems / 2; q += nt) {
      // q enumerates the pairs: insert a 0 at bit (b + lgc) of the LDS position
      const size_t lowmask = (size_t(1) << (b + lgc)) - 1;
      const size_t lo = ((q & ~lowmask) << 1) | (q & lowmask), hi2 = lo | (size_t(1) << (b + lgc));
      if (NTT) {
        const size_t m = lo >> lgc, c = lo & ((size_t(1) << lgc) - 1);
        const size_t j = ((m & ((size_t(1) << b) - 1)) << s_lo) | (lowblk << lgc) | c;   // index bits below s
        const u64 w = tw[j << (L - s)];
        T t = ElemOps<EXT>::mulb(A[hi2], w), u = A[lo];
        A[lo] = ElemOps<EXT>::add(u, t); A[hi2] = ElemOps<EXT>::sub(u, t);
      } else A[hi2] = ElemOps<EXT>::sub(A[hi2], A[lo]);
    }
    __syncthreads();
  }
  for (size_t q = tid; q < telems; q += nt) { size_t m = q >> lgc, c = q & ((size_t(1) << lgc) - 1); p[base | (m << s_lo) | c] = A[q]; }
}
// K5+K6+K7 for a small polynomial entirely in LDS: evaluations -> coefficients (Moebius), coset scale, zero-pad,
// radix-2 DIT NTT on 2n points, bit-reversed store; also the bit-reversed copy of the evaluations. One workgroup per
// polynomial (blockIdx.x), dynamic LDS = 3n elements.
template <bool EXT>
KBODY k_commit_small(const SmallCommitDesc* d, unsigned nv, unsigned L, const u64* tw, const u64* pow7) {
  typedef typename ElemOps<EXT>::T T;
  DP_LDS_DYN0(lds_raw);
  T* A = (T*)lds_raw;  // n coefficients
  size_t n = size_t(1) << nv, N = 2 * n;
  T* Bf = A + n;       // 2n NTT buffer
  SmallCommitDesc pd = d[blockIdx.x];
  const T* ev = (const T*)pd.evals;
  T* bh = (T*)pd.bh;
  T* cw = (T*)pd.cw;
  int tid = threadIdx.x, nt = blockDim.x;
  for (size_t i = tid; i < n; i += nt) {
    T v = ev[i];
    A[i] = v;
    bh[__brev((unsigned)i) >> (32 - nv)] = v;
  }
  __syncthreads();
  for (unsigned s = 0; s < nv; s++) {
    size_t half = size_t(1) << s;
    for (size_t b = tid; b < n / 2; b += nt) {
      size_t lo = ((b >> s) << (s + 1)) | (b & (half - 1));
      A[lo + half] = ElemOps<EXT>::sub(A[lo + half], A[lo]);
    }
    __syncthreads();
  }
  for (size_t i = tid; i < n; i += nt) {
    size_t j = __brev((unsigned)i) >> (32 - nv);
    T v = ElemOps<EXT>::mulb(A[i], pow7[j << (L - nv)]);
    Bf[2 * i] = v; Bf[2 * i + 1] = v;
  }
  __syncthreads();
  for (unsigned s = 1; s <= nv; s++) {
    size_t half = size_t(1) << s;
    for (size_t b = tid; b < n; b += nt) {
      size_t j = b & (half - 1);
      size_t lo = ((b >> s) << (s + 1)) | j;
      T t = ElemOps<EXT>::mulb(Bf[lo + half], tw[j << (L - s)]), u = Bf[lo];
      Bf[lo] = ElemOps<EXT>::add(u, t);
      Bf[lo + half] = ElemOps<EXT>::sub(u, t);
    }
    __syncthreads();
  }
  for (size_t o = tid; o < N; o += nt) cw[o] = Bf[__brev((unsigned)o) >> (32 - (nv + 1))];
}

// ---- medium polynomials (2^12..2^14 base elements: the witness columns of a convolution layer), many at once: blockIdx.y
// (or .x) = polynomial. Four launches replace the 2 nv + 4 per-stage launches of the generic path, for the whole group.
constexpr unsigned MED_NTT_LG = 13;  // an NTT block of 2^13 base elements (64 KB) lives in LDS
// K5 + K6 + coset scaling: evaluations -> LDS, all Moebius stages there, then tmp[2i] = tmp[2i+1] = coeff[i] * shift^bitrev(i)
// (the zero-padded, bit-reversed DIT input after its trivial first stage) and bh[bitrev(i)] = evals[i]
KBODY k_med_prepare(const SmallCommitDesc* d, unsigned nv, unsigned L, const u64* pow7) {
  DP_LDS_DYN0(lds_med);
  u64* A = (u64*)lds_med;
  SmallCommitDesc pd = d[blockIdx.x];
  const u64* ev = (const u64*)pd.evals; u64* bh = (u64*)pd.bh; u64* tmp = (u64*)pd.tmp;
  size_t n = size_t(1) << nv;
  int tid = threadIdx.x, nt = blockDim.x;
  for (size_t i = tid; i < n; i += nt) { u64 v = ev[i]; A[i] = v; bh[__brev((unsigned)i) >> (32 - nv)] = v; }
  __syncthreads();
  for (unsigned s = 0; s < nv; s++) {
    size_t half = size_t(1) << s;
    for (size_t b = tid; b < n / 2; b += nt) { size_t lo = ((b >> s) << (s + 1)) | (b & (half - 1)); A[lo + half] = gl_sub(A[lo + half], A[lo]); }
    __syncthreads();
  }
  for (size_t i = tid; i < n; i += nt) {
    size_t j = __brev((unsigned)i) >> (32 - nv);
    u64 v = gl_mul(A[i], pow7[j << (L - nv)]);
    ((ulonglong2*)tmp)[i] = make_ulonglong2(v, v);
  }
}
// DIT stages 1..smax (butterfly span <= 2^MED_NTT_LG) of the 2n-point NTT, one LDS-resident block per workgroup
KBODY k_med_ntt_local(const SmallCommitDesc* d, unsigned lgblk, unsigned smax, const u64* tw, unsigned L) {
  DP_LDS_DYN0(lds_med);
  u64* B = (u64*)lds_med;
  size_t blk = size_t(1) << lgblk;
  u64* p = (u64*)d[blockIdx.y].tmp + blockIdx.x * blk;
  int tid = threadIdx.x, nt = blockDim.x;
  for (size_t i = tid; i < blk; i += nt) B[i] = p[i];
  __syncthreads();
  for (unsigned s = 1; s <= smax; s++) {
    size_t half = size_t(1) << s;
    for (size_t b = tid; b < blk / 2; b += nt) {
      size_t j = b & (half - 1), lo = ((b >> s) << (s + 1)) | j;
      u64 t = gl_mul(B[lo + half], tw[j << (L - s)]), u = B[lo];
      B[lo] = gl_add(u, t); B[lo + half] = gl_sub(u, t);
    }
    __syncthreads();
  }
  for (size_t i = tid; i < blk; i += nt) p[i] = B[i];
}
KBODY k_ntt_stage_many(const SmallCommitDesc* d, size_t N, unsigned lg_half, const u64* tw, unsigned L) {
  u64* p = (u64*)d[blockIdx.y].tmp;
  size_t half = size_t(1) << lg_half;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < N / 2; b += (size_t)gridDim.x * blockDim.x) {
    size_t j = b & (half - 1), lo = ((b >> lg_half) << (lg_half + 1)) | j;
    u64 t = gl_mul(p[lo + half], tw[j << (L - lg_half)]), u = p[lo];
    p[lo] = gl_add(u, t); p[lo + half] = gl_sub(u, t);
  }
}
KBODY k_bitrev_many(const SmallCommitDesc* d, unsigned lg) {
  const u64* src = (const u64*)d[blockIdx.y].tmp; u64* dst = (u64*)d[blockIdx.y].cw;
  size_t n = size_t(1) << lg;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[__brevll((unsigned long long)i) >> (64 - lg)] = src[i];
}
// one Merkle layer of many equally shaped trees (one Poseidon2 compress per lane): blockIdx.y = tree
KBODY k_merkle_layer_many(const TailDesc* td, size_t off, size_t cnt) {
  u64* nd = td[blockIdx.y].nodes;
  const u64* in = nd + 4 * off; u64* out = nd + 4 * (off + cnt);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cnt / 2; i += (size_t)gridDim.x * blockDim.x) {
    const ulonglong2* p = (const ulonglong2*)(in + 8 * i);
    ulonglong2 x01 = p[0], x23 = p[1], y01 = p[2], y23 = p[3];
    u64 x[4] = {x01.x, x01.y, x23.x, x23.y}, y[4] = {y01.x, y01.y, y23.x, y23.y}, o[4];
    merkle_compress(x, y, o);
    ulonglong2* q = (ulonglong2*)(out + 4 * i);
    q[0] = make_ulonglong2(o[0], o[1]); q[1] = make_ulonglong2(o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------ single-launch sumcheck round
__device__ void sc_publish_fwd(Ext* result, const Ext* part, const int* tk, const int* toff, int nterms, int wpt, unsigned long long* flag, unsigned long long seq, int lane);
__device__ void sc_wait_challenge_fwd(const unsigned long long* mailbox, unsigned long long seq, unsigned long long* chal);
struct ScSmallArgs {
  const void* in[MAX_TABS]; Ext* out[MAX_TABS]; int in_ext[MAX_TABS];
  int k[MAX_TERMS]; int t[MAX_TERMS][SC_MAXK]; int off[MAX_TERMS];  // off[i] = sum_{j<i} (k_j + 1): slot of term i in the published message
  int ntabs, nterms, has_r; size_t n_after; Ext r;
};
__device__ __forceinline__ Ext block_reduce_ext_n(Ext v, Ext* sm) {
  v = wave_reduce_ext(v);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  Ext r = ex_zero();
  if (threadIdx.x == 0) { r = sm[0]; for (int i = 1; i < (int)(blockDim.x >> 6); i++) r = ex_add(r, sm[i]); }
  return r;
}
// K1 + K3 + final reduction in ONE workgroup for small tables: fold with r (if any), then every term's round sums.
// Terms are spread over the waves of the block (a term with many pairs is split over several waves), so the only
// block-wide barriers are the one after the fold and the one before the final combine; wave 0 then writes
// result[term*4 + t] straight into host-mapped memory and releases `flag = seq`.
// LDS frame of k_sc_small (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_sc_small {
  Ext part[64 * SC_SLOTS];  // [slot][t], slot = term * wpt + sub  (<= 64 slots)
};
template <bool HI>
KBODY k_sc_small(const ScSmallArgs& a, Ext* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_sc_small, lf); auto& part = lf.part;
  int tid = threadIdx.x, nt = blockDim.x;
  size_t n = a.n_after;
  if (a.has_r) {
    for (int t = 0; t < a.ntabs; t++) {
      Ext* o = a.out[t];
      if (a.in_ext[t]) { const Ext* p = (const Ext*)a.in[t]; for (size_t i = tid; i < n; i += nt) o[i] = ex_lerp(p[2 * i], p[2 * i + 1], a.r); }
      else { const u64* p = (const u64*)a.in[t]; for (size_t i = tid; i < n; i += nt) o[i] = ex_lerp_base(p[2 * i], p[2 * i + 1], a.r); }
    }
    __syncthreads();
  }
  size_t npairs = n / 2;
  int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  int wpt = a.nterms >= W ? 1 : W / a.nterms;  // waves per term
  for (int term = wave / wpt; term < a.nterms; term += (wpt == 1 ? W : a.nterms + W)) {
    int sub = wave % wpt;
    int k = a.k[term];
    GlobalPairs L;
#pragma unroll
    for (int j = 0; j < ScW<HI>::K; j++) { int ti = a.t[term][j < k ? j : 0]; L.p[j] = a.has_r ? (const void*)a.out[ti] : a.in[ti]; L.e[j] = a.has_r ? true : a.in_ext[ti]; }
    Ext acc[SC_SLOTS];
    sc_accumulate<HI>(k, L, (size_t)sub * 64 + lane, (size_t)wpt * 64, npairs, acc);
#pragma unroll
    for (int t = 0; t < SC_SLOTS; t++) if (t <= k) acc[t] = wave_reduce_ext(acc[t]);
    if (lane == 0) { Ext* o = part + (size_t)(term * wpt + sub) * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
    if (wpt > 1) break;  // with several waves per term every wave owns exactly one (term, sub)
  }
  __syncthreads();
  if (wave == 0) sc_publish_fwd(result, part, a.k, a.off, a.nterms, wpt, flag, seq, lane);
}

// ------------------------------------------------------------------------------------------------ device-side Fiat-Shamir
// With many proofs in flight the per-round trip to the host (publish the round sums, the host runs the sponge, the kernel
// polls the mailbox) is what a proof spends its time on: the host threads serve several proofs each and every hop crosses
// PCIe. A persistent sumcheck can instead keep the transcript to itself: it gets the sponge state of the host transcript
// (DuplexChallenger<F,P,8,4>, poseidon/src/challenger.rs:14-46 — poseidon2.h `Challenger`), combines the term sums into the
// round message exactly as sumcheck_prove does (coefficients, extrapolation to max_degree + 1 points: prover.rs:498-585),
// absorbs it, squeezes the challenge (transcript/src/basic.rs:8-54) and goes on; at the end ONE publication carries all
// round messages, all challenges, the final evaluations and the sponge state back to the host transcript.
// Field arithmetic is exact and canonical, so the messages and challenges are the host's bit for bit.
// The sponge runs on wave 0 with the lane-parallel permutation (p2l_permute: state[i] in lane i of every group of 8).
// the reply poll of wc_request: bounded in time like sc_wait_challenge (the emulator of tests/ defines both macros itself and serves
// the request from inside the poll)
#ifndef WC_POLL_PAUSE
#define WC_POLL_BEGIN const unsigned long long wc_t0 = dp_realtime();
#define WC_POLL_PAUSE(spin) wc_poll_pause(wc_t0, spin)
__device__ __forceinline__ bool wc_poll_pause(unsigned long long t0, unsigned spin) {
  if ((spin & 63) == 63 && dp_realtime() - t0 > c_poll_timeout_ticks) return true;
  for (int q = 0; q < c_poll_sleep; q++) __builtin_amdgcn_s_sleep(16);
  return false;
}
#endif
struct ScFsArgs {
  u64 state[8]; u64 in_buf[4]; int in_len, out_len;  // the host Challenger at the start of the first round
  int md, rounds;                                    // max_degree of the virtual polynomial, rounds the kernel runs
  u64 label[2]; int nlabel, pad;                     // "Internal round" as transcript words
  Ext coeff[MAX_TERMS];                              // coefficient of every product term
  u64 io[16];                                        // device side: the words of a round staged for wc_io (the host leaves them alone)
};
__constant__ u64 c_extrap[(SC_MAXK + 1) * (SC_MAXK + 1) * (SC_MAXK + 1)];  // [k][at][i]: extrapolation_coeffs(k, at)[i] of sumcheck.h
// Host mode (req != nullptr, DP_HOST_SPONGE=1; sponge_host.h): the sponge stays in the host transcript. Observed words are staged in the
// mapped request area by lane 0; a sample posts the request (tag = sequence + checksum: the host re-reads until it is complete) and
// every lane polls the reply area for the sponge's output buffer (uniform decision: the tag and length lane 0 read, the four outputs
// lanes 0..3 read, validated by the reply's own tag). 2.9 us per round trip against ~12 us per permutation on an 8-lane wave.
struct WaveChallenger {
#ifdef DP_WG_TIMES
  unsigned long long dbg_sp = 0, dbg_np = 0;  // (filled under DP_WG_PHASES only)
#endif
  u64 st, ib; int in_len, out_len;
  P2lK k;  // this lane's Poseidon2 constants (p2l_load), in registers for the life of the kernel
  u64* req = nullptr; const u64* rep = nullptr; unsigned n = 0, consumed = 0, failed = 0; unsigned long long rseq = 0, cs = 0; u64 cache = 0;
};
__device__ __forceinline__ void wc_host_init(WaveChallenger& c, u64* req, const u64* rep, unsigned long long seq0) {
  c.req = req; c.rep = rep; c.rseq = seq0; c.n = c.consumed = c.failed = 0; c.cs = 0; c.cache = 0;
  if (req) c.out_len = 0;  // nothing cached: the first sample asks the host
}
__device__ __forceinline__ void wc_request(WaveChallenger& c, int lane, int want) {
  c.rseq++;
  if (lane == 0) {
    pub_store(c.req + 1, (u64)c.n); pub_store(c.req + 2, (u64)c.consumed); pub_store(c.req + 3, (u64)want);
    pub_store(c.req, wc_req_mix(c.rseq) + c.cs + 3ull * c.n + 5ull * c.consumed + 7ull * (u64)want);
  }
  const unsigned long long base = wc_rep_mix(c.rseq);
  u64 ol = 0, o = 0;
  bool ok = false;
  WC_POLL_BEGIN
  u64 seen = __hip_atomic_load(c.rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (the previous reply's tag)
  seen = shfl_u64(seen, 0);
  for (unsigned spin = 0;; spin++) {
    // one PCIe read per poll (every lane asks for the same word): the payload is only fetched once the tag word has changed —
    // 264 workgroups polling three words each saturate the link's read rate and slow every poll down
    u64 tag = __hip_atomic_load(c.rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    tag = shfl_u64(tag, 0);
    if (tag != seen || spin == 0) {
      ol = __hip_atomic_load(c.rep + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      o = __hip_atomic_load(c.rep + 2 + (lane & 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      ol = shfl_u64(ol, 0);
      const u64 w = o * (u64)((lane & 3) + 1);
      const u64 sum = ol + shfl_u64(w, 0) + shfl_u64(w, 1) + shfl_u64(w, 2) + shfl_u64(w, 3);
      if (tag == base + sum && ol <= 4) { ok = true; break; }
    }
    if (WC_POLL_PAUSE(spin)) break;
  }
  c.n = 0; c.cs = 0; c.consumed = 0;
  if (ok) { c.out_len = (int)ol; c.cache = o; } else { c.failed = 1; c.out_len = 4; c.cache = 0; }
}
// end of a kernel: the words observed since the last sample, and the samples popped since the last reply, reach the host before the
// kernel's own message does (the host transcript is complete when the proof's thread sees that message)
__device__ __forceinline__ void wc_finish(WaveChallenger& c, int lane) { if (c.req) wc_request(c, lane, 0); }
__device__ __forceinline__ void wc_duplex(WaveChallenger& c, int lane) {
  if ((lane & 7) < c.in_len) c.st = c.ib;
  c.in_len = 0;
#ifdef DP_WG_PHASES
  const unsigned long long dbg_t = dp_realtime();
#endif
  c.st = p2l_permute(c.st, lane, c.k);
#ifdef DP_WG_PHASES
  c.dbg_sp += dp_realtime() - dbg_t; c.dbg_np++;
#endif
  c.out_len = 4;
}
__device__ __forceinline__ void wc_observe_host(WaveChallenger& c, u64 v, int lane) {
  c.out_len = 0;
  if (lane == 0) { pub_store(c.req + 4 + c.n, v); c.cs += (unsigned long long)(c.n + 1) * v; }
  if (++c.n == WC_REQ_CAP) wc_request(c, lane, 0);
}
__device__ __forceinline__ u64 wc_sample_host(WaveChallenger& c, int lane) {
  if (c.n != 0 || c.out_len == 0) wc_request(c, lane, 1);
  --c.out_len; c.consumed++;
  return shfl_u64(c.cache, c.out_len);
}
__device__ __forceinline__ void wc_observe(WaveChallenger& c, u64 v, int lane) {  // v uniform over the wave
  if (c.req) { wc_observe_host(c, v, lane); return; }
  c.out_len = 0;
  if ((lane & 7) == c.in_len) c.ib = v;
  if (++c.in_len == 4) wc_duplex(c, lane);
}
__device__ __forceinline__ u64 wc_sample(WaveChallenger& c, int lane) {
  if (c.req) return wc_sample_host(c, lane);
  if (c.in_len != 0 || c.out_len == 0) wc_duplex(c, lane);
  --c.out_len;
  return shfl_u64(c.st, c.out_len);
}
// A run of transcript operations from ONE call site: absorb w[0 .. nin) (LDS or global memory, the same address on every lane), then draw nout <= 2 samples.
// The same sponge states as wc_observe x nin followed by wc_sample x nout — but the permutation is inlined ONCE however long the run is. wc_observe /
// wc_sample inline a copy of it (~17 KB of code) per call, and a Fiat-Shamir round written with them walks through 12 copies: ~200 KB of instructions per
// round through a 64 KB instruction cache shared by two CUs, every permutation fetched cold (10.6 us under load against 7.3 us in a loop, profiles/r05_*).
__device__ __forceinline__ void wc_io(WaveChallenger& c, const u64* w, int nin, u64& o0, u64& o1, int nout, int lane) {
  if (c.req) {
    for (int i = 0; i < nin; i++) wc_observe_host(c, w[i], lane);
    if (nout > 0) o0 = wc_sample_host(c, lane);
    if (nout > 1) o1 = wc_sample_host(c, lane);
    return;
  }
  int wi = 0, oi = 0;
  for (;;) {
    if (wi < nin) {
      c.out_len = 0;
      if ((lane & 7) == c.in_len) c.ib = w[wi];
      wi++;
      if (++c.in_len < 4) continue;
    } else if (oi < nout) {
      if (c.in_len == 0 && c.out_len != 0) {
        --c.out_len;
        const u64 v = shfl_u64(c.st, c.out_len);
        if (oi == 0) o0 = v; else o1 = v;
        oi++;
        continue;
      }
    } else break;
    wc_duplex(c, lane);
  }
}
__device__ __forceinline__ Ext sc_term_sum(const Ext* part, int term, int t, int wpt) {
  if (wpt == 1) return part[(size_t)term * SC_SLOTS + t];
  Ext v = ex_zero();
  for (int sb = 0; sb < wpt; sb++) v = ex_add(v, part[(size_t)(term * wpt + sb) * SC_SLOTS + t]);
  return v;
}
// host result area of a device-driven sumcheck, in words: [rounds x (md+1) message values][rounds challenges][ntabs finals][14 sponge words]
__device__ __forceinline__ size_t fs_msg_word(const ScFsArgs& f, int round, int j) { return ((size_t)round * (f.md + 1) + j) * 2; }
__device__ __forceinline__ size_t fs_chal_word(const ScFsArgs& f, int round) { return ((size_t)f.rounds * (f.md + 1) + round) * 2; }
__device__ __forceinline__ size_t fs_final_word(const ScFsArgs& f) { return ((size_t)f.rounds * (f.md + 2)) * 2; }
// One round on wave 0 (all 64 lanes): part[] holds the raw term sums. Returns the challenge; `cs` accumulates the checksum
// of the words this lane has sent to the host.
__device__ __forceinline__ Ext sc_fs_round(WaveChallenger& wc, ScFsArgs& f, const Ext* part, const int* tk, int nterms, int wpt, u64* rw, int round, unsigned long long& cs, int lane) {
  const int j = lane & 7, tg = lane >> 3;
  Ext acc = ex_zero();
  if (j <= f.md) {
    for (int t = tg; t < nterms; t += 8) {
      int k = tk[t];
      Ext v;
      if (j <= k) v = sc_term_sum(part, t, j, wpt);
      else {
        const u64* c = c_extrap + ((size_t)k * (SC_MAXK + 1) + j) * (SC_MAXK + 1);
        v = ex_zero();
        for (int i = 0; i <= k; i++) v = ex_add(v, ex_mul_base(sc_term_sum(part, t, i, wpt), c[i]));
      }
      acc = ex_add(acc, ex_mul(v, f.coeff[t]));
    }
  }
#pragma unroll
  for (int d = 8; d <= 32; d <<= 1) {
    Ext o = ex(shfl_u64(acc.c0, lane ^ d), shfl_u64(acc.c1, lane ^ d));
    acc = ex_add(acc, o);
  }
  // lanes 0..md hold the message: staged in LDS with the round label behind it, absorbed and answered from ONE wc_io site (see there)
  const int nmsg = 2 * (f.md + 1);
  if (lane <= f.md) {
    f.io[2 * lane] = acc.c0; f.io[2 * lane + 1] = acc.c1;
    const size_t w = fs_msg_word(f, round, lane);
    MSG_PUT(rw + w, acc.c0); MSG_PUT(rw + w + 1, acc.c1); cs += (unsigned long long)(w + 1) * acc.c0 + (unsigned long long)(w + 2) * acc.c1;
  } else if (lane - (f.md + 1) < f.nlabel) f.io[nmsg + lane - (f.md + 1)] = f.label[lane - (f.md + 1)];
  DP_WAVE_SYNC();
  u64 r0 = 0, r1 = 0;
  wc_io(wc, f.io, nmsg + f.nlabel, r0, r1, 2, lane);
  if (lane == 0) { size_t w = fs_chal_word(f, round); MSG_PUT(rw + w, r0); MSG_PUT(rw + w + 1, r1); cs += (unsigned long long)(w + 1) * r0 + (unsigned long long)(w + 2) * r1; }
  return ex(r0, r1);
}
// the last message of a device-driven sumcheck: final evaluation of every table (src[e * stride]) and the sponge complete the message in LDS (rw); it leaves for the
// host (host) in one burst, the tag behind it
__device__ __forceinline__ void sc_fs_finish(const WaveChallenger& wc, const ScFsArgs& f, const Ext* const* srcs, const Ext* src, size_t stride, int ntabs, u64* rw, u64* host, unsigned long long* flag, unsigned long long seq, unsigned long long cs, int lane) {
  size_t w0 = fs_final_word(f);
  for (int e = lane; e < ntabs; e += 64) {
    Ext v = srcs ? srcs[e][0] : src[(size_t)e * stride];
    size_t w = w0 + 2 * e;
    MSG_PUT(rw + w, v.c0); MSG_PUT(rw + w + 1, v.c1);
    cs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
  }
  size_t ws = w0 + 2 * (size_t)ntabs;
  if (lane < 8) { MSG_PUT(rw + ws + lane, wc.st); cs += (unsigned long long)(ws + lane + 1) * wc.st; }
  if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rw + ws + 8 + lane, v); cs += (unsigned long long)(ws + 8 + lane + 1) * v; }
  if (lane == 0) {
    u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
    MSG_PUT(rw + ws + 12, a); MSG_PUT(rw + ws + 13, b);
    cs += (unsigned long long)(ws + 13) * a + (unsigned long long)(ws + 14) * b;
  }
  cs = pub_wave_sum(cs);
  msg_flush(host, rw, ws + 14, lane);
  if (lane == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
}
__device__ __forceinline__ void wc_load(WaveChallenger& wc, const ScFsArgs& f, int lane) {
  wc.st = f.state[lane & 7]; wc.ib = f.in_buf[lane & 3]; wc.in_len = f.in_len; wc.out_len = f.out_len;
}

// ------------------------------------------------------------------------------------------------ persistent sumcheck
// A whole (tail of a) sumcheck in ONE launch of ONE workgroup: per round the kernel publishes the raw term sums to
// host-mapped memory, the host runs the Fiat-Shamir sponge and posts the challenge into a host-mapped mailbox which
// the kernel polls; then the kernel folds every table and goes on. No kernel launch, no stream synchronisation and no
// memcpy on the per-round critical path — only two PCIe hops. Ends by publishing the final evaluation of every table.
struct ScPersistArgs {
  const void* in[MAX_TABS]; int in_ext[MAX_TABS];
  Ext* bufA[MAX_TABS]; Ext* bufB[MAX_TABS];
  int k[MAX_TERMS]; int t[MAX_TERMS][SC_MAXK]; int off[MAX_TERMS];
  int ntabs, nterms, has_r0; size_t n0; Ext r0;
  unsigned long long* dbg;  // optional: per-phase cycle counters (DP_SC_DEBUG=1)
  int eq_tab, eq_k;         // eq_tab >= 0: table eq_tab (an extension buffer in global memory) is eq(., eq_pt) and is built here first
  Ext eq_pt[MAX_PT];
  // multi-workgroup phase (k_sc_persist only): workgroup g of nwg owns the contiguous slice [g n0/nwg, (g+1) n0/nwg) of
  // every table, publishes the sums of its slice into result slot g (slot_ext extension values apart, flag word g) and
  // leaves after `rounds_a` folds; the host adds the shares. nwg = 1, rounds_a = 0: the whole sumcheck in one workgroup.
  int nwg, rounds_a, slot_ext;
};
// out[i] = prod_t (i_t ? pt[t] : 1 - pt[t]) for i < 2^k, by the whole workgroup (ends with a barrier)
__device__ __forceinline__ void wg_build_eq(Ext* out, const Ext* pt, int k) {
  size_t n = size_t(1) << k;
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
    Ext v = ex_one();
    for (int t = 0; t < k; t++) { Ext r = pt[t]; v = ex_mul(v, ((i >> t) & 1) ? r : ex_sub(ex_one(), r)); }
    out[i] = v;
  }
  __syncthreads();
}
__device__ __forceinline__ void sc_fold_all(const ScPersistArgs& a, const void* const* cur, const int* cur_ext, Ext* const* dst, size_t n_after, Ext r, size_t dst_off = 0) {
  int tid = threadIdx.x, nt = blockDim.x;
  for (int t = 0; t < a.ntabs; t++) {
    Ext* o = dst[t] + dst_off;
    if (cur_ext[t]) { const Ext* p = (const Ext*)cur[t]; for (size_t i = tid; i < n_after; i += nt) o[i] = ex_lerp(p[2 * i], p[2 * i + 1], r); }
    else { const u64* p = (const u64*)cur[t]; for (size_t i = tid; i < n_after; i += nt) o[i] = ex_lerp_base(p[2 * i], p[2 * i + 1], r); }
  }
}
// LDS frame of k_sc_persist (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_sc_persist {
  ScPersistArgs a;  // the launch's arguments, copied once: the body reads them in every round, and the kernarg segment / the pack table is HOST memory (a PCIe round trip per uncached scalar load)
  Ext part[64 * SC_SLOTS];
  unsigned long long chal[3];
  const void* cur[MAX_TABS];
  int cur_ext[MAX_TABS];
  Ext* dstA[MAX_TABS];
  Ext* dstB[MAX_TABS];
  ScFsArgs fsl;
};
template <bool HI>
KBODY k_sc_persist(const ScPersistArgs& a_in, Ext* result, unsigned long long* flag, const unsigned long long* mailbox, unsigned long long seq0, const ScFsArgs* fs) {
  DP_LDS_FRAME(Lds_k_sc_persist, lf); auto& part = lf.part;
  for (int i = threadIdx.x; i < (int)(sizeof(ScPersistArgs) / 8); i += blockDim.x) ((u64*)&lf.a)[i] = ((const u64*)&a_in)[i];
  __syncthreads();
  const ScPersistArgs& a = lf.a; auto& chal = lf.chal; auto& cur = lf.cur; auto& cur_ext = lf.cur_ext; auto& dstA = lf.dstA; auto& dstB = lf.dstB; auto& fsl = lf.fsl;
  DP_LDS_DYN(lds_msg, u64);
  u64* const mb = (u64*)lds_msg;  // device-side Fiat-Shamir: the message is assembled here (the launch brings rounds (md + 2) 2 + 2 ntabs + 14 words of dynamic LDS)
  int tid = threadIdx.x, nt = blockDim.x;
  int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  const bool autofs = fs != nullptr;  // device-side Fiat-Shamir (single workgroup only): no host round trips
  if (autofs) for (int i = tid; i < (int)(sizeof(ScFsArgs) / 8); i += nt) ((u64*)&fsl)[i] = ((const u64*)fs)[i];
  if (a.eq_tab >= 0) wg_build_eq((Ext*)a.in[a.eq_tab], a.eq_pt, a.eq_k);
  const size_t g = blockIdx.x;
  size_t n = a.n0 / (size_t)a.nwg;  // local slice length
  if (tid < a.ntabs) { cur[tid] = (const char*)a.in[tid] + g * n * (a.in_ext[tid] ? 16 : 8); cur_ext[tid] = a.in_ext[tid]; dstA[tid] = a.bufA[tid]; dstB[tid] = a.bufB[tid]; }
  result += g * (size_t)a.slot_ext; flag += g;
  int folds = 0;
  size_t lvl_off = 0;
  __syncthreads();
  unsigned long long seq = seq0;
  bool useA = true;
  WaveChallenger wc; wc.k = p2l_load(lane); wc.st = wc.ib = 0; wc.in_len = wc.out_len = 0;
  if (autofs) wc_load(wc, fsl, lane);
  unsigned long long fcs = 0; int round = 0;
  if (a.has_r0) {
    // (several workgroups: the fold with the pending challenge fills this workgroup's slice of the first level region of bufA;
    // the regions of the later levels follow it — see the comment at the round fold below)
    const size_t off0 = a.nwg > 1 ? g * (n / 2) : 0;
    sc_fold_all(a, cur, cur_ext, dstA, n / 2, a.r0, off0);
    __syncthreads();
    if (tid < a.ntabs) { cur[tid] = dstA[tid] + off0; cur_ext[tid] = 1; }
    __syncthreads();
    n /= 2; useA = false;
    if (a.nwg > 1) lvl_off = (size_t)a.nwg * n;
  }
  int wpt = a.nterms >= W ? 1 : W / a.nterms;
  for (;;) {
    size_t npairs = n / 2;
    for (int term = wave / wpt; term < a.nterms; term += (wpt == 1 ? W : a.nterms + W)) {
      int sub = wave % wpt;
      int k = a.k[term];
      GlobalPairs L;
#pragma unroll
      for (int j = 0; j < ScW<HI>::K; j++) { int ti = a.t[term][j < k ? j : 0]; L.p[j] = cur[ti]; L.e[j] = cur_ext[ti]; }
      Ext acc[SC_SLOTS];
      sc_accumulate<HI>(k, L, (size_t)sub * 64 + lane, (size_t)wpt * 64, npairs, acc);
#pragma unroll
      for (int t = 0; t < SC_SLOTS; t++) if (t <= k) acc[t] = wave_reduce_ext(acc[t]);
      if (lane == 0) { Ext* o = part + (size_t)(term * wpt + sub) * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
      if (wpt > 1) break;
    }
    __syncthreads();
    ++seq;
    if (wave == 0) {
      if (autofs) { Ext rr = sc_fs_round(wc, fsl, part, a.k, a.nterms, wpt, mb, round, fcs, lane); if (lane == 0) { chal[0] = 1; chal[1] = rr.c0; chal[2] = rr.c1; } }
      else { sc_publish_fwd(result, part, a.k, a.off, a.nterms, wpt, flag, seq, lane); if (lane == 0) sc_wait_challenge_fwd(mailbox, seq, chal); }
    }
    round++;
    __syncthreads();
    if (chal[0] == 0) {  // host never answered: publish an abort marker and leave
      if (tid == 0) pub_store((u64*)flag, ~0ull);
      return;
    }
    Ext r = ex(chal[1], chal[2]);
    // One workgroup: ping-pong between bufA and bufB. Several workgroups: the folded slice goes to its place in the compact
    // folded table of this level, and every level has its own region of bufA (level 1 at 0, level 2 behind it, ..): the
    // workgroups sit on different XCDs whose L2s are not coherent with each other, so no address may be written by two
    // workgroups during the life of the kernel (a stale dirty line of an old level could be written back over a new one).
    Ext* const* dst = (a.nwg > 1 || useA) ? dstA : dstB;
    size_t off = a.nwg > 1 ? lvl_off + g * (n / 2) : 0;
    sc_fold_all(a, cur, cur_ext, dst, n / 2, r, off);
    __syncthreads();
    if (tid < a.ntabs) { cur[tid] = dst[tid] + off; cur_ext[tid] = 1; }
    __syncthreads();
    lvl_off += (size_t)a.nwg * (n / 2);
    n /= 2; useA = !useA;
    if (++folds == a.rounds_a) return;  // end of the multi-workgroup phase: the compact folded tables are complete
    if (n == 1) {
      ++seq;
      if (wave == 0 && autofs) sc_fs_finish(wc, fsl, (const Ext* const*)cur, nullptr, 0, a.ntabs, mb, (u64*)result, flag, seq0 + 1, fcs, lane);
      else if (wave == 0) {
        unsigned long long cs = 0; u64* rw = (u64*)result;
        for (int e = lane; e < a.ntabs; e += 64) { Ext v = ((const Ext*)cur[e])[0]; pub_store(rw + 2 * e, v.c0); pub_store(rw + 2 * e + 1, v.c1); cs += (unsigned long long)(2 * e + 1) * v.c0 + (unsigned long long)(2 * e + 2) * v.c1; }
        cs = pub_wave_sum(cs);
        if (lane == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
      }
      return;
    }
  }
}

#ifdef DP_LOGUP_TAIL_V1
#include "../../tools/archive/k_logup_tail_v1.inc"
#else
// ------------------------------------------------------------------------------------------------ whole logup-GKR layer loop
// Dev::logup_tail (dev.h): every layer of a logup-GKR batch proof (logup_layers of logup.h: absorb the claim, the batched
// layer sumcheck with its Fiat-Shamir rounds, the three layer challenges, the next claim) in ONE launch of one workgroup —
// one device wait per lookup argument instead of one per tree layer; in full mode (Dev::logup_full, DP_DEVICE_LOGUP=2) also
// the trees, the circuit outputs, the initial challenges and the column claims. Default in throughput mode (DP_DEVICE_LOGUP=0 / 1 select the
// layer-by-layer path / the layer loop only); written against the contract pinned by the CPU double (tests/support/cpu_dev.hpp),
// checked on the SIMT emulator and on MI355X (tests/test_gpu_fused.py).
//
// Round 5 form (the round-4 form is tools/archive/k_logup_tail_v1.inc; -DDP_LOGUP_TAIL_V1 builds it instead). A member of a merged launch is a chain of
// ~220 sponge permutations on ONE wave (7.3 us each); round 4 spent another 1.5 x that time between them — the round sums over tables in GLOBAL memory
// (a dependent L2 round trip per table and round), three workgroup barriers and a separate fold per Fiat-Shamir round. Here:
//  * the tables of a tree layer live in LDS (dynamic, dl.lds_ext extension values) in bit-reversed order from the first round in which they fit: pair b of a
//    table of length m is (b, b + m/2), a fold writes its results where it read (no hazard, no ping-pong); the tree itself stays in global memory and is
//    read once per layer, by all lanes at once. Tables longer than their share of LDS start with global rounds (natural order, ping-pong through bufA / bufB);
//  * ONE pass per Fiat-Shamir round: it folds the tables with the challenge of the previous round AND accumulates this round's sums from the folded pairs;
//  * a pass gives four lanes to every (instance, pair): lane t of the quad folds table t of the instance, the quad exchanges the folded pairs (DPP quad
//    broadcasts) and lane t evaluates the batched product at t — the terms arrive combined with their coefficients, the reduction is 4 steps over one value;
//    evaluating a degree-2 term at t = 3 is what extrapolating it from t = 0..2 gives (exact field arithmetic: same element);
//  * rounds with at most 16 (instance, pair) items — all but the first few rounds of the widest layers — run on the sponge wave alone: no workgroup barrier
//    on the chain at all; wider rounds use every wave and two barriers.
// Result area, in words, one block per layer lv = 1..L followed by the
// sponge: [lv x 4 message values][lv challenges][batching][final evaluations without eq] ... [8 state, 4 input buffer,
// in_len, out_len]; the tag is mix(seq) + sum over blocks of sum_i (i + 1) * word_i with i relative to the block.
static_assert(LT_MAX_TABS == MAX_TABS, "logup_tail.h: table capacity");
// the line through (0, lo) and (1, hi) at the small integer t
__device__ __forceinline__ Ext ex_at(Ext lo, Ext hi, u64 t) {
  const Ext d = ex_sub(hi, lo);
#if DP_GX_ON
  return ex(gl_canon_any(gx::fma(d.c0, t, lo.c0)), gl_canon_any(gx::fma(d.c1, t, lo.c1)));
#else
  return ex_add(lo, ex_mul_base(d, t));
#endif
}
// lane K of every quad, seen by the whole quad
template <int K> __device__ __forceinline__ Ext ex_quad_bcast(Ext v) {
  constexpr int C = K | (K << 2) | (K << 4) | (K << 6);
  return ex(dpp_u64<C>(v.c0), dpp_u64<C>(v.c1));
}
__device__ __forceinline__ unsigned lt_brev(unsigned x, unsigned bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
// LDS frame of k_logup_tail (static __shared__ behind kg / kc); the tables follow in the launch's dynamic LDS
struct Lds_k_logup_tail {
  LogupTailDesc dl;
  Ext part[16 * 4];           // wide passes: the four message values of every wave
  Ext chal;                   // wide passes: the challenge of the round at hand
  const void* cur[MAX_TABS];  // the layer's tables in the tree (global memory, natural order)
  int cur_ext[MAX_TABS];
  Ext pt[MAX_PT];
  Ext glue[4];                // batching, alpha, lambda, claim of the layer at hand
  Ext ca[LT_MAXI];            // alpha^i: the coefficient of instance i in the layer at hand
  Ext fin[MAX_TABS];          // final evaluations of the layer's tables (without eq)
  alignas(16) u64 pre[2];     // full mode: pre[1] = the number of instances — the word the transcript takes right before the outputs
  Ext outs[LT_MAXI * 4];      // full mode: [n0, n1, d0, d1] of every instance (directly behind pre: one run of words for wc_io)
  Ext chip[8];                // full mode: chi^j
  u64 io[16];                 // words staged for wc_io
};
static_assert(offsetof(Lds_k_logup_tail, outs) == offsetof(Lds_k_logup_tail, pre) + 16, "k_logup_tail: the outputs follow the instance count");
// One pass of the layer loop over the (instance, pair) items quad number `qid` of `qn` is responsible for (every lane of the wave runs the same number of
// iterations: the cross-lane moves sit in wave-uniform control flow): fold the tables with r when `fold`, store the folded pairs (dst 1: LDS, 2: the other
// global buffer, 0: nowhere — round 0 of tables that do not fit), return this lane's share of the round message at t = lane & 3.
//   src_lds: tables (and eq) are in LDS, bit-reversed; else in global memory, natural order: gsrc 0 = the tree (lf.cur; eq in LDS when eq_lds, else dl.eq),
//   1 / 2 = bufA / bufB. eqsel: which half of the eq double buffer holds the current eq table (the fold writes the other one).
__device__ __forceinline__ Ext lt_pass(Lds_k_logup_tail& lf, Ext* LT, unsigned S, Ext* EQ0, Ext* EQ1, bool fold, bool src_lds, int gsrc, bool eq_lds, int dst, int eqsel,
                                       unsigned npairs, unsigned lgp, int tpi, bool init_lk, Ext r, unsigned qid, unsigned qn, int lane) {
  const LogupTailDesc& dl = lf.dl;
  const int t = lane & 3;
  const unsigned nitems = (unsigned)dl.ninst * npairs;
  const Ext la = lf.glue[2];
  Ext* const eq_cur = eqsel ? EQ1 : EQ0;
  Ext* const eq_nxt = eqsel ? EQ0 : EQ1;
  Ext acc = ex_zero();
  for (unsigned base = 0; base < nitems; base += qn) {
    const unsigned it = base + qid;
    const bool on = it < nitems;
    const unsigned i = on ? it >> lgp : 0u, b = it & (npairs - 1);
    const int tau = 1 + (int)i * tpi + t;
    const bool mine = on && t < tpi;
    Ext elo = ex_zero(), ehi = ex_zero(), tlo = ex_zero(), thi = ex_zero();
    if (src_lds) {  // (always a fold: round 0 reads the tree)
      if (on) { elo = ex_lerp(eq_cur[b], eq_cur[b + 2 * npairs], r); ehi = ex_lerp(eq_cur[b + npairs], eq_cur[b + 3 * npairs], r); }
      if (mine) {
        Ext* p = LT + (size_t)tau * S;
        tlo = ex_lerp(p[b], p[b + 2 * npairs], r); thi = ex_lerp(p[b + npairs], p[b + 3 * npairs], r);
        p[b] = tlo; p[b + npairs] = thi;
      }
      if (on && i == 0 && t == 0) { eq_nxt[b] = elo; eq_nxt[b + npairs] = ehi; }
    } else {
      const unsigned c = dst == 1 ? lt_brev(b, lgp) : b;  // the pair this item stands for, in natural order
      if (on) {
        if (!fold && eq_lds) { elo = eq_cur[b]; ehi = eq_cur[b + npairs]; }
        else {
          const Ext* pe = gsrc == 0 ? (const Ext*)dl.eq : gsrc == 1 ? (const Ext*)dl.bufA[0] : (const Ext*)dl.bufB[0];
          if (fold) { elo = ex_lerp(pe[4 * (size_t)c], pe[4 * (size_t)c + 1], r); ehi = ex_lerp(pe[4 * (size_t)c + 2], pe[4 * (size_t)c + 3], r); }
          else { elo = pe[2 * (size_t)c]; ehi = pe[2 * (size_t)c + 1]; }
        }
      }
      if (mine) {
        const void* p = gsrc == 0 ? lf.cur[tau] : gsrc == 1 ? (const void*)dl.bufA[tau] : (const void*)dl.bufB[tau];
        const bool pext = gsrc == 0 ? lf.cur_ext[tau] != 0 : true;
        if (pext) {
          const Ext* q = (const Ext*)p;
          if (fold) { tlo = ex_lerp(q[4 * (size_t)c], q[4 * (size_t)c + 1], r); thi = ex_lerp(q[4 * (size_t)c + 2], q[4 * (size_t)c + 3], r); }
          else { tlo = q[2 * (size_t)c]; thi = q[2 * (size_t)c + 1]; }
        } else {
          const u64* q = (const u64*)p;
          if (fold) { tlo = ex_lerp_base(q[4 * (size_t)c], q[4 * (size_t)c + 1], r); thi = ex_lerp_base(q[4 * (size_t)c + 2], q[4 * (size_t)c + 3], r); }
          else { tlo = ex_base(q[2 * (size_t)c]); thi = ex_base(q[2 * (size_t)c + 1]); }
        }
        if (dst == 1) { Ext* o = LT + (size_t)tau * S; o[b] = tlo; o[b + npairs] = thi; }
        else if (dst == 2) { Ext* o = gsrc == 1 ? dl.bufB[tau] : dl.bufA[tau]; o[2 * (size_t)c] = tlo; o[2 * (size_t)c + 1] = thi; }
      }
      if (on && i == 0 && t == 0 && (fold || !eq_lds)) {
        if (dst == 1) { Ext* o = fold ? eq_nxt : eq_cur; o[b] = elo; o[b + npairs] = ehi; }
        else if (dst == 2) { Ext* o = gsrc == 1 ? dl.bufB[0] : dl.bufA[0]; o[2 * (size_t)c] = elo; o[2 * (size_t)c + 1] = ehi; }
      }
    }
    // the quad's four folded pairs, seen by each of its lanes (table order of an instance: nlo, dhi, nhi, dlo; the initial lookup layer: dhi, dlo)
    const Ext a0 = ex_quad_bcast<0>(tlo), b0 = ex_quad_bcast<0>(thi), a1 = ex_quad_bcast<1>(tlo), b1 = ex_quad_bcast<1>(thi);
    const Ext a2 = ex_quad_bcast<2>(tlo), b2 = ex_quad_bcast<2>(thi), a3 = ex_quad_bcast<3>(tlo), b3 = ex_quad_bcast<3>(thi);
    const u64 tt = (u64)t;
    const Ext e = ex_mul(lf.ca[i], ex_at(elo, ehi, tt));
    Ext x;
    if (!init_lk) {
      const Ext nlo = ex_at(a0, b0, tt), dhi = ex_at(a1, b1, tt), nhi = ex_at(a2, b2, tt), dlo = ex_at(a3, b3, tt);
      x = ex_add(ex_add(ex_mul(nlo, dhi), ex_mul(nhi, dlo)), ex_mul(la, ex_mul(dlo, dhi)));
    } else {
      const Ext dhi = ex_at(a0, b0, tt), dlo = ex_at(a1, b1, tt);
      x = ex_sub(ex_mul(la, ex_mul(dlo, dhi)), ex_add(dhi, dlo));
    }
    if (on) acc = ex_add(acc, ex_mul(e, x));
  }
#pragma unroll
  for (int d = 4; d <= 32; d <<= 1) acc = ex_add(acc, ex(shfl_u64(acc.c0, lane ^ d), shfl_u64(acc.c1, lane ^ d)));
  return acc;
}
KBODY k_logup_tail(const LogupTailDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_DYN(lds_dyn, Lds_k_logup_tail);
  DP_LDS_FRAME(Lds_k_logup_tail, lf);
  LogupTailDesc& dl = lf.dl;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
#ifdef DP_WG_TIMES
  const unsigned long long dbg_t_in = dp_realtime();
#endif
  for (int i = tid; i < (int)(sizeof(LogupTailDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  if (tid == 0) {
    lf.glue[0] = dl.batching; lf.glue[1] = dl.alpha; lf.glue[2] = dl.lambda; lf.glue[3] = dl.claim; lf.pt[0] = dl.batching;
    Ext c = ex_one();
    for (int i = 0; i < dl.ninst; i++) { lf.ca[i] = c; c = ex_mul(c, dl.alpha); }
  }
#ifdef DP_WG_PHASES
  unsigned long long dbg_ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dbg_tp = dbg_t_in, dbg_spp = 0;
#define DBG_PHASE(k) do { const unsigned long long now_ = dp_realtime(); dbg_ph[k] += (now_ - dbg_tp) - (wc.dbg_sp - dbg_spp); dbg_tp = now_; dbg_spp = wc.dbg_sp; } while (0)
#else
#define DBG_PHASE(k) ((void)0)
#endif
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  size_t wbase = 0;
  // The message is assembled in LDS (behind the table slots) and leaves for the host in ONE burst at the end: a store to host-mapped memory is acknowledged
  // across PCIe, and the next wait for outstanding memory operations (a fence, a barrier, a flat access) stalls until it is — microseconds per round with
  // hundreds of proofs sharing the link (alone: 0.36 ms of a member outside the sponge, at 448 in flight: 1.5 ms; profiles/r05_*)
  u64* const mb = (u64*)((Ext*)lds_dyn + dl.lds_ext);
  __syncthreads();
  if (dl.full) {
    // ---- full mode (Dev::logup_full). The fractional-sum tree of every instance, as k_logup_tree builds it: denominators
    // c + sum_j chi^j col_j, then layer by layer (n1 d2 + d1 n2, d1 d2) over the pairs (i, i + half) — all instances side by side, one barrier per level
    const size_t n = dl.n;
    const unsigned lgn = (unsigned)dl.nlayers;
    if (tid == 0) { Ext pw = ex_one(); for (int j = 0; j < dl.cpi; j++) { lf.chip[j] = pw; pw = ex_mul(pw, dl.chi); } }
    __syncthreads();
    for (size_t idx = tid; idx < (size_t)dl.ninst * n; idx += nt) {
      const int s = (int)(idx >> lgn); const size_t i = idx & (n - 1);
      Ext acc = dl.c;
      for (int j = 0; j < dl.cpi; j++) acc = ex_add(acc, ex_mul_base(lf.chip[j], dl.col[s][j][i]));
      dl.den_all[s][i] = acc;
    }
    __syncthreads();
    {
      int mode = dl.is_table ? 1 : 0;  // 0: all numerators are -1 (lookup), 1: base-field multiplicities (table), 2: extension
      size_t len = n, doff = 0, noff = 0, nprev = 0;
      unsigned lgh = lgn - 1;
      while (len > 2) {
        const size_t half = len / 2;
        for (size_t idx = tid; idx < (size_t)dl.ninst * half; idx += nt) {
          const int s = (int)(idx >> lgh); const size_t i = idx & (half - 1);
          const Ext* dcur = dl.den_all[s] + doff;
          const Ext d1 = dcur[i], d2 = dcur[i + half];
          Ext nn;
          if (mode == 0) nn = ex_neg(ex_add(d1, d2));
          else if (mode == 1) { const u64* q = dl.mult; nn = ex_add(ex_mul_base(d2, q[i]), ex_mul_base(d1, q[i + half])); }
          else { const Ext* q = dl.num_all[s] + nprev; nn = ex_add(ex_mul(q[i], d2), ex_mul(d1, q[i + half])); }
          dl.num_all[s][noff + i] = nn;
          dl.den_all[s][doff + len + i] = ex_mul(d1, d2);
        }
        __syncthreads();
        mode = 2; nprev = noff;
        doff += len; noff += half; len = half; lgh--;
      }
      if (tid < 4 * dl.ninst) {  // the 2-element top layers: [n0, n1, d0, d1]
        const int s = tid >> 2, q = tid & 3;
        Ext v;
        if (q < 2) { if (mode == 0) v = ex_neg(ex_one()); else if (mode == 1) v = ex_base(dl.mult[q]); else v = (dl.num_all[s] + nprev)[q]; }
        else v = (dl.den_all[s] + doff)[q - 2];
        lf.outs[tid] = v;
      }
    }
    if (tid == 0) {
      lf.pre[1] = (u64)dl.ninst;  // (the transcript takes the number of instances, then their outputs: one run of words)
      for (int s = 0; s < dl.ninst; s++)
        for (int li = 0; li < dl.nlayers; li++) {
          dl.den[s][li] = dl.den_all[s] + (2 * n - ((2 * n) >> li));
          dl.num[s][li] = li == 0 ? (const void*)dl.mult : (const void*)(dl.num_all[s] + (n - ((2 * n) >> li)));
        }
    }
    __syncthreads();
    if (wave == 0)  // the outputs open the message
      for (int e = lane; e < 4 * dl.ninst; e += 64) {
        const Ext v = lf.outs[e];
        const size_t w = 2 * (size_t)e;
        mb[w] = v.c0; mb[w + 1] = v.c1;
        fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
      }
    wbase = (size_t)dl.ninst * 8;
  }
  DBG_PHASE(0);
  Ext* const LT = (Ext*)lds_dyn;
  // lv = 0 stands for what precedes the first layer: (full mode) the outputs, the three initial challenges and the first claim; then, as after every layer, the
  // claim and the sumcheck header of the layer that follows. Everything the transcript does outside the rounds goes through ONE wc_io site below, the rounds
  // through a second one: the sponge permutation is inlined twice in this kernel instead of once per absorbed word (round 4: 37 copies, 640 KB of code streamed
  // through a 64 KB instruction cache in every round).
  for (int lv = 0; lv <= dl.total_layers; lv++) {
    const unsigned half = 1u << lv;
    const int li = dl.nlayers - 1 - lv;  // layers().iter().rev().skip(1)
    const bool init_lk = !dl.is_table && li == 0;   // initial lookup layer: all numerators are -1
    const bool nbase = dl.is_table && li == 0;      // table layer 0: base-field multiplicities
    const int tpi = init_lk ? 2 : 4;
    const int ntab = 1 + tpi * dl.ninst;
    u64* rw = mb + wbase;
    Ext r = ex_zero();
    // LDS: slot tau of S values for table tau >= 1; the eq table ping-pongs between slot 0 and slot ntab (its folds are read by every instance's quad)
    unsigned S = 2;
    while ((size_t)2 * S * (size_t)(ntab + 1) <= (size_t)dl.lds_ext) S *= 2;
    if (lv > 0) {
      Ext* const EQ0 = LT; Ext* const EQ1 = LT + (size_t)ntab * S;
      const bool eq_lds = half <= S;
      // eq(point, .) over the layer's lv variables — in LDS at the bit-reversed position, or in global memory in natural order — and the layer's tables in the tree
      for (unsigned q = (unsigned)tid; q < half; q += (unsigned)nt) {
        const unsigned i = eq_lds ? lt_brev(q, (unsigned)lv) : q;
        Ext v = ex_one();
        for (int t = 0; t < lv; t++) { const Ext rr = lf.pt[t]; v = ex_mul(v, ((i >> t) & 1) ? rr : ex_sub(ex_one(), rr)); }
        if (eq_lds) EQ0[q] = v; else dl.eq[q] = v;
      }
      if (tid == nt - 1) {
        lf.cur[0] = dl.eq; lf.cur_ext[0] = 1;
        for (int i = 0; i < dl.ninst; i++) {
          const Ext* dlo = dl.den[i][li];
          const Ext* dhi = dlo + half;
          const int tb = 1 + i * tpi;
          if (!init_lk) {
            const void* nlo = dl.num[i][li];
            const void* nhi = (const char*)nlo + (size_t)half * (nbase ? 8 : 16);
            lf.cur[tb] = nlo; lf.cur_ext[tb] = nbase ? 0 : 1;
            lf.cur[tb + 1] = dhi; lf.cur_ext[tb + 1] = 1;
            lf.cur[tb + 2] = nhi; lf.cur_ext[tb + 2] = nbase ? 0 : 1;
            lf.cur[tb + 3] = dlo; lf.cur_ext[tb + 3] = 1;
          } else {
            lf.cur[tb] = dhi; lf.cur_ext[tb] = 1;
            lf.cur[tb + 1] = dlo; lf.cur_ext[tb + 1] = 1;
          }
        }
      }
      __syncthreads();
      DBG_PHASE(1);
      unsigned m = half;       // length of the tables of round j
      bool src_lds = false;    // where the tables of round j - 1 sit (the source of round j's fold)
      int gsrc = 0, eqsel = 0;
      for (int j = 0; j < lv; j++) {
        const unsigned npairs = m / 2;
        const unsigned lgp = (unsigned)(lv - j - 1);
        const unsigned nitems = (unsigned)dl.ninst * npairs;
        const bool wide = W > 1 && nitems > 16;
        const bool fold = j > 0;
        const int dst = src_lds ? 1 : m <= S ? 1 : fold ? 2 : 0;
        Ext acc = ex_zero();
        if (wide) {
          if (fold) r = lf.chal;
          acc = lt_pass(lf, LT, S, EQ0, EQ1, fold, src_lds, gsrc, eq_lds, dst, eqsel, npairs, lgp, tpi, init_lk, r, (unsigned)(tid >> 2), (unsigned)(nt >> 2), lane);
          if (lane < 4) lf.part[wave * 4 + lane] = acc;
          __syncthreads();
          if (wave == 0) { acc = ex_zero(); if (lane < 4) for (int w = 0; w < W; w++) acc = ex_add(acc, lf.part[w * 4 + lane]); }
        } else if (wave == 0) {
          acc = lt_pass(lf, LT, S, EQ0, EQ1, fold, src_lds, gsrc, eq_lds, dst, eqsel, npairs, lgp, tpi, init_lk, r, (unsigned)(lane >> 2), 16u, lane);
        }
        DBG_PHASE(2);
        // where round j's tables are now
        if (fold && src_lds) eqsel ^= 1;
        else if (fold && dst == 1) eqsel = 1;          // global -> LDS fold: eq went to the other half of the double buffer
        if (dst == 1) src_lds = true;
        else if (dst == 2) gsrc = gsrc == 1 ? 2 : 1;
        if (wave == 0) {
          // the round message (lanes 0..3 hold its values at t = 0..3) and the round label are absorbed, the challenge is drawn
          if (lane < 4) {
            lf.io[2 * lane] = acc.c0; lf.io[2 * lane + 1] = acc.c1;
            const size_t w = ((size_t)j * 4 + lane) * 2;
            rw[w] = acc.c0; rw[w + 1] = acc.c1; fcs += (unsigned long long)(w + 1) * acc.c0 + (unsigned long long)(w + 2) * acc.c1;
          } else if (lane < 6) lf.io[4 + lane] = dl.lab_round[lane - 4];
          DP_WAVE_SYNC();
          u64 r0, r1;
          wc_io(wc, lf.io, 10, r0, r1, 2, lane);
          if (lane == 0) { const size_t w = ((size_t)lv * 4 + j) * 2; rw[w] = r0; rw[w + 1] = r1; fcs += (unsigned long long)(w + 1) * r0 + (unsigned long long)(w + 2) * r1; }
          r = ex(r0, r1);
          if (lane == 0) lf.pt[j] = r;  // (the eq table of this layer is built: pt may take the new point)
        }
        const bool wide_next = j + 1 < lv && W > 1 && (unsigned)dl.ninst * (npairs / 2) > 16;
        if (wide_next) { if (tid == 0) lf.chal = r; __syncthreads(); }
        DBG_PHASE(3);
        m = npairs;
      }
    }
    // ---- the end of layer lv (of the preamble when lv = 0) on the sponge wave
    if (wave == 0) {
      const bool pre = lv == 0;
      if (!pre) {  // every table is two values in LDS now; the last challenge folds them: the layer's evaluations
        const int i = lane >> 2, t = lane & 3;
        if (i < dl.ninst && t < tpi) { const Ext* p = LT + (size_t)(1 + i * tpi + t) * S; lf.fin[i * tpi + t] = ex_lerp(p[0], p[1], r); }
        DP_WAVE_SYNC();
      }
      const size_t wb = (size_t)lv * 10;  // behind lv * 4 message values and lv challenges
      // steps of the script: -1 the outputs (full mode's preamble), 0..2 the three challenges (batching, alpha, lambda: label in, challenge out), 3 the next
      // layer's claim and sumcheck header. The tail form enters with the challenges and the claim the host drew (lv = 0: step 3 only).
      const int first = pre ? (dl.full ? -1 : 3) : 0, last = lv == dl.total_layers ? 2 : 3;
      const u64* labels = pre ? dl.lab_ibatching : dl.lab_batching;
      Ext nb = lf.glue[0], na = lf.glue[1], nl = lf.glue[2];
      for (int c3 = first; c3 <= last; c3++) {
        const u64* words; int nin, nout;
        if (c3 < 0) { words = &lf.pre[1]; nin = 1 + 8 * dl.ninst; nout = 0; }
        else if (c3 < 3) { words = labels + 2 * c3; nin = 2; nout = 2; }
        else {
          if (!(pre && !dl.full)) {
            // the powers of the new alpha (every lane), then instance i's share of the next claim on lane i
            Ext acomb = ex_one(), mine = ex_one();
            for (int i = 0; i < dl.ninst; i++) { if (lane == i) mine = acomb; if (lane == 0) lf.ca[i] = acomb; acomb = ex_mul(acomb, na); }
            Ext share = ex_zero();
            if (lane < dl.ninst) {
              if (pre) {
                const Ext* e = lf.outs + 4 * lane;
                const Ext a = ex_add(ex_mul(nb, ex_sub(e[1], e[0])), e[0]);
                const Ext b = ex_add(ex_mul(nb, ex_sub(e[3], e[2])), e[2]);
                share = ex_mul(mine, ex_add(a, ex_mul(nl, b)));
              } else {
                const Ext* f = lf.fin + lane * tpi;
                const Ext a = ex_add(ex_mul(nb, ex_sub(f[2], f[0])), f[0]);
                const Ext b = ex_add(ex_mul(nb, ex_sub(f[1], f[3])), f[3]);
                share = ex_mul(mine, ex_add(a, ex_mul(nl, b)));
              }
            }
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) share = ex_add(share, ex(shfl_u64(share.c0, lane ^ d), shfl_u64(share.c1, lane ^ d)));
            if (lane == 0) { lf.glue[0] = nb; lf.glue[1] = na; lf.glue[2] = nl; lf.glue[3] = share; lf.pt[lv] = nb; }
            DP_WAVE_SYNC();
          }
          if (lane == 0) { const Ext c = lf.glue[3]; lf.io[0] = c.c0; lf.io[1] = c.c1; lf.io[2] = (u64)(lv + 1); lf.io[3] = 3; }
          DP_WAVE_SYNC();
          words = lf.io; nin = 4; nout = 0;
        }
        u64 o0 = 0, o1 = 0;
        wc_io(wc, words, nin, o0, o1, nout, lane);
        if (c3 == 0) nb = ex(o0, o1); else if (c3 == 1) na = ex(o0, o1); else if (c3 == 2) nl = ex(o0, o1);
      }
      if (!pre) {
        if (lane == 0) { rw[wb] = nb.c0; rw[wb + 1] = nb.c1; fcs += (unsigned long long)(wb + 1) * nb.c0 + (unsigned long long)(wb + 2) * nb.c1; }
        for (int e = lane; e < ntab - 1; e += 64) {
          const Ext v = lf.fin[e];
          const size_t w = wb + 2 + 2 * (size_t)e;
          rw[w] = v.c0; rw[w + 1] = v.c1;
          fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
        }
        if (last == 2 && lane == 0) lf.pt[lv] = nb;  // the last layer: the final point's last coordinate (no claim follows; final_round_claim, prover.rs:201-237, has no reader)
      }
    }
    if (lv > 0) wbase += ((size_t)lv * 5 + 1 + (size_t)(ntab - 1)) * 2;
    __syncthreads();
    DBG_PHASE(4);
  }
  if (dl.full) {
    // ---- full mode: the output claims — [multiplicities,] columns evaluated at the final point (sum_i eq(point, i) col[i])
    wg_build_eq(dl.eqn, lf.pt, dl.nlayers);
    const int tcol = dl.is_table ? 1 : 0;
    const int ncol = tcol + dl.ninst * dl.cpi;
    u64* rw = mb + wbase;
    for (int c0 = 0; c0 < ncol; c0 += 4) {  // four columns per pass over the rows
      Ext acc[4];
#pragma unroll
      for (int q = 0; q < 4; q++) acc[q] = ex_zero();
      const u64* col[4];
#pragma unroll
      for (int q = 0; q < 4; q++) { const int cidx = c0 + q < ncol ? c0 + q : c0; col[q] = cidx < tcol ? dl.mult : dl.col[(cidx - tcol) / dl.cpi][(cidx - tcol) % dl.cpi]; }
      for (size_t i = tid; i < dl.n; i += nt) {
        const Ext e = dl.eqn[i];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = ex_add(acc[q], ex_mul_base(e, col[q][i]));
      }
#pragma unroll
      for (int q = 0; q < 4; q++) { acc[q] = wave_reduce_ext(acc[q]); if (lane == 0) lf.part[wave * 4 + q] = acc[q]; }
      __syncthreads();
      if (wave == 0 && lane < 4 && c0 + lane < ncol) {
        Ext v = ex_zero();
        for (int w = 0; w < W; w++) v = ex_add(v, lf.part[w * 4 + lane]);
        const size_t w = 2 * (size_t)(c0 + lane);
        rw[w] = v.c0; rw[w + 1] = v.c1; fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
      }
      __syncthreads();
    }
    wbase += 2 * (size_t)ncol;
  }
  DBG_PHASE(5);
  if (wave == 0) {  // the sponge goes back to the host transcript; the tag closes the message
    u64* rw = mb + wbase;
    if (lane < 8) { rw[lane] = wc.st; fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; rw[8 + lane] = v; fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      rw[12] = a; rw[13] = b;
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    DP_WAVE_SYNC();
    for (size_t w = (size_t)lane; w < wbase + 14; w += 64) pub_store(result + w, mb[w]);  // the whole message in one burst
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
#ifdef DP_WG_TIMES
    if (tid == 0) dbg_wg_record(dbg_t_in);
#endif
#ifdef DP_WG_PHASES
    DBG_PHASE(6);
    if (tid == 0) { dbg_sponge_record(dbg_t_in, wc.dbg_sp, wc.dbg_np); const int big_ = ((size_t(1) << dl.nlayers) > 1024) ? 8 : 0; for (int k = 0; k < 7; k++) atomicAdd(&g_phase_ticks[big_ + k], dbg_ph[k]); atomicAdd(&g_phase_ticks[big_ + 7], 1ull); }  // (members with columns of more than 1024 rows apart)
#endif
  }
}
#undef DBG_PHASE
#endif

// ------------------------------------------------------------------------------------------------ batch-opening sumcheck tail
// Dev::classic_tail (dev.h, classic_tail.h): the remaining rounds of the batch-opening sumcheck of pcs_batch_open — per round
// fold every (f, eq) pair, the per-pair sums of Dev::classic_round, the 3-coefficient message of classic_round_message
// (pcs.h), absorb, squeeze "sumcheck round" — in ONE launch of one workgroup once every table is short. A pair belongs to
// one wave per phase; the phases of a round are separated by barriers. Default in throughput mode (DP_DEVICE_CLASSIC=0 turns
// it off); checked on the SIMT emulator of tests/ and on MI355X (tests/test_gpu_fused.py).
// LDS frame of k_classic_tail (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_classic_tail {
  ClassicTailDesc dl;
  Ext raw[2 * CT_MAXP];
  const void* curf[CT_MAXP];
  const Ext* cure[CT_MAXP];
  unsigned clen[CT_MAXP];
  unsigned cext[CT_MAXP];
  unsigned toA[CT_MAXP];
  unsigned long long chal[3];
};
KBODY k_classic_tail(const ClassicTailDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_classic_tail, lf); auto& dl = lf.dl; auto& raw = lf.raw; auto& curf = lf.curf; auto& cure = lf.cure; auto& clen = lf.clen; auto& cext = lf.cext; auto& toA = lf.toA; auto& chal = lf.chal;
  DP_LDS_DYN(lds_msg, u64);
  u64* const host_result = result; result = (u64*)lds_msg;  // the message is assembled in LDS and leaves in one burst at the end (MSG_PUT / msg_flush)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < (int)(sizeof(ClassicTailDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  const int np = dl.np;
  for (int i = tid; i < np; i += nt) { curf[i] = dl.f[i]; cure[i] = dl.eq[i]; clen[i] = dl.len[i]; cext[i] = dl.f_ext[i]; toA[i] = 1; }
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  const int R = (int)(dl.num_vars - dl.round);
  Ext r = dl.r, sum = dl.sum;
  bool have_r = dl.has_r != 0;
  __syncthreads();
  for (int q = 0; q < R; q++) {
    if (have_r) {
      // fold f and eq of every pair that is longer than one value
      for (int i = wave; i < np; i += W) {
        const unsigned n = clen[i];
        if (n <= 1) continue;
        const unsigned half = n / 2;
        Ext* df = toA[i] ? dl.fA[i] : dl.fB[i];
        Ext* de = toA[i] ? dl.eA[i] : dl.eB[i];
        const Ext* e = cure[i];
        if (cext[i]) { const Ext* f = (const Ext*)curf[i]; for (unsigned j = lane; j < half; j += 64) df[j] = ex_lerp(f[2 * j], f[2 * j + 1], r); }
        else { const u64* f = (const u64*)curf[i]; for (unsigned j = lane; j < half; j += 64) df[j] = ex_lerp_base(f[2 * j], f[2 * j + 1], r); }
        for (unsigned j = lane; j < half; j += 64) de[j] = ex_lerp(e[2 * j], e[2 * j + 1], r);
      }
      __syncthreads();
      for (int i = tid; i < np; i += nt)
        if (clen[i] > 1) { curf[i] = toA[i] ? dl.fA[i] : dl.fB[i]; cure[i] = toA[i] ? dl.eA[i] : dl.eB[i]; cext[i] = 1; clen[i] /= 2; toA[i] ^= 1; }
      __syncthreads();
    }
    // per pair: c0 = sum_j f[2j] eq[2j], c2 = sum_j (f[2j+1] - f[2j]) (eq[2j+1] - eq[2j]); a single value gives (f eq, 0)
    for (int i = wave; i < np; i += W) {
      const unsigned n = clen[i];
      const Ext* e = cure[i];
      Ext c0 = ex_zero(), c2 = ex_zero();
      if (n == 1) { if (lane == 0) c0 = ex_mul(ld_elem(curf[i], cext[i] != 0, 0), e[0]); }
      else
        for (unsigned j = lane; j < n / 2; j += 64) {
          Ext l0 = e[2 * j], l1 = e[2 * j + 1], r0 = ld_elem(curf[i], cext[i] != 0, 2 * j), r1 = ld_elem(curf[i], cext[i] != 0, 2 * j + 1);
          c0 = ex_add(c0, ex_mul(l0, r0));
          c2 = ex_add(c2, ex_mul(ex_sub(l1, l0), ex_sub(r1, r0)));
        }
      c0 = wave_reduce_ext(c0); c2 = wave_reduce_ext(c2);
      if (lane == 0) { raw[2 * i] = c0; raw[2 * i + 1] = c2; }
    }
    __syncthreads();
    if (wave == 0) {
      // the message [h0, h1, h2] (classic_round_message of pcs.h), the transcript, the next claim
      const size_t size = size_t(1) << (dl.num_vars - (dl.round + (unsigned)q) - 1);
      Ext h0 = ex_zero(), h2 = ex_zero();
      for (int i = lane; i < np; i += 64) {
        const size_t poly_len = clen[i];
        Ext c0 = raw[2 * i], c2 = raw[2 * i + 1];
        size_t multiple;
        if (poly_len == 1) multiple = size;
        else if (size < poly_len || size == 1) multiple = 1;
        else multiple = size / (poly_len >> 1);
        if (multiple != 1) { Ext m = ex_from_u64((u64)multiple); c0 = ex_mul(c0, m); c2 = ex_mul(c2, m); }
        h0 = ex_add(h0, ex_mul(dl.eq_xt[i], c0));
        h2 = ex_add(h2, ex_mul(dl.eq_xt[i], c2));
      }
      h0 = wave_reduce_ext(h0); h2 = wave_reduce_ext(h2);
      h0 = ex(shfl_u64(h0.c0, 0), shfl_u64(h0.c1, 0)); h2 = ex(shfl_u64(h2.c0, 0), shfl_u64(h2.c1, 0));
      const Ext h1 = ex_sub(ex_sub(sum, ex_dbl(h0)), h2);
      wc_observe(wc, h0.c0, lane); wc_observe(wc, h0.c1, lane);
      wc_observe(wc, h1.c0, lane); wc_observe(wc, h1.c1, lane);
      wc_observe(wc, h2.c0, lane); wc_observe(wc, h2.c1, lane);
      wc_observe(wc, dl.lab[0], lane); wc_observe(wc, dl.lab[1], lane);
      const u64 r0 = wc_sample(wc, lane), r1 = wc_sample(wc, lane);
      const Ext ch = ex(r0, r1);
      if (lane == 0) {
        const Ext m[3] = {h0, h1, h2};
        for (int j = 0; j < 3; j++) {
          size_t w = ((size_t)q * 3 + j) * 2;
          MSG_PUT(result + w, m[j].c0); MSG_PUT(result + w + 1, m[j].c1);
          fcs += (unsigned long long)(w + 1) * m[j].c0 + (unsigned long long)(w + 2) * m[j].c1;
        }
        size_t w = ((size_t)R * 3 + q) * 2;
        MSG_PUT(result + w, r0); MSG_PUT(result + w + 1, r1);
        fcs += (unsigned long long)(w + 1) * r0 + (unsigned long long)(w + 2) * r1;
        chal[1] = r0; chal[2] = r1;
      }
      sum = ex_add(h0, ex_mul(ch, ex_add(h1, ex_mul(ch, h2))));
    }
    __syncthreads();
    r = ex(chal[1], chal[2]);
    have_r = true;
  }
  if (wave == 0) {  // the sponge goes back to the host transcript; the tag closes the message
    u64* rw = result + (size_t)R * 8;
    if (lane < 8) { MSG_PUT(rw + lane, wc.st); fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rw + 8 + lane, v); fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      MSG_PUT(rw + 12, a); MSG_PUT(rw + 13, b);
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    msg_flush(host_result, result, (size_t)R * 8 + 14, lane);
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
  }
}

// ------------------------------------------------------------------------------------------------ dense layer in one launch
// Dev::dense_tail (dev.h, dense_tail.h): the bias at the output point, W(point, .) — the one-pass fix_high over the base-field
// weights — and the degree-2 sumcheck of sum_c W(point, c) in(c) with its transcript, in ONE launch of one workgroup: a
// 1024 x 1024 layer is 8 MB of weights through one CU (~0.15 ms), cheaper than the five dispatches it replaces when the
// GPU serves hundreds of proofs. Default in throughput mode (DP_DEVICE_DENSE=0 turns it off); checked on the SIMT
// emulator of tests/ and on MI355X (tests/test_gpu_fused.py).
// LDS frame of k_dense_tail (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_dense_tail {
  DenseTailDesc dl;
  Ext part[64 * SC_SLOTS];
  unsigned long long chal[3];
  int tk[1];
  ScFsArgs fsl;
};
KBODY k_dense_tail(const DenseTailDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_dense_tail, lf); auto& dl = lf.dl; auto& part = lf.part; auto& chal = lf.chal; auto& tk = lf.tk; auto& fsl = lf.fsl;
  DP_LDS_DYN(lds_msg, u64);
  u64* const host_result = result; result = (u64*)lds_msg;  // the message is assembled in LDS and leaves in one burst at the end (MSG_PUT / msg_flush)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < (int)(sizeof(DenseTailDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  if (tid == 0) { fsl.md = 2; fsl.rounds = (int)dl.lgC; fsl.label[0] = dl.lab_round[0]; fsl.label[1] = dl.lab_round[1]; fsl.nlabel = 2; fsl.pad = 0; fsl.coeff[0] = ex_one(); tk[0] = 2; }
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  const size_t R = dl.R, C = dl.C;
  wg_build_eq(dl.eqr, dl.pt, (int)dl.lgR);  // eq(point, .) over the rows (ends with a barrier)
  // bias at the point
  {
    Ext acc = ex_zero();
    for (size_t i = tid; i < R; i += nt) acc = ex_add(acc, ex_mul_base(dl.eqr[i], dl.bias[i]));
    acc = wave_reduce_ext(acc);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (wave == 0) {
      Ext v = lane < W ? part[lane] : ex_zero();
      v = wave_reduce_ext(v);
      if (lane == 0) { MSG_PUT(result, v.c0); MSG_PUT(result + 1, v.c1); fcs += (unsigned long long)1 * v.c0 + (unsigned long long)2 * v.c1; }
    }
    __syncthreads();
  }
  // W(point, c) = sum_r eq(point, r) W[r][c]: consecutive threads read consecutive columns of a row
  for (size_t c = tid; c < C; c += nt) {
    Ext acc = ex_zero();
    for (size_t r = 0; r < R; r++) acc = ex_add(acc, ex_mul_base(dl.eqr[r], dl.W[r * C + c]));
    dl.mat[c] = acc;
  }
  __syncthreads();
  // the sumcheck of mat * in: header, then log2(C) rounds
  if (wave == 0) { wc_observe(wc, (u64)dl.lgC, lane); wc_observe(wc, (u64)2, lane); }
  const Ext* cur[2] = {dl.mat, dl.in};
  u64* rw = result + 2;
  size_t n = C;
  bool useA = true;
  for (int round = 0; round < (int)dl.lgC; round++) {
    const size_t npairs = n / 2;
    {
      GlobalPairs L;
      L.p[0] = cur[0]; L.e[0] = true; L.p[1] = cur[1]; L.e[1] = true; L.p[2] = cur[0]; L.e[2] = true;
      Ext acc[SC_SLOTS];
      sc_accumulate<false>(2, L, (size_t)tid, (size_t)nt, npairs, acc);  // every wave takes a share of the one term
#pragma unroll
      for (int t = 0; t < SC_SLOTS; t++) if (t <= 2) acc[t] = wave_reduce_ext(acc[t]);
      if (lane == 0) { Ext* o = part + (size_t)wave * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
    }
    __syncthreads();
    if (wave == 0) {
      Ext rr = sc_fs_round(wc, fsl, part, tk, 1, W, rw, round, fcs, lane);  // wpt = W: the term's sums are spread over all waves
      if (lane == 0) { chal[1] = rr.c0; chal[2] = rr.c1; }
    }
    __syncthreads();
    const Ext r = ex(chal[1], chal[2]);
    Ext* const* dst = useA ? dl.bufA : dl.bufB;
    for (int t = 0; t < 2; t++) { const Ext* q = cur[t]; Ext* o = dst[t]; for (size_t i = tid; i < npairs; i += nt) o[i] = ex_lerp(q[2 * i], q[2 * i + 1], r); }
    __syncthreads();
    cur[0] = dst[0]; cur[1] = dst[1];
    n = npairs; useA = !useA;
  }
  if (wave == 0) {
    const size_t wf = (size_t)dl.lgC * 8;  // behind 3 evaluations and one challenge per round
    if (lane < 2) { Ext v = cur[lane][0]; size_t w = wf + 2 * (size_t)lane; MSG_PUT(rw + w, v.c0); MSG_PUT(rw + w + 1, v.c1); fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1; }
    u64* rs = result + (1 + (size_t)dl.lgC * 4 + 2) * 2;
    if (lane < 8) { MSG_PUT(rs + lane, wc.st); fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rs + 8 + lane, v); fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      MSG_PUT(rs + 12, a); MSG_PUT(rs + 13, b);
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    msg_flush(host_result, result, (1 + (size_t)dl.lgC * 4 + 2) * 2 + 14, lane);
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
  }
}

// ------------------------------------------------------------------------------------------------ eq tables + sumcheck in one launch
// Dev::eqsum_tail (dev.h, eqsum_tail.h): the eq tables of an accumulation sumcheck (Requant: three plain tables; same_poly:
// one table accumulated from scaled eq's) and the whole sumcheck over them with its transcript, in ONE launch of one
// workgroup. Default in throughput mode (DP_DEVICE_EQSUM=0 turns it off); checked on the SIMT emulator and on MI355X.
// LDS frame of k_eqsum_tail (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_eqsum_tail {
  EqSumDesc dl;
  Ext part[64 * SC_SLOTS];
  unsigned long long chal[3];
  const void* cur[ES_MAXT];
  int cur_ext[ES_MAXT];
  ScFsArgs fsl;
};
KBODY k_eqsum_tail(const EqSumDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_eqsum_tail, lf); auto& dl = lf.dl; auto& part = lf.part; auto& chal = lf.chal; auto& cur = lf.cur; auto& cur_ext = lf.cur_ext; auto& fsl = lf.fsl;
  DP_LDS_DYN(lds_msg, u64);
  u64* const host_result = result; result = (u64*)lds_msg;  // the message is assembled in LDS and leaves in one burst at the end (MSG_PUT / msg_flush)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < (int)(sizeof(EqSumDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  const int ntab = dl.ntabs, nterm = dl.nterms;
  if (tid == 0) { fsl.md = (int)dl.md; fsl.rounds = (int)dl.nv; fsl.label[0] = dl.lab_round[0]; fsl.label[1] = dl.lab_round[1]; fsl.nlabel = 2; fsl.pad = 0; }
  for (int i = tid; i < nterm; i += nt) fsl.coeff[i] = dl.coeff[i];
  for (int i = tid; i < ntab; i += nt) { cur[i] = dl.tab[i]; cur_ext[i] = dl.tab_ext[i]; }
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  const size_t n0 = size_t(1) << dl.nv;
  // the eq tables, in order: out[idx] (+)= scale * prod_t (idx_t ? pt[t] : 1 - pt[t])
  for (int j = 0; j < dl.njobs; j++) {
    Ext* out = dl.job_out[j];
    const Ext sc = dl.job_scale[j];
    for (size_t i = tid; i < n0; i += nt) {
      Ext v = sc;
      for (unsigned t = 0; t < dl.nv; t++) { Ext r = dl.job_pt[j][t]; v = ex_mul(v, ((i >> t) & 1) ? r : ex_sub(ex_one(), r)); }
      out[i] = dl.job_acc[j] ? ex_add(out[i], v) : v;
    }
    __syncthreads();
  }
  if (wave == 0) { wc_observe(wc, (u64)dl.nv, lane); wc_observe(wc, (u64)dl.md, lane); }  // header of the sumcheck
  const int wpt = nterm >= W ? 1 : W / nterm;
  size_t n = n0;
  bool useA = true;
  for (int round = 0; round < (int)dl.nv; round++) {
    const size_t npairs = n / 2;
    for (int term = wave / wpt; term < nterm; term += (wpt == 1 ? W : nterm + W)) {
      const int sub = wave % wpt;
      const int k = dl.tk[term];
      GlobalPairs L;
#pragma unroll
      for (int j = 0; j < 3; j++) { int ti = dl.tt[term][j < k ? j : 0]; L.p[j] = cur[ti]; L.e[j] = cur_ext[ti] != 0; }
      Ext acc[SC_SLOTS];
      sc_accumulate<false>(k, L, (size_t)sub * 64 + lane, (size_t)wpt * 64, npairs, acc);
#pragma unroll
      for (int t = 0; t < SC_SLOTS; t++) if (t <= k) acc[t] = wave_reduce_ext(acc[t]);
      if (lane == 0) { Ext* o = part + (size_t)(term * wpt + sub) * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
      if (wpt > 1) break;  // with several waves per term every wave owns exactly one (term, sub)
    }
    __syncthreads();
    if (wave == 0) {
      Ext rr = sc_fs_round(wc, fsl, part, dl.tk, nterm, wpt, result, round, fcs, lane);
      if (lane == 0) { chal[1] = rr.c0; chal[2] = rr.c1; }
    }
    __syncthreads();
    const Ext r = ex(chal[1], chal[2]);
    Ext* const* dst = useA ? dl.bufA : dl.bufB;
    for (int t = 0; t < ntab; t++) {
      Ext* o = dst[t];
      if (cur_ext[t]) { const Ext* q = (const Ext*)cur[t]; for (size_t i = tid; i < npairs; i += nt) o[i] = ex_lerp(q[2 * i], q[2 * i + 1], r); }
      else { const u64* q = (const u64*)cur[t]; for (size_t i = tid; i < npairs; i += nt) o[i] = ex_lerp_base(q[2 * i], q[2 * i + 1], r); }
    }
    __syncthreads();
    if (tid < ntab) { cur[tid] = dst[tid]; cur_ext[tid] = 1; }
    __syncthreads();
    n = npairs; useA = !useA;
  }
  if (wave == 0) {
    const size_t wf = (size_t)dl.nv * (dl.md + 2) * 2;
    for (int e = lane; e < ntab; e += 64) {
      Ext v = ((const Ext*)cur[e])[0];
      size_t w = wf + 2 * (size_t)e;
      MSG_PUT(result + w, v.c0); MSG_PUT(result + w + 1, v.c1);
      fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
    }
    u64* rs = result + wf + 2 * (size_t)ntab;
    if (lane < 8) { MSG_PUT(rs + lane, wc.st); fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rs + 8 + lane, v); fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      MSG_PUT(rs + 12, a); MSG_PUT(rs + 13, b);
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    msg_flush(host_result, result, wf + 2 * (size_t)ntab + 14, lane);
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
  }
}

// Dev::deleg_tail (dev.h, deleg_tail.h): the delegation sumchecks of one batch FFT / iFFT of the convolution protocol
// (delegate_matrix_evaluation, zkml/src/iop/prover.rs:164-211) — a chain of |f_middle| degree-3 sumchecks over 2^fm .. 2 entries, each
// on (beta(point so far), phi(previous point's last coordinate), f_middle[l]) and each starting where the one before ended — in ONE
// launch of one workgroup: phi and beta are built here, the rounds are k_eqsum_tail's, the transcript stays on the device throughout.
// A CNN-264k proof has six such chains of ~10 sumchecks; each sumcheck used to be its own launch and its own device wait.
struct Lds_k_deleg_tail {
  DelegDesc dl;
  Ext part[64 * SC_SLOTS];
  unsigned long long chal[3];
  const void* cur[3];
  int tk[4];
  Ext r2[DG_MAXV + 1];
  ScFsArgs fsl;
};
KBODY k_deleg_tail(const DelegDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_deleg_tail, lf); auto& dl = lf.dl; auto& part = lf.part; auto& chal = lf.chal; auto& cur = lf.cur; auto& tk = lf.tk; auto& r2 = lf.r2; auto& fsl = lf.fsl;
  DP_LDS_DYN(lds_msg, u64);
  u64* const host_result = result; result = (u64*)lds_msg;  // the message is assembled in LDS and leaves in one burst at the end (MSG_PUT / msg_flush)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < (int)(sizeof(DelegDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  const int fm = dl.fm;
  if (tid == 0) { fsl.md = 3; fsl.rounds = fm; fsl.label[0] = dl.lab_round[0]; fsl.label[1] = dl.lab_round[1]; fsl.nlabel = 2; fsl.pad = 0; fsl.coeff[0] = ex_one(); tk[0] = 3; }
  for (int i = tid; i <= fm; i += nt) r2[i] = dl.r2[i];
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  u64* rw = result;
  __syncthreads();
  for (int l = fm - 1; l >= 0; l--) {
    const unsigned nv = (unsigned)l + 1;
    const size_t n0 = size_t(1) << nv;
    // phi (prover.rs:178-195) and beta = eq(., the first nv coordinates of the point)
    {
      const Ext r1e = dl.r1[(fm - 1) - l], one_m = ex_sub(ex_one(), r1e), last = r2[nv];
      const unsigned shift = (unsigned)((fm - 1) - l);
      const bool first = !dl.is_fft && l == fm - 1;
      const Ext f = first ? ex_sub(ex_one(), last) : ex_mul(ex_sub(ex_one(), ex_dbl(last)), r1e);
      for (size_t i = tid; i < n0; i += nt) {
        const u64 w = dl.omegas[i << shift];
        dl.phi[i] = first ? ex_mul(f, ex_add(one_m, ex_mul_base(r1e, w))) : ex_add(one_m, ex_mul_base(f, w));
        Ext v = ex_one();
        for (unsigned t = 0; t < nv; t++) { Ext r = r2[t]; v = ex_mul(v, ((i >> t) & 1) ? r : ex_sub(ex_one(), r)); }
        dl.beta[i] = v;
      }
    }
    if (tid == 0) { fsl.rounds = (int)nv; cur[0] = dl.beta; cur[1] = dl.phi; cur[2] = dl.fmid + (n0 - 2); }
    __syncthreads();
    if (wave == 0) { wc_observe(wc, (u64)nv, lane); wc_observe(wc, (u64)3, lane); }  // header of the sumcheck
    size_t n = n0;
    bool useA = true;
    for (int round = 0; round < (int)nv; round++) {
      const size_t npairs = n / 2;
      {  // one product of three tables: every wave takes a slice of the pairs
        GlobalPairs L;
#pragma unroll
        for (int j = 0; j < 3; j++) { L.p[j] = cur[j]; L.e[j] = true; }
        Ext acc[SC_SLOTS];
        sc_accumulate<false>(3, L, (size_t)wave * 64 + lane, (size_t)W * 64, npairs, acc);
#pragma unroll
        for (int t = 0; t < SC_SLOTS; t++) if (t <= 3) acc[t] = wave_reduce_ext(acc[t]);
        if (lane == 0) { Ext* o = part + (size_t)wave * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
      }
      __syncthreads();
      if (wave == 0) {
        Ext rr = sc_fs_round(wc, fsl, part, tk, 1, W, rw, round, fcs, lane);
        if (lane == 0) { chal[1] = rr.c0; chal[2] = rr.c1; }
      }
      __syncthreads();
      const Ext r = ex(chal[1], chal[2]);
      if (tid == 0) r2[round] = r;  // the next sumcheck's point (its coordinates 0 .. nv - 1; this one read its own before the rounds)
      Ext* const* dst = useA ? dl.bufA : dl.bufB;
      for (int t = 0; t < 3; t++) {
        Ext* o = dst[t];
        const Ext* q = (const Ext*)cur[t];
        for (size_t i = tid; i < npairs; i += nt) o[i] = ex_lerp(q[2 * i], q[2 * i + 1], r);
      }
      __syncthreads();
      if (tid < 3) cur[tid] = dst[tid];
      __syncthreads();
      n = npairs; useA = !useA;
    }
    if (wave == 0) {
      const size_t wf = (size_t)nv * 5 * 2;
      for (int e = lane; e < 3; e += 64) {
        Ext v = ((const Ext*)cur[e])[0];
        size_t w = wf + 2 * (size_t)e;
        MSG_PUT(rw + w, v.c0); MSG_PUT(rw + w + 1, v.c1);
        fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
      }
    }
    rw += ((size_t)nv * 5 + 3) * 2;
    __syncthreads();
  }
  if (wave == 0) {
    if (lane < 8) { MSG_PUT(rw + lane, wc.st); fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rw + 8 + lane, v); fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      MSG_PUT(rw + 12, a); MSG_PUT(rw + 13, b);
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    msg_flush(host_result, result, (size_t)(rw - result) + 14, lane);
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
  }
}

// ------------------------------------------------------------------------------------------------ Basefold commit-phase tail
// Dev::commit_tail (dev.h, commit_tail.h): the last rounds of the Basefold commit phase (commit_rounds of pcs.h) — per round the
// pending sumcheck message absorbed, the folding challenge, the merge of the committed codewords of the oracle's size, the FRI
// fold (k_fri_fold's formula), the fold of the sumcheck pairs, the next message (k_bf_msg's sums), the Merkle tree of the folded
// oracle (k_merkle_tail's layer loop) and its root absorbed; in the last round the final message absorbed — in ONE launch of
// one workgroup once the oracle is short. Default in throughput mode (DP_DEVICE_COMMIT=0 turns it off); checked on the SIMT
// emulator of tests/ and on MI355X (tests/test_gpu_fused.py).
// LDS frame of k_commit_tail (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_commit_tail {
  CommitTailDesc dl;
  Ext part[64 * 3];
  unsigned long long chal[3];
  Ext s_last[3];
};
KBODY k_commit_tail(const CommitTailDesc* dp, u64* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_commit_tail, lf); auto& dl = lf.dl; auto& part = lf.part; auto& chal = lf.chal; auto& s_last = lf.s_last;
  DP_LDS_DYN(lds_msg, u64);
  u64* const host_result = result; result = (u64*)lds_msg;  // the message is assembled in LDS and leaves in one burst at the end (MSG_PUT / msg_flush)
  const int tid = threadIdx.x, nt = blockDim.x;
  const int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < (int)(sizeof(CommitTailDesc) / 8); i += nt) ((u64*)&dl)[i] = ((const u64*)dp)[i];
  __syncthreads();
  if (tid < 3) s_last[tid] = dl.last[tid];
  WaveChallenger wc; wc.k = p2l_load(lane);
  wc.st = dl.state[lane & 7]; wc.ib = dl.in_buf[lane & 3]; wc.in_len = dl.in_len; wc.out_len = dl.out_len;
  wc_host_init(wc, dl.sp_req, dl.sp_rep, dl.sp_seq);
  unsigned long long fcs = 0;
  const Ext* prev = dl.folded;   // the folded oracle of the previous round
  const Ext* eq = dl.eq;
  const Ext* f = dl.f;
  size_t m = dl.m;
  bool useA = true;
  __syncthreads();
  for (int j = 0; j < dl.rounds; j++) {
    const size_t n = (size_t)dl.n >> j, half = n / 2;
    const bool final_round = j == dl.rounds - 1;
    // transcript: the pending message, then the folding challenge
    if (wave == 0) {
      for (int q = 0; q < 3; q++) { Ext v = s_last[q]; wc_observe(wc, v.c0, lane); wc_observe(wc, v.c1, lane); }
      wc_observe(wc, dl.lab[0], lane); wc_observe(wc, dl.lab[1], lane);
      const u64 r0 = wc_sample(wc, lane), r1 = wc_sample(wc, lane);
      if (lane == 0) { chal[1] = r0; chal[2] = r1; }
    }
    __syncthreads();
    const Ext c = ex(chal[1], chal[2]);
    // the committed codewords as long as the oracle join it (into a fresh buffer: `prev` is the leaf array of a tree)
    const Ext* src = prev;
    if (dl.nmerge[j] > 0) {
      Ext* run = dl.run[j];
      for (size_t i = tid; i < n; i += nt) {
        Ext acc = prev[i];
        for (int k = 0; k < dl.nmerge[j]; k++) {
          const Ext co = dl.mcoeff[j][k];
          acc = ex_add(acc, dl.mext[j][k] ? ex_mul(((const Ext*)dl.mcw[j][k])[i], co) : ex_mul_base(co, ((const u64*)dl.mcw[j][k])[i]));
        }
        run[i] = acc;
      }
      src = run;
      __syncthreads();
    }
    // FRI fold (K9): out[i] = y0 + (c - x0)(y1 - y0) w, x0 = gamma * w_{2^(level+1)}^{bitrev(i)}, w = -1/(2 x0); the last round's
    // folded oracle is never used
    if (!final_round) {
      const unsigned level = dl.level[j], L = dl.L;
      Ext* out = dl.leaves[j];
      for (size_t i = tid; i < half; i += nt) {
        size_t b = level ? (size_t)(__brevll((unsigned long long)i) >> (64 - level)) : 0;
        u64 root = dl.tw[b << (L - level)];
        u64 x0 = gl_mul(root, dl.gamma[j]);
        u64 rinv = b == 0 ? 1 : gl_neg(dl.tw[((size_t(1) << level) - b) << (L - level)]);
        u64 w = gl_mul(dl.ninv[j], rinv);
        Ext y0 = src[2 * i], y1 = src[2 * i + 1];
        Ext t = ex_mul(ex(gl_sub(c.c0, x0), c.c1), ex_sub(y1, y0));
        out[i] = ex_add(y0, ex_mul_base(t, w));
      }
    }
    // the sumcheck pairs fold with the same challenge
    Ext* eqd = useA ? dl.eqA : dl.eqB;
    Ext* fd = useA ? dl.fA : dl.fB;
    for (size_t i = tid; i < m / 2; i += nt) { eqd[i] = ex_lerp(eq[2 * i], eq[2 * i + 1], c); fd[i] = ex_lerp(f[2 * i], f[2 * i + 1], c); }
    __syncthreads();
    eq = eqd; f = fd; m /= 2; useA = !useA;
    if (!final_round) {
      // the next message (K10 on evaluation-form pairs): [sum a ea, sum (b ea + a eb), sum b eb]; a single value: three times it
      Ext c0 = ex_zero(), c1 = ex_zero(), c2 = ex_zero();
      for (size_t q = tid; q < m / 2; q += nt) {
        Ext a = f[2 * q], b = ex_sub(f[2 * q + 1], a), ea = eq[2 * q], eb = ex_sub(eq[2 * q + 1], ea);
        c0 = ex_add(c0, ex_mul(a, ea));
        c1 = ex_add(c1, ex_add(ex_mul(b, ea), ex_mul(a, eb)));
        c2 = ex_add(c2, ex_mul(b, eb));
      }
      c0 = wave_reduce_ext(c0); c1 = wave_reduce_ext(c1); c2 = wave_reduce_ext(c2);
      if (lane == 0) { part[wave * 3] = c0; part[wave * 3 + 1] = c1; part[wave * 3 + 2] = c2; }
      // layer 0 of the tree: leaf pairs packed, no hashing
      u64* nd = dl.nodes[j];
      const Ext* lv = dl.leaves[j];
      for (size_t i = tid; i < half / 2; i += nt) { Ext a = lv[2 * i], b = lv[2 * i + 1]; u64* o = nd + 4 * i; o[0] = a.c0; o[1] = a.c1; o[2] = b.c0; o[3] = b.c1; }
      __syncthreads();
      if (wave == 0) {
        Ext v0 = lane < W ? part[lane * 3] : ex_zero(), v1 = lane < W ? part[lane * 3 + 1] : ex_zero(), v2 = lane < W ? part[lane * 3 + 2] : ex_zero();
        v0 = wave_reduce_ext(v0); v1 = wave_reduce_ext(v1); v2 = wave_reduce_ext(v2);
        if (lane == 0) {
          if (m == 1) { s_last[0] = f[0]; s_last[1] = f[0]; s_last[2] = f[0]; }
          else { s_last[0] = v0; s_last[1] = v1; s_last[2] = v2; }
        }
      }
      // upper layers: Poseidon2 compress, one node per lane while the layer is wide, 8 lanes per node when it is narrow
      size_t off = 0, cnt = half / 2;
      while (cnt > 1) {
        const size_t next = cnt / 2;
        const u64* in = nd + 4 * off;
        u64* out = nd + 4 * (off + cnt);
        if (next > (size_t)nt) {
          for (size_t i = tid; i < next; i += nt) {
            u64 o[4];
            p2f::compress(in + 8 * i, in + 8 * i + 4, o, c_rc);
            out[4 * i] = o[0]; out[4 * i + 1] = o[1]; out[4 * i + 2] = o[2]; out[4 * i + 3] = o[3];
          }
        } else {
          // every lane takes part in the permutation (no divergence around the cross-lane moves); idle groups redo the last node
          const size_t groups = (size_t)nt >> 3;
          for (size_t g0 = 0; g0 < next; g0 += groups) {
            const size_t g = g0 + ((size_t)tid >> 3);
            const size_t gg = g < next ? g : next - 1;
            const int i8 = lane & 7;
            u64 sv = i8 < 4 ? in[8 * gg + i8] : 0;
            sv = p2l_permute(sv, lane, wc.k);
            if (i8 < 4) sv = in[8 * gg + 4 + i8];
            sv = p2l_permute(sv, lane, wc.k);
            if (g < next && i8 < 4) out[4 * g + (3 - i8)] = sv;
          }
        }
        __syncthreads();
        off += cnt; cnt = next;
      }
      // the message and the root: published, and the root absorbed (the message is absorbed at the top of the next round)
      if (wave == 0) {
        const u64* root = nd + 4 * (half - 2);
        for (int q = 0; q < 4; q++) wc_observe(wc, root[q], lane);
        if (lane == 0) {
          u64* rw = result + (size_t)j * 10;
          for (int q = 0; q < 3; q++) {
            Ext v = s_last[q];
            size_t w = (size_t)j * 10 + 2 * q;
            MSG_PUT(rw + 2 * q, v.c0); MSG_PUT(rw + 2 * q + 1, v.c1);
            fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
          }
          for (int q = 0; q < 4; q++) { size_t w = (size_t)j * 10 + 6 + q; MSG_PUT(rw + 6 + q, root[q]); fcs += (unsigned long long)(w + 1) * root[q]; }
        }
      }
      __syncthreads();
      prev = dl.leaves[j];
    } else {
      // the final message: the folded sum_evals in bit-reversed index order, absorbed in its natural order
      if (wave == 0) {
        unsigned lg = 0; while ((size_t(1) << lg) < m) lg++;
        u64* rw = result + (size_t)(dl.rounds - 1) * 10;
        for (size_t r = 0; r < m; r++) {
          size_t src_i = lg ? (size_t)(__brevll((unsigned long long)r) >> (64 - lg)) : 0;
          Ext v = f[src_i];
          wc_observe(wc, v.c0, lane); wc_observe(wc, v.c1, lane);
          if (lane == 0) {
            size_t w = (size_t)(dl.rounds - 1) * 10 + 2 * r;
            MSG_PUT(rw + 2 * r, v.c0); MSG_PUT(rw + 2 * r + 1, v.c1);
            fcs += (unsigned long long)(w + 1) * v.c0 + (unsigned long long)(w + 2) * v.c1;
          }
        }
      }
    }
  }
  if (wave == 0) {  // the sponge goes back to the host transcript; the tag closes the message
    u64* rs = result + (size_t)(dl.rounds - 1) * 10 + 2 * m;
    if (lane < 8) { MSG_PUT(rs + lane, wc.st); fcs += (unsigned long long)(lane + 1) * wc.st; }
    if (lane < 4) { u64 v = lane < wc.in_len ? wc.ib : 0; MSG_PUT(rs + 8 + lane, v); fcs += (unsigned long long)(8 + lane + 1) * v; }
    if (lane == 0) {
      u64 a = (u64)wc.in_len, b = (u64)wc.out_len;
      MSG_PUT(rs + 12, a); MSG_PUT(rs + 13, b);
      fcs += (unsigned long long)13 * a + (unsigned long long)14 * b;
    }
    fcs = pub_wave_sum(fcs);
    wc_finish(wc, lane);  // (host sponge: the transcript is complete before this message is)
    msg_flush(host_result, result, (size_t)(dl.rounds - 1) * 10 + 2 * m + 14, lane);
    if (lane == 0) pub_store((u64*)flag, wc.failed ? ~0ull : pub_mix(seq) + fcs);
  }
}

// Same protocol as k_sc_persist, but the tables live in LDS after the first fold (bit-reversed index order, so a fold
// pairs positions q and q + m/2 and is done in place with no hazards): after the first round no table byte touches
// global memory again. Dynamic LDS = ntabs * (n0/2) extension elements.
// ---- device -> host publication without fences -------------------------------------------------------------------
// A system-scope release makes the wave wait for an L2 write-back; with many proofs in flight on one GPU that stalls
// every round behind other proofs' dirty lines. Instead every payload word goes out as a relaxed system-scope store
// (the result area is fine-grained host memory, nothing is cached) and the flag word carries a TAG that binds the
// sequence number to the payload: tag = mix(seq) + sum_i (i+1) * word_i. The host accepts a message only when the tag
// it recomputes from the words it reads matches, so any reordering of the posted writes is harmless.
__device__ __forceinline__ void sc_publish(Ext* result, const Ext* part, const int* tk, const int* toff, int nterms, int wpt, unsigned long long* flag, unsigned long long seq, int lane) {
  unsigned long long cs = 0;
  u64* rw = (u64*)result;
  for (int e = lane; e < nterms * SC_SLOTS; e += 64) {
    int term = e / SC_SLOTS, t = e - term * SC_SLOTS;
    if (t > tk[term]) continue;  // a degree-k term publishes k + 1 values, packed back to back
    Ext v = ex_zero();
    if (wpt == 1) v = part[(size_t)term * SC_SLOTS + t];
    else for (int sb = 0; sb < wpt; sb++) v = ex_add(v, part[(size_t)(term * wpt + sb) * SC_SLOTS + t]);
    int o = toff[term] + t;
    pub_store(rw + 2 * o, v.c0); pub_store(rw + 2 * o + 1, v.c1);
    cs += (unsigned long long)(2 * o + 1) * v.c0 + (unsigned long long)(2 * o + 2) * v.c1;
  }
  cs = pub_wave_sum(cs);
  if (lane == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
}
// publish `n` extension values held in `src` (LDS or global) by one wave
__device__ __forceinline__ void sc_publish_vals(Ext* result, const Ext* src, size_t stride, int n, unsigned long long* flag, unsigned long long seq, int lane) {
  unsigned long long cs = 0;
  u64* rw = (u64*)result;
  for (int e = lane; e < n; e += 64) {
    Ext v = src[(size_t)e * stride];
    pub_store(rw + 2 * e, v.c0); pub_store(rw + 2 * e + 1, v.c1);
    cs += (unsigned long long)(2 * e + 1) * v.c0 + (unsigned long long)(2 * e + 2) * v.c1;
  }
  cs = pub_wave_sum(cs);
  if (lane == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
}
// sharded sumcheck, device-resident exchange (Dev::ShareExchange): `gathered` = the ranks' shares of a round's raw sums, rank
// major, `next` extension values each; their sum mod p goes to the host as ONE message (one host wait per round)
struct Lds_k_shares_sum_publish { Ext res[1024]; };
KBODY k_shares_sum_publish(const u64* gathered, int world, int next, Ext* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_shares_sum_publish, lf); auto& res = lf.res;
  for (int e = threadIdx.x; e < next; e += blockDim.x) {
    Ext acc = ex_zero();
    for (int g = 0; g < world; g++) { const u64* w = gathered + ((size_t)g * next + e) * 2; acc = ex_add(acc, ex(w[0], w[1])); }
    res[e] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 64) sc_publish_vals(result, res, 1, next, flag, seq, threadIdx.x);
}
// sharded sumcheck, peer exchange (csrc/peer_mailbox.h holds the protocol and the argument why two parities suffice): the all-gather AND what follows it in
// one one-workgroup kernel, with no collective library and no host hop between the ranks. `mine`: this rank's `nwords` words; `boxes`: the `world` mailbox
// base addresses as mapped in THIS process (device memory, rank order); `xnum`: the group's exchange number.
//  (a) post: the words and their tag go into slot (xnum & 1, rank) of EVERY rank's mailbox, this rank's own included — relaxed system-scope stores, destinations
//      strided over the waves;
//  (b) gather: slot (xnum & 1, sender) of this rank's OWN mailbox is polled for every sender with relaxed system-scope loads (every load of mailbox bytes is
//      such a load: it bypasses L1, and a stale or torn read fails the tag and is read again) until the tag verifies; a sleep between polls, the wait bounded in
//      TIME by c_poll_timeout_ticks as wc_poll_pause bounds its own; on timeout the failure marker ~0 goes to the host flag and the kernel ends;
//  (c) publish: PEER_MODE_SUM — the shares added mod p (nwords even), as k_shares_sum_publish; PEER_MODE_GATHER — the world x nwords words in rank order.
// Messages of up to PEER_FAST_WORDS words (32 extension values: every round of the usual virtual polynomials) take the fast path: one wave per sender polls its
// slot — one word per lane, the checksum a wave reduction — all senders at once, and leaves the validated words in LDS. Longer ones, up to PEER_SLOT_WORDS, are
// read sender by sender by the whole workgroup.
constexpr int PEER_FAST_WORDS = 64;
struct PeerSt { __device__ __forceinline__ void operator()(u64* p, u64 v) const { pub_store(p, v); } };
struct PeerLd { __device__ __forceinline__ u64 operator()(const u64* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); } };
__device__ __forceinline__ bool peer_poll_pause(unsigned long long t0, unsigned spin) {
  if ((spin & 63) == 63 && dp_realtime() - t0 > c_poll_timeout_ticks) return true;
  for (int q = 0; q < c_poll_sleep; q++) __builtin_amdgcn_s_sleep(4);
  return false;
}
struct alignas(16) Lds_k_peer_exchange_publish { u64 buf[PEER_SLOT_WORDS]; u64 acc[PEER_SLOT_WORDS]; unsigned long long part[16]; int status; int fail; };
KBODY k_peer_exchange_publish(const u64* mine, int nwords, u64* const* boxes, int rank, int world, unsigned long long xnum, int mode, Ext* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_peer_exchange_publish, lf);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  if (tid == 0) lf.fail = 0;
  for (int d = wave; d < world; d += nwaves) {
    u64* slot = boxes[d] + peer_slot(xnum, rank, world);
    const u64 cs = pub_wave_sum(peer_post_words(PeerSt(), slot, mine, (size_t)nwords, (size_t)lane, (size_t)64));
    if (lane == 0) pub_store(slot + PEER_SLOT_WORDS, peer_tag(xnum, cs, (size_t)nwords));
  }
  __syncthreads();
  const u64* box = boxes[rank];
  u64* rw = (u64*)result;
  const unsigned long long t0 = dp_realtime();
  if (nwords <= PEER_FAST_WORDS) {
    for (int s = wave; s < world; s += nwaves) {
      const u64* slot = box + peer_slot(xnum, s, world);
      bool gone = false;
      for (unsigned spin = 0;; spin++) {
        const u64 v = lane < nwords ? PeerLd()(slot + lane) : 0;
        const u64 tag = PeerLd()(slot + PEER_SLOT_WORDS);
        const u64 cs = pub_wave_sum((u64)(lane + 1) * v);  // (lane 0 holds the sum, and decides for the wave)
        if (__shfl((int)(tag == peer_tag(xnum, cs, (size_t)nwords)), 0, 64)) { lf.buf[s * PEER_FAST_WORDS + lane] = v; break; }
        if (__shfl((int)peer_poll_pause(t0, spin), 0, 64)) { gone = true; break; }
      }
      if (gone) { if (lane == 0) lf.fail = 1; break; }
    }
    __syncthreads();
    if (lf.fail) { if (tid == 0) pub_store((u64*)flag, ~0ull); return; }
    if (mode == PEER_MODE_SUM) {
      if (tid < nwords) { u64 a = 0; for (int s = 0; s < world; s++) a = gl_add(a, lf.buf[s * PEER_FAST_WORDS + tid]); lf.acc[tid] = a; }
      __syncthreads();
      if (wave == 0) sc_publish_vals(result, (const Ext*)lf.acc, 1, nwords / 2, flag, seq, lane);
    } else if (wave == 0) {
      unsigned long long cs = 0;
      for (int idx = lane; idx < world * nwords; idx += 64) {
        const int s = idx / nwords, i = idx - s * nwords;
        const u64 v = lf.buf[s * PEER_FAST_WORDS + i];
        pub_store(rw + idx, v); cs += (unsigned long long)(idx + 1) * v;
      }
      cs = pub_wave_sum(cs);
      if (lane == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
    }
    return;
  }
  unsigned long long gcs = 0;  // PEER_MODE_GATHER: this thread's share of the checksum of the message to the host
  for (int i = tid; i < nwords; i += blockDim.x) lf.acc[i] = 0;
  for (int s = 0; s < world; s++) {
    const u64* slot = box + peer_slot(xnum, s, world);
    for (unsigned spin = 0;; spin++) {
      const u64 cs = pub_wave_sum(peer_read_words(PeerLd(), slot, lf.buf, (size_t)nwords, (size_t)tid, (size_t)blockDim.x));
      if (lane == 0) lf.part[wave] = cs;
      __syncthreads();
      if (tid == 0) {
        u64 t = 0; for (int w = 0; w < nwaves; w++) t += lf.part[w];
        lf.status = PeerLd()(slot + PEER_SLOT_WORDS) == peer_tag(xnum, t, (size_t)nwords) ? 1 : peer_poll_pause(t0, spin) ? 2 : 0;
      }
      __syncthreads();
      if (lf.status) break;  // (the same word for every thread: thread 0 writes it again only behind the next barrier)
    }
    if (lf.status == 2) { if (tid == 0) pub_store((u64*)flag, ~0ull); return; }
    if (mode == PEER_MODE_SUM) peer_sum_into(lf.acc, lf.buf, (size_t)nwords, (size_t)tid, (size_t)blockDim.x);
    else for (int i = tid; i < nwords; i += blockDim.x) { const size_t idx = (size_t)s * nwords + i; const u64 v = lf.buf[i]; pub_store(rw + idx, v); gcs += (unsigned long long)(idx + 1) * v; }
    __syncthreads();  // lf.buf and lf.status are free for the next sender
  }
  if (mode == PEER_MODE_SUM) { if (wave == 0) sc_publish_vals(result, (const Ext*)lf.acc, 1, nwords / 2, flag, seq, lane); return; }
  gcs = pub_wave_sum(gcs);
  if (lane == 0) lf.part[wave] = gcs;
  __syncthreads();
  if (tid == 0) { unsigned long long t = 0; for (int w = 0; w < nwaves; w++) t += lf.part[w]; pub_store((u64*)flag, pub_mix(seq) + t); }
}
// lane 0 of wave 0: poll the host mailbox [seq, c0, c1, tag] for `seq`, leave {ok, c0, c1} in chal[]. The seq word is polled
// with relaxed loads; once it matches, an acquire fence orders the payload loads after it, and the tag word — mix(seq) + c0 +
// 2*c1, written by the host with the payload (post_challenge) — is checked against what was read: a stale or torn payload is
// re-polled instead of becoming a wrong challenge (same protocol as the device-to-host direction, wait_flag). The wait is
// bounded in TIME (c_poll_timeout_ticks of the 100 MHz s_memrealtime clock; DP_POLL_TIMEOUT_S, default 20 s: below the host's
// own 30 s), not in spins: a host that serves hundreds of proofs from a few threads is slow, not gone.
__device__ __forceinline__ unsigned long long chal_mix(unsigned long long seq) { return seq * 0x9E3779B97F4A7C15ull + 0x7F4A7C159E3779B9ull; }
// One poll = the four mailbox words read by back-to-back loads: ONE PCIe round trip from the host's write to the challenge in
// registers, not two (seq first, payload after it); the tag makes a torn read harmless. (Keeping two polls in flight half a
// sleep apart was tried: the compiler's s_waitcnt vmcnt(0) at the first check waits for both, the wait gets longer, not shorter.)
struct ChalPoll { unsigned long long w[4]; };
__device__ __forceinline__ ChalPoll chal_poll(const unsigned long long* mailbox) {
  ChalPoll p;
#pragma unroll
  for (int i = 0; i < 4; i++) p.w[i] = __hip_atomic_load(mailbox + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return p;
}
__device__ __forceinline__ void sc_wait_challenge(const unsigned long long* mailbox, unsigned long long seq, unsigned long long* chal) {
  const unsigned long long t0 = dp_realtime();
  bool ok = false;
  unsigned long long c0 = 0, c1 = 0;
  for (unsigned spin = 0;; spin++) {
    const ChalPoll p = chal_poll(mailbox);
    if (p.w[0] == seq && p.w[3] == chal_mix(seq) + p.w[1] + 2 * p.w[2]) { c0 = p.w[1]; c1 = p.w[2]; ok = true; break; }
    if ((spin & 63) == 63 && dp_realtime() - t0 > c_poll_timeout_ticks) break;
    for (int q = 0; q < c_poll_sleep; q++) __builtin_amdgcn_s_sleep(4);  // every poll is a PCIe read: keep the rate of all kernels in flight bounded
  }
  chal[0] = ok ? 1 : 0; chal[1] = c0; chal[2] = c1;
}
__device__ void sc_publish_fwd(Ext* result, const Ext* part, const int* tk, const int* toff, int nterms, int wpt, unsigned long long* flag, unsigned long long seq, int lane) { sc_publish(result, part, tk, toff, nterms, wpt, flag, seq, lane); }
__device__ void sc_publish_vals_fwd(Ext* result, const Ext* src, size_t stride, int n, unsigned long long* flag, unsigned long long seq, int lane) { sc_publish_vals(result, src, stride, n, flag, seq, lane); }
__device__ void sc_wait_challenge_fwd(const unsigned long long* mailbox, unsigned long long seq, unsigned long long* chal) { sc_wait_challenge(mailbox, seq, chal); }
// LDS frame of k_sc_persist_lds (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
constexpr int SPEC_MAXT = 64;     // (term, point) tasks of a speculated round: sum over the terms of k + 1
constexpr size_t SPEC_MAX_H = 128;  // rounds of at most this many pairs are speculated (above, a round's symbolic form costs more than the wait it hides)
struct Lds_k_sc_persist_lds {
  ScPersistArgs a;  // (as in Lds_k_sc_persist)
  Ext part[64 * SC_SLOTS];
  unsigned long long chal[3];
  ScFsArgs fsl;
  int sp_term[SPEC_MAXT], sp_t[SPEC_MAXT], sp_nt;
  Ext spec[SPEC_MAXT * (SC_MAXK + 1)];  // task (term, t): the coefficients in r of the term's NEXT round sum at t
};
// The round AFTER the one whose challenge is still out, computed symbolically in that challenge while it is awaited (round 5). Folding with r turns every
// table entry into a + r (b - a), so a factor of a product term at the evaluation point t is c_t + r d_t, the product of a term's k factors a polynomial of
// degree k in r, and its sum over the pairs k + 1 coefficients: E(r). When r arrives the next message is E(r) (Horner, k multiplications) — the same field
// element as folding first and summing then (exact arithmetic) — and it leaves for the host (or into the sponge) at once; the fold of the tables happens beside
// it. A Fiat-Shamir round of the persistent sumcheck was: sums (6.5 us) -> publish -> wait (10 us: two PCIe hops and the host's sponge) -> fold (6 us); now the
// sums of round j + 1 and the wait of round j overlap. Workers: every wave but wave 0 (which talks to the host / runs the sponge). Tables in LDS, bit-reversed,
// length 2 h: round j pairs (q, q + h); after the fold the pairs of round j + 1 are (q, q + h / 2), i.e. the quad q, q + h/2 | q + h, q + h/2 + h of this round.
template <bool HI>
__device__ __forceinline__ void sc_speculate(const ScPersistArgs& a, const int* sp_term, const int* sp_t, int ntask, const Ext* L, unsigned lgf, size_t h, Ext* spec, int wl, int nwl) {
  constexpr int K = ScW<HI>::K;
  const size_t hq = h / 2;
  unsigned lg = 0; while (lg < 6 && (size_t(2) << lg) <= hq && (ntask << (lg + 1)) <= nwl) lg++;  // 2^lg lanes share a task's quads: as many as the quads and one pass of the workers allow
  const int G = 1 << lg, total = ntask << lg;
  const int lane = wl & 63;
  for (int base = 0; base < total; base += nwl) {
    const int id = base + wl;
    const bool active = id < total;
    const int task = active ? id >> lg : 0, s = id & (G - 1);
    const int term = sp_term[task], k = a.k[term];
    const u64 t = (u64)sp_t[task];
    Ext e[K + 1];
#pragma unroll
    for (int u = 0; u <= K; u++) e[u] = ex_zero();
    if (active)
      for (size_t q = (size_t)s; q < hq; q += (size_t)G) {
        Ext P[K + 1];
#pragma unroll
        for (int u = 0; u <= K; u++) P[u] = ex_zero();
#pragma unroll
        for (int i = 0; i < K; i++) {
          if (i < k) {
            const Ext* T = L + ((size_t)a.t[term][i] << lgf);
            const Ext a0 = T[q], a1 = T[q + h], a2 = T[q + hq], a3 = T[q + hq + h];
            const Ext c = ex_at(a0, a2, t), d = ex_at(ex_sub(a1, a0), ex_sub(a3, a2), t);  // the factor at t: c + r d
            if (i == 0) { P[0] = c; P[1] = d; }
            else {
#pragma unroll
              for (int u = K; u >= 0; u--) {
                if (u <= i + 1) {
                  Ext v = ex_zero();
                  if (u <= i) v = ex_mul(P[u], c);
                  if (u >= 1) v = ex_add(v, ex_mul(P[u - 1], d));
                  P[u] = v;
                }
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u <= K; u++) if (u <= k) e[u] = ex_add(e[u], P[u]);
      }
    for (int d = 1; d < G; d <<= 1) {
#pragma unroll
      for (int u = 0; u <= K; u++) e[u] = ex_add(e[u], ex(shfl_u64(e[u].c0, lane ^ d), shfl_u64(e[u].c1, lane ^ d)));
    }
    if (active && s == 0) {
#pragma unroll
      for (int u = 0; u <= K; u++) if (u <= k) spec[(size_t)task * (SC_MAXK + 1) + u] = e[u];
    }
  }
}
template <bool HI>
KBODY k_sc_persist_lds(const ScPersistArgs& a_in, Ext* result, unsigned long long* flag, const unsigned long long* mailbox, unsigned long long seq0, const ScFsArgs* fs) {
  DP_LDS_DYN(lds_dyn, Lds_k_sc_persist_lds);
  Ext* L = (Ext*)lds_dyn;
  DP_LDS_FRAME(Lds_k_sc_persist_lds, lf); auto& part = lf.part; auto& chal = lf.chal; auto& fsl = lf.fsl;
  for (int i = threadIdx.x; i < (int)(sizeof(ScPersistArgs) / 8); i += blockDim.x) ((u64*)&lf.a)[i] = ((const u64*)&a_in)[i];
  __syncthreads();
  const ScPersistArgs& a = lf.a;
  int tid = threadIdx.x, nt = blockDim.x;
  int W = nt >> 6, wave = tid >> 6, lane = tid & 63;
  int wpt = a.nterms >= W ? 1 : W / a.nterms;
  const bool autofs = fs != nullptr;  // device-side Fiat-Shamir: no host round trips
  if (autofs) { for (int i = tid; i < (int)(sizeof(ScFsArgs) / 8); i += nt) ((u64*)&fsl)[i] = ((const u64*)fs)[i]; __syncthreads(); }
  WaveChallenger wc; wc.k = p2l_load(lane); wc.st = wc.ib = 0; wc.in_len = wc.out_len = 0;
  if (autofs) wc_load(wc, fsl, lane);
  unsigned long long fcs = 0; int round = 0;
  if (a.eq_tab >= 0) wg_build_eq((Ext*)a.in[a.eq_tab], a.eq_pt, a.eq_k);
  unsigned long long seq = seq0;
  size_t first = a.n0 / 2;
  unsigned lgf = 0; while ((size_t(1) << lgf) < first) lgf++;
  u64* const mb = (u64*)(L + ((size_t)a.ntabs << lgf));  // device-side Fiat-Shamir: the message is assembled behind the tables (the launch brings the words for it)
  Ext r = a.r0;
  unsigned long long c_fold = 0, c_sums = 0, c_pub = 0, c_wait = 0, c_rounds = 0, tk = clock64();
  if (!a.has_r0) {
    // round on the tables as they sit in global memory
    size_t npairs = a.n0 / 2;
    for (int term = wave / wpt; term < a.nterms; term += (wpt == 1 ? W : a.nterms + W)) {
      int sub = wave % wpt;
      int k = a.k[term];
      GlobalPairs L;
#pragma unroll
      for (int j = 0; j < ScW<HI>::K; j++) { int ti = a.t[term][j < k ? j : 0]; L.p[j] = a.in[ti]; L.e[j] = a.in_ext[ti]; }
      Ext acc[SC_SLOTS];
      sc_accumulate<HI>(k, L, (size_t)sub * 64 + lane, (size_t)wpt * 64, npairs, acc);
#pragma unroll
      for (int t = 0; t < SC_SLOTS; t++) if (t <= k) acc[t] = wave_reduce_ext(acc[t]);
      if (lane == 0) { Ext* o = part + (size_t)(term * wpt + sub) * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
      if (wpt > 1) break;
    }
    __syncthreads();
    ++seq;
    if (wave == 0) {
      if (autofs) { Ext rr = sc_fs_round(wc, fsl, part, a.k, a.nterms, wpt, mb, round, fcs, lane); if (lane == 0) { chal[0] = 1; chal[1] = rr.c0; chal[2] = rr.c1; } }
      else { sc_publish(result, part, a.k, a.off, a.nterms, wpt, flag, seq, lane); if (lane == 0) sc_wait_challenge(mailbox, seq, chal); }
    }
    round++;
    __syncthreads();
    if (chal[0] == 0) { if (tid == 0) pub_store((u64*)flag, ~0ull); return; }
    r = ex(chal[1], chal[2]);
  }
  // first fold: global -> LDS (bit-reversed positions)
  for (size_t idx = tid; idx < (size_t)a.ntabs * first; idx += nt) {
    int t = (int)(idx >> lgf); size_t i = idx & (first - 1);
    Ext v = a.in_ext[t] ? ex_lerp(((const Ext*)a.in[t])[2 * i], ((const Ext*)a.in[t])[2 * i + 1], r)
                        : ex_lerp_base(((const u64*)a.in[t])[2 * i], ((const u64*)a.in[t])[2 * i + 1], r);
    size_t pos = lgf ? (__brev((unsigned)i) >> (32 - lgf)) : 0;
    L[((size_t)t << lgf) + pos] = v;
  }
  __syncthreads();
  // the (term, point) tasks of the speculation
  if (tid == 0) {
    int n = 0;
    for (int term = 0; term < a.nterms; term++) for (int t = 0; t <= a.k[term]; t++) { if (n < SPEC_MAXT) { lf.sp_term[n] = term; lf.sp_t[n] = t; } n++; }
    lf.sp_nt = n;
  }
  __syncthreads();
  const int ntask = lf.sp_nt;
  const bool can_spec = W > 1 && ntask <= SPEC_MAXT;
  // what a worker lane pays per quad of its task, in units of a degree-2 term's ~620 instructions: the symbolic round must fit into the wait it hides (~10 us)
  int kmax = 1; for (int term = 0; term < a.nterms; term++) kmax = a.k[term] > kmax ? a.k[term] : kmax;
  const unsigned quad_cost = kmax <= 2 ? 1u : kmax == 3 ? 2u : 4u;
  size_t m = first;
  bool have_spec = false;  // part[] already holds the sums of the round at hand (the previous round's speculation evaluated at its challenge)
  for (;;) {
    if (m == 1) {
      ++seq;
      if (tid == 0 && a.dbg) { atomicAdd(a.dbg + 0, c_fold); atomicAdd(a.dbg + 1, c_sums); atomicAdd(a.dbg + 2, c_pub); atomicAdd(a.dbg + 3, c_wait); atomicAdd(a.dbg + 4, c_rounds); }
      if (wave == 0 && autofs) sc_fs_finish(wc, fsl, nullptr, L, size_t(1) << lgf, a.ntabs, mb, (u64*)result, flag, seq0 + 1, fcs, lane);
      else if (wave == 0) sc_publish_vals(result, L, size_t(1) << lgf, a.ntabs, flag, seq, lane);
      return;
    }
    size_t h = m / 2;
    if (tid == 0) { unsigned long long now = clock64(); c_fold += now - tk; tk = now; }
    if (!have_spec) {
      for (int term = wave / wpt; term < a.nterms; term += (wpt == 1 ? W : a.nterms + W)) {
        int sub = wave % wpt;
        int k = a.k[term];
        LdsPairs LP; LP.h = h;
#pragma unroll
        for (int j = 0; j < ScW<HI>::K; j++) LP.p[j] = L + ((size_t)a.t[term][j < k ? j : 0] << lgf);
        Ext acc[SC_SLOTS];
        sc_accumulate<HI>(k, LP, (size_t)sub * 64 + lane, (size_t)wpt * 64, h, acc);
#pragma unroll
        for (int t = 0; t < SC_SLOTS; t++) if (t <= k) acc[t] = wave_reduce_ext(acc[t]);
        if (lane == 0) { Ext* o = part + (size_t)(term * wpt + sub) * SC_SLOTS; for (int t = 0; t < SC_SLOTS; t++) o[t] = acc[t]; }
        if (wpt > 1) break;
      }
      __syncthreads();
    }
    const int wpt_pub = have_spec ? 1 : wpt;  // (a speculated round's sums sit at part[term][t])
    bool spec_next = can_spec && h >= 2 && h <= SPEC_MAX_H;
    if (spec_next) {  // (sc_speculate's own choice of lanes per task)
      const size_t hq = h / 2; unsigned lg = 0; while (lg < 6 && (size_t(2) << lg) <= hq && (ntask << (lg + 1)) <= nt - 64) lg++;
      spec_next = ((hq >> lg) ? (hq >> lg) : 1) * quad_cost <= 4;
    }
    ++seq;
    if (tid == 0) { unsigned long long now = clock64(); c_sums += now - tk; tk = now; }
    if (wave == 0 && autofs) {
      Ext rr = sc_fs_round(wc, fsl, part, a.k, a.nterms, wpt_pub, mb, round, fcs, lane);
      if (lane == 0) { chal[0] = 1; chal[1] = rr.c0; chal[2] = rr.c1; }
      if (tid == 0) { unsigned long long now = clock64(); c_wait += now - tk; tk = now; c_rounds++; }
    } else if (wave == 0) {
      sc_publish(result, part, a.k, a.off, a.nterms, wpt_pub, flag, seq, lane);
      if (tid == 0) { unsigned long long now = clock64(); c_pub += now - tk; tk = now; }
      if (lane == 0) sc_wait_challenge(mailbox, seq, chal);
      if (tid == 0) { unsigned long long now = clock64(); c_wait += now - tk; tk = now; c_rounds++; }
    } else if (spec_next) {
      const unsigned long long ts0 = clock64();
      sc_speculate<HI>(a, lf.sp_term, lf.sp_t, ntask, L, lgf, h, lf.spec, tid - 64, nt - 64);  // the next round, symbolic in the challenge that is out
      if (tid == 64 && a.dbg) { atomicAdd(a.dbg + 5, clock64() - ts0); atomicAdd(a.dbg + 6, 1ull); }
    }
    round++;
    const unsigned long long tb1 = clock64();
    __syncthreads();
    if (tid == 0 && a.dbg) atomicAdd(a.dbg + 7, clock64() - tb1);
    if (chal[0] == 0) { if (tid == 0) pub_store((u64*)flag, ~0ull); return; }
    r = ex(chal[1], chal[2]);
    // the next message = the speculated polynomials at r (one task per thread), and the fold of the tables beside it
    if (spec_next)
      for (int id = tid; id < ntask; id += nt) {
        const int term = lf.sp_term[id], kk = a.k[term];
        const Ext* E = lf.spec + (size_t)id * (SC_MAXK + 1);
        Ext v = E[kk];
        for (int u = kk - 1; u >= 0; u--) v = ex_add(ex_mul(v, r), E[u]);
        part[(size_t)term * SC_SLOTS + lf.sp_t[id]] = v;
      }
    unsigned lgh = 0; while ((size_t(1) << lgh) < h) lgh++;
    for (size_t idx = tid; idx < (size_t)a.ntabs * h; idx += nt) {
      size_t t = idx >> lgh, q = idx & (h - 1);
      Ext* p = L + (t << lgf);
      p[q] = ex_lerp(p[q], p[q + h], r);
    }
    __syncthreads();
    m = h; have_spec = spec_next;
  }
}

// out[e] = sum_{b < nblocks} partial[(e / inner) * nblocks * inner + b * inner + (e % inner)], e < nout, computed by ONE
// workgroup (wave w owns outputs w, w+W, ..) and published straight to host-mapped memory with the tag protocol: the
// second stage of every block-partial reduction needs neither a separate publish launch nor a stream synchronisation.
// LDS frame of k_reduce_publish (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_reduce_publish {
  Ext res[REDUCE_LDS_VALUES];
};
KBODY k_reduce_publish(const Ext* partial, size_t nblocks, size_t inner, int nout, Ext* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_reduce_publish, lf); auto& res = lf.res;
  int tid = threadIdx.x, W = blockDim.x >> 6, wave = tid >> 6, lane = tid & 63;
  for (int e = wave; e < nout; e += W) {
    size_t base = ((size_t)e / inner) * nblocks * inner + ((size_t)e % inner);
    Ext acc = ex_zero();
    for (size_t b = lane; b < nblocks; b += 64) acc = ex_add(acc, partial[base + b * inner]);
    acc = wave_reduce_ext(acc);
    if (lane == 0) res[e] = acc;
  }
  __syncthreads();
  if (wave == 0) sc_publish_vals(result, res, 1, nout, flag, seq, lane);
}
// ---- work-proportional grids for batched kernels over items of very different sizes ------------------------------------
// blockIdx.y = item wastes most of a launch when one item is 2^20 long and thirty others are 2^10 (every empty workgroup
// still has to fetch its descriptor before it can leave). Instead the grid is 1-D and `first[i] .. first[i+1]` are the
// workgroups of item i (first[] sits in front of the descriptors, n + 1 entries): one coalesced load finds the owner.
__device__ __forceinline__ int seg_find(const unsigned* first, int n, int* slot) {
  if (threadIdx.x < 64) {
    for (int base = 0; base < n; base += 64) {
      int i = base + (int)threadIdx.x;
      bool mine = i < n && first[i] <= blockIdx.x && blockIdx.x < first[i + 1];
      if (mine) *slot = i;
    }
  }
  __syncthreads();
  return *slot;
}
// One round of the batch-opening sumcheck (sum_check/classic.rs:232-285, coeff.rs:198-345) over every (f, eq) pair in one
// launch: fold both tables by r (if has_r and the pair is longer than 1; the folded tables go to fout / eqout) and, in the
// same pass, the two sums of the FOLDED pair the next message needs: c0 = sum f0 e0, c2 = sum (f1 - f0)(e1 - e0).
// partial[2 * workgroup + {0,1}]; k_classic_reduce adds the workgroups of each pair and publishes.
// ln > 0: the eq table is FACTORED (Dev::classic_round): table[j] = lo[j mod ln] * eq[j / ln] with ln a power of two and n = ln * |eq|;
// a fold halves lo (into loout) while ln > 1, then eq (into eqout). ln == 0: eq is the table itself.
struct ClassicDesc { const void* f; const Ext* eq; Ext* fout; Ext* eqout; size_t n; int fext; unsigned ln; const Ext* lo; Ext* loout; };
// the factored form of one pair in k_classic_fused: the same sums, from f and the two short tables (which stay in the caches)
__device__ __forceinline__ void classic_fused_factored(const ClassicDesc& p, size_t b, size_t nb, Ext r, int has_r, Ext& c0, Ext& c2) {
  const unsigned ln = p.ln, llog = 31 - __clz(ln);
  if (has_r && p.n > 1) {
    const size_t h = p.n / 2;  // length after the fold
    if (h == 1) {              // (ln, |eq|) = (2, 1) or (1, 2)
      if (b == 0 && threadIdx.x == 0) {
        Ext f = p.fext ? ex_lerp(((const Ext*)p.f)[0], ((const Ext*)p.f)[1], r) : ex_lerp_base(((const u64*)p.f)[0], ((const u64*)p.f)[1], r);
        Ext e;
        if (ln == 2) { Ext s = ex_lerp(p.lo[0], p.lo[1], r); p.loout[0] = s; e = ex_mul(s, p.eq[0]); }
        else { Ext g = ex_lerp(p.eq[0], p.eq[1], r); p.eqout[0] = g; e = ex_mul(p.lo[0], g); }
        p.fout[0] = f;
        c0 = ex_mul(f, e);
      }
      return;
    }
    if (ln >= 4) {
      // the low factor folds; four old entries of a pair of new ones lie in one row of the outer product
      if (b == 0) for (unsigned q = threadIdx.x; q < ln / 2; q += blockDim.x) p.loout[q] = ex_lerp(p.lo[2 * q], p.lo[2 * q + 1], r);
      for (size_t j = b * blockDim.x + threadIdx.x; j < h / 2; j += nb * blockDim.x) {
        Ext f0, f1;
        classic_fold_quad(p.f, p.fext, j, r, f0, f1);
        p.fout[2 * j] = f0; p.fout[2 * j + 1] = f1;
        const Ext* ql = p.lo + ((4 * j) & (ln - 1));
        const Ext H = p.eq[(4 * j) >> llog];
        Ext e0 = ex_lerp(ql[0], ql[1], r), e1 = ex_lerp(ql[2], ql[3], r);
        c0 = ex_add(c0, ex_mul(H, ex_mul(f0, e0)));
        c2 = ex_add(c2, ex_mul(H, ex_mul(ex_sub(f1, f0), ex_sub(e1, e0))));
      }
      return;
    }
    // ln == 2: the low factor becomes the scalar s and the folded table s * eq; ln == 1: the scalar stays and eq folds. The sums are
    // linear in the scalar: it multiplies them once at the end.
    Ext s;
    if (ln == 2) {
      s = ex_lerp(p.lo[0], p.lo[1], r);
      if (b == 0 && threadIdx.x == 0) p.loout[0] = s;
    } else s = p.lo[0];
    for (size_t j = b * blockDim.x + threadIdx.x; j < h / 2; j += nb * blockDim.x) {
      Ext f0, f1;
      classic_fold_quad(p.f, p.fext, j, r, f0, f1);
      p.fout[2 * j] = f0; p.fout[2 * j + 1] = f1;
      Ext e0, e1;
      if (ln == 2) { e0 = p.eq[2 * j]; e1 = p.eq[2 * j + 1]; }
      else { const Ext* qe = p.eq + 4 * j; e0 = ex_lerp(qe[0], qe[1], r); e1 = ex_lerp(qe[2], qe[3], r); p.eqout[2 * j] = e0; p.eqout[2 * j + 1] = e1; }
      c0 = ex_add(c0, ex_mul(f0, e0));
      c2 = ex_add(c2, ex_mul(ex_sub(f1, f0), ex_sub(e1, e0)));
    }
    c0 = ex_mul(c0, s); c2 = ex_mul(c2, s);
    return;
  }
  if (p.n == 1) {
    if (b == 0 && threadIdx.x == 0) c0 = ex_mul(ld_elem(p.f, p.fext, 0), ex_mul(p.lo[0], p.eq[0]));
    return;
  }
  if (ln >= 2) {
    for (size_t j = b * blockDim.x + threadIdx.x; j < p.n / 2; j += nb * blockDim.x) {
      const Ext* ql = p.lo + ((2 * j) & (ln - 1));
      const Ext H = p.eq[(2 * j) >> llog], l0 = ql[0], l1 = ql[1];
      if (p.fext) {
        Ext r0 = ((const Ext*)p.f)[2 * j], r1 = ((const Ext*)p.f)[2 * j + 1];
        c0 = ex_add(c0, ex_mul(H, ex_mul(l0, r0)));
        c2 = ex_add(c2, ex_mul(H, ex_mul(ex_sub(l1, l0), ex_sub(r1, r0))));
      } else {
        u64 r0 = ((const u64*)p.f)[2 * j], r1 = ((const u64*)p.f)[2 * j + 1];
        c0 = ex_add(c0, ex_mul(H, ex_mul_base(l0, r0)));
        c2 = ex_add(c2, ex_mul(H, ex_mul_base(ex_sub(l1, l0), gl_sub(r1, r0))));
      }
    }
    return;
  }
  classic_pair_sums(p.f, p.fext, p.eq, b * blockDim.x + threadIdx.x, nb * blockDim.x, p.n / 2, c0, c2);  // ln == 1: the sums are linear in the scalar lo[0], which multiplies them once
  c0 = ex_mul(c0, p.lo[0]); c2 = ex_mul(c2, p.lo[0]);
}
// this workgroup's share of its pair (`slot`: one int of LDS): the fold, and the thread's part of the two sums added to c0 / c2
__device__ __forceinline__ void classic_fused_block(const unsigned* first, const ClassicDesc* d, int np, Ext r, int has_r, int* slot, Ext& c0, Ext& c2) {
  const int pi = seg_find(first, np, slot);
  const ClassicDesc p = d[pi];
  const size_t b = blockIdx.x - first[pi], nb = first[pi + 1] - first[pi];
  if (p.ln) classic_fused_factored(p, b, nb, r, has_r, c0, c2);
  else if (has_r && p.n > 1) {
    const size_t h = p.n / 2;  // length after the fold
    if (h == 1) {
      if (b == 0 && threadIdx.x == 0) {
        Ext f = p.fext ? ex_lerp(((const Ext*)p.f)[0], ((const Ext*)p.f)[1], r) : ex_lerp_base(((const u64*)p.f)[0], ((const u64*)p.f)[1], r);
        Ext e = ex_lerp(p.eq[0], p.eq[1], r);
        p.fout[0] = f; p.eqout[0] = e;
        c0 = ex_mul(f, e);
      }
    } else {
      for (size_t j = b * blockDim.x + threadIdx.x; j < h / 2; j += nb * blockDim.x) {
        Ext f0, f1;
        classic_fold_quad(p.f, p.fext, j, r, f0, f1);
        const Ext* qe = p.eq + 4 * j;
        Ext e0 = ex_lerp(qe[0], qe[1], r), e1 = ex_lerp(qe[2], qe[3], r);
        p.fout[2 * j] = f0; p.fout[2 * j + 1] = f1; p.eqout[2 * j] = e0; p.eqout[2 * j + 1] = e1;
        c0 = ex_add(c0, ex_mul(f0, e0));
        c2 = ex_add(c2, ex_mul(ex_sub(f1, f0), ex_sub(e1, e0)));
      }
    }
  } else if (p.n == 1) {
    if (b == 0 && threadIdx.x == 0) c0 = ex_mul(ld_elem(p.f, p.fext, 0), p.eq[0]);
  } else classic_pair_sums(p.f, p.fext, p.eq, b * blockDim.x + threadIdx.x, nb * blockDim.x, p.n / 2, c0, c2);
}
KBODY k_classic_fused(const unsigned* first, const ClassicDesc* d, int np, Ext r, int has_r, Ext* partial) {
  __shared__ Ext sm[TPB / 64];
  __shared__ int slot;
  Ext c0 = ex_zero(), c2 = ex_zero();
  classic_fused_block(first, d, np, r, has_r, &slot, c0, c2);
  Ext t;
  t = block_reduce_ext(c0, sm); if (threadIdx.x == 0) partial[2 * (size_t)blockIdx.x] = t;
  t = block_reduce_ext(c2, sm); if (threadIdx.x == 0) partial[2 * (size_t)blockIdx.x + 1] = t;
}
// out[j] = lo[j mod ln] * hi[j / ln] (ln a power of two): the factored eq tables of Dev::classic_round written out once they are short;
// blockIdx.y selects the table
struct EqOuterDesc { Ext* out; const Ext* lo; const Ext* hi; unsigned ln; unsigned n; };
KBODY k_eq_outer_many(const EqOuterDesc* d) {
  const EqOuterDesc p = d[blockIdx.y];
  const unsigned llog = 31 - __clz(p.ln);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gridDim.x * blockDim.x) p.out[i] = ex_mul(p.lo[i & (p.ln - 1)], p.hi[i >> llog]);
}
// out[2 i + t] = sum over the workgroups of pair i of partial[2 w + t], published to the host (np <= 512)
// LDS frame of k_classic_reduce (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_classic_reduce {
  Ext res[REDUCE_LDS_VALUES];
};
// one workgroup adds up the workgroups of each pair (wave w owns pairs w, w + W, ..) and publishes; `ld` loads one block sum
template <class Load>
__device__ __forceinline__ void classic_reduce_pairs(const unsigned* first, int np, const Ext* partial, Ext* res, Ext* result, unsigned long long* flag, unsigned long long seq, Load ld) {
  const int W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < np; i += W) {
    Ext a0 = ex_zero(), a2 = ex_zero();
    for (unsigned w = first[i] + lane; w < first[i + 1]; w += 64) { a0 = ex_add(a0, ld(&partial[2 * (size_t)w])); a2 = ex_add(a2, ld(&partial[2 * (size_t)w + 1])); }
    a0 = wave_reduce_ext(a0); a2 = wave_reduce_ext(a2);
    if (lane == 0) { res[2 * i] = a0; res[2 * i + 1] = a2; }
  }
  __syncthreads();
  if (wave == 0) sc_publish_vals(result, res, 1, 2 * np, flag, seq, lane);
}
KBODY k_classic_reduce(const unsigned* first, int np, const Ext* partial, Ext* result, unsigned long long* flag, unsigned long long seq) {
  DP_LDS_FRAME(Lds_k_classic_reduce, lf);
  classic_reduce_pairs(first, np, partial, lf.res, result, flag, seq, [](const Ext* p) { return *p; });
}
// k_classic_fused whose LAST workgroup is the round's k_classic_reduce (the last-workgroup epilogue: sc_store_through). `counter` is the ticket of ONE proof:
// in a merged cohort launch every blockIdx.z brings its own (and its own result and flag), gridDim.x is the same for all of them.
KBODY k_classic_fused_pub(const unsigned* first, const ClassicDesc* d, int np, Ext r, int has_r, Ext* partial, unsigned* counter, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext sm[TPB / 64];
  __shared__ int slot;
  Ext c0 = ex_zero(), c2 = ex_zero();
  classic_fused_block(first, d, np, r, has_r, &slot, c0, c2);
  Ext t;
  t = block_reduce_ext(c0, sm); if (threadIdx.x == 0) sc_store_through(&partial[2 * (size_t)blockIdx.x], t);
  t = block_reduce_ext(c2, sm); if (threadIdx.x == 0) sc_store_through(&partial[2 * (size_t)blockIdx.x + 1], t);
  if (!sums_ticket_take(counter)) return;
  DP_LDS_FRAME(Lds_k_classic_reduce, lf);
  classic_reduce_pairs(first, np, partial, lf.res, result, flag, seq, [](const Ext* p) { return ld_through(p); });
  if (threadIdx.x == 0) sums_ticket_return(counter);
}
struct EqDesc { Ext* out; unsigned k; unsigned pad; Ext pt[MAX_PT]; };
// many eq tables in one launch: blockIdx.y selects the table (batch_open builds one per opened polynomial)
// eq(i, pt) = lo[i mod 2^kl] * hi[i >> kl]: a workgroup owns EQ_CHUNK consecutive entries of one table, builds the 2^kl
// low-part products (kl <= 8) and its EQ_CHUNK / 2^kl high-part products in LDS, then spends ONE multiplication per entry
// instead of k. (Products in the field are exact: the entries are those of build_eq_x_r_vec bit for bit.)
constexpr unsigned EQ_CHUNK = 4096;
// LDS frame of k_eq_table_many (static __shared__ behind kg / kc, the head of the worker's LDS arena behind the resident executor)
struct Lds_k_eq_table_many {
  Ext lo[256];
  Ext hi[EQ_CHUNK / 256 > 16 ? EQ_CHUNK / 256 : 16];
  int slot;
};
KBODY k_eq_table_many(const unsigned* first, const EqDesc* d, int nd) {
  DP_LDS_FRAME(Lds_k_eq_table_many, lf); auto& lo = lf.lo; auto& hi = lf.hi; auto& slot = lf.slot;
  const int di = seg_find(first, nd, &slot);
  const EqDesc& e = d[di];
  const size_t n = size_t(1) << e.k;
  const unsigned kl = e.k < 8 ? e.k : 8;
  const size_t base = (size_t)(blockIdx.x - first[di]) * EQ_CHUNK;
  const size_t cnt = n - base < EQ_CHUNK ? n - base : EQ_CHUNK;   // entries of this workgroup (a multiple of 2^kl)
  if (threadIdx.x < (1u << kl)) {
    Ext v = ex_one();
    for (unsigned t = 0; t < kl; t++) { Ext r = e.pt[t]; v = ex_mul(v, ((threadIdx.x >> t) & 1) ? r : ex_sub(ex_one(), r)); }
    lo[threadIdx.x] = v;
  }
  const size_t nhi = cnt >> kl;
  if (threadIdx.x < nhi) {
    size_t h = (base >> kl) + threadIdx.x;
    Ext v = ex_one();
    for (unsigned t = kl; t < e.k; t++) { Ext r = e.pt[t]; v = ex_mul(v, ((h >> (t - kl)) & 1) ? r : ex_sub(ex_one(), r)); }
    hi[threadIdx.x] = v;
  }
  __syncthreads();
  for (size_t q = threadIdx.x; q < cnt; q += blockDim.x) e.out[base + q] = ex_mul(lo[q & ((size_t(1) << kl) - 1)], hi[q >> kl]);
}
// (AxpyDesc / AxpyClass: axpy_many.h)
// acc[i] = init[i] (or 0) + sum_d x_d[i >> lg_rep_d] * coeff_d over all descriptors (K11: every codeword / evaluation table merged into
// the running oracle in ONE pass over acc instead of one launch and one read-modify-write of acc per polynomial)
__device__ __forceinline__ void axpy_many_body(Ext* acc, const Ext* init, size_t n_acc, const AxpyDesc* d, int nd) {
  // four elements per thread in flight: the loop is a chain of dependent-latency loads (one codeword word per descriptor), and a
  // worker of the resident executor has only its own four waves to hide them (per element the sum runs over q in order, as before)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n_acc; i += 4 * stride) {
    Ext a[4];
#pragma unroll
    for (int u = 0; u < 4; u++) a[u] = init ? init[i + u * stride] : ex_zero();
    int q = 0;
    for (; q + 1 < nd; q += 2) {  // two base-field descriptors at a time: eight loads in flight per thread
      const AxpyDesc d0 = d[q], d1 = d[q + 1];
      if (d0.xext || d1.xext) break;
      u64 x0[4], x1[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { x0[u] = ((const u64*)d0.x)[(i + u * stride) >> d0.lg_rep]; x1[u] = ((const u64*)d1.x)[(i + u * stride) >> d1.lg_rep]; }
#pragma unroll
      for (int u = 0; u < 4; u++) { a[u] = ex_add(a[u], ex_mul_base(d0.coeff, x0[u])); a[u] = ex_add(a[u], ex_mul_base(d1.coeff, x1[u])); }
    }
    for (; q < nd; q++) {
      const AxpyDesc dq = d[q];
      if (dq.xext) {
        Ext x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = ((const Ext*)dq.x)[(i + u * stride) >> dq.lg_rep];
        if (dq.xext == 2) {
#pragma unroll
          for (int u = 0; u < 4; u++) a[u] = ex_add(a[u], x[u]);
        } else {
#pragma unroll
          for (int u = 0; u < 4; u++) a[u] = ex_add(a[u], ex_mul(x[u], dq.coeff));
        }
      } else {
        u64 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = ((const u64*)dq.x)[(i + u * stride) >> dq.lg_rep];
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = ex_add(a[u], ex_mul_base(dq.coeff, x[u]));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) acc[i + u * stride] = a[u];
  }
  for (; i < n_acc; i += stride) {
    Ext a = init ? init[i] : ex_zero();
    for (int q = 0; q < nd; q++) {
      size_t j = i >> d[q].lg_rep;
      Ext m = d[q].xext == 2 ? ((const Ext*)d[q].x)[j] : d[q].xext ? ex_mul(((const Ext*)d[q].x)[j], d[q].coeff) : ex_mul_base(d[q].coeff, ((const u64*)d[q].x)[j]);
      a = ex_add(a, m);
    }
    acc[i] = a;
  }
}
KBODY k_axpy_many(Ext* acc, const Ext* init, size_t n_acc, const AxpyDesc* d, int nd) { axpy_many_body(acc, init, n_acc, d, nd); }
// The polynomials of a batch opening that are SHORTER than the accumulator (x_d repeated 2^lg_rep_d times: 33 of the 37 of a Dense-4M proof) are
// first summed among their own length: class c = descriptors [first, first + count) of one length n, out_c[i] = sum_d x_d[i] * coeff_d (blockIdx.y = c);
// k_axpy_many then ADDS the class sums (xext = 2) with their repetition. The multiplications run over sum_d |x_d| elements instead of
// nd * n_acc: field arithmetic is exact and every stored value canonical, so the accumulator is bit-identical either way.
KBODY k_axpy_classes(const AxpyClass* c, const AxpyDesc* d) {
  const AxpyClass cl = c[blockIdx.y];
  axpy_many_body(cl.out, nullptr, cl.n, d + cl.first, cl.count);
}
// last fold of a sumcheck, results published directly
KBODY k_finish_publish(const FoldArgs& a, Ext r, int ntabs, Ext* result, unsigned long long* flag, unsigned long long seq) {
  __shared__ Ext res[MAX_TABS];
  int t = threadIdx.x;
  if (t < ntabs) {
    Ext v;
    if (a.ext[t]) { const Ext* p = (const Ext*)a.in[t]; v = ex_lerp(p[0], p[1], r); }
    else { const u64* p = (const u64*)a.in[t]; v = ex_lerp_base(p[0], p[1], r); }
    res[t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) sc_publish_vals(result, res, 1, ntabs, flag, seq, threadIdx.x);
}

// Bulk download with per-chunk tags. A copy kernel followed by a separate "done" publication is only safe across a kernel boundary
// (the end-of-kernel release makes the copy's writes to host memory visible first); between two steps of the resident executor
// nothing orders the PCIe writes of one CU before the tag another CU writes later — round 3 saw stale staging words in downloaded
// proofs exactly that way. So every DL_CHUNK words carry their own tag = dl_mix(seq, chunk) + sum_i (i + 1) * word_i (index within
// the chunk), written after the payload by the workgroup that copied it; the host accepts a chunk when the tag matches what it read.
constexpr unsigned DL_CHUNK = 2048;
__device__ __forceinline__ unsigned long long dl_mix(unsigned long long seq, unsigned long long chunk) { return (seq * 0x9E3779B97F4A7C15ull + chunk) * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull; }
KBODY k_download(const u64* src, u64* dst, size_t nwords, u64* tags, unsigned long long seq) {
  __shared__ unsigned long long dl_part[TPB / 64];
  const size_t nch = (nwords + DL_CHUNK - 1) / DL_CHUNK;
  for (size_t ch = blockIdx.x; ch < nch; ch += gridDim.x) {
    const size_t lo = ch * DL_CHUNK, hi = lo + DL_CHUNK < nwords ? lo + DL_CHUNK : nwords;
    unsigned long long cs = 0;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) { u64 v = src[i]; pub_store(dst + i, v); cs += (unsigned long long)(i - lo + 1) * v; }
    cs = pub_wave_sum(cs);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dl_part[threadIdx.x >> 6] = cs;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 0; for (unsigned w = 0; w < (blockDim.x >> 6); w++) t += dl_part[w]; pub_store(tags + ch, dl_mix(seq, ch) + t); }
  }
}
// copy a small device result into host-mapped memory and publish it
// (launched with ONE wave so that payload stores and the releasing flag store come from the same wave)
KBODY k_publish(const u64* src, u64* dst, size_t nwords, unsigned long long* flag, unsigned long long seq) {
  if (threadIdx.x >= 64) return;  // ONE wave publishes, whatever the size of the workgroup (the resident executor's workers have 256 threads)
  unsigned long long cs = 0;
  for (size_t i = threadIdx.x; i < nwords; i += 64) { u64 v = src[i]; pub_store(dst + i, v); cs += (unsigned long long)(i + 1) * v; }
  cs = pub_wave_sum(cs);
  if (threadIdx.x == 0) pub_store((u64*)flag, pub_mix(seq) + cs);
}

