// Test support: the hand-written gfx950 field forms (deep-prove_amd/csrc/gl64_gfx950.h) and everything the kernels build from them, run as FUNCTIONS on
// inputs read from a file, results written to files. It computes no expected value: tests/support/field_cases.py makes the inputs and holds the reference
// (Python integers), tests/test_gpu_field_forms.py and tests/test_field_forms_host.py compare. It does not link the product library: it includes the
// product's headers and a cut of csrc/kernels.inc (tests/support/kernel_emul/extract.py, built by __graft_entry__.build_field_probe()).
//
// One source, three builds:
//   hipcc --offload-arch=gfx950                      the asm forms (what the library runs)
//   hipcc --offload-arch=gfx950 -DDP_NO_GFX950_ASM   the portable device forms (what every diagnostic library gets)
//   g++ -x c++ -DDP_PROBE_HOST                       every section a plain loop on the host; the flag, DPP and p2l_* sections are left out
//
// usage: field_probe <input file> <output directory>       (file layout: field_cases.py)
// Every HIP call and the synchronisation after every launch is checked; the first error is printed and ends the program, nothing further is launched.
#include "../../deep-prove_amd/csrc/poseidon2.h"
#include "../../deep-prove_amd/csrc/poseidon2_fast.h"
#include "../../deep-prove_amd/csrc/gl64_lazy.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace dp;

#ifdef DP_PROBE_HOST
#define PHD inline
#define __device__
#define __forceinline__ inline
static const u64* const c_rc = POSEIDON2_RC_HOST;
#include "field_probe_host_cut.inc"  // L3, l3_split, p2l_ref_join3, p2l_ref_fma3
#else
#include <hip/hip_runtime.h>
#define PHD __device__ __forceinline__
__constant__ u64 c_rc[DP_POSEIDON2_RC_WORDS];
#include "field_probe_cut.inc"  // the dpp_* helpers and the lane-parallel Poseidon2 (p2l_*)
#endif

constexpr u64 MAGIC = 0x4650524F42453031ULL, SENTINEL = 0xD15EA5ED0BADC0DEULL;
enum { TAG_FORM = 1, TAG_CANON = 2, TAG_LAZY = 3, TAG_ACC = 5, TAG_MADDW = 6, TAG_LIN = 7, TAG_PERM = 8, TAG_PERM1 = 9 };
constexpr int A_OUT = 10, B_OUT = 3, CANON_OUT = 13, LAZY_OUT = 6, LIN_OUT = 6, PERM_OUT = 44, PERM1_OUT = 12;
constexpr size_t MAX_LAUNCH = (size_t(1) << 17) - 1;

// ------------------------------------------------------------------------------------------------ the raw forms, each build's own
PHD u64 probe_fma(u64 a, u64 b, u64 d) {
#ifdef DP_GFX950_ASM
  return gx::fma(a, b, d);
#else
  const unsigned __int128 x = (unsigned __int128)a * b + d;
  return p2f::red128((u64)x, (u64)(x >> 64));
#endif
}
PHD u64 probe_mul_small(u64 a, u32 k) {
#ifdef DP_GFX950_ASM
  return gx::mul_small(a, k);
#else
  return p2f::mul(a, (u64)k);
#endif
}
// section a. record (a, b, d, x, e, A, B, C) -> mul, fma, mul_small x 5, mul_f<true>, fma3_f<true>, join3_f<true>
PHD void body_a(const u64* r, u64* o) {
  const u64 a = r[0], b = r[1], d = r[2], x = r[3], e = r[4];
  const u32 A = (u32)r[5], B = (u32)r[6], C = (u32)r[7];
  o[0] = p2f::mul(a, b);
  o[1] = probe_fma(a, b, d);
  o[2] = probe_mul_small(a, 0u);
  o[3] = probe_mul_small(a, 1u);
  o[4] = probe_mul_small(a, 7u);
  o[5] = probe_mul_small(a, 1u << 31);
  o[6] = probe_mul_small(a, 0xFFFFFFFFu);
#ifdef DP_PROBE_HOST
  { const unsigned __int128 v = (unsigned __int128)a * b; o[7] = p2f::red128((u64)v, (u64)(v >> 64)); }
  o[8] = p2l_ref_fma3(x, e, A, B, C);
  o[9] = p2l_ref_join3(A, B, C);
#else
  u64 flag = 0, pend = 0;  // (the FIX forms leave them alone)
  L3 v; v.a = A; v.b = B; v.c = C;
  o[7] = p2l_mul<true>(a, b, flag, pend);
  o[8] = p2l_fma3<true>(x, e, v, flag, pend);
  o[9] = p2l_join3<true>(v, flag, pend);
#endif
}
// section c, canonical operands (a, b, r in the extension): the wrappers as the kernels call them
PHD void body_canon(const u64* r, u64* o) {
  const Ext a = ex(r[0], r[1]), b = ex(r[2], r[3]), t = ex(r[4], r[5]);
  o[0] = gl_mul(a.c0, b.c0);
  o[1] = gl_sqr(a.c0);
  o[2] = gl_mul7(a.c0);
  const Ext m = ex_mul(a, b);                      o[3] = m.c0; o[4] = m.c1;
  const Ext mb = ex_mul_base(a, b.c0);             o[5] = mb.c0; o[6] = mb.c1;
  const Ext l = ex_lerp(a, b, t);                  o[7] = l.c0; o[8] = l.c1;
  const Ext lb = ex_lerp_base(a.c0, b.c0, t);      o[9] = lb.c0; o[10] = lb.c1;
  const Ext iv = ex_inv(a);                        o[11] = iv.c0; o[12] = iv.c1;
}
// section c, any representative in, canonicalised as the callers do: a b, b + r a, b0 + r a0
PHD void body_lazy(const u64* r, u64* o) {
  const Ext a = ex(r[0], r[1]), b = ex(r[2], r[3]), t = ex(r[4], r[5]);
  const Ext m = lz::ex_canon(lz::ex_mul(a, b));              o[0] = m.c0; o[1] = m.c1;
  const Ext f = lz::ex_canon(lz::ex_fma(t, a, b));           o[2] = f.c0; o[3] = f.c1;
  const Ext fb = lz::ex_canon(lz::ex_fma_base(t, a.c0, b.c0)); o[4] = fb.c0; o[5] = fb.c1;
}
// section c, ExAcc: record (start, count, step, -) sums pool[(start + j step) % m], j < count
PHD void body_acc(const u64* r, const u64* pool, u64 m, u64* o) {
  lz::ExAcc acc = lz::acc_zero();
  for (u64 j = 0; j < r[1]; j++) { const u64 i = (r[0] + j * r[2]) % m; lz::acc_add(acc, ex(pool[4 * i], pool[4 * i + 1])); }
  const Ext v = lz::acc_value(acc);
  o[0] = v.c0; o[1] = v.c1;
}
// section c, the internal layer's d_i x_i + row sum: record (a, b, w0 .. w7)
PHD void body_maddw(const u64* r, u64* o) {
  p2f::W sum = p2f::w_of(r[2]);
  for (int i = 1; i < 8; i++) sum = p2f::w_add64(sum, r[2 + i]);
  o[0] = p2f::canon(p2f::mul_add_w(r[0], r[1], p2f::w_reduce(sum), sum));
}
// section e, one permutation per lane
PHD void body_perm1(const u64* r, u64* o) {
  u64 s[8];
  for (int i = 0; i < 8; i++) s[i] = r[i];
  p2f::permute(s, c_rc);
  for (int i = 0; i < 8; i++) o[i] = p2f::canon(s[i]);
  p2f::compress(r, r + 4, o + 8, c_rc);
}

// ------------------------------------------------------------------------------------------------ kernels
#ifndef DP_PROBE_HOST
#define TID const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; if (i >= n) return
// masked: the call is made under `if (lane & 1)`; the other lanes keep the sentinel their outputs were filled with
__global__ void __launch_bounds__(256) k_a(const u64* in, u64* out, size_t n, int masked) {
  TID;
  if (!masked || (threadIdx.x & 1)) body_a(in + 8 * i, out + A_OUT * i);
}
// section b: the deferred-borrow forms in a row, as a permutation chains them; r1 r2 r3 per lane, flag and pend per wave (by the first lane that ran)
__global__ void __launch_bounds__(256) k_b(const u64* in, u64* out, u64* fl, size_t n, int masked) {
  TID;
  const int lane = threadIdx.x & 63;
  if (!masked || (lane & 1)) {
    const u64* r = in + 8 * i;
    L3 v; v.a = (u32)r[5]; v.b = (u32)r[6]; v.c = (u32)r[7];
    u64 flag = 0, pend = 0;
    const u64 r1 = p2l_mul<false>(r[0], r[1], flag, pend);
    const u64 r2 = p2l_fma3<false>(r[3], r[4], v, flag, pend);
    const u64 r3 = p2l_join3<false>(v, flag, pend);
    out[B_OUT * i] = r1; out[B_OUT * i + 1] = r2; out[B_OUT * i + 2] = r3;
    if (lane == (masked ? 1 : 0)) { fl[2 * (i >> 6)] = flag; fl[2 * (i >> 6) + 1] = pend; }
  }
}
__global__ void __launch_bounds__(256) k_canon(const u64* in, u64* out, size_t n) { TID; body_canon(in + 6 * i, out + CANON_OUT * i); }
__global__ void __launch_bounds__(256) k_lazy(const u64* in, u64* out, size_t n) { TID; body_lazy(in + 6 * i, out + LAZY_OUT * i); }
__global__ void __launch_bounds__(256) k_acc(const u64* in, u64* out, size_t n, u64 m) { TID; body_acc(in + 4 * i, in + 4 * n, m, out + 2 * i); }
__global__ void __launch_bounds__(256) k_maddw(const u64* in, u64* out, size_t n) { TID; body_maddw(in + 10 * i, out + i); }
__global__ void __launch_bounds__(256) k_perm1(const u64* in, u64* out, size_t n) { TID; body_perm1(in + 8 * i, out + PERM1_OUT * i); }
// section d: n is a multiple of 8 (whole groups); record (x, rc) -> limbs of lin_full(x, rc), limbs of lin_sum8(x)
__global__ void __launch_bounds__(256) k_lin(const u64* in, u64* out, size_t n) {
  TID;
  const L3 f = p2l_lin_full(in[2 * i], l3_split(in[2 * i + 1])), s = p2l_lin_sum8(in[2 * i]);
  u64* o = out + LIN_OUT * i;
  o[0] = f.a; o[1] = f.b; o[2] = f.c; o[3] = s.a; o[4] = s.b; o[5] = s.c;
}
// section e: G states on one 64-lane block, 8 lanes per state, looped over as k_merkle_tail loops over a narrow layer (groups of the wave fall idle).
// per state: permute_impl<false> (8) | permute_impl<true> (8) | p2l_permute (8) | p2l_compress (4) | flag as each lane saw it (8) | pend (8)
__global__ void __launch_bounds__(64) k_perm(const u64* in, u64* out, int G) {
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 7;
  P2lK k = p2l_load(lane);
  // lanes 0 .. 22 of k.tab are read from EVERY lane (v_readlane in p2l_add_int_rc), so they must be computed while those lanes are active. Nothing tells the
  // compiler: it sank the limb split of p2l_load below the divergent `g < G` guard of this loop, and with G = 1 lanes 8 .. 22 then held no limbs. The library's
  // kernels load P2lK in front of an enclosing loop (k_merkle_tail, the tails) or launch whole waves (k_merkle_layer_lp); here the values are pinned.
  asm volatile("" : "+v"(k.tab.a), "+v"(k.tab.b), "+v"(k.tab.c));
  for (int g = tid >> 3; g < G; g += 8) {
    const u64 s = in[8 * g + i];
    u64* o = out + PERM_OUT * g;
    u64 flag = 0, pend = 0, f2 = 0, p2 = 0;
    o[i] = p2f::canon(p2l_permute_impl<false>(s, lane, k, flag, pend));
    o[28 + i] = flag; o[36 + i] = pend;
    o[8 + i] = p2f::canon(p2l_permute_impl<true>(s, lane, k, f2, p2));
    o[16 + i] = p2l_permute(s, lane, k);
    p2l_compress(in + 8 * g, o + 24, lane, k);
  }
}
#define CK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "field_probe: %s failed: %s\n", #call, hipGetErrorString(e_)); exit(1); } } while (0)
// in -> device, out (sentinel-filled) -> device, one launch, checked synchronisation, out <- device
template <class F> static void on_device(const std::vector<u64>& in, std::vector<u64>& out, F launch) {
  u64 *di = nullptr, *dout = nullptr;
  CK(hipMalloc(&di, in.size() * 8)); CK(hipMalloc(&dout, out.size() * 8));
  CK(hipMemcpy(di, in.data(), in.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dout, out.data(), out.size() * 8, hipMemcpyHostToDevice));
  launch(di, dout);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost));
  CK(hipFree(di)); CK(hipFree(dout));
}
#define RUN(kernel, ...) on_device(in, out, [&](u64* di, u64* dout) { hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const u64*)di, dout, __VA_ARGS__); })
#else
#define RUN(kernel, ...)
#endif

static void die(const char* what) { fprintf(stderr, "field_probe: %s\n", what); exit(1); }
static void append(FILE* f, const std::vector<u64>& v) { if (!v.empty() && fwrite(v.data(), 8, v.size(), f) != v.size()) die("short write"); }

int main(int argc, char** argv) {
  if (argc != 3) die("usage: field_probe <input file> <output directory>");
  std::vector<u64> file;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input file");
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 8) die("the input file is not a sequence of u64");
    file.resize((size_t)bytes / 8);
    if (fread(file.data(), 8, file.size(), f) != file.size()) die("short read");
    fclose(f);
  }
  FILE* sec[5];
  for (int s = 0; s < 5; s++) {
    const std::string p = std::string(argv[2]) + "/" + "abcde"[s] + ".bin";
    if (!(sec[s] = fopen(p.c_str(), "wb"))) die("cannot open an output file");
  }
#ifdef DP_PROBE_HOST
  printf("variant: host\n");
#else
  CK(hipMemcpyToSymbol(HIP_SYMBOL(c_rc), POSEIDON2_RC_HOST, sizeof(POSEIDON2_RC_HOST)));
#ifdef DP_NO_GFX950_ASM
  printf("variant: portable device forms\n");
#else
  printf("variant: gfx950 asm\n");
#endif
#endif
  size_t pos = 0, blocks = 0;
  while (pos < file.size()) {
    if (pos + 5 > file.size() || file[pos] != MAGIC) die("bad block header");
    const u64 tag = file[pos + 1], mode = file[pos + 2], n = file[pos + 3], wpr = file[pos + 4];
    if (n == 0 || n > MAX_LAUNCH || wpr == 0 || wpr > 16 || pos + 5 + n * wpr > file.size()) die("bad block size");
    const std::vector<u64> in(file.begin() + pos + 5, file.begin() + pos + 5 + n * wpr);
    pos += 5 + n * wpr; blocks++;
    std::vector<u64> out;
    switch (tag) {
      case TAG_FORM: {
        if (wpr != 8 || mode > 1) die("FORM: bad record");
        const int masked = (int)mode;
        out.assign(n * A_OUT, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < n; i++) if (!masked || (i & 1)) body_a(&in[8 * i], &out[A_OUT * i]);
        append(sec[0], out);
#else
        RUN(k_a, (size_t)n, masked);
        append(sec[0], out);
        const size_t waves = (n + 63) / 64;
        out.assign(n * B_OUT + 2 * waves, SENTINEL);
        on_device(in, out, [&](u64* di, u64* dout) { hipLaunchKernelGGL(k_b, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const u64*)di, dout, dout + n * B_OUT, (size_t)n, masked); });
        append(sec[1], out);
#endif
        break;
      }
      case TAG_CANON:
        if (wpr != 6) die("CANON: bad record");
        out.assign(n * CANON_OUT, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < n; i++) body_canon(&in[6 * i], &out[CANON_OUT * i]);
#endif
        RUN(k_canon, (size_t)n);
        append(sec[2], out);
        break;
      case TAG_LAZY:
        if (wpr != 6) die("LAZY: bad record");
        out.assign(n * LAZY_OUT, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < n; i++) body_lazy(&in[6 * i], &out[LAZY_OUT * i]);
#endif
        RUN(k_lazy, (size_t)n);
        append(sec[2], out);
        break;
      case TAG_ACC: {  // `mode` records, then the pool
        if (wpr != 4 || mode == 0 || mode >= n) die("ACC: bad record");
        const size_t na = (size_t)mode; const u64 m = n - mode;
        for (size_t i = 0; i < na; i++) if (in[4 * i + 1] > 4096) die("ACC: count too large");
        out.assign(2 * na, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < na; i++) body_acc(&in[4 * i], &in[4 * na], m, &out[2 * i]);
#else
        on_device(in, out, [&](u64* di, u64* dout) { hipLaunchKernelGGL(k_acc, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, 0, (const u64*)di, dout, na, m); });
#endif
        append(sec[2], out);
        break;
      }
      case TAG_MADDW:
        if (wpr != 10) die("MADDW: bad record");
        out.assign(n, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < n; i++) body_maddw(&in[10 * i], &out[i]);
#endif
        RUN(k_maddw, (size_t)n);
        append(sec[2], out);
        break;
      case TAG_LIN:
        if (wpr != 2 || n % 8) die("LIN: records come in whole groups of 8");
#ifndef DP_PROBE_HOST
        out.assign(n * LIN_OUT, SENTINEL);
        RUN(k_lin, (size_t)n);
        append(sec[3], out);
#endif
        break;
      case TAG_PERM:
        if (wpr != 8 || n > 64) die("PERM: bad record");
#ifndef DP_PROBE_HOST
        out.assign(n * PERM_OUT, SENTINEL);
        on_device(in, out, [&](u64* di, u64* dout) { hipLaunchKernelGGL(k_perm, dim3(1), dim3(64), 0, 0, (const u64*)di, dout, (int)n); });
        append(sec[4], out);
#endif
        break;
      case TAG_PERM1:
        if (wpr != 8) die("PERM1: bad record");
        out.assign(n * PERM1_OUT, SENTINEL);
#ifdef DP_PROBE_HOST
        for (size_t i = 0; i < n; i++) body_perm1(&in[8 * i], &out[PERM1_OUT * i]);
#endif
        RUN(k_perm1, (size_t)n);
        append(sec[4], out);
        break;
      default: die("unknown block tag");
    }
  }
  for (int s = 0; s < 5; s++) if (fclose(sec[s]) != 0) die("cannot close an output file");
  printf("field_probe: %zu blocks done\n", blocks);
  return 0;
}
