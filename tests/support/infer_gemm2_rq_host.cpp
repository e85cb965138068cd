// TEST HARNESS (tests/ only): what infer_fuse_plan (csrc/infer.h) marks for k_infer_gemm2_i8_rq, as a stand-alone program built with
// -fsanitize=address,undefined by tests/test_infer_gemm2_rq_host.py. No device, nothing of it is loaded into Python.
// usage: infer_gemm2_rq_host <model blob file: int64 words> ...
// prints per model one line per IO_GEMM2: "gemm2 <op> rq <op of the absorbed Requant, -1: none> flags <d[1]> softmax <op, -1: none> back <the
// Softmax's d[5]> masked <the planner's masked constant> table16 <bytes of the 16-bit table image>"
#include "../../deep-prove_amd/csrc/zkml.h"
#include "../../deep-prove_amd/csrc/blob.h"
#include "../../deep-prove_amd/csrc/fiber.h"
#define DP_INFER_PLANNER
#include "../../deep-prove_amd/csrc/infer.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  for (int arg = 1; arg < argc; arg++) {
    FILE* f = fopen(argv[arg], "rb");
    if (!f) { perror(argv[arg]); return 2; }
    std::vector<int64_t> blob;
    int64_t w;
    while (fread(&w, 8, 1, f) == 1) blob.push_back(w);
    fclose(f);
    try {
      dp::ModelSpec m = dp::parse_model(blob.data(), blob.size());
      dp::validate_model(m);
      const dp::InferProgram p = dp::infer_plan(m, dp::INFER_ALL_KINDS);
      printf("model %d ops %zu\n", arg - 1, p.ops.size());
      for (size_t i = 0; i < p.ops.size(); i++) {
        const dp::InferOp& o = p.ops[i];
        if (o.kind != dp::IO_GEMM2) continue;
        const bool sm = o.nfused && (o.d[1] & dp::IG2_SM);
        const dp::InferOp* s = sm ? &p.ops[o.d[2]] : nullptr;
        if (s && (s->kind != dp::IO_SOFTMAX || s->out != o.in0 || !(o.d[1] & dp::IG2_SM_SKIP) != (dp::infer_softmax_masked(p, *s) != 0))) { fprintf(stderr, "FAIL: op %zu names no Softmax of its own\n", i); return 1; }
        printf("gemm2 %zu rq %d flags %zu softmax %d back %zu masked %lld table16 %zu\n", i, o.nfused ? o.fused[0] : -1, o.nfused ? o.d[1] : (size_t)0, s ? (int)o.d[2] : -1, s ? s->d[5] : (size_t)0,
               s ? (long long)dp::infer_softmax_masked(p, *s) : 0LL, s ? p.consts[(size_t)s->table].w8.size() : (size_t)0);
      }
    } catch (const dp::DpError& e) { fprintf(stderr, "DpError: %s\n", e.what()); return 1; }
  }
  printf("infer_gemm2_rq_host ok: %d models\n", argc - 1);
  return 0;
}
