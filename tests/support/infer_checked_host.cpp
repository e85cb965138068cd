// TEST HARNESS (tests/ only): the host half of the device inference's refusals — the per-sample Softmax shift step (csrc/infer.h:
// infer_softmax_shifts, reached the way hip_infer_run reaches it, through InferProgram::shifts) — as a stand-alone program,
// built with -fsanitize=address,undefined by tests/test_infer_checked_host.py. No device, nothing of it is loaded into Python.
// usage: infer_checked_host <model blob file: int64 words of a softmax_only model>
#include "../../deep-prove_amd/csrc/zkml.h"
#include "../../deep-prove_amd/csrc/blob.h"
#include "../../deep-prove_amd/csrc/fiber.h"  // (host_cpu_budget, which the shift step sizes its threads by)
#define DP_INFER_PLANNER
#include "../../deep-prove_amd/csrc/infer.h"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <vector>

static uint64_t rs = 7;
static uint64_t rnd() { rs += 0x9E3779B97F4A7C15ULL; uint64_t z = rs; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: infer_checked_host <blob file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int64_t> blob;
  int64_t w;
  while (fread(&w, 8, 1, f) == 1) blob.push_back(w);
  fclose(f);
  setenv("DP_HOST_THREADS", "4", 1);  // (the batch below is large enough for the step to use them)
  try {
    dp::ModelSpec m = dp::parse_model(blob.data(), blob.size());
    dp::validate_model(m);
    const dp::InferProgram p = dp::infer_plan(m, dp::INFER_ALL_KINDS);
    const dp::InferOp* op = nullptr;
    for (const dp::InferOp& o : p.ops) if (o.kind == dp::IO_SOFTMAX) op = &o;
    CHECK(op, "no Softmax op in the program");
    const dp::LayerSpec& sm = m.layers[(size_t)op->node];
    const size_t C = op->d[0], R = op->d[1], K = op->d[2], rows = C * R, per = rows * K, nb = 200;
    CHECK(per == p.tensors[(size_t)op->in0].len && rows == p.tensors[(size_t)op->in1].len, "shapes");
    const int64_t lim = int64_t(1) << 24;
    const std::set<size_t> bad = {1, 77, nb - 1}, refused = {3, 150, 151};
    std::vector<int64_t> x(nb * per), shifts(nb * rows, -12345);
    std::vector<uint32_t> status(nb, 0);
    for (size_t b = 0; b < nb; b++) for (size_t j = 0; j < per; j++) {
      const uint64_t r = rnd();
      x[b * per + j] = b % 3 == 0 ? (int64_t)(r % 4001) - 2000 : (int64_t)(r % (2 * (uint64_t)lim + 1)) - lim;  // small rows, and rows over the whole allowed range
    }
    x[5 * per + 2] = lim; x[5 * per + 7] = -lim;  // the bounds themselves are allowed
    for (size_t b : bad) x[b * per + (b * 5) % per] = b == 77 ? -lim - 1 : lim + 1;
    for (size_t b : refused) {  // what later kernels may have made of a sample an earlier op refused
      status[b] = b == 3 ? dp::INFER_BAD_LAYERNORM : b == 151 ? dp::INFER_BAD_LAYERNORM_TABLE : dp::INFER_BAD_REQUANT;  // (151: the internal class)
      for (size_t j = 0; j < per; j++) x[b * per + j] = j % 2 ? std::numeric_limits<int64_t>::max() : std::numeric_limits<int64_t>::min();
    }
    const std::vector<uint32_t> status_before = status;
    p.shifts(*op, x.data(), nb, shifts.data(), status.data());
    size_t ngood = 0;
    for (size_t b = 0; b < nb; b++) {
      if (refused.count(b)) {
        CHECK(status[b] == status_before[b] && status[b], "sample %zu: a refused sample's reason changed to %u", b, status[b]);
        for (size_t i = 0; i < rows; i++) CHECK(shifts[b * rows + i] == 0, "sample %zu row %zu: shift %lld of a refused sample", b, i, (long long)shifts[b * rows + i]);
      } else if (bad.count(b)) {
        CHECK(status[b] == dp::INFER_BAD_SOFTMAX, "sample %zu: status %u, expected INFER_BAD_SOFTMAX", b, status[b]);
        for (size_t i = 0; i < rows; i++) CHECK(shifts[b * rows + i] == 0, "sample %zu row %zu: shift of a sample out of range", b, i);
      } else {
        CHECK(status[b] == dp::INFER_OK, "sample %zu: status %u of a good sample", b, status[b]);
        for (size_t i = 0; i < rows; i++) {
          const int64_t want = dp::softmax_row_shift(sm, &x[b * per + i * K], i % R + 1);
          CHECK(shifts[b * rows + i] == want, "sample %zu row %zu: shift %lld, softmax_row_shift %lld", b, i, (long long)shifts[b * rows + i], (long long)want);
        }
        ngood++;
      }
    }
    // on the good samples alone (what a plain call that goes on has at the step) it gives the same shifts and leaves every word zero; of the
    // first three samples it refuses the one out of range and serves the other two
    std::vector<int64_t> gx, gs, plain;
    for (size_t b = 0; b < nb; b++) if (!status[b]) { gx.insert(gx.end(), &x[b * per], &x[b * per] + per); gs.insert(gs.end(), &shifts[b * rows], &shifts[b * rows] + rows); }
    plain.assign(gs.size(), -1);
    std::vector<uint32_t> gst(ngood, 0);
    p.shifts(*op, gx.data(), ngood, plain.data(), gst.data());
    CHECK(plain == gs && gst == std::vector<uint32_t>(ngood, 0), "infer_softmax_shifts on the good samples");
    std::vector<int64_t> three(&x[0], &x[0] + 3 * per), s3(3 * rows, -1);  // (sample 1 is out of range, none of the three is garbage)
    std::vector<uint32_t> st3(3, 0);
    p.shifts(*op, three.data(), 3, s3.data(), st3.data());
    CHECK(st3 == (std::vector<uint32_t>{0, dp::INFER_BAD_SOFTMAX, 0}), "infer_softmax_shifts on three samples: status %u %u %u", st3[0], st3[1], st3[2]);
    for (size_t i = 0; i < 3 * rows; i++) CHECK(s3[i] == (i / rows == 1 ? 0 : dp::softmax_row_shift(sm, &three[i * K], i % R + 1)), "infer_softmax_shifts on three samples: shift %zu", i);
    // a batch of one, good and bad
    uint32_t st1 = 0;
    std::vector<int64_t> s1(rows, -1);
    p.shifts(*op, &x[0], 1, s1.data(), &st1);
    CHECK(st1 == 0 && std::equal(s1.begin(), s1.end(), shifts.begin()), "batch of one, good");
    p.shifts(*op, &x[per], 1, s1.data(), &st1);
    CHECK(st1 == dp::INFER_BAD_SOFTMAX && s1 == std::vector<int64_t>(rows, 0), "batch of one, bad");
    printf("infer_checked_host ok: %zu samples of %zu rows x %zu, %zu good, %zu out of range, %zu refused before\n", nb, rows, K, ngood, bad.size(), refused.size());
  } catch (const dp::DpError& e) { fprintf(stderr, "DpError: %s\n", e.what()); return 1; }
  return 0;
}
