// TEST HARNESS (tests/ only): the trace row (csrc/trace_row.h) as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_trace_row.py. For every model blob and input given: run_model -> trace_to_row -> trace_from_row must give back every field of the
// Trace (in / in2 / in3 / out / more_out, conv[*], mha, argmax_max), and witness_host of both traces must agree (flat, mflat, col_len, the
// number of pending lookups) — the context is made over the CPU double of tests/support/cpu_dev.hpp. The taps the device planner records
// (infer_plan) must follow the layout entry by entry. No device, nothing of it is loaded into Python.
// usage: trace_row_check <blob file> <input file> [<blob file> <input file> ...]   (files of int64 words)
#include "cpu_dev.hpp"
#include "../../deep-prove_amd/csrc/zkml.h"
#include "../../deep-prove_amd/csrc/blob.h"
#include "../../deep-prove_amd/csrc/fiber.h"
#define DP_INFER_PLANNER
#include "../../deep-prove_amd/csrc/infer.h"
#include <cstdio>
#include <vector>

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static std::vector<int64_t> read_words(const char* path) {
  std::vector<int64_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  int64_t w;
  while (fread(&w, 8, 1, f) == 1) v.push_back(w);
  fclose(f);
  return v;
}
static bool same_conv(const dp::ConvTrace& a, const dp::ConvTrace& b) {
  return a.input_pad == b.input_pad && a.input_fft == b.input_fft && a.prod == b.prod && a.output_as_element == b.output_as_element;
}

static int check_one(const char* blob_path, const char* input_path) {
  const std::vector<int64_t> blob = read_words(blob_path), input = read_words(input_path);
  dp::ModelSpec m = dp::parse_model(blob.data(), blob.size());
  dp::validate_model(m);
  dp::CpuDev dev;
  std::unique_ptr<dp::Context> ctx = dp::context_generate(dev, m);
  const dp::ModelSpec& spec = ctx->model;
  const dp::Trace a = dp::run_model(spec, input);
  const dp::TraceLayout lay = dp::trace_layout(spec);
  size_t end = 0;
  for (const dp::TraceEntry& e : lay.entries) { CHECK(e.off == end && e.len > 0, "%s: entry at %zu, expected %zu", blob_path, (size_t)e.off, end); end += e.len; }
  CHECK(end == lay.row_words && !lay.entries.empty(), "%s: row_words", blob_path);
  std::vector<int64_t> row(lay.row_words + 2, 0x5a5a5a5a5a5a5a5aLL);  // (a guard word on either side)
  dp::trace_to_row(spec, lay, a, row.data() + 1);
  CHECK(row.front() == 0x5a5a5a5a5a5a5a5aLL && row.back() == 0x5a5a5a5a5a5a5a5aLL, "%s: trace_to_row wrote outside the row", blob_path);
  const dp::Trace b = dp::trace_from_row(spec, input.data(), row.data() + 1);
  CHECK(a.in == b.in, "%s: in", blob_path);
  CHECK(a.in2 == b.in2, "%s: in2", blob_path);
  CHECK(a.in3 == b.in3, "%s: in3", blob_path);
  CHECK(a.out == b.out, "%s: out", blob_path);
  CHECK(a.more_out == b.more_out, "%s: more_out", blob_path);
  CHECK(a.argmax_max == b.argmax_max, "%s: argmax_max", blob_path);
  CHECK(a.conv.size() == b.conv.size(), "%s: conv size %zu / %zu", blob_path, a.conv.size(), b.conv.size());
  for (size_t i = 0; i < a.conv.size(); i++) CHECK(same_conv(a.conv[i], b.conv[i]), "%s: conv[%zu]", blob_path, i);
  CHECK(a.mha.size() == b.mha.size(), "%s: mha size", blob_path);
  for (const auto& kv : a.mha) {
    auto it = b.mha.find(kv.first);
    CHECK(it != b.mha.end() && kv.second.softmax_in == it->second.softmax_in && kv.second.softmax_out == it->second.softmax_out, "%s: mha[%zu]", blob_path, kv.first);
  }
  const dp::WitnessHost wa = dp::witness_host(*ctx, a), wb = dp::witness_host(*ctx, b);
  CHECK(wa.flat == wb.flat && wa.mflat == wb.mflat && wa.col_len == wb.col_len && wa.pend.size() == wb.pend.size(), "%s: witness_host", blob_path);
  // the device planner's taps: one per entry, the same offsets and lengths, tensors of that length
  const dp::InferProgram p = dp::infer_plan(spec, dp::INFER_ALL_KINDS);
  CHECK(p.taps.size() == lay.entries.size() && p.row_words == lay.row_words, "%s: taps", blob_path);
  for (size_t k = 0; k < p.taps.size(); k++)
    CHECK(p.taps[k].off == lay.entries[k].off && p.taps[k].len == lay.entries[k].len && p.taps[k].tensor >= 0 && p.tensors[(size_t)p.taps[k].tensor].len == p.taps[k].len, "%s: tap %zu", blob_path, k);
  printf("trace_row_check ok: %s: %zu nodes, %zu entries, %zu words, %zu conv, %zu mha, %zu argmax, witness %zu words\n", blob_path, spec.layers.size(), lay.entries.size(), lay.row_words,
         a.conv.size(), a.mha.size(), a.argmax_max.size(), wa.flat.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3 || argc % 2 == 0) { fprintf(stderr, "usage: trace_row_check <blob file> <input file> ...\n"); return 2; }
  try {
    for (int i = 1; i + 1 < argc; i += 2) if (int rc = check_one(argv[i], argv[i + 1])) return rc;
  } catch (const dp::DpError& e) { fprintf(stderr, "DpError: %s\n", e.what()); return 1; }
  return 0;
}
