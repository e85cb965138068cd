// decode_step / decode_limit of csrc/infer.h (the one step of dp_model_decode that the host loop and k_infer_next_token share) on the host, under
// AddressSanitizer and UndefinedBehaviorSanitizer: built and run by tests/test_decode_host.py. Two parts, both at seq = 4 with `out` and
// `tokens` in heap blocks of exactly seq words, so that an index outside them is reported:
//   1. single steps over every (length 0..5, limit 0..5, eos -1..3, status 0..2, stop before 0..4, chosen token 0..3): the result against the
//      steps as the header states them, and nothing but tokens[length] written;
//   2. whole decodes over every (prompt_len 1..4, max_new 0..5, eos -1..3, a toy model 0..3, the step at which the inference is refused): the
//      loop over decode_step against the loop written out literally (limits, inference, end-of-sequence, append).
#include "../../deep-prove_amd/csrc/infer.h"
#include <cstdio>
#include <cstring>
#include <memory>

using namespace dp;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

constexpr uint32_t SEQ = 4;
// the toy model: position j chooses a token from its own token, its position and the salt
static void toy(const int64_t* tokens, int64_t* out, int salt) { for (uint32_t j = 0; j < SEQ; j++) out[j] = (tokens[j] * 3 + j + salt) % 4; }

int main() {
  size_t singles = 0, decodes = 0;
  for (uint32_t length = 0; length <= 5; length++) for (uint32_t limit = 0; limit <= 5; limit++) for (int64_t eos = -1; eos <= 3; eos++)
    for (uint32_t status = 0; status <= 2; status++) for (uint32_t before = 0; before <= 4; before++) for (int64_t chosen = 0; chosen <= 3; chosen++) {
      std::unique_ptr<int64_t[]> out(new int64_t[SEQ]), tokens(new int64_t[SEQ]);
      for (uint32_t j = 0; j < SEQ; j++) { out[j] = 7; tokens[j] = 100 + j; }
      if (length >= 1 && length <= SEQ) out[length - 1] = chosen;
      uint32_t len = length, stop = before;
      decode_step(len, stop, limit, SEQ, eos, status, out.get(), tokens.get());
      // the steps as the header states them; an append is followed by the limits of the new length
      uint32_t wlen = length, wstop = before; int64_t wtok = -1;
      if (!before) {
        if (status) wstop = DECODE_STOP_REFUSED;
        else if (length == 0 || length >= SEQ) wstop = DECODE_STOP_WINDOW;
        else if (length >= limit) wstop = DECODE_STOP_MAX_NEW;
        else if (eos >= 0 && chosen == eos) wstop = DECODE_STOP_EOS;
        else { wtok = chosen; wlen = length + 1; wstop = wlen >= SEQ ? DECODE_STOP_WINDOW : wlen >= limit ? DECODE_STOP_MAX_NEW : 0; }
      }
      CHECK(len == wlen && stop == wstop, "single step (length %u limit %u eos %lld status %u before %u chosen %lld): length %u stop %u, want %u %u", length, limit, (long long)eos, status, before,
            (long long)chosen, len, stop, wlen, wstop);
      for (uint32_t j = 0; j < SEQ; j++) CHECK(tokens[j] == (wtok >= 0 && j == length ? wtok : 100 + j), "single step: token %u", j);
      CHECK(decode_limit(length, limit, SEQ) == (length == 0 || length >= SEQ ? DECODE_STOP_WINDOW : length >= limit ? DECODE_STOP_MAX_NEW : 0u), "decode_limit");
      singles++;
    }
  for (uint32_t pl = 1; pl <= SEQ; pl++) for (uint32_t max_new = 0; max_new <= 5; max_new++) for (int64_t eos = -1; eos <= 3; eos++) for (int salt = 0; salt < 4; salt++)
    for (int refuse_at = -1; refuse_at <= 3; refuse_at++) {
      const int64_t pad = 1;
      // the loop written out: limits first, then the inference (refused at its refuse_at-th run), then the end-of-sequence test, then the append
      int64_t wt[SEQ], wo[SEQ]; uint32_t wlen = pl, wstop = 0; int runs = 0;
      for (uint32_t j = 0; j < SEQ; j++) wt[j] = j < pl ? (int64_t)((j + salt) % 4) : pad;
      while (!wstop) {
        if (wlen == SEQ) { wstop = DECODE_STOP_WINDOW; break; }
        if (wlen == pl + max_new) { wstop = DECODE_STOP_MAX_NEW; break; }
        if (runs++ == refuse_at) { wstop = DECODE_STOP_REFUSED; break; }
        toy(wt, wo, salt);
        if (wo[wlen - 1] == eos) { wstop = DECODE_STOP_EOS; break; }
        wt[wlen] = wo[wlen - 1]; wlen++;
      }
      // the loop over decode_step, as dp_model_decode_host runs it
      std::unique_ptr<int64_t[]> out(new int64_t[SEQ]), tokens(new int64_t[SEQ]);
      for (uint32_t j = 0; j < SEQ; j++) { tokens[j] = j < pl ? (int64_t)((j + salt) % 4) : pad; out[j] = -5; }
      const uint32_t limit = pl + max_new < SEQ ? pl + max_new : SEQ;
      uint32_t len = pl, stop = 0, status = 0; int got_runs = 0, steps = 0;
      while (!stop) {
        if (!decode_limit(len, limit, SEQ)) { if (got_runs++ == refuse_at) status = 2; else toy(tokens.get(), out.get(), salt); }
        decode_step(len, stop, limit, SEQ, eos, status, out.get(), tokens.get());
        CHECK(++steps <= (int)SEQ + 1, "decode: the loop does not end");
      }
      CHECK(len == wlen && stop == wstop && got_runs == runs, "decode (prompt_len %u max_new %u eos %lld salt %d refuse_at %d): length %u stop %u runs %d, want %u %u %d", pl, max_new, (long long)eos, salt,
            refuse_at, len, stop, got_runs, wlen, wstop, runs);
      CHECK(!memcmp(tokens.get(), wt, sizeof(wt)), "decode (prompt_len %u max_new %u eos %lld salt %d refuse_at %d): tokens", pl, max_new, (long long)eos, salt, refuse_at);
      decodes++;
    }
  printf("decode_step_host ok: %zu single steps, %zu decodes\n", singles, decodes);
  return 0;
}
