// The prepare-ahead hand-over of deep-prove_amd/csrc/prep_ahead.h driven without a GPU: four consumer threads (the proving fibers' side: they draw item numbers
// from a common counter and take() each) and two helper threads (helper_loop) over 2 000 items. make() yields at random, throws for a fixed subset of the items
// when a HELPER calls it and for a smaller subset whoever calls it. Checked:
//   - every item is taken exactly once, and made at most once by a helper and at most once by a consumer;
//   - an item whose helper failed was made again by its consumer, and that succeeded; an item a helper made is the one the consumer got;
//   - an item that fails for everybody surfaces the CONSUMER's own exception;
//   - a helper never makes an item at or beyond next + ahead, nor one of the first (which start at once);
//   - stop() ends helpers that wait for the consumers to come nearer;
// and a watchdog ends the program with a non-zero status if it does not finish (a lost hand-over shows as a consumer that waits for ever).
#include "../../deep-prove_amd/csrc/prep_ahead.h"

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <stdexcept>
#include <thread>
#include <vector>

namespace {
constexpr size_t N = 2000, CONSUMERS = 4, HELPERS = 2, AHEAD = 16;
struct Item { size_t i; bool by_helper; uint64_t sum; };
struct MakeError : std::runtime_error { size_t i; bool by_helper; MakeError(size_t i_, bool h) : std::runtime_error("make failed"), i(i_), by_helper(h) {} };
bool fails_for_helpers(size_t i) { return i % 7 == 3; }
bool fails_for_everybody(size_t i) { return i % 97 == 5; }
uint64_t sum_of(size_t i) { return (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull; }

std::atomic<size_t> g_next{0};  // the consumers' counter: the item handed out next
std::atomic<int> g_failures{0};
std::atomic<int> g_helper_calls[N], g_consumer_calls[N], g_taken[N];
std::atomic<size_t> g_from_helper{0}, g_repeated{0}, g_own_errors{0};
void fail(const char* what, size_t i) { fprintf(stderr, "FAIL: %s (item %zu)\n", what, i); g_failures++; }

void dawdle(std::mt19937& rng) { const unsigned r = rng() % 16; if (r < 5) std::this_thread::yield(); else if (r == 5) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 100)); }
std::unique_ptr<Item> make(size_t i, bool by_helper, std::mt19937& rng) {
  if (by_helper) {
    if (i < CONSUMERS) fail("a helper made one of the items that start at once", i);
    if (i >= g_next.load() + AHEAD) fail("a helper ran further ahead than allowed", i);  // (next only grows: the helper saw a smaller one)
    if (g_helper_calls[i].fetch_add(1) != 0) fail("two helpers made the same item", i);
  } else if (g_consumer_calls[i].fetch_add(1) != 0) fail("two consumers made the same item", i);
  dawdle(rng);
  if (fails_for_everybody(i) || (by_helper && fails_for_helpers(i))) throw MakeError(i, by_helper);
  dawdle(rng);
  return std::unique_ptr<Item>(new Item{i, by_helper, sum_of(i)});
}

void consumer(dp::PrepAhead<Item>* pa, unsigned seed) {
  std::mt19937 rng(seed);
  for (;;) {
    const size_t i = g_next.fetch_add(1);
    if (i >= N) return;
    try {
      std::unique_ptr<Item> it = pa->take(i, [&](size_t k) { return make(k, false, rng); }, [] { std::this_thread::yield(); });
      if (!it || it->i != i || it->sum != sum_of(i)) { fail("the consumer got another item than its own", i); continue; }
      if (fails_for_everybody(i)) fail("an item that fails for everybody was handed over", i);
      if (it->by_helper) { g_from_helper++; if (fails_for_helpers(i)) fail("a helper's failed item was handed over", i); if (g_consumer_calls[i].load() != 0) fail("made by a helper AND by its consumer", i); }
      else if (g_helper_calls[i].load() != 0) { g_repeated++; if (!fails_for_helpers(i)) fail("the consumer repeated an item its helper had made", i); }
    } catch (const MakeError& e) {
      if (!fails_for_everybody(i) || e.i != i) fail("an exception for an item that does not fail", i);
      if (e.by_helper) fail("the consumer saw the helper's exception, not its own", i);
      g_own_errors++;
    }
    if (g_taken[i].fetch_add(1) != 0) fail("an item was taken twice", i);
    std::this_thread::sleep_for(std::chrono::microseconds(20 + rng() % 120));  // (the "proof": the helpers get ahead meanwhile)
  }
}
}  // namespace

int main() {
  std::atomic<bool> finished{false};
  std::thread watchdog([&] {  // (polls: nothing here may depend on what is being checked)
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(120);
    while (!finished.load()) {
      if (std::chrono::steady_clock::now() > until) { fprintf(stderr, "FAIL: watchdog: the hand-over did not finish\n"); std::_Exit(3); }
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
  });
  {
    dp::PrepAhead<Item> pa(N, CONSUMERS, AHEAD);
    g_next.store(0);
    std::atomic<int> helpers_left{0};
    std::vector<std::thread> hs, cs;
    for (size_t h = 0; h < HELPERS; h++) hs.emplace_back([&, h] { std::mt19937 rng(99u + (unsigned)h); pa.helper_loop(g_next, [&](size_t k) { return make(k, true, rng); }); helpers_left++; });
    for (size_t c = 0; c < CONSUMERS; c++) cs.emplace_back(consumer, &pa, 1234u + 77u * (unsigned)c);
    for (auto& t : cs) t.join();
    pa.stop();
    for (auto& t : hs) t.join();
    if (helpers_left.load() != (int)HELPERS) fail("a helper did not leave", 0);
    size_t everybody = 0;
    for (size_t i = 0; i < N; i++) {
      if (g_taken[i].load() != 1) fail("an item was not taken exactly once", i);
      if (g_helper_calls[i].load() > 1 || g_consumer_calls[i].load() > 1) fail("an item was made more than once by one side", i);
      if (g_helper_calls[i].load() + g_consumer_calls[i].load() == 0) fail("an item was never made", i);
      if (g_helper_calls[i].load() == 1 && (fails_for_helpers(i) || fails_for_everybody(i)) && g_consumer_calls[i].load() != 1) fail("a helper's failure was not repeated by the consumer", i);
      everybody += fails_for_everybody(i);
    }
    if (g_own_errors.load() != everybody) fail("not every item that fails for everybody surfaced its consumer's exception", g_own_errors.load());
    if (!g_from_helper.load() || !g_repeated.load()) fail("the helpers never got ahead: nothing was handed over (or nothing repeated)", g_from_helper.load());
  }
  {
    // stop(): nobody consumes (next stays 0), the helpers may make item 0 only and then wait for the consumers to come nearer — until they are told to leave
    dp::PrepAhead<Item> pa(100, 0, 1);
    std::atomic<size_t> next{0}, made{0}, left{0};
    std::vector<std::thread> hs;
    for (size_t h = 0; h < HELPERS; h++) hs.emplace_back([&] { pa.helper_loop(next, [&](size_t k) { made++; return std::unique_ptr<Item>(new Item{k, true, sum_of(k)}); }); left++; });
    while (made.load() == 0) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
    if (left.load() != 0 || made.load() != 1) fail("helpers with nothing to do ran on or left before stop()", made.load());
    pa.stop();
    for (auto& t : hs) t.join();
    if (left.load() != HELPERS || made.load() != 1) fail("stop() did not end the helpers where they were", made.load());
    std::unique_ptr<Item> it = pa.take(0, [](size_t) -> std::unique_ptr<Item> { throw std::runtime_error("item 0 was ready"); }, [] {});
    if (!it || it->i != 0 || !it->by_helper) fail("the item made before stop() is not handed over", 0);
  }
  finished.store(true); watchdog.join();
  printf("prep ahead ok=%d items %zu from helpers %zu repeated %zu own errors %zu failures %d\n", g_failures.load() == 0, N, g_from_helper.load(), g_repeated.load(), g_own_errors.load(), g_failures.load());
  return g_failures.load() ? 1 : 0;
}
