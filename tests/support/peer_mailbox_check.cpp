// The mailbox protocol of the peer exchange (deep-prove_amd/csrc/peer_mailbox.h) on the CPU: W threads act as the ranks, every mailbox is an array of
// std::atomic<uint64_t>, posts and polls are the header's own functions with relaxed accesses — what k_peer_exchange_publish does with relaxed system-scope
// accesses on the device. 200 exchanges per world size with message lengths 1, 2, 8, 520 and 2048 words, both modes, and random per-rank delays, so that a
// rank regularly runs a full exchange ahead of another: every rank must gather exactly what was posted. A stale slot (the previous contents of the parity) and
// a torn one (tag of one exchange, words of another) must be rejected. Built plain, with -fsanitize=thread and with -fsanitize=address,undefined
// (tests/test_peer_mailbox_host.py).
#include "../../deep-prove_amd/csrc/peer_mailbox.h"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

using namespace dp;
typedef std::atomic<uint64_t> Word;
struct St { void operator()(Word* p, u64 v) const { p->store(v, std::memory_order_relaxed); } };
struct Ld { u64 operator()(const Word* p) const { return p->load(std::memory_order_relaxed); } };

static u64 splitmix(u64 x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
// word i of rank r's message in exchange e: a canonical field element (mode SUM adds them mod p)
static u64 word_of(int world, int r, unsigned long long e, size_t i) { return splitmix(((u64)world << 56) ^ ((u64)r << 48) ^ (e << 20) ^ (u64)i) % GL_P; }
static const size_t LENS[5] = {1, 2, 8, 520, 2048};
static size_t len_of(unsigned long long e) { return LENS[e % 5]; }
static int mode_of(unsigned long long e) { return (len_of(e) % 2 == 0 && (e / 5) % 2 == 0) ? PEER_MODE_SUM : PEER_MODE_GATHER; }

static std::atomic<int> g_fail{0};
static std::atomic<long> g_ahead{0}, g_repolls{0};
#define CHECK(c, ...) do { if (!(c)) { if (g_fail.fetch_add(1) < 10) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static void run_world(int world, int exchanges) {
  std::vector<std::unique_ptr<Word[]>> boxes;
  for (int r = 0; r < world; r++) { boxes.emplace_back(new Word[peer_mailbox_words(world)]); for (size_t i = 0; i < peer_mailbox_words(world); i++) boxes[r][i].store(0, std::memory_order_relaxed); }
  std::vector<std::atomic<unsigned long long>> done(world);  // the last exchange a rank has finished gathering
  for (auto& d : done) d.store(0);
  std::vector<std::thread> th;
  for (int r = 0; r < world; r++) th.emplace_back([&, r] {
    std::vector<u64> mine(PEER_SLOT_WORDS), got(PEER_SLOT_WORDS), acc(PEER_SLOT_WORDS), all((size_t)world * PEER_SLOT_WORDS);
    u64 rng = splitmix(0xC0FFEE ^ ((u64)world << 8) ^ (u64)r);
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(120);
    for (unsigned long long e = 1; e <= (unsigned long long)exchanges; e++) {  // the group's counter: 1 at connect, + 1 per exchange
      rng = splitmix(rng);
      if ((rng & 3) == 0) std::this_thread::sleep_for(std::chrono::microseconds((rng >> 8) % 300));  // a slow rank: its peers get an exchange ahead
      const size_t n = len_of(e);
      for (size_t i = 0; i < n; i++) mine[i] = word_of(world, r, e, i);
      for (int d = 0; d < world; d++) if (done[d].load() + 1 < e) g_ahead++;  // d still gathers e - 1 while this rank posts e: a full exchange ahead
      for (int d = 0; d < world; d++) peer_post(St(), boxes[d].get(), e, r, world, mine.data(), n);
      for (size_t i = 0; i < n; i++) acc[i] = 0;
      for (int s = 0; s < world; s++) {
        for (unsigned spin = 0;; spin++) {
          if (peer_try_read(Ld(), (const Word*)boxes[r].get(), e, s, world, got.data(), n)) break;
          g_repolls++;
          std::this_thread::yield();
          if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() > deadline) { CHECK(false, "world %d rank %d: exchange %llu of sender %d never arrived", world, r, e, s); return; }
        }
        if (mode_of(e) == PEER_MODE_SUM) peer_sum_into(acc.data(), got.data(), n, 0, 1);
        else for (size_t i = 0; i < n; i++) all[(size_t)s * n + i] = got[i];
      }
      if (mode_of(e) == PEER_MODE_SUM) {
        for (size_t i = 0; i < n; i++) {
          unsigned __int128 t = 0; for (int s = 0; s < world; s++) t += word_of(world, s, e, i);
          CHECK(acc[i] == (u64)(t % GL_P), "world %d rank %d exchange %llu: sum word %zu", world, r, e, i);
        }
      } else {
        for (int s = 0; s < world; s++) for (size_t i = 0; i < n; i++) CHECK(all[(size_t)s * n + i] == word_of(world, s, e, i), "world %d rank %d exchange %llu: word %zu of sender %d", world, r, e, i, s);
      }
      done[r].store(e);
    }
  });
  for (auto& t : th) t.join();
}

// a slot that holds something else than the exchange asked for is refused, whatever it is
static void rejections() {
  const int world = 2, s = 1;
  std::unique_ptr<Word[]> box(new Word[peer_mailbox_words(world)]);
  for (size_t i = 0; i < peer_mailbox_words(world); i++) box[i].store(0);
  std::vector<u64> a(PEER_SLOT_WORDS), b(PEER_SLOT_WORDS), got(PEER_SLOT_WORDS);
  for (size_t n : LENS) {
    const unsigned long long e = 7;
    for (size_t i = 0; i < n; i++) { a[i] = word_of(world, s, e, i); b[i] = word_of(world, s, e + 2, i); }
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e, s, world, got.data(), n) || n == 0, "an empty slot was accepted (n = %zu)", n);
    peer_post(St(), box.get(), e, s, world, a.data(), n);
    CHECK(peer_try_read(Ld(), (const Word*)box.get(), e, s, world, got.data(), n), "the posted message was refused (n = %zu)", n);
    for (size_t i = 0; i < n; i++) CHECK(got[i] == a[i], "word %zu read back wrong", i);
    // stale: the next exchange of this parity finds the previous contents
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 2, s, world, got.data(), n), "a stale slot (exchange e for e + 2) was accepted (n = %zu)", n);
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e - 2, s, world, got.data(), n), "a slot of a later exchange was accepted (n = %zu)", n);
    if (n > 1) CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e, s, world, got.data(), n - 1), "a message of another length was accepted (n = %zu)", n);
    // torn, one way: the words of e + 2 have landed, the tag is still that of e
    Word* slot = box.get() + peer_slot(e, s, world);
    peer_post_words(St(), slot, b.data(), n, 0, 1);
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e, s, world, got.data(), n), "torn slot (tag e, words e + 2) accepted as e (n = %zu)", n);
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 2, s, world, got.data(), n), "torn slot (tag e, words e + 2) accepted as e + 2 (n = %zu)", n);
    // torn, the other way: the tag of e + 2 has landed, the words are still those of e (and half-way: the first word only)
    peer_post(St(), box.get(), e + 2, s, world, b.data(), n);
    peer_post_words(St(), slot, a.data(), n, 0, 1);
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 2, s, world, got.data(), n), "torn slot (tag e + 2, words e) accepted (n = %zu)", n);
    peer_post_words(St(), slot, b.data(), n, 0, 1);
    if (n > 1) { St()(slot + (n - 1), a[n - 1]); CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 2, s, world, got.data(), n), "a slot with one old word was accepted (n = %zu)", n); St()(slot + (n - 1), b[n - 1]); }
    CHECK(peer_try_read(Ld(), (const Word*)box.get(), e + 2, s, world, got.data(), n), "the completed message of e + 2 was refused (n = %zu)", n);
    // the other sender's slot and the other parity were never written
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 2, 0, world, got.data(), n), "another sender's empty slot was accepted");
    CHECK(!peer_try_read(Ld(), (const Word*)box.get(), e + 1, s, world, got.data(), n), "the other parity's empty slot was accepted");
    for (size_t i = 0; i < peer_mailbox_words(world); i++) box[i].store(0);
  }
  // layout: the slots of a mailbox are disjoint and inside it
  for (int w : {1, 2, 4, 8, 16}) for (int par = 0; par < 2; par++) for (int r = 0; r < w; r++) {
    const size_t o = peer_slot((unsigned long long)par, r, w);
    CHECK(o == ((size_t)par * w + r) * PEER_SLOT_STRIDE && o + PEER_SLOT_STRIDE <= peer_mailbox_words(w), "slot (%d, %d) of a world of %d", par, r, w);
  }
}

int main(int argc, char** argv) {
  const int exchanges = argc > 1 ? atoi(argv[1]) : 200;
  rejections();
  for (int world : {1, 2, 4, 8}) run_world(world, exchanges);
  printf("peer mailbox: exchanges %d per world, posts a full exchange ahead of a peer %ld, re-polls %ld, failures %d\n", exchanges, g_ahead.load(), g_repolls.load(), g_fail.load());
  printf("peer mailbox ok=%d\n", g_fail.load() == 0 ? 1 : 0);
  return g_fail.load() == 0 ? 0 : 1;
}
