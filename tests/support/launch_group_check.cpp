// The launch group of deep-prove_amd/csrc/cohort.h driven without a GPU: four host threads (cohorts) of three members each share ONE group and issue a
// common sequence of 300 launches, every thread giving its members turns the way a fiber scheduler does, with random yields between submits. Members leave
// at different launch numbers — one "fails" early, in the middle of a step — and every fourth launch is one whose result a member waits for before it goes on
// (where it reports what it has seen executed, as HipDev's waits do). The fire function stands in for the kernel launch: it records the launch and checks
//   - every launch number fired exactly once, in order;
//   - count = the members still present at that number, each member's pack intact in its own slot;
//   - the ring region of a launch is never written again before the launch is known to have run (nor before it fired) — and, in a second part, that a full
//     ring refuses a launch instead of handing out the region of one in flight;
// and a watchdog ends the program with a non-zero status if it does not finish (a wrong lock shows as a hung batch).
#include "../../deep-prove_amd/csrc/cohort.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

using dp::LaunchGroup;

namespace {
constexpr int THREADS = 4, PER_THREAD = 3, MEMBERS = THREADS * PER_THREAD, LAUNCHES = 300, WAIT_EVERY = 4;
constexpr size_t RING_BYTES = 16 << 10;  // ~20 launches of 12 packs: the ring wraps a dozen times
struct Pack { uint64_t member, launch, body[5], sum; };  // 64 bytes
static_assert(sizeof(Pack) == 64, "pack size");
Pack make_pack(int member, size_t launch) {
  Pack p; p.member = (uint64_t)member; p.launch = launch; p.sum = p.member * 31 + p.launch;
  for (int i = 0; i < 5; i++) { p.body[i] = (p.member + 1) * 0x9E3779B97F4A7C15ull + launch * (uint64_t)(i + 3); p.sum += p.body[i]; }
  return p;
}
// when member m leaves: the launch number of its first launch it no longer takes part in
const int leave_at[MEMBERS] = {LAUNCHES, 17, 120,  LAUNCHES, 200, 200,  64, LAUNCHES, 233,  150, 151, LAUNCHES};
int present_at(size_t n) { int c = 0; for (int m = 0; m < MEMBERS; m++) c += (size_t)leave_at[m] > n; return c; }

LaunchGroup* g_group = nullptr;
std::atomic<size_t> g_fired{0};  // launches fired so far (the "device": a launch's result is visible once it has been fired)
std::atomic<int> g_failures{0};
void fail(const char* what, size_t n) { fprintf(stderr, "FAIL: %s (launch %zu)\n", what, n); g_failures++; }

struct Record { size_t number; int count; size_t phys, bytes; std::vector<char> snapshot; bool retired; };
std::mutex g_rec_mu;
std::vector<Record> g_recs;
size_t g_retired = 0;  // records [0, g_retired) have been checked against their ring regions and retired

// the launch's ring region: where it should be, inside the ring, and overlapping no region of a launch that is fired and not known to have run
void record_launch(const LaunchGroup::Pending& p, size_t n) {
  if (p.packs_dev != p.packs || p.packs != g_group->ring + p.ring_begin % g_group->ring_cap) fail("pack address", n);
  const size_t bytes = (size_t)p.count * p.pack_bytes;
  if (p.ring_begin % g_group->ring_cap + bytes > g_group->ring_cap) fail("a ring region straddles the end", n);
  std::lock_guard<std::mutex> lk(g_rec_mu);
  for (size_t i = g_retired; i < g_recs.size(); i++) {
    const Record& r = g_recs[i];
    const size_t a = p.ring_begin % g_group->ring_cap;
    if (a < r.phys + r.bytes && r.phys < a + bytes) fail("ring region overlaps an in-flight launch", n);
  }
  g_recs.push_back(Record{n, p.count, p.ring_begin % g_group->ring_cap, bytes, std::vector<char>(p.packs, p.packs + bytes), false});
}
void fire(const LaunchGroup::Pending& p, void* stream) {  // (called with the group's lock held)
  const size_t n = g_group->q_base;
  if (stream != (void*)&g_group) fail("fire got another stream", n);
  if (n != g_fired.load()) fail("launch fired out of order or twice", n);
  if (p.count != present_at(n) || p.count != p.expected) fail("count differs from the members present", n);
  if (p.pack_bytes != sizeof(Pack) || p.gx != 7 || p.gy != 1 || p.bx != 256 || p.lds != n % 3) fail("launch shape", n);
  bool seen[MEMBERS] = {};
  for (int k = 0; k < p.count; k++) {
    Pack q; memcpy(&q, p.packs + (size_t)k * sizeof(Pack), sizeof(Pack));
    const Pack want = make_pack((int)(q.member % MEMBERS), n);
    if (q.member >= (uint64_t)MEMBERS || memcmp(&q, &want, sizeof(Pack)) != 0) { fail("a pack is not intact in its slot", n); continue; }
    if (seen[q.member] || (size_t)leave_at[q.member] <= n) fail("a pack of a member that is not (or twice) in this launch", n);
    seen[q.member] = true;
  }
  record_launch(p, n);
  g_fired.store(n + 1, std::memory_order_release);
}
// the ring alone: launches of two members, no checks of who is in them
void fire_plain(const LaunchGroup::Pending& p, void*) { record_launch(p, g_group->q_base); g_fired.store(g_group->q_base + 1, std::memory_order_release); }
// a member has seen the result of launch `li`: every launch before it has run — until now nobody may have written into their ring regions
void retire_before(size_t li) {
  std::lock_guard<std::mutex> lk(g_rec_mu);
  while (g_retired < g_recs.size() && g_recs[g_retired].number < li) {
    Record& r = g_recs[g_retired];
    if (memcmp(g_group->ring + r.phys, r.snapshot.data(), r.bytes) != 0) fail("the ring region of a launch was overwritten while it was in flight", r.number);
    r.retired = true; r.snapshot.clear(); r.snapshot.shrink_to_fit();
    g_retired++;
  }
}

char* ring_alloc(size_t bytes, const char** dev_view) { char* r = (char*)malloc(bytes); *dev_view = r; return r; }
void ring_release(char* r) { free(r); }

struct Member { int id; size_t li; bool waiting; bool gone; };

void cohort_thread(int t, unsigned seed) {
  std::mt19937 rng(seed);
  Member ms[PER_THREAD];
  for (int k = 0; k < PER_THREAD; k++) ms[k] = Member{t * PER_THREAD + k, 0, false, false};
  int live = PER_THREAD;
  auto dawdle = [&] { const unsigned r = rng() % 16; if (r < 5) std::this_thread::yield(); else if (r == 5) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 200)); };
  try {
    while (live) {
      for (Member& m : ms) {
        if (m.gone) continue;
        // one turn of this member: run until it has to wait (or leaves), as a fiber does
        for (;;) {
          if (m.waiting) {
            if (g_fired.load(std::memory_order_acquire) < m.li) break;  // its last launch has not been fired: the turn goes to the next member
            m.waiting = false;
            retire_before(m.li - 1);
            g_group->note_executed(m.li - 1);
          }
          if (m.li >= (size_t)leave_at[m.id]) { g_group->leave(m.li); m.gone = true; live--; break; }
          const Pack p = make_pack(m.id, m.li);
          g_group->submit(m.li, &fire, "k_check", 7, 1, 256, m.li % 3, &p, sizeof p);
          m.li++;
          dawdle();
          if (m.li % WAIT_EVERY == 0) { m.waiting = true; break; }
        }
        dawdle();
      }
    }
  } catch (const std::exception& e) { fprintf(stderr, "FAIL: thread %d: %s\n", t, e.what()); g_failures++; std::_Exit(2); }
}
}  // namespace

int main() {
  std::atomic<bool> finished{false};
  std::thread watchdog([&] {  // (polls: nothing here may depend on what is being checked)
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(120);
    while (!finished.load()) {
      if (std::chrono::steady_clock::now() > until) { fprintf(stderr, "FAIL: watchdog: the launch group did not finish\n"); std::_Exit(3); }
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
  });
  size_t launches = 0, packs = 0;
  {
    LaunchGroup group((void*)&g_group, RING_BYTES / 2, LaunchGroup::RingHooks{&ring_alloc, &ring_release});
    g_group = &group;
    group.configure(THREADS, RING_BYTES);  // (four cohorts: the ring grows to the sum of theirs)
    if (group.ring_cap != RING_BYTES || group.ncohorts != THREADS) fail("configure", 0);
    for (int m = 0; m < MEMBERS; m++) if (group.join() != 0) fail("join returned a launch number other than the first", 0);
    bool threw = false;
    try { group.configure(THREADS, RING_BYTES); } catch (const dp::DpError&) { threw = true; }
    if (!threw) fail("a group with members was regrouped", 0);
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; t++) th.emplace_back(cohort_thread, t, 1234u + 77u * (unsigned)t);
    for (auto& t : th) t.join();
    const size_t mark = group.drain_begin();
    group.drain_end(mark);
    retire_before(mark);
    group.take_stats(&launches, &packs);
    if (mark != (size_t)LAUNCHES || g_fired.load() != (size_t)LAUNCHES || launches != (size_t)LAUNCHES) fail("not every launch was fired", mark);
    size_t want = 0; for (int m = 0; m < MEMBERS; m++) want += (size_t)leave_at[m];
    if (packs != want) fail("pack count", packs);
    if (group.members != 0 || !group.q.empty() || !group.inflight.empty()) fail("the group is not empty after the batch", mark);
    // the out-of-step checks stay: a pack for a launch that was fired, a launch whose shape differs from its group-mates', a proof that joins in mid-step
    group.join(); group.join();
    const Pack p = make_pack(0, 0);
    threw = false;
    try { group.submit(0, &fire, "k_late", 7, 1, 256, 0, &p, sizeof p); } catch (const dp::DpError&) { threw = true; }
    if (!threw) fail("a pack for a fired launch was accepted", 0);
    group.submit(LAUNCHES, &fire, "k_check", 7, 1, 256, LAUNCHES % 3, &p, sizeof p);
    threw = false;
    try { group.submit(LAUNCHES, &fire, "k_other", 9, 1, 256, LAUNCHES % 3, &p, sizeof p); } catch (const dp::DpError&) { threw = true; }
    if (!threw) fail("a launch of another shape was merged", LAUNCHES);
    threw = false;
    try { group.join(); } catch (const dp::DpError&) { threw = true; }
    if (!threw) fail("a proof joined in the middle of a step", LAUNCHES);
    g_group = nullptr;
  }
  {
    // The ring alone, one thread: two members submit launch after launch and nobody reports anything executed — the ring must REFUSE (DP_ERR_OOM) before a region
    // of an in-flight launch is handed out again; once a member has seen a result, the space behind it is free again.
    LaunchGroup group((void*)&g_group, 4096, LaunchGroup::RingHooks{&ring_alloc, &ring_release});
    g_group = &group; g_fired.store(0);
    { std::lock_guard<std::mutex> lk(g_rec_mu); g_recs.clear(); g_retired = 0; }
    group.join(); group.join();
    size_t li = 0; bool refused = false;
    for (; li < 200 && !refused; li++) {
      const Pack a = make_pack(0, li), b = make_pack(1, li);
      try { group.submit(li, &fire_plain, "k_ring", 1, 1, 64, 0, &a, sizeof a); group.submit(li, &fire_plain, "k_ring", 1, 1, 64, 0, &b, sizeof b); }
      catch (const dp::DpError& e) { refused = e.code == dp::DP_ERR_OOM; if (!refused) fail("the ring failed with another error", li); break; }
    }
    if (!refused || li < 16 || li > 32) fail("a 4 KB ring holds 32 launches of two 64-byte packs: it must refuse the 33rd, not earlier and not later", li);
    const size_t fired_then = g_fired.load();
    retire_before(fired_then - 1); group.note_executed(fired_then - 1);
    const Pack a = make_pack(0, li), b = make_pack(1, li);
    try { group.submit(li, &fire_plain, "k_ring", 1, 1, 64, 0, &a, sizeof a); group.submit(li, &fire_plain, "k_ring", 1, 1, 64, 0, &b, sizeof b); }
    catch (const dp::DpError&) { fail("the ring did not take back the space of launches that have run", li); }
    if (g_fired.load() != fired_then + 1) fail("the launch after the refusal was not fired", li);
    g_group = nullptr;
  }
  finished.store(true); watchdog.join();
  printf("launch group ok=%d launches %zu packs %zu failures %d\n", g_failures.load() == 0, launches, packs, g_failures.load());
  return g_failures.load() ? 1 : 0;
}
