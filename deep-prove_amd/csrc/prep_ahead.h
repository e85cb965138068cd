// The hand-over between the helper threads that prepare the inputs of a batch AHEAD and the workers that consume them (capi.cpp prove_batch_body: inference and
// the host half of the witness generation of the next inputs, made while the proofs in flight wait for the device). Lock-free, nothing of HIP:
// tests/support/prep_ahead_check.cpp drives it from plain threads, once under ThreadSanitizer.
// State of item i: 0 nobody has touched it, 1 being made, 2 ready in its slot, 3 the helper failed (the worker repeats it so that the error is its own).
#pragma once
#include <atomic>
#include <chrono>
#include <cstddef>
#include <memory>
#include <thread>
#include <vector>

namespace dp {

template <class P>
class PrepAhead {
 public:
  // n items; the helpers start at item `first` (the items before it start at once: their workers make them themselves) and stay less than `ahead` items
  // beyond the one handed out last
  PrepAhead(size_t n, size_t first, size_t ahead) : n_(n), ahead_(ahead), prep_(n), pst_(new std::atomic<int>[n]), pnext_(first) {
    for (size_t i = 0; i < n; i++) pst_[i].store(0, std::memory_order_relaxed);
  }
  // a helper thread: `next` is the workers' counter (the number of the item handed out next), make(i) the item (it may throw)
  template <class Make>
  void helper_loop(const std::atomic<size_t>& next, Make&& make) {
    for (;;) {
      const size_t i = pnext_.fetch_add(1);
      if (i >= n_) return;
      while (!pstop_.load(std::memory_order_relaxed) && i >= next.load(std::memory_order_relaxed) + ahead_) std::this_thread::sleep_for(std::chrono::microseconds(200));
      if (pstop_.load(std::memory_order_relaxed)) return;
      if (i < next.load(std::memory_order_relaxed)) continue;  // handed out meanwhile (or the batch is being abandoned)
      int e = 0;
      if (!pst_[i].compare_exchange_strong(e, 1)) continue;
      try { prep_[i] = make(i); pst_[i].store(2, std::memory_order_release); } catch (...) { pst_[i].store(3, std::memory_order_release); }
    }
  }
  // the worker that was handed item i: makes it, or waits (yield()) for the helper that is making it and takes what it made — or makes it again if that failed
  template <class Make, class Yield>
  std::unique_ptr<P> take(size_t i, Make&& make, Yield&& yield) {
    int e = 0;
    if (pst_[i].compare_exchange_strong(e, 1)) return make(i);
    while ((e = pst_[i].load(std::memory_order_acquire)) == 1) yield();
    return e == 2 ? std::move(prep_[i]) : make(i);
  }
  void stop() { pstop_.store(true); }  // the helpers leave (before they are joined)

 private:
  size_t n_, ahead_;
  std::vector<std::unique_ptr<P>> prep_;
  std::unique_ptr<std::atomic<int>[]> pst_;
  std::atomic<size_t> pnext_;
  std::atomic<bool> pstop_{false};
};

}  // namespace dp
