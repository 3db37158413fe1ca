// The launch pipeline of one device, shared by -m bsgs (engine.cpp) and -m address / rmd160 / xpoint
// (address_host.cpp): up to `depth` batches queued on the GPU, the next batch prepared while the GPU scans, each
// collected batch handed back to the search after its successor has been submitted, and a batch whose candidates
// overflowed the device's ring rescanned in two parts (recursively) ahead of new chunks.  Nothing here calls the
// device library: the search supplies it as `Ops`, so the ordering rules are testable on a CPU
// (tests/native/test_pipeline_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <deque>
#include <utility>
#include <vector>

namespace khb {

// What every batch says about its launch.  A batch type derives from this and adds
//   size_t jobs() const;                              the launch's job count
//   void slice(size_t j0, size_t j1, B& out) const;   copy its own vectors for the jobs [j0, j1)
struct BatchRange {
  uint32_t group_begin = 0;   // groups [group_begin, group_begin + group_count) of every job;
  uint32_t group_count = 0;   // 0 = the whole chunk
  bool part = false;          // a rescan part of a batch whose candidate ring overflowed
};

// The two halves of a batch whose candidates overflowed the ring (the caller rescans): by jobs, or
// a single job by its group range, cut at a multiple of gpl (the groups per GPU lane: the alignment a submitted
// group range must have).  `groups`: the groups of a whole chunk.  false: a single job of at most gpl groups
// (cannot be split further).
template <class B>
bool split_batch(const B& b, uint32_t groups, uint32_t gpl, B& lo, B& hi) {
  const size_t n = b.jobs();
  const uint32_t g0 = b.group_begin, gc = b.group_count ? b.group_count : groups;
  auto part = [&](B& o, size_t j0, size_t j1, uint32_t pb, uint32_t pc) {
    b.slice(j0, j1, o);
    o.group_begin = pb;
    o.group_count = pc;
    o.part = true;
  };
  if (n > 1) {
    part(lo, 0, n / 2, g0, gc);
    part(hi, n / 2, n, g0, gc);
    return true;
  }
  if (n == 0 || gc <= gpl) return false;
  const uint32_t half = (gc / 2 + gpl - 1) / gpl * gpl;     // gpl <= half < gc
  part(lo, 0, 1, g0, half);
  part(hi, 0, 1, g0 + half, gc - half);
  return true;
}

// Reserve the device's `depth` submission slots up front (`reserve(depth)`, the library's return code).  Without
// the memory for them (`enomem`) the device runs one batch at a time instead of failing, with one warning.
template <class Reserve, class Warn>
int reserve_depth(int& depth, int enomem, Reserve&& reserve, Warn&& warn) {
  if (depth <= 1) return 0;
  const int rc = reserve(depth);
  if (rc != enomem) return rc;
  depth = 1;
  warn("[W] no device memory for a second submission slot: one batch in flight");
  return 0;
}

constexpr int kRescan = 1;   // Ops::done: the batch overflowed and was split

// Runs the search's launches to the end; returns 0 or the first error.  Ops (each reports its own failure to the
// search; codes are negative):
//   bool stopped();                      the search is over: nothing more is prepared
//   bool fresh(B&);                      claim new chunks and build their centres; false: none left
//   int submit(const B&);                launch; 0 or an error
//   int collect();                       wait for the oldest launch and keep its result; 0 or an error
//   int done(const B&, B& lo, B& hi);    the collected batch and the result kept by collect(): 0 = confirmed,
//                                        kRescan = overflowed, lo and hi are its halves (split_batch), otherwise
//                                        the search's error (an overflow that cannot be split)
//   bool drop_on_stop;                   a prepared batch is dropped, not launched, once stopped() has become true
template <class B, class Ops>
int run_pipeline(Ops& ops, int depth) {
  std::vector<B> ring(depth + 1);   // the batches in flight and the one being prepared or handed back
  std::deque<B> parts;              // rescan parts of overflowed batches, launched before new chunks
  std::deque<int> q;                // ring slots on the GPU, oldest first
  int next = 0;                     // ring slots are used and released in FIFO order
  int rc = 0;                       // the first error: nothing more is prepared or submitted, the queue is drained
  auto take = [&]() { const int i = next; next = (next + 1) % (int)ring.size(); return i; };
  auto prepare = [&](B& b) {
    if (ops.stopped()) return false;
    if (!parts.empty()) {
      b = std::move(parts.front());
      parts.pop_front();
      return true;
    }
    b.group_begin = b.group_count = 0;
    b.part = false;
    return ops.fresh(b);
  };
  auto submit = [&](int i) {
    if (!(rc = ops.submit(ring[i]))) q.push_back(i);
  };
  auto fill = [&]() {               // queue up to `depth` batches
    while (!rc && (int)q.size() < depth && prepare(ring[next])) submit(take());
  };
  fill();
  int pre = -1;                     // prepared, not yet submitted
  while (!q.empty()) {
    if (pre < 0 && !rc && prepare(ring[next])) pre = take();   // overlaps the GPU scan
    const int i = q.front();
    q.pop_front();
    if (const int crc = ops.collect()) {   // keep draining the queue
      if (!rc) rc = crc;
      continue;
    }
    if (pre >= 0 && !rc && !(ops.drop_on_stop && ops.stopped())) submit(pre);
    pre = -1;
    if (rc) continue;
    B lo, hi;
    const int d = ops.done(ring[i], lo, hi);   // overlaps the GPU scan of the queue
    if (d == kRescan) {
      parts.push_front(std::move(hi));
      parts.push_front(std::move(lo));
    } else if (d) {
      rc = d;
    }
    // The queue ran empty with rescan parts pending (they were cut from the last launch in flight): launch up to
    // `depth` of them.  How many parts are queued at once is scheduling only: parts are taken lo before hi, ahead of
    // new chunks, and launches are collected in submission order, so no result, statistic or on_found order depends
    // on it.
    if (q.empty()) fill();
  }
  return rc;
}

}  // namespace khb
