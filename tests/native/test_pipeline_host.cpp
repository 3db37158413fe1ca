// host/pipeline.hpp (run_pipeline, split_batch) driven by a scripted fake device: the ordering rules that the GPU
// tests cannot see.  No GPU, no libkhbsgs.  Prints "ok" and exits 0 only if every case holds.
#include "../../keyhuntm1cpu_amd/csrc/host/pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <deque>
#include <map>
#include <tuple>
#include <vector>

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      printf("FAIL %s (line %d): %s\n", g_case, __LINE__, #c);                \
      ++g_failed;                                                             \
    }                                                                         \
  } while (0)

struct FBatch : khb::BatchRange {
  int id = -1;             // the new batch this is, or is a part of
  int tag = -1;            // of a rescan part: 2 * rescan number (lo), + 1 (hi)
  std::vector<int> job;    // job numbers within the new batch
  size_t jobs() const { return job.size(); }
  void slice(size_t j0, size_t j1, FBatch& o) const {
    o.id = id;
    o.job.assign(job.begin() + j0, job.begin() + j1);
  }
};

struct Event {
  char what;    // 'p' fresh batch prepared, 's' submit, 'c' collect, 'd' done
  FBatch b;     // 'c': the launch the fake device finished
};

struct FakeOps {
  // the script
  int n_batches = 8, jobs_per_batch = 2;
  uint32_t groups = 4, gpl = 2;
  uint64_t threshold = ~0ull;            // a launch of more jobs x groups overflows
  bool drop_on_stop = false;
  int fail_submit = -1, fail_submit_rc = 0;         // the submit call (from 0) that fails
  std::map<int, int> fail_collect;                  // collect call (from 0) -> its error
  int stop_in_collect = -1;                         // the collect call during which the caller's stop is raised
  // the record
  std::vector<Event> log;
  std::deque<FBatch> flying;
  FBatch last;                                      // the launch collected last
  size_t max_flying = 0;
  int fresh_calls = 0, submits = 0, collects = 0, rescans = 0, parts_pending = 0;
  bool stop = false, fresh_with_parts_pending = false;

  uint64_t work(const FBatch& b) const { return (uint64_t)b.jobs() * (b.group_count ? b.group_count : groups); }
  bool stopped() { return stop; }
  bool fresh(FBatch& b) {
    if (fresh_calls >= n_batches) return false;
    if (parts_pending) fresh_with_parts_pending = true;
    b.id = fresh_calls++;
    b.tag = -1;
    b.job.clear();
    for (int j = 0; j < jobs_per_batch; ++j) b.job.push_back(j);
    log.push_back({'p', b});
    return true;
  }
  int submit(const FBatch& b) {
    if (submits++ == fail_submit) return fail_submit_rc;
    if (b.part) --parts_pending;
    log.push_back({'s', b});
    flying.push_back(b);
    max_flying = std::max(max_flying, flying.size());
    return 0;
  }
  int collect() {
    CHECK(!flying.empty());
    if (flying.empty()) return -99;
    last = flying.front();
    flying.pop_front();
    log.push_back({'c', last});
    const int n = collects++;
    if (n == stop_in_collect) stop = true;
    return fail_collect.count(n) ? fail_collect[n] : 0;
  }
  int done(const FBatch& b, FBatch& lo, FBatch& hi) {
    CHECK(b.id == last.id && b.job == last.job && b.group_begin == last.group_begin &&
          b.group_count == last.group_count);        // the batch handed back is the launch collected last
    log.push_back({'d', b});
    if (work(b) <= threshold) return 0;
    if (!khb::split_batch(b, groups, gpl, lo, hi)) return -100;
    lo.tag = 2 * rescans;
    hi.tag = 2 * rescans + 1;
    ++rescans;
    parts_pending += 2;
    return khb::kRescan;
  }

  // positions in the log
  std::vector<int> ids(char what) const {
    std::vector<int> v;
    for (const Event& e : log)
      if (e.what == what) v.push_back(e.b.id);
    return v;
  }
  size_t count(char what) const { return ids(what).size(); }
  size_t last_pos(char what) const {
    size_t p = 0;
    for (size_t i = 0; i < log.size(); ++i)
      if (log[i].what == what) p = i + 1;
    return p;     // 0: none
  }
};

static std::vector<int> iota(int n) {
  std::vector<int> v;
  for (int i = 0; i < n; ++i) v.push_back(i);
  return v;
}

static void case_no_overflow(int depth) {
  g_case = depth == 1 ? "no overflow, depth 1" : "no overflow, depth 2";
  FakeOps o;
  CHECK(khb::run_pipeline<FBatch>(o, depth) == 0);
  CHECK(o.ids('p') == iota(8));
  CHECK(o.ids('s') == iota(8));          // submits in prepare order
  CHECK(o.ids('c') == iota(8));          // collects in submit order
  CHECK(o.ids('d') == iota(8));          // every batch handed to done exactly once
  CHECK(o.max_flying == (size_t)depth);
  CHECK(o.flying.empty());
  // the batch prepared during launch k's scan (k + depth) is submitted before done(k)
  for (int k = 0; k + depth < 8; ++k) {
    size_t s = 0, d = 0;
    for (size_t i = 0; i < o.log.size(); ++i) {
      if (o.log[i].what == 's' && o.log[i].b.id == k + depth) s = i;
      if (o.log[i].what == 'd' && o.log[i].b.id == k) d = i;
    }
    CHECK(s < d);
  }
}

static void case_overflow(int depth) {
  g_case = depth == 1 ? "overflow, depth 1" : "overflow, depth 2";
  FakeOps o;
  o.n_batches = 3;
  o.jobs_per_batch = 4;
  o.groups = 8;
  o.threshold = 4;
  CHECK(khb::run_pipeline<FBatch>(o, depth) == 0);
  CHECK(o.flying.empty() && o.parts_pending == 0);
  // over all launches that did not overflow, each (batch, job, group) exactly once
  std::map<std::tuple<int, int, uint32_t>, int> cover;
  int overflowed = 0;
  std::map<int, size_t> tag_pos;
  for (size_t i = 0; i < o.log.size(); ++i) {
    const Event& e = o.log[i];
    if (e.what != 's') continue;
    const uint32_t gc = e.b.group_count ? e.b.group_count : o.groups;
    CHECK(e.b.group_begin % o.gpl == 0 && (e.b.group_begin + gc) % o.gpl == 0);   // every cut a multiple of gpl
    CHECK(e.b.group_begin + gc <= o.groups);
    CHECK(e.b.part == (e.b.tag >= 0));
    if (e.b.tag >= 0) {
      CHECK(!tag_pos.count(e.b.tag));
      tag_pos[e.b.tag] = i;
    }
    if (o.work(e.b) > o.threshold) {
      ++overflowed;
      continue;
    }
    for (int j : e.b.job)
      for (uint32_t g = e.b.group_begin; g < e.b.group_begin + gc; ++g) cover[{e.b.id, j, g}]++;
  }
  // the halves of an overflowed launch go to the front of the pending parts, lo first, and parts are launched from
  // the front
  std::deque<int> pending;
  int rescan = 0;
  for (const Event& e : o.log) {
    if (e.what == 'd' && o.work(e.b) > o.threshold) {
      pending.push_front(2 * rescan + 1);
      pending.push_front(2 * rescan);
      ++rescan;
    } else if (e.what == 's' && e.b.part) {
      CHECK(!pending.empty() && pending.front() == e.b.tag);
      if (!pending.empty()) pending.pop_front();
    }
  }
  CHECK(cover.size() == 3u * 4u * 8u);
  for (const auto& kv : cover) CHECK(kv.second == 1);
  CHECK(overflowed == o.rescans);
  // 4 x 8 -> 2 x 8 -> 1 x 8 -> 1 x 4: 1 + 2 + 4 overflowed launches a batch, down to group ranges
  CHECK(o.rescans == 3 * 7);
  CHECK(tag_pos.size() == 2u * o.rescans);
  for (int r = 0; r < o.rescans; ++r) CHECK(tag_pos[2 * r] < tag_pos[2 * r + 1]);   // lo runs before hi
  CHECK(!o.fresh_with_parts_pending);   // every part is launched before any batch prepared after the overflow
  CHECK(o.count('c') == o.count('s') && o.count('d') == o.count('s'));
  CHECK(o.max_flying <= (size_t)depth);
}

static void case_unsplittable() {
  g_case = "unsplittable";
  FakeOps o;
  o.n_batches = 4;
  o.jobs_per_batch = 1;
  o.groups = 2;          // one job of gpl groups
  o.threshold = 1;
  CHECK(khb::run_pipeline<FBatch>(o, 2) == -100);     // the search's failure code
  CHECK(o.flying.empty());                            // launches in flight are still collected
  CHECK(o.count('s') == 3 && o.count('c') == 3);      // two queued and the one prepared during the first scan
  CHECK(o.count('d') == 1 && o.rescans == 0);
  CHECK(o.last_pos('s') < o.last_pos('d') && o.last_pos('p') < o.last_pos('d'));   // nothing submitted afterwards
}

static void case_collect_error() {
  g_case = "collect error";
  FakeOps o;
  o.fail_collect[1] = -4;      // the second of the two launches in flight
  o.fail_collect[2] = -7;      // a later error does not replace the first
  CHECK(khb::run_pipeline<FBatch>(o, 2) == -4);
  CHECK(o.flying.empty());                            // the queue is drained
  CHECK(o.ids('s') == iota(3) && o.ids('c') == iota(3));
  CHECK(o.ids('d') == iota(1));
  size_t failed_at = 0, n = 0;
  for (size_t i = 0; i < o.log.size(); ++i)
    if (o.log[i].what == 'c' && n++ == 1) failed_at = i + 1;
  CHECK(o.last_pos('p') < failed_at && o.last_pos('s') < failed_at && o.last_pos('d') < failed_at);
}

static void case_submit_error() {
  g_case = "submit error";
  FakeOps o;
  o.fail_submit = 2;           // the batch prepared during the first scan
  o.fail_submit_rc = -5;
  CHECK(khb::run_pipeline<FBatch>(o, 2) == -5);
  CHECK(o.flying.empty());                            // the queue is drained
  CHECK(o.submits == 3 && o.ids('s') == iota(2) && o.ids('c') == iota(2));
  CHECK(o.ids('p') == iota(3));                       // nothing is prepared afterwards
  CHECK(o.count('d') == 0);
}

static void case_stop(bool drop) {
  g_case = drop ? "stop, prepared batch dropped" : "stop, prepared batch submitted";
  FakeOps o;
  o.drop_on_stop = drop;
  o.stop_in_collect = 0;       // batch 2 is prepared before this collect and would be submitted after it
  CHECK(khb::run_pipeline<FBatch>(o, 2) == 0);
  CHECK(o.flying.empty());
  CHECK(o.ids('p') == iota(3));
  const std::vector<int> ran = iota(drop ? 2 : 3);
  CHECK(o.ids('s') == ran && o.ids('c') == ran && o.ids('d') == ran);
}

int main() {
  case_no_overflow(1);
  case_no_overflow(2);
  case_overflow(1);
  case_overflow(2);
  case_unsplittable();
  case_collect_error();
  case_submit_error();
  case_stop(true);
  case_stop(false);
  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("ok\n");
  return 0;
}
