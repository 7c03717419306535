// job.hpp — the state of one style 1 job (from_file, optflow.cpp) and what its two kinds of
// workers share: the per-pair worker (pair_worker.cpp) and the strip-batch worker
// (strip_worker.cpp), one thread each per GPU and pair in flight.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "config.hpp"
#include "decode_pool.hpp"
#include "device.hpp"

namespace ofcli {

struct PairResult {
  bool done = false;
  bool ok = false;
  std::vector<Value> pms;   // point-match records (random_points)
  Value stats;
};

struct JobState {
  Value &args;
  Value images;         // args["images"]
  const size_t n;       // pairs
  const bool plan_only;
  const bool debug, skip_existing;
  std::vector<int> devices;
  DecodePool &pool;
  std::vector<PairResult> results;
  std::vector<Value> plans;   // --plan: one entry per pair
  std::atomic<int> hard_error{0};   // a GPU could not be opened: the job ends with status 1

  // the pairs the per-pair workers solve (all of them unless strip batching takes some), taken
  // `chunk` at a time through `next`
  std::vector<size_t> todo;
  std::atomic<size_t> next{0};
  size_t chunk = 1;

  // the strip batch workers' pairs, in order, taken `bchunk` at a time through `bnext`; a pair
  // that turns out not to fit a batch is marked `deferred` and joins `todo` afterwards
  std::vector<size_t> batched;
  std::vector<char> batch_ok;   // the pair goes to the strip batch workers (--plan reports it)
  std::vector<char> deferred;
  std::atomic<size_t> bnext{0};
  size_t bchunk = 0;
  std::vector<std::string> roi_keys;   // sorted, like solve_rois' std::map (optflow.cpp:339)
  int roi_top = 0, roi_bottom = 0;

  JobState(Value &a, bool plan, DecodePool &p)
      : args(a), images(a["images"]), n(images.size()), plan_only(plan), debug(a.get("debug", false).asBool()),
        skip_existing(a.get("skip_existing", false).asBool()), pool(p), results(n), plans(n), batch_ok(n, 0),
        deferred(n, 0) {}
};

void run_pair_worker(JobState &job, int device);    // pair_worker.cpp
void run_strip_worker(JobState &job, int device);   // strip_worker.cpp
// --plan: the entry of one pair (optflow.cpp); w0 x h0 is the pre-scaled frame0
Value plan_entry(const JobState &job, size_t i, const Value &im, const PairConfig &cfg, const Value &rois, int w0,
                 int h0);
int from_list(Value &args, bool plan_only);   // "style": 2 (from_list.cpp)

// Per-stage host timing of a job (the build-only "timing_json" key, tools/cli_e2e.py): where
// a strip job's wall time goes -- band reads on the decode pool, and per batch worker the
// wait for its chunk's bands, packing, upload, solve, point sampling, flow read-back and
// output writes.  Seconds of each thread's own clock, summed.
inline std::mutex g_stage_mutex;
inline Value g_stage_workers;   // one object per batch worker

// A worker's walk over a shared list of m entries in chunks, one chunk ahead of itself: queue(s)
// is told of a chunk starting at s when it becomes the next one, so its slices decode while
// the current chunk is solved.
struct ChunkWalk {
  std::atomic<size_t> &next;
  const size_t chunk, m;
  size_t start = 0, next_start = 0;
  template <class Queue>
  ChunkWalk(std::atomic<size_t> &n, size_t c, size_t m_, Queue queue) : next(n), chunk(c), m(m_) {
    take_next(queue);
  }
  template <class Queue>
  bool advance(Queue queue) {   // false: the list is used up
    start = next_start;
    if (start >= m) return false;
    take_next(queue);
    return true;
  }
  size_t end() const { return std::min(m, start + chunk); }
  size_t next_end() const { return std::min(m, next_start + chunk); }

 private:
  template <class Queue>
  void take_next(Queue queue) {
    next_start = next.fetch_add(chunk);
    if (next_start < m) queue(next_start);
  }
};

inline bool file_exists(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}
// "skip_existing": the flow files of every ROI key of a pair are there already
template <class Keys>
bool outputs_exist(const std::string &output, const Keys &keys) {
  bool all = true;
  for (const auto &key : keys) {
    const std::string base = output + roi_suffix(key);
    all = all && file_exists(base + "_x.tiff") && file_exists(base + "_y.tiff");
  }
  return all;
}

// move_pm (optflow.cpp:574-593)
inline Value move_pm(Value &im) {
  Value single;
  single["pGroupId"] = im["pGroupId"];
  single["pId"] = im["pId"];
  single["qGroupId"] = im["qGroupId"];
  single["qId"] = im["qId"];
  single["matches"] = im["point_matches"];
  im["point_matches"].clear();
  im["point_matches"] = Value();
  return single;
}

// Test hook: OPTFLOW_INJECT_FAULT="i,j,..." makes the first attempt of those pairs fail as
// a device error would (before any device work), to exercise the workers' recovery.
inline bool inject_fault(size_t pair) {
  static const std::vector<size_t> list = [] {
    std::vector<size_t> v;
    if (const char *e = getenv("OPTFLOW_INJECT_FAULT"))
      for (const char *q = e; *q;) {
        char *end;
        const unsigned long x = strtoul(q, &end, 10);
        if (end == q) break;
        v.push_back(x);
        q = *end ? end + 1 : end;
      }
    return v;
  }();
  return std::find(list.begin(), list.end(), pair) != list.end();
}

// failure recovery: work that failed on a device error is done once more on a fresh
// context (engine ctx, stream and buffers rebuilt)
inline bool rebuild_device(DeviceCtx &dc, int device, std::string &err) {
  dc.close();
  std::string e2;
  if (dc.open(device, e2)) return true;
  err = "device context could not be rebuilt: " + e2;
  return false;
}
// a worker's own context, or the job's hard error
inline bool open_or_hard_error(DeviceCtx &dc, int device, JobState &job) {
  std::string err;
  if (dc.open(device, err)) return true;
  std::lock_guard<std::mutex> lk(g_io_mutex);
  fprintf(stderr, "Error: cannot use GPU %d: %s\n", device, err.c_str());
  dc.close();
  job.hard_error = 1;
  return false;
}

}  // namespace ofcli
