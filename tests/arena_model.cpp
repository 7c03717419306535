// csrc/tvl1_arena.hpp on a CPU (tests/test_arena_cpu.py builds this with ASan + UBSan): a second
// backend for the memory lifecycle.  The model device keeps a queue of operations per stream,
// each tagged with the block it touches; nothing runs until the script completes an event (its
// stream drains up to the record, and so does whatever that stream waited for) or something
// drains the device, as a free does.  Addresses and handles are numbers: nothing is dereferenced.
// After every step the driver checks what the header promises; a broken promise prints
// "FAIL <script>: <what>" and the program exits 1.  Each script that passes prints "ok <script>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tvl1_arena.hpp"

using namespace tvl1k;

static const char *g_script = "";
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      printf("FAIL %s: ", g_script);          \
      printf(__VA_ARGS__);                    \
      printf(" (line %d)\n", __LINE__);       \
      exit(1);                                \
    }                                         \
  } while (0)

enum Kind { kFill, kUse, kRecord, kWait };
struct Op {
  int id;
  Kind kind;
  char *block;          // kFill, kUse
  int event;            // kRecord
  int wstream, wop;     // kWait: the record it waits for
};

struct Model {
  using Stream = int;
  using Event = int;
  static constexpr int kErr = 7, kNoMem = 2, kNotReady = 600;

  std::map<int, std::deque<Op>> q;       // pending operations per stream
  std::set<int> dead;                    // destroyed streams
  int next_op = 1, next_event = 1;
  uintptr_t next_addr = 0x10000;
  std::set<int> executed;
  struct Ev { int stream = -1, op = 0; };   // its latest record (op 0: never recorded)
  std::map<int, Ev> events;              // live events
  std::map<char *, size_t> live;         // live allocations
  std::set<char *> freed;
  std::map<char *, int> fill_op;         // the zero fill of a live allocation
  std::map<char *, std::vector<int>> retired_events;   // filled in by the driver after a reserve
  // injected failures
  int fail_mallocs = 0;
  int fail_create = 0;                   // the next n creates
  int fail_record_on = -1;               // the next record on this stream inside a reserve (a failed
                                         // record is ignored for good only where nothing is ordered by it)
  bool in_reserve = false;
  // what the current call may do
  bool frees_need_done_events = true;    // off in the ENOMEM retry and in release_all
  // counters
  int n_malloc = 0, n_free = 0, n_enqueued = 0, n_wait = 0, n_clear = 0;
  size_t last_malloc_bytes = 0;

  bool done(int op) const { return op == 0 || executed.count(op) != 0; }
  void drain(int s, int upto) {
    auto &d = q[s];
    while (!d.empty() && d.front().id <= upto) {
      const Op op = d.front();
      if (op.kind == kWait && !done(op.wop)) drain(op.wstream, op.wop);
      executed.insert(op.id);
      d.pop_front();
    }
  }
  void drain_all() {
    for (auto &kv : q) drain(kv.first, next_op);
  }
  // must operation `f` have run before a new operation at the end of stream s can?
  bool precedes(int f, int s) const {
    if (done(f)) return true;
    std::set<std::pair<int, int>> seen;
    return reach(f, s, next_op, seen);
  }
  bool reach(int f, int s, int upto, std::set<std::pair<int, int>> &seen) const {
    if (!seen.insert({s, upto}).second) return false;
    const auto it = q.find(s);
    if (it == q.end()) return false;
    for (const Op &op : it->second) {
      if (op.id > upto) break;
      if (op.id == f) return true;
      if (op.kind == kWait && !done(op.wop) && reach(f, op.wstream, op.wop, seen)) return true;
    }
    return false;
  }
  int push(int s, Op op) {
    op.id = next_op++;
    q[s].push_back(op);
    ++n_enqueued;
    return op.id;
  }
  int use(int s, char *block) {   // the driver's kernel
    CHECK(live.count(block), "a kernel on a block that is not allocated");
    return push(s, Op{0, kUse, block, 0, 0, 0});
  }
  void destroy_stream(int s) {
    drain(s, next_op);
    dead.insert(s);
  }

  // ---- the backend interface
  int malloc(char **p, size_t n) {
    ++n_malloc;
    last_malloc_bytes = n;
    if (fail_mallocs > 0) {
      --fail_mallocs;
      frees_need_done_events = false;   // the retry may drop everything
      return kNoMem;
    }
    *p = reinterpret_cast<char *>(next_addr);
    next_addr += 0x10000;
    live[*p] = n;
    return 0;
  }
  int free(char *p) {
    ++n_free;
    CHECK(!freed.count(p), "block %p freed twice", (void *)p);
    CHECK(live.count(p), "free of %p, which was never allocated", (void *)p);
    if (frees_need_done_events && retired_events.count(p))
      for (int e : retired_events[p])
        CHECK(events.count(e) && done(events[e].op), "block %p freed before its event %d was done", (void *)p, e);
    drain_all();   // as hipFree does
    live.erase(p);
    fill_op.erase(p);
    retired_events.erase(p);
    freed.insert(p);
    return 0;
  }
  int memset_async(char *p, int, size_t n, int s) {
    CHECK(live.count(p) && live[p] == n, "zero fill of %zu bytes on a block of another size", n);
    fill_op[p] = push(s, Op{0, kFill, p, 0, 0, 0});
    return 0;
  }
  int event_create(int *e) {
    if (fail_create > 0) {
      --fail_create;
      return kErr;
    }
    *e = next_event++;
    events[*e] = Ev{};
    return 0;
  }
  int event_record(int e, int s) {
    CHECK(events.count(e), "record of event %d, which is not live", e);
    if (dead.count(s)) return kErr;
    if (in_reserve && fail_record_on == s) {
      fail_record_on = -1;
      return kErr;
    }
    events[e] = Ev{s, push(s, Op{0, kRecord, nullptr, e, 0, 0})};
    return 0;
  }
  int event_query(int e) {
    CHECK(events.count(e), "query of event %d, which is not live", e);
    return done(events[e].op) ? 0 : kNotReady;
  }
  int event_sync(int e) {
    CHECK(events.count(e), "sync of event %d, which is not live", e);
    if (!done(events[e].op)) drain(events[e].stream, events[e].op);
    return 0;
  }
  int event_destroy(int e) {
    if (e == 0) return 0;
    CHECK(events.count(e), "event %d destroyed twice", e);
    events.erase(e);
    return 0;
  }
  int stream_wait(int s, int e) {
    CHECK(events.count(e), "wait for event %d, which is not live", e);
    if (dead.count(s)) return kErr;
    ++n_wait;
    push(s, Op{0, kWait, nullptr, 0, events[e].stream, events[e].op});
    return 0;
  }
  void clear_error() { ++n_clear; }
  const char *error_string(int e) { return e == kNoMem ? "out of memory" : "model error"; }
};

// One ctx: the arena over the model, three blocks, and the checks around every call.
struct Ctx {
  static constexpr int kBlocks = 3;
  Arena<Model> a;
  Block blk[kBlocks];
  int last_op = 0, last_stream = -1;   // the ctx's latest kernel
  int entered = -1;                    // the stream of its latest call

  Ctx() {
    a.own = 0;
    CHECK(a.init(), "init failed");
  }
  Model &m() { return a.dev; }

  // an entry point: enter, reserve, then a kernel on the block
  tvl1_status call(int s, int b, size_t need, size_t floor = 0) {
    Model &d = m();
    const int enq0 = d.n_enqueued;
    d.frees_need_done_events = true;
    a.enter(s);
    if (entered == s || entered < 0)
      CHECK(d.n_enqueued == enq0, "enter on an unchanged stream enqueued %d operations", d.n_enqueued - enq0);
    entered = s;
    const Block before = blk[b];
    const int enq1 = d.n_enqueued, mal1 = d.n_malloc, free1 = d.n_free;
    const size_t held = a.retired.size();
    d.in_reserve = true;
    const tvl1_status r = a.reserve(blk[b], need, s, floor);
    d.in_reserve = false;
    d.frees_need_done_events = true;
    CHECK(a.retired.size() <= kRetiredMax, "%zu blocks retired after a reserve", a.retired.size());
    for (const auto &rt : a.retired) d.retired_events[rt.p] = rt.done;
    if (need <= before.bytes) {
      CHECK(r == TVL1_OK && blk[b].p == before.p && blk[b].bytes == before.bytes, "a reserve that fits changed the block");
      CHECK(d.n_enqueued == enq1 && d.n_malloc == mal1 && d.n_free == free1 && a.retired.size() == held,
            "a reserve that fits enqueued, allocated or freed");
    } else if (r == TVL1_OK) {
      CHECK(blk[b].p && blk[b].p != before.p && blk[b].bytes == std::max(need, floor), "grown block of the wrong size");
      CHECK(d.live.count(blk[b].p) && d.live[blk[b].p] == blk[b].bytes, "grown block is not a live allocation");
      CHECK(d.fill_op.count(blk[b].p), "grown block was not zero-filled");
    } else {
      CHECK(r == TVL1_ENOMEM && !blk[b].p && blk[b].bytes == 0, "a failed reserve left the block set");
    }
    for (int k = 0; k < kBlocks; ++k)
      if (blk[k].p) CHECK(d.live.count(blk[k].p), "block %d points at freed memory", k);
    if (r != TVL1_OK || !blk[b].p) return r;
    // the kernel: behind the ctx's previous kernel, and behind the block's zero fill
    if (last_op)
      CHECK(d.precedes(last_op, s), "stream %d does not wait for stream %d's last operation", s, last_stream);
    CHECK(d.precedes(d.fill_op[blk[b].p], s), "a kernel on stream %d may run before the block's zero fill", s);
    last_op = d.use(s, blk[b].p);
    last_stream = s;
    return r;
  }
  void complete(int event) { m().event_sync(event); }
  void destroy() {
    m().frees_need_done_events = false;
    a.release_all(blk[0], blk[1], blk[2]);
    CHECK(m().live.empty(), "%zu allocations leaked", m().live.size());
    CHECK(m().events.empty(), "%zu events leaked", m().events.size());
    CHECK(a.retired.empty() && !blk[0].p && !blk[1].p && !blk[2].p, "release_all left a block");
  }
};

static void ok(const char *name) { printf("ok %s\n", name); }
#define SCRIPT(name) static void name() { g_script = #name;
#define END ok(g_script); }

SCRIPT(noop_reserve)
  Ctx c;
  CHECK(c.call(1, 0, 1000) == TVL1_OK, "first reserve");
  const int mal = c.m().n_malloc;
  CHECK(c.call(1, 0, 1000) == TVL1_OK && c.call(1, 0, 10) == TVL1_OK && c.call(1, 0, 0) == TVL1_OK, "fits");
  CHECK(c.m().n_malloc == mal, "a fitting reserve allocated");   // (call() checks the rest)
  CHECK(c.call(1, 1, 0) == TVL1_OK && !c.blk[1].p, "an empty reserve of an empty block allocated");
  c.destroy();
END

SCRIPT(floor_applies_to_growth_only)
  Ctx c;
  CHECK(c.call(1, 0, 10, 64 << 10) == TVL1_OK && c.blk[0].bytes == (64 << 10), "floor");
  CHECK(c.call(1, 0, (64 << 10) + 1, 64 << 10) == TVL1_OK && c.blk[0].bytes == (64 << 10) + 1, "above the floor");
  c.destroy();
END

SCRIPT(one_stream_enqueues_no_wait)
  Ctx c;   // the own stream throughout: not even the zero fill needs an event
  for (size_t n = 100; n < 2000; n += 300) CHECK(c.call(0, 0, n) == TVL1_OK, "reserve");
  CHECK(c.m().n_wait == 0, "%d stream waits on a ctx that stayed on its own stream", c.m().n_wait);
  Ctx d;   // a caller's stream: one wait per growth (the zero fill), none for a call that fits
  CHECK(d.call(3, 0, 100) == TVL1_OK && d.call(3, 0, 50) == TVL1_OK && d.call(3, 1, 70) == TVL1_OK, "reserve");
  CHECK(d.m().n_wait == 2, "%d stream waits for two growths on one stream", d.m().n_wait);
  c.destroy();
  d.destroy();
END

SCRIPT(stream_switch_waits_for_the_previous_stream)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK, "on stream 1");
  const int w = c.m().n_wait;
  CHECK(c.call(2, 0, 100) == TVL1_OK, "on stream 2");   // call() checks the order
  CHECK(c.m().n_wait == w + 1, "a switch of streams enqueued %d waits", c.m().n_wait - w);
  CHECK(c.call(2, 0, 100) == TVL1_OK && c.m().n_wait == w + 1, "staying on stream 2 enqueued a wait");
  c.destroy();
END

SCRIPT(zero_fill_orders_the_first_use)
  Ctx c;
  CHECK(c.call(4, 0, 100) == TVL1_OK, "grow");
  // the fill is on the own stream and pending; stream 4's queue: the wait, then the kernel
  const auto &q4 = c.m().q[4];
  CHECK(q4.size() == 2 && q4[0].kind == kWait && q4[1].kind == kUse, "stream 4 holds %zu operations", q4.size());
  CHECK(!c.m().done(c.m().fill_op[c.blk[0].p]), "the fill ran by itself");
  c.destroy();
END

SCRIPT(retired_bound_under_alternating_growth)
  Ctx c;
  size_t n = 100;
  for (int i = 0; i < 12; ++i, n += 100) {   // nothing ever completes by itself
    CHECK(c.call(1 + i % 2, i % 3, n) == TVL1_OK, "grow");
    CHECK(c.a.retired.size() <= kRetiredMax, "bound");
    // two are held without a wait; the third is waited for, and its free drains the device, so
    // the others' events are done too
    CHECK(c.a.retired.size() == (size_t)(i < 3 ? 0 : (i - 3) % 3 + 1) % 3, "%zu retired after growth %d",
          c.a.retired.size(), i);
  }
  c.destroy();
END

SCRIPT(reap_frees_once_every_event_is_done)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK && c.call(2, 0, 200) == TVL1_OK, "grow");
  CHECK(c.a.retired.size() == 1, "retired");
  const std::vector<int> ev = c.a.retired[0].done;
  CHECK(ev.size() == 3, "%zu events for streams 1, 2 and own", ev.size());
  const int frees = c.m().n_free;
  c.complete(ev[0]);
  c.complete(ev[1]);
  CHECK(c.call(2, 0, 10) == TVL1_OK && c.m().n_free == frees, "freed with an event pending");
  c.complete(ev[2]);
  CHECK(c.call(2, 0, 10) == TVL1_OK && c.m().n_free == frees + 1 && c.a.retired.empty(), "not freed with every event done");
  c.destroy();
END

SCRIPT(enomem_with_retired_blocks)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK && c.call(1, 0, 200) == TVL1_OK && c.call(1, 1, 50) == TVL1_OK &&
        c.call(1, 1, 90) == TVL1_OK, "grow");
  CHECK(c.a.retired.size() == 2, "two retired");
  const int mal = c.m().n_malloc, frees = c.m().n_free;
  c.m().fail_mallocs = 1;
  CHECK(c.call(1, 2, 300) == TVL1_OK, "the retry did not succeed");
  CHECK(c.m().n_malloc == mal + 2, "%d allocations tried", c.m().n_malloc - mal);
  CHECK(c.m().n_free == frees + 2 && c.a.retired.empty(), "the retired blocks were not all freed");
  c.destroy();
END

SCRIPT(enomem_without_retired_blocks)
  Ctx c;
  const int mal = c.m().n_malloc;
  c.m().fail_mallocs = 1;
  CHECK(c.call(1, 0, 5000) == TVL1_ENOMEM, "status");   // call() checks the block is empty
  CHECK(c.m().n_malloc == mal + 1, "retried with nothing to release");
  CHECK(!strcmp(c.a.err, "hipMalloc(5000) failed: out of memory"), "text: %s", c.a.err);
  CHECK(c.call(1, 0, 1000) == TVL1_OK && c.blk[0].bytes == 1000, "a later smaller reserve");
  // growth of a live block that fails twice: the old block is retired and then dropped, not leaked
  c.m().fail_mallocs = 2;
  CHECK(c.call(1, 0, 9000) == TVL1_ENOMEM && c.a.retired.empty(), "status of the second failure");
  CHECK(c.m().live.empty(), "%zu allocations held after the failure", c.m().live.size());
  CHECK(c.call(1, 0, 100) == TVL1_OK, "a reserve after it");
  c.destroy();
END

SCRIPT(destroyed_stream)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK && c.call(2, 0, 100) == TVL1_OK, "streams 1 and 2");
  c.m().destroy_stream(1);
  const int clears = c.m().n_clear;
  CHECK(c.call(2, 0, 200) == TVL1_OK, "grow");
  CHECK(c.a.retired.size() == 1 && c.a.retired[0].done.size() == 2, "events of stream 2 and own only");
  CHECK(c.m().n_clear > clears, "the failed record's error was not cleared");
  CHECK(c.m().events.size() == 2 + 2, "the failed record's event was not destroyed");
  for (int e : std::vector<int>(c.a.retired[0].done)) c.complete(e);
  CHECK(c.call(2, 0, 10) == TVL1_OK && c.a.retired.empty(), "not reaped once the other events were done");
  // the previous stream destroyed before a switch: no wait, nothing hangs
  c.m().destroy_stream(2);
  CHECK(c.call(3, 0, 10) == TVL1_OK, "after the previous stream was destroyed");
  c.destroy();
END

SCRIPT(failed_event_create_and_record)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK && c.call(2, 0, 100) == TVL1_OK, "streams 1 and 2");
  c.m().fail_create = 1;      // the first of the three events
  c.m().fail_record_on = 2;   // and the record on stream 2
  CHECK(c.call(2, 0, 200) == TVL1_OK, "grow");
  CHECK(c.a.retired.size() == 1 && c.a.retired[0].done.size() == 1, "%zu events kept", c.a.retired[0].done.size());
  c.destroy();
END

SCRIPT(stream_window)
  Ctx c;
  for (int s = 1; s <= 8; ++s) CHECK(c.call(s, 0, 100) == TVL1_OK, "note");
  CHECK(c.a.streams.size() == 8 && c.a.streams.front() == 1 && c.a.streams.back() == 8, "eight streams");
  CHECK(c.call(2, 0, 100) == TVL1_OK, "re-note");
  CHECK(c.a.streams.size() == 8 && c.a.streams.back() == 2 && c.a.streams[1] == 3, "re-noting moves to the end");
  CHECK(c.call(9, 0, 100) == TVL1_OK, "ninth");
  CHECK(c.a.streams.size() == 8 && c.a.streams.front() == 3 && c.a.streams.back() == 9, "the ninth evicts the oldest");
  CHECK(c.call(9, 0, 200) == TVL1_OK, "grow");   // own joins: the oldest of the eight goes
  CHECK(c.a.retired[0].done.size() == 8, "%zu events at retirement", c.a.retired[0].done.size());
  c.destroy();
END

SCRIPT(release_all_with_history)
  Ctx c;
  CHECK(c.call(1, 0, 100) == TVL1_OK && c.call(2, 0, 200) == TVL1_OK && c.call(3, 1, 50) == TVL1_OK &&
        c.call(1, 1, 90) == TVL1_OK, "grow");
  c.m().fail_mallocs = 2;
  CHECK(c.call(2, 2, 70) == TVL1_ENOMEM, "a failed allocation");
  CHECK(c.call(2, 2, 30) == TVL1_OK && c.call(3, 2, 60) == TVL1_OK, "grow again");
  CHECK(!c.a.retired.empty(), "nothing retired to release");
  c.destroy();   // checks that nothing is left
  Ctx d;         // and a ctx that never allocated
  d.destroy();
END

// seeded random sequences of enter + reserve, complete event, destroy stream and injected failures,
// over 3 blocks and 10 streams
static void random_sequences(int seeds, int steps) {
  g_script = "random_sequences";
  for (int seed = 1; seed <= seeds; ++seed) {
    std::mt19937 rng((unsigned)seed);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Ctx c;
    std::vector<int> alive = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};   // 0 is the own stream (never destroyed)
    for (int i = 0; i < steps; ++i) {
      const int what = pick(100);
      if (what < 60) {
        const int s = alive[(size_t)pick((int)alive.size())], b = pick(Ctx::kBlocks);
        const size_t have = c.blk[b].bytes;
        const size_t need = pick(3) ? have + 1 + (size_t)pick(500) : (size_t)pick((int)have + 1);
        if (pick(12) == 0) c.m().fail_mallocs = 1 + pick(2);
        if (pick(10) == 0) c.m().fail_create = 1 + pick(2);
        // (not on the own stream: a zero fill whose order event cannot be recorded is TVL1_EHIP)
        if (pick(10) == 0) c.m().fail_record_on = alive[1 + (size_t)pick((int)alive.size() - 1)];
        const tvl1_status r = c.call(s, b, need, pick(2) ? 256 : 0);
        CHECK(r == TVL1_OK || r == TVL1_ENOMEM, "seed %d step %d: status %d", seed, i, (int)r);
        c.m().fail_mallocs = c.m().fail_create = 0;
        c.m().fail_record_on = -1;
      } else if (what < 92) {   // an event completes: a retired block's, or whatever a stream's queue holds
        if (!c.a.retired.empty() && pick(2)) {
          const auto &r = c.a.retired[(size_t)pick((int)c.a.retired.size())];
          if (!r.done.empty()) c.complete(r.done[(size_t)pick((int)r.done.size())]);
        } else {
          const int s = alive[(size_t)pick((int)alive.size())];
          auto &q = c.m().q[s];
          if (!q.empty()) c.m().drain(s, q[(size_t)pick((int)q.size())].id);
        }
      } else if (alive.size() > 3) {
        const size_t k = 1 + (size_t)pick((int)alive.size() - 1);
        c.m().destroy_stream(alive[k]);
        alive.erase(alive.begin() + (long)k);
      }
    }
    c.destroy();
  }
  ok(g_script);
}

int main(int argc, char **argv) {
  const int seeds = argc > 1 ? atoi(argv[1]) : 300;
  noop_reserve();
  floor_applies_to_growth_only();
  one_stream_enqueues_no_wait();
  stream_switch_waits_for_the_previous_stream();
  zero_fill_orders_the_first_use();
  retired_bound_under_alternating_growth();
  reap_frees_once_every_event_is_done();
  enomem_with_retired_blocks();
  enomem_without_retired_blocks();
  destroyed_stream();
  failed_event_create_and_record();
  stream_window();
  release_all_with_history();
  random_sequences(seeds, 120);
  return 0;
}
