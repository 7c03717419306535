// tvl1_arena.hpp — who owns a context's device memory, as plain C++17: the scratch blocks,
// the blocks they outgrew, and the stream ordering around both.
//
// No HIP header, like tvl1_walk.hpp: streams and events are the backend's opaque handles.  This
// code decides when memory a kernel may still read is released and which stream waits for
// which; a slip here is silent.  The engine is one backend (a struct of one-line HIP calls);
// tests/arena_model.cpp is the other, a device of per-stream queues on the CPU that checks
// every step (tests/test_arena_cpu.py).
//
// Dev, the backend (each call but the last three returns 0 on success, else an error code):
//   malloc(&p, bytes)  free(p)           free waits for the whole device, as hipFree does
//   memset_async(p, value, bytes, stream)
//   event_create(&e)   event_record(e, stream)   event_query(e)   event_sync(e)
//   stream_wait(stream, e)
//   event_destroy(e)   clear_error()   error_string(code)
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/tvl1.h"

namespace tvl1k {

// One device allocation of a ctx: null and 0 when empty.
struct Block {
  char *p = nullptr;
  size_t bytes = 0;
  template <class T>
  T *as(size_t offset = 0) const { return reinterpret_cast<T *>(p + offset); }
};

constexpr size_t kRetiredMax = 2;   // outgrown blocks held after a reserve returns
constexpr size_t kStreamsMax = 8;   // recent streams that mark a retired block's last use

template <class Dev>
struct Arena {
  using Stream = typename Dev::Stream;
  using Event = typename Dev::Event;
  struct Retired {   // a block outgrown while work enqueued earlier may still read it
    char *p;
    std::vector<Event> done;   // recorded on every recent stream when it was retired
  };

  Dev dev;
  Stream own{};                 // the ctx's stream: zero fills run on it
  Event ev_order{};             // orders work on the caller's stream after a zero fill
  Event ev_switch{};            // orders a call on a new stream after the previous stream
  Stream last_stream{};         // the stream the ctx's last call enqueued on
  bool last_stream_valid = false;
  std::vector<Retired> retired;
  std::vector<Stream> streams;  // streams the ctx's work was enqueued on, most recent last
  char err[160] = "";           // why the last failed reserve failed

  bool init() { return dev.event_create(&ev_order) == 0 && dev.event_create(&ev_switch) == 0; }

  // The prologue of every call that touches a block.  The blocks are reused (and re-laid in
  // place) by every call, so a call on a stream other than the previous call's must not start
  // before that stream's work on them is done: one event record + stream wait per switch of
  // streams; a ctx that stays on one stream pays nothing.  A stream the caller has destroyed
  // since has nothing left on it: its record fails and is ignored.  Then the stream is noted,
  // and the retired blocks whose work has finished are released without waiting.
  void enter(Stream st) {
    if (last_stream_valid && !(last_stream == st)) {
      if (dev.event_record(ev_switch, last_stream) == 0) (void)dev.stream_wait(st, ev_switch);
      dev.clear_error();
    }
    last_stream = st;
    last_stream_valid = true;
    note(st);
    if (!retired.empty()) reap(false);
  }

  // Grow block b to at least `need` bytes (max(need, floor) are allocated), zero-filled, for
  // work on stream `use`; a block that is large enough is left alone and nothing is enqueued.
  // The old allocation may still be read by work the ctx enqueued (tvl1_calc is asynchronous).
  // It is retired, not freed at once: events recorded on the ctx's recent streams (the last
  // kStreamsMax, and the own stream) mark its last use, and reap releases it once they are
  // done, or waits for the oldest when more than kRetiredMax are held, or at release_all.
  // What makes the release safe is the free itself: on ROCm hipFree synchronises the whole
  // device before it frees, so a retired block is never freed under a kernel that still reads
  // it, whatever stream that kernel is on.  The price is that a reap stalls every other
  // context's pairs in flight for that moment; it happens only when a block was outgrown (at
  // most kRetiredMax held), never in the steady state of a job whose sizes repeat.  Blocks are
  // only ever grown: a smaller layout re-lays the existing allocation (ensure_geometry,
  // ensure_batch), ordered across streams by enter.  The work on `use` is ordered after the
  // zero fill by an event, not by a host wait.  (The stream-ordered allocator, hipMallocAsync /
  // hipFreeAsync, would release in stream order too, but it deadlocked against a concurrent
  // hipStreamDestroy on this ROCm, so it is not used.)
  tvl1_status reserve(Block &b, size_t need, Stream use, size_t floor = 0) {
    if (need <= b.bytes) return TVL1_OK;
    const size_t bytes = std::max(need, floor);
    note(use);
    if (b.p) {
      Retired r{b.p, {}};
      note(own);
      for (Stream s : streams) {
        Event e{};
        if (dev.event_create(&e) != 0) {
          dev.clear_error();
          continue;
        }
        if (dev.event_record(e, s) != 0) {   // a destroyed stream: nothing left on it
          dev.clear_error();
          (void)dev.event_destroy(e);
          continue;
        }
        r.done.push_back(e);
      }
      retired.push_back(r);
      b = Block{};
      reap(true);
    }
    int e = dev.malloc(&b.p, bytes);
    if (e != 0 && !retired.empty()) {
      // out of memory with outgrown blocks held: release them (the free waits for the device;
      // a rare path, better than failing) and try once more
      dev.clear_error();
      for (Retired &r : retired) drop(r);
      retired.clear();
      e = dev.malloc(&b.p, bytes);
    }
    if (e != 0) {
      dev.clear_error();   // not sticky: the caller may retry smaller
      b = Block{};
      snprintf(err, sizeof err, "hipMalloc(%zu) failed: %s", bytes, dev.error_string(e));
      return TVL1_ENOMEM;
    }
    b.bytes = bytes;
    // zero once so pitch padding starts finite, on the own stream (the legacy null stream is
    // unordered with non-blocking streams)
    e = dev.memset_async(b.p, 0, bytes, own);
    if (e == 0 && !(use == own)) {
      e = dev.event_record(ev_order, own);
      if (e == 0) e = dev.stream_wait(use, ev_order);
    }
    if (e != 0) {
      snprintf(err, sizeof err, "zero fill of a grown block failed: %s", dev.error_string(e));
      return TVL1_EHIP;
    }
    return TVL1_OK;
  }

  // The destroy path: every live block, every retired block and every event.
  template <class... Blocks>
  void release_all(Blocks &...blocks) {
    for (Block *b : std::initializer_list<Block *>{&blocks...}) {
      if (b->p) (void)dev.free(b->p);
      *b = Block{};
    }
    for (Retired &r : retired) drop(r);
    retired.clear();
    (void)dev.event_destroy(ev_order);
    (void)dev.event_destroy(ev_switch);
    ev_order = ev_switch = Event{};
  }

 private:
  // Remember a stream the ctx enqueues work on, so a retired block can be released once every
  // such stream has passed the point of its retirement.
  void note(Stream s) {
    const auto at = std::find(streams.begin(), streams.end(), s);
    if (at != streams.end()) streams.erase(at);
    streams.push_back(s);
    if (streams.size() > kStreamsMax) streams.erase(streams.begin());
  }

  void drop(Retired &r) {
    (void)dev.free(r.p);
    for (Event e : r.done) (void)dev.event_destroy(e);
    r.done.clear();
  }

  // Release the retired blocks whose work has finished (every event done); with `wait`, the
  // oldest ones are waited for too until at most kRetiredMax remain.  A caller that alternates
  // geometries therefore holds a bounded number of old blocks.
  void reap(bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < retired.size(); ++i) {
      Retired &r = retired[i];
      const bool must = wait && retired.size() - i > kRetiredMax;
      bool done = true;
      for (Event e : r.done) {
        if (must) (void)dev.event_sync(e);
        else if (dev.event_query(e) != 0) done = false;
      }
      dev.clear_error();   // "not ready" is not an error
      if (done) drop(r);
      else if (keep++ != i) retired[keep - 1] = r;
    }
    retired.resize(keep);
  }
};

}  // namespace tvl1k
