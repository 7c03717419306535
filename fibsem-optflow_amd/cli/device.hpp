// device.hpp — what a worker holds on one GPU: the engine context, its stream, grow-only
// buffers (DevBuf, PinnedPair), the page-locked host pool (PinnedPool), and how an engine
// failure is reported (engine_failed).  Shared by the per-pair worker, the strip worker and
// the slice-list driver.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <initializer_list>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tvl1.h"
#include "config.hpp"
#include "imageio.hpp"

namespace ofcli {

inline std::mutex g_io_mutex;   // stdout / stderr lines of concurrent workers

using Clock = std::chrono::steady_clock;
inline const Clock::time_point g_t0 = Clock::now();
inline double secs_since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

// A device allocation that only grows and frees itself.  Whoever replaces one that queued work
// may still use synchronises that work's stream first (DeviceCtx::reserve*).
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;   // bytes
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
  bool alloc(size_t bytes) {   // of exactly `bytes`, whatever it held
    reset();
    if (hipMalloc(&p, bytes) != hipSuccess) {
      p = nullptr;
      return false;
    }
    cap = bytes;
    return true;
  }
  bool reserve(size_t bytes) { return bytes <= cap || alloc(bytes); }
  uint8_t *u8() const { return (uint8_t *)p; }
  float *f32() const { return (float *)p; }
};
// buffers that are sized together: all freed, then all allocated, so the old set never stands
// beside the new one; after a failure none is left
inline bool alloc_together(std::initializer_list<DevBuf *> bufs, size_t bytes) {
  for (DevBuf *b : bufs) b->reset();
  for (DevBuf *b : bufs)
    if (!b->alloc(bytes)) {
      for (DevBuf *c : bufs) c->reset();
      return false;
    }
  return true;
}

// Two page-locked host buffers of one size, grown together (a strip chunk's packed frames)
struct PinnedPair {
  uint8_t *a = nullptr, *b = nullptr;
  size_t cap = 0;
  PinnedPair() = default;
  PinnedPair(const PinnedPair &) = delete;
  PinnedPair &operator=(const PinnedPair &) = delete;
  ~PinnedPair() { reset(); }
  void reset() {
    for (void *q : {(void *)a, (void *)b})
      if (q) (void)hipHostFree(q);
    a = b = nullptr, cap = 0;
  }
  bool reserve(size_t bytes) {
    if (bytes <= cap) return true;
    reset();
    if (hipHostMalloc((void **)&a, bytes, hipHostMallocPortable) != hipSuccess ||
        hipHostMalloc((void **)&b, bytes, hipHostMallocPortable) != hipSuccess)
      return false;
    cap = bytes;
    return true;
  }
};

// An engine status that leaves the device context in doubt (a HIP call failed, memory ran
// out): the pair is retried on a rebuilt context.  TVL1_EINVAL / TVL1_ESIZE are input or
// config errors (a bad medianFiltering, an ROI the solver rejects): reported like the
// reference's input errors, without a context rebuild.
inline bool device_fault(tvl1_status s) { return s == TVL1_EHIP || s == TVL1_ENOMEM || s == TVL1_ENODEV; }

// Device context of one worker: engine ctx, stream and buffers.
struct DeviceCtx {
  int device = 0;
  tvl1_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  DevBuf d0, d1;   // the pair's frames
  DevBuf dw;       // warpAffine target of frame1 (feature pre-alignment)
  DevBuf du, dv;   // the flow of the ROI being solved
  DevBuf dub, dvb, dsc;   // a check's backward flow and score of that ROI
  // frame reuse: the (name, scale) currently resident in d0 / d1
  std::string key0, key1;
  ofio::Image8 h0, h1;
  bool faulted = false;   // a HIP / engine call failed: the context is reset before reuse

  bool open(int device, std::string &err);
  void close();
  // Frames of img_bytes and flow planes of flow_bytes.  Buffers that must grow may still be in
  // use by queued work, so the stream is synchronised first; *frames_replaced: d0 / d1 hold
  // nothing any more (the resident-slice keys are cleared).
  bool reserve(size_t img_bytes, size_t flow_bytes, bool &frames_replaced, std::string &err);
  // the three planes a check adds, of the size of the largest ROI's flow
  bool reserve_check(size_t flow_bytes, std::string &err);
  // s != TVL1_OK: the engine's message (after `what`) in err, faulted when the context is in doubt
  bool failed(tvl1_status s, std::string &err, const char *what = "") {
    if (s == TVL1_OK) return false;
    err = std::string(what) + tvl1_last_error(ctx);
    faulted = device_fault(s);
    return true;
  }
  // a HIP call of the worker's own failed: always false, to be returned
  bool hip_error(const char *what, std::string &err) {
    err = what;
    faulted = true;
    return false;
  }
};

inline bool DeviceCtx::open(int dev, std::string &err) {
  device = dev;
  tvl1_params p;
  tvl1_params_default(&p);
  if (tvl1_create(&ctx, dev, &p) != TVL1_OK) {
    err = tvl1_last_error(nullptr);
    ctx = nullptr;
    return false;
  }
  (void)hipSetDevice(dev);
  if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
    err = "hipStreamCreate failed";
    stream = nullptr;
    return false;
  }
  faulted = false;
  return true;
}

inline void DeviceCtx::close() {
  if (stream) (void)hipStreamSynchronize(stream);
  if (ctx) tvl1_destroy(ctx);
  if (stream) (void)hipStreamDestroy(stream);
  for (DevBuf *b : {&d0, &d1, &dw, &du, &dv, &dub, &dvb, &dsc}) b->reset();
  ctx = nullptr;
  stream = nullptr;
  key0.clear();
  key1.clear();
}

inline bool DeviceCtx::reserve(size_t img_bytes, size_t flow_bytes, bool &frames_replaced, std::string &err) {
  frames_replaced = false;
  if ((img_bytes > d0.cap || flow_bytes > du.cap) && stream)
    (void)hipStreamSynchronize(stream);  // buffers may still be in use by queued work
  if (img_bytes > d0.cap) {
    frames_replaced = true;
    if (!alloc_together({&d0, &d1, &dw}, img_bytes)) return hip_error("hipMalloc failed for frames", err);
    key0.clear();
    key1.clear();
  }
  if (flow_bytes > du.cap && !alloc_together({&du, &dv}, flow_bytes)) return hip_error("hipMalloc failed for flow", err);
  return true;
}

inline bool DeviceCtx::reserve_check(size_t flow_bytes, std::string &err) {
  if (flow_bytes <= dsc.cap) return true;
  if (stream) (void)hipStreamSynchronize(stream);
  if (!alloc_together({&dub, &dvb, &dsc}, flow_bytes)) return hip_error("hipMalloc failed for the backward flow", err);
  return true;
}

// The flows of n solves of one W x H geometry with what a check reads and writes: one ROI of a
// pair (n 1, strides 0) or a chunk's packed strips of one ROI key.
struct FlowSet {
  int n = 1;
  const uint8_t *I0 = nullptr, *I1 = nullptr;   // the views the solve saw
  size_t pitch0 = 0, stride0 = 0, pitch1 = 0, stride1 = 0;
  float *u = nullptr, *v = nullptr;             // the forward flow
  float *ub = nullptr, *vb = nullptr;           // the backward flow (forward-backward check)
  float *score = nullptr;
  size_t fpitch = 0, fstride = 0;               // of all five planes
  int W = 0, H = 0;
};
// A check's score of the raw flows, before the post-process.  "zncc": one call on the views the
// solve saw.  "consistency": backward() first solves the same views swapped into ub / vb (a
// seed negated; an "auto" pair is estimated once, forward), then the two flows are scored.
template <class Backward>
tvl1_status score_flows(const DeviceCtx &dc, const FlowSet &s, const FlowCheck &check, Backward backward) {
  if (check.zncc())
    return tvl1_zncc_score_batch(dc.ctx, s.n, s.I0, s.pitch0, s.stride0, s.I1, s.pitch1, s.stride1, s.u, s.v,
                                 s.fpitch, s.fstride, s.W, s.H, check.radius, s.score, s.fpitch, s.fstride,
                                 dc.stream);
  const tvl1_status st = backward();
  if (st != TVL1_OK) return st;
  return tvl1_fb_score_batch(dc.ctx, s.n, s.u, s.v, s.fpitch, s.fstride, s.ub, s.vb, s.fpitch, s.fstride, s.W, s.H,
                             check.alpha, s.score, s.fpitch, s.fstride, dc.stream);
}
// After the post-process (the reference applies its own mask after the map add,
// optflow.cpp:468-473): zero the px that failed the check; rejected[n] arrives with it
inline tvl1_status reject_flows(const DeviceCtx &dc, const FlowSet &s, const FlowCheck &check, uint64_t *rejected) {
  return tvl1_zero_above_batch(dc.ctx, s.n, s.u, s.v, s.fpitch, s.fstride, s.score, s.fpitch, s.fstride, s.W, s.H,
                               check.beta, rejected, dc.stream);
}

// Page-locked host buffers for what crosses PCIe (the reference uploads
// with GpuMat::upload, optflow.cpp:315-316): the decode pool writes each slice straight
// into one, so its upload is a single DMA with no pageable staging copy, and full flow
// fields download into them.  hipHostMalloc costs milliseconds per 25 MB slice, so a
// released buffer returns to a free list (best fit, up to 4x the request) instead of
// being unpinned; the list keeps at most kKeep bytes and the pool pins at most kMax, past
// which buffers are pageable; buffers under kMin stay pageable.  Pinning runs outside the
// pool's lock, so decode threads never wait on each other's hipHostMalloc.  A buffer is released only
// after the stream that read or wrote it was synchronised (each pair's solve and downloads
// end in a stream sync before the next pair replaces DeviceCtx::h0 / h1).
class PinnedPool {
 public:
  static void *alloc(size_t n) { return pool().get(n); }
  static void release(void *p, size_t n) { pool().put(p, n); }
  static size_t pinned_bytes() {
    std::lock_guard<std::mutex> lk(pool().m_);
    return pool().pinned_;
  }
  // pins, free-list hits, pageable fallbacks and the time spent pinning (OPTFLOW_PINNED_TRACE)
  static std::string summary() {
    PinnedPool &q = pool();
    std::lock_guard<std::mutex> lk(q.m_);
    char b[200];
    snprintf(b, sizeof b, "pinned pool: %zu MiB pinned, %ld pins (%.1f ms), %ld reuses, %ld pageable",
             q.pinned_ >> 20, q.n_pin_, q.pin_ms_, q.n_hit_, q.n_page_);
    return b;
  }
  // build-only "pinned_host" (env OPTFLOW_PINNED overrides): page-locked slices and flow
  // fields, installed before the first image is allocated.  Off by default: on 96-pair jobs it
  // measured 2-5 % slower end to end -- each 25 MB buffer costs 10-20 ms to pin, a
  // C2 job's decode-ahead window spans ~100 slices, and the pageable upload it replaces (~1 ms
  // per pair) runs on a worker that is not the bound
  static void install_if_asked(bool key, bool plan_only) {
    bool pinned = key;
    if (const char *e = getenv("OPTFLOW_PINNED")) pinned = atoi(e) != 0;
    if (!plan_only && pinned) ofio::set_host_alloc({PinnedPool::alloc, PinnedPool::release});
  }

 private:
  static constexpr size_t kMin = 256u << 10, kKeep = 2ull << 30, kMax = 16ull << 30;
  static PinnedPool &pool() {
    static PinnedPool *p = new PinnedPool;   // never destroyed: buffers may outlive main's locals
    return *p;
  }
  void *get(size_t n) {
    if (n >= kMin && !off_) {
      const size_t cap = (n + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
      std::vector<void *> drop;
      {
        std::lock_guard<std::mutex> lk(m_);
        auto it = free_.lower_bound(cap);   // smallest kept buffer that holds n, up to 4x
        if (it != free_.end() && it->first <= 4 * cap) {
          void *p = it->second;
          kept_ -= it->first;
          live_[p] = it->first;
          free_.erase(it);
          ++n_hit_;
          return p;
        }
        // make room under kMax from the free list before pinning more
        while (pinned_ + cap > kMax && !free_.empty()) {
          auto f = free_.begin();
          drop.push_back(f->second);
          pinned_ -= f->first;
          kept_ -= f->first;
          free_.erase(f);
        }
        if (pinned_ + cap <= kMax) pinned_ += cap;   // reserved; pinned outside the lock
        else {
          ++n_page_;
          return ::operator new(n, std::nothrow);
        }
      }
      for (void *q : drop) (void)hipHostFree(q);
      void *p = nullptr;   // hipHostMalloc takes milliseconds: other threads go on meanwhile
      const auto t0 = std::chrono::steady_clock::now();
      if (hipHostMalloc(&p, cap, hipHostMallocPortable) == hipSuccess && p) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::lock_guard<std::mutex> lk(m_);
        live_[p] = cap;
        ++n_pin_;
        pin_ms_ += ms;
        return p;
      }
      std::lock_guard<std::mutex> lk(m_);
      pinned_ -= cap;
      off_ = true;   // no device / no pinnable memory: pageable from here on
    }
    return ::operator new(n, std::nothrow);
  }
  void put(void *p, size_t) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> lk(m_);
      auto it = live_.find(p);
      if (it != live_.end()) {
        const size_t cap = it->second;
        live_.erase(it);
        if (kept_ + cap <= kKeep) {
          free_.emplace(cap, p);
          kept_ += cap;
        } else {
          (void)hipHostFree(p);
          pinned_ -= cap;
        }
        return;
      }
    }
    ::operator delete(p);
  }
  std::mutex m_;
  std::multimap<size_t, void *> free_;   // capacity -> buffer
  std::map<void *, size_t> live_;        // pinned buffers handed out -> capacity
  size_t kept_ = 0, pinned_ = 0;
  std::atomic<bool> off_{false};
  long n_pin_ = 0, n_hit_ = 0, n_page_ = 0;
  double pin_ms_ = 0;
};

}  // namespace ofcli
