// decode_pool.hpp — the decode-ahead pool.  A 6144x4096 PNG takes ~0.3 s of one
// core to decode (zlib inflate ~0.23 s), 5x one pair's GPU solve, so slices are read + pre-scaled
// by a pool of host threads while the GPU works: a worker queues every slice of its current and
// next chunk of pairs and then takes them in pair order.
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "device.hpp"
#include "imageio.hpp"
#include "json.hpp"

namespace ofcli {

struct Loaded {
  bool ok = false;
  ofio::Image8 img;
  std::string err;
  // load_bands: the pre-scaled slice's size and the row bands asked for
  int W = 0, H = 0;
  std::vector<ofio::Image8> bands;
  bool partial = false;   // only the bands' source rows were read
};
using LoadFuture = std::shared_future<std::shared_ptr<Loaded>>;

// band reads of the whole job, for timing_json
inline std::atomic<int64_t> g_band_read_ns{0}, g_band_reads{0};

class DecodePool {
 public:
  explicit DecodePool(int n) {
    for (int i = 0; i < n; ++i) th_.emplace_back([this] { run(); });
  }
  // build-only "decode_threads": host threads decoding slices ahead of the GPU
  static int threads_asked(const ofjson::Value &args) {
    const unsigned hc = std::max(2u, std::thread::hardware_concurrency());
    return args.get("decode_threads", (int)std::min(16u, hc - 1)).asInt();
  }
  ~DecodePool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  int threads() const { return (int)th_.size(); }
  // imread(IMREAD_GRAYSCALE) + resize(scale) (optflow.cpp:104-131) on a pool thread
  LoadFuture load(const std::string &path, float scale) {
    return enqueue([path, scale] {
      auto r = std::make_shared<Loaded>();
      ofio::Image8 img;
      if (!ofio::read_gray8(path, img, r->err) || img.width == 0 || img.height == 0) return r;
      if (scale != 1) ofio::resize_u8(img, scale, scale, r->img);
      else r->img = std::move(img);
      r->ok = true;
      return r;
    });
  }
  // imread + resize(scale) of only the rows of get_rois' top / bottom ROIs (SURVEY 3.2's
  // production strips): bands in `keys` order, top = [0, top), bottom = [H - bottom, H) of
  // the pre-scaled slice (ofio::read_gray8_bands: strip-organised TIFF reads just those rows)
  LoadFuture load_bands(const std::string &path, float scale, std::vector<std::string> keys, int top, int bottom) {
    return enqueue([=] {
      const auto t0 = Clock::now();
      auto r = std::make_shared<Loaded>();
      r->ok = ofio::read_gray8_bands(
          path, scale,
          [&](int, int h) {
            std::vector<std::pair<int, int>> b;
            for (const auto &k : keys) b.push_back(k == "top" ? std::make_pair(0, top)
                                                              : std::make_pair(h - bottom, h));
            return b;
          },
          r->W, r->H, r->bands, r->err, &r->partial);
      g_band_read_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count();
      ++g_band_reads;
      return r;
    });
  }
  // any host job (the strip workers' point sampling runs here while their batch solves)
  std::shared_future<void> submit(std::function<void()> fn) { return enqueue(std::move(fn)); }

 private:
  template <class F>
  auto enqueue(F fn) -> std::shared_future<decltype(fn())> {
    auto task = std::make_shared<std::packaged_task<decltype(fn())()>>(std::move(fn));
    auto f = task->get_future().share();
    {
      std::lock_guard<std::mutex> lk(m_);
      q_.emplace_back([task] { (*task)(); });
    }
    cv_.notify_one();
    return f;
  }
  void run() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        job = std::move(q_.front());
        q_.pop_front();
      }
      job();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  std::vector<std::thread> th_;
  bool stop_ = false;
};

}  // namespace ofcli
