// points.hpp — random_points (optflow.cpp:522-572 of the reference) without HIP: the private
// glibc generator, the exact shuffle of debug runs, the sampled draw of the others, and the one
// routine through which every path turns candidates into a pair's "point_matches".
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <ctime>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "config.hpp"

namespace ofcli {

using Points = std::vector<std::pair<int, int>>;   // (x, y) within the ROI

// The reference draws with glibc rand() after std::srand(time(0)) (or, with "debug",
// from the unseeded default state = seed 1).  Other code in this process (the HIP
// runtime) also consumes rand(), so use a PRIVATE generator with glibc's exact
// rand() algorithm (random_r on a 128-byte TYPE_3 state, what rand()/srand() use).
struct GlibcRand {
  random_data rd{};
  char state[128];
  GlibcRand() { initstate_r(1, state, sizeof state, &rd); }
  GlibcRand(const GlibcRand &) = delete;   // rd points into state
  GlibcRand &operator=(const GlibcRand &) = delete;
  void seed(unsigned s) { srandom_r(s, &rd); }
  int next() {
    int32_t r;
    random_r(&rd, &r);
    return r;
  }
};
inline std::mutex g_rand_mutex;
inline GlibcRand &g_rand() {
  static GlibcRand r;
  return r;
}

// The point_matches fields of random_points (optflow.cpp:537-569) for the chosen points;
// any == false gives the dummy point.
inline void emit_points(const Points &pts, const std::vector<float> &vx, const std::vector<float> &vy, bool any,
                        Value &im, const Rect &r0, const Rect &r1, float inv_scale, bool features) {
  Value &pm = im["point_matches"];
  for (size_t i = 0; i < pts.size(); ++i) {
    const int px = pts[i].first, py = pts[i].second;
    pm["w"].append(1);
    pm["p"][0].append((double)((px + r0.x) * inv_scale));
    pm["p"][1].append((double)((py + r0.y) * inv_scale));
    if (features) {
      pm["q"][0].append((double)((vx[i] + r1.x) * inv_scale));
      pm["q"][1].append((double)((vy[i] + r1.y) * inv_scale));
    } else {
      pm["q"][0].append((double)((px + r1.x + vx[i]) * inv_scale));
      pm["q"][1].append((double)((py + r1.y + vy[i]) * inv_scale));
    }
  }
  if (!any) {  // dummy point so the fields are full
    pm["p"][0].append(-1);
    pm["p"][1].append(-1);
    pm["q"][0].append(-1);
    pm["q"][1].append(-1);
    pm["w"].append(0);
  }
}

// A check's selection: of the candidates (px, their flow and score, in drawing order) keep the
// first npoints with score <= beta; returns how many are kept
inline size_t keep_consistent(Points &pts, std::vector<float> &vx, std::vector<float> &vy,
                              const std::vector<float> &sc, float beta, int npoints) {
  size_t k = 0;
  for (size_t i = 0; i < pts.size() && k < (size_t)std::max(npoints, 0); ++i)
    if (sc[i] <= beta) {   // false for NaN and +inf
      pts[k] = pts[i], vx[k] = vx[i], vy[k] = vy[i];
      ++k;
    }
  pts.resize(k), vx.resize(k), vy.resize(k);
  return k;
}

// Every path's last step: the candidates in drawing order with their flow (and, for a checked
// pair, their score) become the pair's point_matches.  Unchecked, all of them are reported
// (any_masked == false: the mask was empty, the dummy point); checked, the first npoints that
// pass, or the dummy point when none does.  Returns the drawn and the reported counts.
inline PointCount report_points(Points pts, std::vector<float> vx, std::vector<float> vy,
                                const std::vector<float> &score, const PairConfig &cfg, bool any_masked,
                                Value &im, const Rect &r0, const Rect &r1, float inv_scale, bool features) {
  PointCount n;
  n.candidates = n.kept = pts.size();
  bool any = any_masked;
  if (cfg.check.on) {
    n.kept = keep_consistent(pts, vx, vy, score, cfg.check.beta, cfg.npoints);
    any = n.kept > 0;
  }
  emit_points(pts, vx, vy, any, im, r0, r1, inv_scale, features);
  return n;
}

// how many px a pair draws: npoints, or a check's candidates
inline int draw_count(const PairConfig &cfg) {
  return (int)std::min<size_t>(candidates_of(cfg.npoints, cfg.check), (size_t)INT32_MAX);
}

// random_points' own order (optflow.cpp:522-535): the masked px, row-major as cv::findNonZero
// lists them, through libstdc++'s std::random_shuffle on rand(); unseeded with "debug" (so the
// output is reproducible), else seeded with the time.
inline Points shuffled_mask(const std::vector<uint8_t> &mask, int W, int H, bool debug) {
  Points loc;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      if (mask[(size_t)y * W + x]) loc.emplace_back(x, y);
  std::lock_guard<std::mutex> lk(g_rand_mutex);
  if (!debug) g_rand().seed((unsigned)std::time(0));
  for (size_t i = 1; i < loc.size(); ++i) {
    const size_t j = (size_t)g_rand().next() % (i + 1);
    if (i != j) std::swap(loc[i], loc[j]);
  }
  return loc;
}

// random_points on whole host planes (debug runs): the first draw_count px of the exact
// shuffle are the candidates
inline PointCount random_points(const float *fx, const float *fy, const float *score, int W, int H, Value &im,
                                const PairConfig &cfg, const Rect &r0, const Rect &r1,
                                const std::vector<uint8_t> &mask, bool features) {
  const Points loc = shuffled_mask(mask, W, H, cfg.debug);
  Points pts(loc.begin(), loc.begin() + std::min<size_t>(loc.size(), candidates_of(cfg.npoints, cfg.check)));
  std::vector<float> vx(pts.size()), vy(pts.size()), sc(cfg.check.on ? pts.size() : 0);
  for (size_t i = 0; i < pts.size(); ++i) {
    const size_t at = (size_t)pts[i].second * W + pts[i].first;
    vx[i] = fx[at];
    vy[i] = fy[at];
    if (cfg.check.on) sc[i] = score[at];
  }
  const float inv_scale = 1. / cfg.scale;
  return report_points(std::move(pts), std::move(vx), std::move(vy), sc, cfg, !loc.empty(), im, r0, r1, inv_scale,
                       features);
}

// The px the sampled random_points draws: npoints distinct px of the mask (frame0 > 1) |
// (frame1 > 1) over a W x H ROI whose rows are row0(y) / row1(y); *total = the mask's size.
// Without the debug flag the reference seeds rand() with the time (optflow.cpp:532-535) and
// keeps the first npoints of a random_shuffle of all the masked px: npoints distinct uniformly
// random masked px in random order is the same distribution.  Drawn by a partial Fisher-Yates
// over the implicit list (row counts + a sparse swap map): no 25 M-entry shuffle, and only
// those px's flow values need to be read back.
template <class R0, class R1>
Points sample_points(R0 row0, R1 row1, int W, int H, int npoints, uint64_t *total_out) {
  // mask = (frame0 > 1) | (frame1 > 1) on the ROIs (optflow.cpp:486-494), counted per row
  std::vector<uint64_t> prefix((size_t)H + 1, 0);
  for (int y = 0; y < H; ++y) {
    const uint8_t *a = row0(y), *b = row1(y);
    unsigned c = 0;
    for (int x = 0; x < W; ++x) c += (a[x] > 1) | (b[x] > 1);
    prefix[y + 1] = prefix[y] + c;
  }
  const uint64_t total = prefix[H];
  std::vector<uint64_t> pick;
  {
    std::lock_guard<std::mutex> lk(g_rand_mutex);
    g_rand().seed((unsigned)std::time(0));
    std::map<uint64_t, uint64_t> swapped;   // sparse Fisher-Yates: index -> current value
    auto at = [&](uint64_t i) {
      auto it = swapped.find(i);
      return it == swapped.end() ? i : it->second;
    };
    const uint64_t k = std::min<uint64_t>(total, (uint64_t)std::max(npoints, 0));
    for (uint64_t i = 0; i < k; ++i) {
      const uint64_t r = ((uint64_t)g_rand().next() << 31) ^ (uint64_t)g_rand().next();
      const uint64_t j = i + r % (total - i);
      const uint64_t vi = at(i), vj = at(j);
      swapped[i] = vj;
      swapped[j] = vi;
      pick.push_back(vj);
    }
  }
  Points pts;
  for (uint64_t idx : pick) {
    const int y = (int)(std::upper_bound(prefix.begin(), prefix.end(), idx) - prefix.begin()) - 1;
    uint64_t left = idx - prefix[y];
    const uint8_t *a = row0(y), *b = row1(y);
    int x = 0;
    for (;; ++x)
      if (((a[x] > 1) | (b[x] > 1)) && left-- == 0) break;
    pts.emplace_back(x, y);
  }
  *total_out = total;
  return pts;
}

}  // namespace ofcli
