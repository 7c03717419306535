// tvl1_align_plan.hpp — the host planning of the feature pre-alignment path (tvl1_align.hpp,
// tvl1_find_alignment / tvl1_orb_detect / tvl1_match_knn2 in tvl1_engine.hip): the ORB pyramid
// geometry and per-level quota, which levels are skipped, the layout of the ctx's align
// scratch, and how a train set is cut into ka_match2's segments.  Plain C++17, no HIP header:
// tests/align_plan_dump.cpp builds it with g++ and the host sanitizers
// (tests/test_align_edges_cpu.py), so a capacity that a quota can outgrow fails on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tvl1k {

constexpr int kOrbPatch = 31, kOrbHalf = 15, kOrbBits = 256;
constexpr int kOrbDescBytes = kOrbBits / 8;

// ka_select's level table, a keypoint as ka_describe reads it, and ka_match2's per-segment
// stable top-2 (train indices, Hamming distances)
struct SelLevel {
  unsigned off, cap, quota;
};
struct OrbKp {
  float x, y;        // level coordinates
  float angle;       // radians (filled by ka_describe)
  int level;
};
struct Top2 {
  int b0, b1, d0, d1;
};

inline size_t plan_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One frame's ORB pyramid geometry and its quota per level (ORB_Impl::detectAndCompute:
// nfeatures * (1 - f) / (1 - f^L) * f^l rounded per level, the remainder on the last level).
// The rounded quotas can add up to more than nfeatures (16 levels at 1.1 and 16 features: 17;
// 12 at 1.2 and 24: 25) and OpenCV then returns that many keypoints, so does this path:
// kcap = max(nfeatures, sum of the quotas) is what every per-keypoint buffer holds.
struct OrbGeom {
  int L = 0;
  std::vector<int> w, h, p, quota;
  std::vector<unsigned> cap, off;   // key-list capacity / offset per level
  size_t keys = 0, lev_floats = 0;
  unsigned kmax = 0;
  int kcap = 0;
};

inline OrbGeom orb_geom(int W, int H, int nfeatures, double scale_factor, int nlevels,
                        int first_level) {
  OrbGeom g;
  g.L = std::max(1, nlevels);
  const double sf = scale_factor;
  g.w.resize(g.L);
  g.h.resize(g.L);
  g.p.resize(g.L);
  g.quota.assign(g.L, 0);
  g.cap.resize(g.L);
  g.off.resize(g.L);
  for (int l = 0; l < g.L; ++l) {
    const double scale = 1.0 / std::pow(sf, l - first_level);
    g.w[l] = l == 0 ? W : std::max(1, (int)std::lrint(W * scale));
    g.h[l] = l == 0 ? H : std::max(1, (int)std::lrint(H * scale));
    g.p[l] = (int)plan_align_up((size_t)g.w[l], 64);
    g.lev_floats += plan_align_up((size_t)g.p[l] * g.h[l], 64);
    g.cap[l] = (unsigned)(((size_t)g.w[l] + 1) / 2 * (((size_t)g.h[l] + 1) / 2));
    g.off[l] = (unsigned)g.keys;
    g.keys += plan_align_up(g.cap[l], 32);
  }
  const double f = 1.0 / sf;
  double nd = nfeatures * (1 - f) / (1 - std::pow(f, g.L));
  int sum = 0;
  for (int l = 0; l < g.L - 1; ++l) {
    g.quota[l] = (int)std::lrint(nd);
    sum += g.quota[l];
    nd *= f;
  }
  g.quota[g.L - 1] = std::max(nfeatures - sum, 0);
  sum += g.quota[g.L - 1];
  for (int l = 0; l < g.L; ++l) g.kmax = std::max(g.kmax, (unsigned)g.quota[l]);
  g.kcap = std::max(nfeatures, sum);
  return g;
}

// FAST corners keep this far from a level's border: the caller's edgeThreshold, and at least
// the descriptor patch's radius + 1 (ka_describe reads the radius-15 disc unchecked).
inline int orb_border(int edge_threshold) { return std::max(edge_threshold, kOrbHalf + 1); }

// A level with no px inside the border, or with no quota, is not searched.
inline bool orb_level_skipped(const OrbGeom &g, int l, int border) {
  return g.w[l] <= 2 * border || g.h[l] <= 2 * border || g.quota[l] == 0;
}

// ka_match2's grid y: the train set in nseg segments of seg descriptors (a multiple of the
// 64-descriptor LDS tile), about kMatchSegPx each and at most kMatchSegs of them.  Rounding
// seg up can leave the last `empty` segments without a descriptor (nt = 4097: 16 segments of
// 320, 13 used): they report no neighbour and the merge passes them over.
constexpr int kMatchSegs = 16, kMatchSegPx = 256, kMatchTile = 64;
struct MatchPlan {
  int nseg, seg, empty;
};
inline MatchPlan match_plan(int nt) {
  MatchPlan m;
  m.nseg = std::max(1, std::min(kMatchSegs, (nt + kMatchSegPx - 1) / kMatchSegPx));
  m.seg = (int)plan_align_up((size_t)((std::max(nt, 1) + m.nseg - 1) / m.nseg), kMatchTile);
  m.empty = m.nseg - std::max(1, (nt + m.seg - 1) / m.seg);
  return m;
}

// The align scratch as byte offsets: [kps | desc q | desc t | match best | match dist | match
// partials | pyramid | blurred pyramid | score | keys | counts | selected keys | nsel | level
// table | level pointers | level pitches], carved per frame.  The per-keypoint parts come
// first and depend on kcap alone, so two frames' carves of one call share them.
struct AlignCarve {
  static constexpr size_t kNone = ~(size_t)0;
  size_t kps = 0, desc[2] = {0, 0}, best = 0, dist = 0, part = 0;
  size_t lev = 0, blur = kNone, score = 0, keys = 0, cnt = 0, sel = 0, nsel = 0, lv = 0, dlev = 0,
         dlp = 0;
  size_t bytes = 0;
};

inline AlignCarve align_carve(const OrbGeom &g, bool blur, int kcap) {
  AlignCarve cv;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += plan_align_up(std::max<size_t>(bytes, 1), 256);
    return at;
  };
  const size_t n = (size_t)std::max(kcap, g.kcap);
  cv.kps = take(n * sizeof(OrbKp));
  cv.desc[0] = take(n * kOrbDescBytes);
  cv.desc[1] = take(n * kOrbDescBytes);
  cv.best = take(n * 2 * sizeof(int32_t));
  cv.dist = take(n * 2 * sizeof(int32_t));
  cv.part = take(n * kMatchSegs * sizeof(Top2));
  cv.lev = take(g.lev_floats * 4);
  cv.blur = blur ? take(g.lev_floats * 4) : AlignCarve::kNone;
  cv.score = take((size_t)g.w[0] * g.h[0] * 4);
  cv.keys = take(g.keys * 8);
  cv.cnt = take(g.L * 4);
  cv.sel = take((size_t)g.L * g.kmax * 8);
  cv.nsel = take(g.L * 4);
  cv.lv = take(g.L * sizeof(SelLevel));
  cv.dlev = take(g.L * sizeof(float *));
  cv.dlp = take(g.L * 4);
  cv.bytes = o;
  return cv;
}

}  // namespace tvl1k
