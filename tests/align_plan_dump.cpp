// align_plan_dump: prints what csrc/tvl1_align_plan.hpp plans for the query lines of a file,
// one result line per query (tests/test_align_edges_cpu.py builds it with g++ and the host
// sanitizers, as tests/test_plan_cpu.py builds plan_dump; no GPU).
//   geom w h nfeatures scale_factor nlevels edge_threshold
//        -> L kcap sum_quota border | w h quota skipped   (the last four per level)
//   match nt        -> nseg seg empty last   (last: descriptors in the last used segment)
//   carve w h nfeatures scale_factor nlevels blur
//        -> bytes kps desc0 desc1 best dist part lev   (byte offsets of the per-keypoint parts)
//   sweep nf0 nf1   -> cases overflows: nfeatures nf0..nf1 x nlevels {2, 3, 4, 8, 12, 16} x
//        scale_factor {1.1, 1.2, 1.5, 2.0}; an overflow is a per-keypoint buffer of the carve
//        (kps, desc q, desc t, best, dist, part) shorter than the quota sum needs
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "tvl1_align_plan.hpp"

using namespace tvl1k;

static int quota_sum(const OrbGeom &g) {
  int s = 0;
  for (int l = 0; l < g.L; ++l) s += g.quota[l];
  return s;
}

// true when every per-keypoint buffer of the carve holds n keypoints
static bool carve_holds(const AlignCarve &a, size_t n) {
  return a.desc[0] - a.kps >= n * sizeof(OrbKp) && a.desc[1] - a.desc[0] >= n * kOrbDescBytes &&
         a.best - a.desc[1] >= n * kOrbDescBytes && a.dist - a.best >= n * 8 &&
         a.part - a.dist >= n * 8 && a.lev - a.part >= n * kMatchSegs * sizeof(Top2);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream s(line);
    std::string what;
    s >> what;
    if (what == "geom") {
      int w, h, nf, nl, et;
      double sf;
      s >> w >> h >> nf >> sf >> nl >> et;
      const OrbGeom g = orb_geom(w, h, nf, (double)(float)sf, nl, 0);
      const int border = orb_border(et);
      printf("%d %d %d %d |", g.L, g.kcap, quota_sum(g), border);
      for (int l = 0; l < g.L; ++l)
        printf(" %d %d %d %d", g.w[l], g.h[l], g.quota[l], orb_level_skipped(g, l, border) ? 1 : 0);
      printf("\n");
    } else if (what == "match") {
      int nt;
      s >> nt;
      const MatchPlan m = match_plan(nt);
      const int used = m.nseg - m.empty;
      printf("%d %d %d %d\n", m.nseg, m.seg, m.empty, nt - (used - 1) * m.seg);
    } else if (what == "carve") {
      int w, h, nf, nl, blur;
      double sf;
      s >> w >> h >> nf >> sf >> nl >> blur;
      const OrbGeom g = orb_geom(w, h, nf, (double)(float)sf, nl, 0);
      const AlignCarve a = align_carve(g, blur != 0, g.kcap);
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", a.bytes, a.kps, a.desc[0], a.desc[1], a.best, a.dist,
             a.part, a.lev);
    } else if (what == "sweep") {
      int nf0, nf1;
      s >> nf0 >> nf1;
      static const int levels[] = {2, 3, 4, 8, 12, 16};
      static const float sfs[] = {1.1f, 1.2f, 1.5f, 2.0f};
      long cases = 0, bad = 0;
      for (int nf = nf0; nf <= nf1; ++nf)
        for (int nl : levels)
          for (float sf : sfs) {
            const OrbGeom g = orb_geom(400, 300, nf, (double)sf, nl, 0);
            const int sum = quota_sum(g);
            ++cases;
            if (g.kcap < sum || g.kcap < nf || !carve_holds(align_carve(g, false, g.kcap), (size_t)sum)) {
              if (bad++ < 5)
                fprintf(stderr, "nfeatures %d nlevels %d scale %g: quota sum %d, capacity %d\n", nf, nl,
                        (double)sf, sum, g.kcap);
            }
          }
      printf("%ld %ld\n", cases, bad);
    } else {
      fprintf(stderr, "bad query: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
