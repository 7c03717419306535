// plan_dump: prints what csrc/tvl1_plan.hpp (and tvl1_walk.hpp's WarpSched) plans for the cases
// of a file, one result line per case line (tests/test_plan_cpu.py builds it with g++ and the
// host sanitizers; no GPU).
//   seg bands rows k slots                                  -> seg_rows
//   site NAME w h k px slots fill roll_seg pairs seg_min    -> bands seg_rows waves
//   blocked w h k          -> iterate_blocks, then tiles_x out_h blocks of tb and of tb4
//   cap w h                -> partials of a single pair, of a pair of a batch
//   pyr w h nscales step   -> L ws... hs...
//   sched prev thr n iters kmax eps_pos        -> k calc_end prev_end   (doubles as %a)
//   warp thr iters kmax eps_pos r1 r2 ...      -> the iteration counts of a warp's checks, '|',
//        its iterations: WarpSched (csrc/tvl1_walk.hpp) stepped pass by pass; r_n (in units of
//        thr) is the residual a check at iteration count n reads
//   capsweep w0 w1 h0 h1   -> cases violations: every launch plan of every frame size in the
//        range against the capacity reserved for that size
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "tvl1_plan.hpp"
#include "tvl1_walk.hpp"

using namespace tvl1k;

// the launch sites of tvl1_engine.hip, by name (kWiMargin = 6, BW = 128)
enum Site { kWarpRing, kWarpIter, kRoll, kKbWarpIter, kKbWarpRing, kKbRoll, kSites };
static const char *const kSiteNames[kSites] = {"warp_ring", "warp_iter", "roll", "kb_warp_iter", "kb_warp_ring",
                                               "kb_roll"};
static StreamPlan site(Site which, int w, int h, int k, int px, int slots, int fill, int roll_seg, int pairs,
                       int seg_min) {
  switch (which) {
    case kWarpRing: return plan_warp_ring(w, h, 6, fill_slots(slots, fill), roll_seg);
    case kWarpIter: return plan_warp_iter(w, h, 128, 6, fill_slots(slots, fill), roll_seg);
    case kRoll: return plan_roll(w, h, k, px, fill_slots(slots, fill), roll_seg);
    case kKbWarpIter: return plan_warp_iter(w, h, 128, 6, slots, 0, pairs);
    case kKbWarpRing: return plan_warp_ring(w, h, 6, slots, 0, pairs);
    default: return plan_roll(w, h, k, px, slots, roll_seg, std::min(h, seg_min), pairs);
  }
}

static long g_cases = 0, g_bad = 0;
static void within(int need, int cap, const char *what, int w, int h, int k, int px, int seg, int slots) {
  ++g_cases;
  if (need <= cap) return;
  if (g_bad++ < 5)
    fprintf(stderr, "%s: %d > capacity %d at %dx%d k %d px %d roll_seg %d slots %d\n", what, need, cap, w,
            h, k, px, seg, slots);
}

static void capsweep(int w0, int w1, int h0, int h1) {
  static const int segs[] = {0, 8, 64}, slotsv[] = {1, 256, 4096}, pairs[] = {1, 3}, mins[] = {0, 128};
  for (int w = w0; w <= w1; ++w)
    for (int h = h0; h <= h1; ++h) {
      const int cap = partials_capacity(w, h), bcap = batch_partials_capacity(w, h);
      within(iterate_blocks(w, h), cap, "k_iterate", w, h, 1, 0, 0, 0);
      for (int k = 1; k <= 4; ++k) {
        within(tb_plan(w, h, k).blocks, cap, "k_iterate_tb", w, h, k, 0, 0, 0);
        within(tb4_plan(w, h, k).blocks, cap, "k_iterate_tb4", w, h, k, 0, 0, 0);
      }
      for (int seg : segs)
        for (int sl : slotsv) {
          within(site(kWarpRing, w, h, 6, 0, sl, 100, seg, 1, 0).waves, cap, "k_warp_ring", w, h, 6, 0, seg, sl);
          within(site(kWarpIter, w, h, 8, 0, sl, 100, seg, 1, 0).waves, cap, "k_warp_iter", w, h, 8, 0, seg, sl);
          for (int k = 1; k <= 4; ++k)
            for (int px : {1, 2, 4}) {
              const int waves = site(kRoll, w, h, k, px, sl, 100, seg, 1, 0).waves;
              within(waves, cap, "k_iterate_roll", w, h, k, px, seg, sl);
              if (k == 4 && px == 2) within(2 * waves, cap, "k_iterate_roll_mid", w, h, k, px, seg, sl);
            }
          for (int n : pairs) {
            within(site(kKbWarpIter, w, h, 8, 0, sl, 100, 0, n, 0).waves, bcap, "kb_warp_iter", w, h, 8, 0, 0, sl);
            within(site(kKbWarpRing, w, h, 6, 0, sl, 100, 0, n, 0).waves, bcap, "kb_warp_ring", w, h, 6, 0, 0, sl);
            for (int k = 1; k <= 4; ++k)
              for (int px : {1, 2})
                for (int mn : mins)
                  within(site(kKbRoll, w, h, k, px, sl, 100, seg, n, mn).waves, bcap, "kb_iterate_roll", w, h,
                         k, px, seg, sl);
          }
        }
    }
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string cmd;
    if (!(ss >> cmd)) continue;
    if (cmd == "seg") {
      int bands, rows, k, slots;
      ss >> bands >> rows >> k >> slots;
      printf("%d\n", roll_segment(bands, rows, k, slots));
    } else if (cmd == "site") {
      std::string name;
      int w, h, k, px, slots, fill, roll_seg, pairs, seg_min;
      ss >> name >> w >> h >> k >> px >> slots >> fill >> roll_seg >> pairs >> seg_min;
      int which = 0;
      while (which < kSites && name != kSiteNames[which]) ++which;
      if (which == kSites) {
        fprintf(stderr, "unknown site %s\n", name.c_str());
        return 2;
      }
      const StreamPlan p = site((Site)which, w, h, k, px, slots, fill, roll_seg, pairs, seg_min);
      printf("%d %d %d\n", p.bands, p.seg_rows, p.waves);
    } else if (cmd == "blocked") {
      int w, h, k;
      ss >> w >> h >> k;
      const BlockedPlan a = tb_plan(w, h, k), b = tb4_plan(w, h, k);
      printf("%d %d %d %d %d %d %d\n", iterate_blocks(w, h), a.tiles_x, a.out_h, a.blocks, b.tiles_x, b.out_h,
             b.blocks);
    } else if (cmd == "cap") {
      int w, h;
      ss >> w >> h;
      printf("%d %d\n", partials_capacity(w, h), batch_partials_capacity(w, h));
    } else if (cmd == "pyr") {
      int w, h, ns, ws[TVL1_MAX_LEVELS], hs[TVL1_MAX_LEVELS];
      std::string step;
      ss >> w >> h >> ns >> step;
      const int L = pyramid_sizes(w, h, ns, strtod(step.c_str(), nullptr), ws, hs);
      printf("%d", L);
      for (int s = 0; s < L; ++s) printf(" %d", ws[s]);
      for (int s = 0; s < L; ++s) printf(" %d", hs[s]);
      printf("\n");
    } else if (cmd == "sched") {
      std::string prev, thr;
      int n, iters, kmax, eps_pos;
      ss >> prev >> thr >> n >> iters >> kmax >> eps_pos;
      bool ce = false;
      double pe = 0.0;
      const int k = sched_after(strtod(prev.c_str(), nullptr), strtod(thr.c_str(), nullptr), n, iters, kmax,
                                eps_pos, &ce, &pe);
      printf("%d %d %a\n", k, ce ? 1 : 0, pe);
    } else if (cmd == "warp") {
      std::string thr_s, r;
      int iters, kmax, eps_pos;
      ss >> thr_s >> iters >> kmax >> eps_pos;
      const double thr = strtod(thr_s.c_str(), nullptr);
      std::vector<double> res(1, 0.0);   // res[n]: the residual read by a check at iteration count n
      while (ss >> r) res.push_back(strtod(r.c_str(), nullptr) * thr);
      WarpSched w;   // the state every solve path keeps per warp
      while (w.active(thr, iters)) {
        const WarpSched::Next nx = w.next(thr, iters, kmax, eps_pos);
        w.ran(nx);
        if (nx.calc_end) {
          w.read(res.at((size_t)w.n));
          printf("%d ", w.n);
        }
      }
      printf("| %d\n", w.n);
    } else if (cmd == "capsweep") {
      int w0, w1, h0, h1;
      ss >> w0 >> w1 >> h0 >> h1;
      const long c0 = g_cases, b0 = g_bad;
      capsweep(w0, w1, h0, h1);
      printf("%ld %ld\n", g_cases - c0, g_bad - b0);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
