// tvl1_plan.hpp — host planning of the TV-L1 solves as plain C++17: the pyramid, procOneScale's
// pass schedule, the launch geometry of every kernel family, the residual-partial capacities the
// arenas reserve for them, the profiling byte models and the speculation predictor.
//
// No HIP header: this compiles with any C++17 compiler, so tests/test_plan_cpu.py pins its
// numbers on the CPU (tests/plan_dump.cpp).  Nothing here changes a result: segmentation and
// the predictor's guesses only decide how fast the same bits are computed, which is why the GPU
// parity tests cannot see a slip in them.  (The loop that acts on the guesses can change bits:
// tvl1_walk.hpp, with a model test of its own.)  tvl1_kernels.hpp includes this header for the
// constants the kernels share with the plan and for sched_after and gate_holds, which k_reduce
// evaluates on the device.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/tvl1.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TVL1_HD __host__ __device__
#else
#define TVL1_HD
#endif

namespace tvl1k {

constexpr int kWave = 64;
constexpr int kSegPx = (kWave - 2) * 4;     // 248 useful px per wave (lanes 1..62)
constexpr int kStripRows = 32;   // rows per wave strip in k_iterate
constexpr int kTbMax = 4;        // max iterations fused per pass in k_iterate_tb
constexpr int kRollMax = 4;      // ... and in k_iterate_roll
constexpr int kRollMinSeg = 8;   // smallest k_iterate_roll segment (rows)
constexpr int kTbRows = 32;      // rows of a k_iterate_tb region (64 x 32, 2 px per lane)
constexpr int kTb4Groups = 16;   // row groups (threads per column) of a region (32: -6 %, r5)
constexpr int kTb4RowsPerThread = 3;

// ---------------------------------------------------------------- schedule
// procOneScale's schedule from a residual: iterations up to and including the next check.
// One definition for the host schedule (single-pair and batched), the speculation predictor
// and k_reduce's evaluation of a speculation gate on the device: the same double operations.
// prev_end: prevError as procOneScale would hold it after those iterations.
TVL1_HD inline int sched_after(double prev, double thr, int n, int iters, int kmax, int eps_pos,
                               bool *calc_end, double *prev_end) {
  int k = 0;
  bool ce = false;
  while (k < kmax && n + k < iters) {
    const bool calc = eps_pos && ((n + k) & 1) && prev < thr;
    ++k;
    if (calc) {
      ce = true;
      break;
    }
    prev -= thr;
  }
  *calc_end = ce;
  *prev_end = prev;
  return k;
}

// Whether the prediction (pk, pcalc) for what follows a check that read e at iteration count n
// is what procOneScale does: pk = 0, the warp stops here; pk > 0, it continues
// with a pass of pk iterations that ends in a check (pcalc) or not.  One definition for
// k_reduce's evaluation of a speculation gate and for the host's verdict on its guess.
TVL1_HD inline bool gate_holds(double e, double thr, int n, int iters, int kmax, int eps_pos, int pk,
                               int pcalc) {
  const bool ends = !(e > thr && n < iters);
  bool ok = ends;
  if (pk > 0) {
    bool ce;
    double pe;
    const int k = sched_after(e, thr, n, iters, kmax, eps_pos, &ce, &pe);
    ok = !ends && k == pk && (int)ce == pcalc;
  }
  return ok;
}

// Pyramid sizes exactly as calcImpl: round-half-even(cols*step), stop < 16.
inline int pyramid_sizes(int w, int h, int nscales, double step, int *ws, int *hs) {
  int L = nscales < TVL1_MAX_LEVELS ? nscales : TVL1_MAX_LEVELS;
  ws[0] = w;
  hs[0] = h;
  for (int s = 1; s < L; ++s) {
    const int nw = (int)std::lrint((double)ws[s - 1] * step);
    const int nh = (int)std::lrint((double)hs[s - 1] * step);
    if (nw < 16 || nh < 16) return s;
    ws[s] = nw;
    hs[s] = nh;
  }
  return L;
}

// resize(): an exact 2x downscale of INTER_LINEAR takes the INTER_AREA fast path
inline int area_fast_of(double sx, double sy) {
  const int ix = (int)std::lrint(sx), iy = (int)std::lrint(sy);
  return std::fabs(sx - ix) < DBL_EPSILON && std::fabs(sy - iy) < DBL_EPSILON && ix == 2 && iy == 2;
}

// IterArgs::taut_small: the projection's ng = 1 + taut*g ignores g below 2^-48 when |taut|
// <= 2^20, so sqrt_nn may skip its (0, 2^-96) form (tvl1_kernels.hpp, sqrt_nn); NaN: false
inline int taut_small(float taut) { return std::fabs(taut) <= 0x1p20f ? 1 : 0; }

// ---------------------------------------------------------------- streaming launches
// Rows per k_iterate_roll segment.  Every wavefront runs (rows + 2K) steps, so the pass
// takes about rounds x (rows + 2K) step times, rounds = ceil(wavefronts / resident slots):
// pick the split into segments that minimises that (a partial last round idles most of
// the device; short segments repeat the 2K-row halo).
inline int roll_segment(int bands, int lh, int k, int slots) {
  if (slots <= 0) slots = 4096;
  int best = lh;
  long best_cost = -1;
  for (int R = 1; R <= 4; ++R) {
    const int segs = std::max(1, R * slots / bands);
    const int seg = std::max(kRollMinSeg, (lh + segs - 1) / segs);
    const long waves = (long)bands * ((lh + seg - 1) / seg);
    const long rounds = (waves + slots - 1) / slots;
    const long cost = rounds * (seg + 2 * k);
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best = seg;
    }
  }
  return best;
}

// A streaming launch (k_warp_ring, k_warp_iter, k_iterate_roll and their batched forms): bands
// of out_w output px down the level, cut into segments of seg_rows rows, one wavefront (or
// block) per band and segment.
struct StreamPlan {
  int bands, seg_rows, waves;
};

// k: the iterations' worth of halo rows a segment repeats; slots: the resident wavefronts the
// launch is sized for; roll_seg: the TVL1_ROLL_SEG override (0: roll_segment's choice, never
// below seg_floor); pairs: the pairs of a batched launch (each runs the plan's wavefronts).
inline StreamPlan stream_plan(int lw, int lh, int out_w, int k, int slots, int roll_seg,
                              int seg_floor = 0, int pairs = 1) {
  StreamPlan p;
  p.bands = (lw + out_w - 1) / out_w;
  p.seg_rows = roll_seg > 0 ? std::max(roll_seg, kRollMinSeg)
                            : std::max(roll_segment(p.bands * pairs, lh, k, slots), seg_floor);
  p.waves = p.bands * ((lh + p.seg_rows - 1) / p.seg_rows);
  return p;
}

// share of the resident slots a single-pair streaming launch is sized for (TVL1_FILL, %)
inline int fill_slots(int slots, int fill) { return slots * fill / 100; }

// The launch sites.  slots: the resident wavefronts (blocks) of the kernel the launch is sized
// for -- a single-pair solve passes fill_slots() of them; the batched gathers and fused passes
// take no TVL1_ROLL_SEG override (roll_seg 0).
// k_warp_ring<M, ..> / kb_warp_ring: 64-px bands with no x halo, M rows of window above and below
inline StreamPlan plan_warp_ring(int lw, int lh, int m, int slots, int roll_seg, int pairs = 1) {
  return stream_plan(lw, lh, 64, m, slots, roll_seg, 0, pairs);
}
// k_warp_iter<M, FM, BW, ..> / kb_warp_iter: BW-px bands of 2 iterations (2 px of halo a side)
inline StreamPlan plan_warp_iter(int lw, int lh, int bw, int m, int slots, int roll_seg, int pairs = 1) {
  return stream_plan(lw, lh, bw - 4, 2 + m, slots, roll_seg, 0, pairs);
}
// k_iterate_roll<G, K, PX> (and _mid: K 4, PX 2) / kb_iterate_roll<K, PX>: 64 lanes of PX px,
// the K-px halo rounded up to whole lanes (roll_halo<K, PX>)
constexpr int roll_halo_of(int k, int px) { return (k + px - 1) / px * px; }
inline StreamPlan plan_roll(int lw, int lh, int k, int px, int slots, int roll_seg, int seg_floor = 0,
                            int pairs = 1) {
  return stream_plan(lw, lh, 64 * px - 2 * roll_halo_of(k, px), k, slots, roll_seg, seg_floor, pairs);
}

// k_iterate_stages<FM, K> (K = 2 or 4, gamma = 0): a block of K wavefronts per 128-px band
// (2 px per lane, the halo of k_iterate_roll<false, K, 2>) and segment; stage n works 2 (n - 1)
// rows behind stage 1.  A segment's block starts at input row stages_r0 and runs
// stages_steps steps (whole trips of stage 1's 3-row load ring): stage 1 has then passed row
// ye - 1 + K and the last stage row ye, where it stores p^K(ye - 1).
TVL1_HD inline int stages_r0(int ys, int k) { return ys - k > 0 ? ys - k : 0; }
TVL1_HD inline int stages_steps(int ys, int ye, int k) {
  return (ye - stages_r0(ys, k) + 2 * k - 1 + 2) / 3 * 3;
}
// share of the resident blocks a launch is sized for while other solves share the device
// (TVL1_FILL_SHARED's 60 % gives 47-row segments on a 4.2 Mpx level, 1.23 x their rows in
// steps; 45 %: 63 rows, 1.17 x)
constexpr int kStagesFillShared = 45;
constexpr int stages_out_w(int k) { return 128 - 2 * roll_halo_of(k, 2); }
// slots: the resident blocks the launch is sized for.  roll_segment's cost of a segment is
// rows + 2 k' steps; a stage block runs rows + 3 K - 1, so k' = ceil(3 K / 2)
inline StreamPlan plan_stages(int lw, int lh, int k, int slots, int roll_seg) {
  return stream_plan(lw, lh, stages_out_w(k), (3 * k + 1) / 2, slots, roll_seg);
}

// ---------------------------------------------------------------- blocked passes
// k_iterate (one iteration, exact division): blocks of 4 wave strips
inline int iterate_blocks(int W, int H) {
  const int segs = (W + kSegPx - 1) / kSegPx;
  const int strips = (H + kStripRows - 1) / kStripRows;
  const int waves = segs * strips;
  return (waves + 3) / 4;
}

// k_iterate_tb (64 x kTbRows regions) and k_iterate_tb4 (64 x 48): k iterations shrink a
// region by k px on every side
struct BlockedPlan {
  int tiles_x, out_h, blocks;
};
inline BlockedPlan blocked_plan(int lw, int lh, int region_rows, int k) {
  BlockedPlan b;
  b.tiles_x = (lw + 55) / 56;
  b.out_h = region_rows - 2 * k;
  b.blocks = b.tiles_x * ((lh + b.out_h - 1) / b.out_h);
  return b;
}
inline BlockedPlan tb_plan(int lw, int lh, int k) { return blocked_plan(lw, lh, kTbRows, k); }
inline BlockedPlan tb4_plan(int lw, int lh, int k) {
  return blocked_plan(lw, lh, kTb4Groups * kTb4RowsPerThread, k);
}

// ---------------------------------------------------------------- partial capacities
// Residual partials a W x H frame reserves (one per block or wavefront of a pass; the
// mid-check pass takes two per wavefront).  Single pair: k_iterate_tb's worst case (RH 32 at
// 4 iterations: 56 x 24 px per block), k_iterate_roll's (56-px bands, segments of
// kRollMinSeg rows).
inline int partials_capacity(int W, int H) {
  const int tb_blocks = ((W + 55) / 56) * ((H + 23) / 24);
  const int roll_waves = ((W + 55) / 56) * ((H + kRollMinSeg - 1) / kRollMinSeg);
  return std::max(std::max(iterate_blocks(W, H), tb_blocks), roll_waves) + 64;
}
// per pair of a batch: blocked regions (56 x 24 px) or rolling / fused waves (>= 56-px bands
// x >= 8-row segments)
inline int batch_partials_capacity(int W, int H) {
  return std::max(((W + 55) / 56) * ((H + 23) / 24), ((W + 55) / 56) * ((H + 7) / 8)) + 64;
}

// ---------------------------------------------------------------- byte models (profiling)
// SURVEY 8(d) byte model with executed iteration counts (reported in stats).
inline double survey_bytes(int L, const int *ws, const int *hs, int warps, const int64_t *iters) {
  double B = 0.0;
  for (int l = 0; l < L; ++l) {
    const double N = (double)ws[l] * hs[l];
    B += N * (12.0 + 16.0 + 40.0 * warps + 64.0 * (double)iters[l]);
    if (l >= 1) B += N * 8.0;
    if (l < L - 1) B += N * 8.0;
  }
  const double N0 = (double)ws[0] * hs[0];
  B += N0 * (2.0 + 8.0) + N0 * 8.0;
  return B;
}

// rows a band's lanes load over a level: every segment's rows plus its halo (clipped)
inline double rows_with_halo(int lh, int seg, int halo) {
  const int segs = (lh + seg - 1) / seg;
  double rows = 0.0;
  for (int sg = 0; sg < segs; ++sg) {
    const int ys = sg * seg, ye = std::min(ys + seg, lh);
    rows += std::min(ye - 1 + halo, lh - 1) - std::max(ys - halo, 0) + 1;
  }
  return rows;
}

// planes an iteration pass loads and stores per px: the warp constants, u and (unless p = 0) p
struct PassPlanes {
  double ld, st;
};
inline PassPlanes pass_planes(bool gam, bool p_zero) {
  const int nu = gam ? 3 : 2, np = gam ? 6 : 4;
  return {(double)(3 + nu + (p_zero ? 0 : np)), (double)(nu + np)};
}

// Compulsory HBM bytes of the fused warp pass (k_warp_iter<M, FM, bw, ..>, window width ww):
// p, u, I0 and the I1 window (x 1 + 2M/BW) per band column and row; u, p (+ the constants) stored
inline double warp_iter_hbm(const StreamPlan &p, int lh, int bw, int ww, double Nl, bool p_zero,
                            bool store_c) {
  const double rows = rows_with_halo(lh, p.seg_rows, 2);
  return (double)p.bands * bw * rows * 4.0 * ((p_zero ? 3 : 7) + (double)ww / bw) +
         Nl * 4.0 * (6.0 + (store_c ? 3.0 : 0.0));
}
// ... of kb_warp_iter's n pairs, nz of them with p = 0, nstore storing the constants
inline double batch_warp_iter_hbm(const StreamPlan &p, int lh, int ww, double Nl, int n, int nz,
                                  int nstore) {
  const double rows = rows_with_halo(lh, p.seg_rows, 2);
  const double band_bytes = (double)p.bands * 128 * rows * 4.0;
  return band_bytes * ((double)nz * 3 + (double)(n - nz) * 7 + (double)n * ww / 128) +
         Nl * 4.0 * (6.0 * n + 3.0 * nstore);
}
// Streaming pass of k iterations (k_iterate_roll<G, k, px>): every band lane loads its column
// over the segment's rows + halo
inline double roll_hbm(const StreamPlan &p, int lh, int k, int px, double Nl, const PassPlanes &pl) {
  const double rows = rows_with_halo(lh, p.seg_rows, k);
  return (double)p.bands * 64.0 * px * rows * 4.0 * pl.ld + Nl * 4.0 * pl.st;
}
// k_iterate_stages<FM, k>: stage 1 loads what k_iterate_roll<false, k, 2>'s wavefront loads (the
// later stages read LDS only), the last stage stores the interior
inline double stages_hbm(const StreamPlan &p, int lh, int k, double Nl, const PassPlanes &pl) {
  return roll_hbm(p, lh, k, 2, Nl, pl);
}
// ... of kb_iterate_roll's n pairs (gamma = 0), nz of them with p = 0
inline double batch_roll_hbm(const StreamPlan &p, int lh, int k, int px, double Nl, int n, int nz) {
  const double rows = rows_with_halo(lh, p.seg_rows, k);
  const double band_bytes = (double)p.bands * 64 * px * rows * 4.0;
  return band_bytes * ((double)n * 5 + (double)(n - nz) * 4) + (double)n * Nl * 4.0 * 6.0;
}
// Blocked pass (k_iterate_tb, k_iterate_tb4): every staged region cell loads I1wx, I1wy, rho, u
// (+p unless p == 0), every px stores u and p once per pass
inline double blocked_hbm(int blocks, int region_rows, double Nl, const PassPlanes &pl) {
  return (double)blocks * 64.0 * region_rows * 4.0 * pl.ld + Nl * 4.0 * pl.st;
}
// k one-iteration launches (k_iterate)
inline double iterate_hbm(double Nl, int k, const PassPlanes &pl) { return Nl * 4.0 * (pl.ld + pl.st) * k; }

// ---------------------------------------------------------------- speculation predictor
// Guesses of the launch that follows a residual check, for one level.  A warp's
// residual (in units of eps^2 W H) after its first check falls steadily, so: the action the
// level's previous warp took at the same iteration count; else the next residual extrapolated
// from the last two (the check after a long run of unchecked iterations comes where the
// schedule's linear model crosses 1: guess a stop); a level's first warp starts where the
// previous level's did (w0_hint, which the solve carries from level to level).
struct Predictor {
  struct Hist {
    double r0 = -1.0, r1 = -1.0;   // the warp's last two residuals / (eps^2 W H); < 0: none
    int n0 = -1, n_last = -1;      // iteration counts at those checks
  };
  int iterations, kmax, warps;
  double scaledEps;
  bool spec_ok, spec_stop_ok, mid;   // mid: 2-iteration continuations may run as mid-check passes
  double w0_hint;   // residual / (eps^2 W H) at a level's first check
  // actions by iteration count of the level's previous and current warp (remembered up to
  // 4096 iterations: a huge `iterations` must not size a huge table)
  std::vector<int> act_prev, act_cur;

  Predictor(int iterations_, int kmax_, double scaledEps_, int warps_, bool spec_ok_,
            bool spec_stop_ok_, bool mid_, double w0_hint_)
      : iterations(iterations_), kmax(kmax_), warps(warps_), scaledEps(scaledEps_), spec_ok(spec_ok_),
        spec_stop_ok(spec_stop_ok_), mid(mid_), w0_hint(w0_hint_),
        act_prev((size_t)std::min(iterations_, 4096) + 1, -2), act_cur(act_prev) {}

  // the residual expected at the check after one at n (the warp's history up to that check)
  double extrapolate(const Hist &h, int n, int wp) const {
    if (h.r1 < 0) return wp == 0 ? w0_hint : 1.5;
    if (n - h.n_last > 2) return 0.9;   // a long unchecked run ends near the model's crossing
    if (h.r0 >= 0 && h.n_last - h.n0 == 2) return h.r1 * (h.r1 / h.r0);   // steady decay
    return h.n_last == 2 ? h.r1 * 0.6 : h.r1 * 0.93;   // after a warp's first check: a drop
  }
  int act_of(double e, int n) const {   // 0: stop, else k << 1 | calc_end
    if (!(e > scaledEps && n < iterations)) return 0;
    bool ce;
    double pe;
    return sched_after(e, scaledEps, n, iterations, kmax, 1, &ce, &pe) << 1 | (ce ? 1 : 0);
  }
  // the bookkeeping of a check read at iteration count n
  void note(Hist &h, double e, int n) {
    h.r0 = h.r1;
    h.n0 = h.n_last;
    h.r1 = e / scaledEps;
    h.n_last = n;
    if ((size_t)n < act_cur.size()) act_cur[n] = act_of(e, n);
  }
  // the speculative launch behind a check guessed that the warp stops at n
  void note_stop_guess(int n) {
    if ((size_t)n < act_cur.size()) act_cur[n] = 0;
  }
  void next_warp() {
    act_prev.swap(act_cur);
    std::fill(act_cur.begin(), act_cur.end(), -2);
  }
  // What to predict after a check at iteration count n of warp wp: pk = 0 the warp stops (its
  // successor's first pass follows), pk > 0 it continues with (pk, pcalc), -1 nothing.
  // alone: no other solve of this process shares the device (or TVL1_SPEC=2); nostore: the
  // warp's fused first pass did not store its constants; last_n: iterations of the level's
  // previous warp; cur: the previous warp is the one still being recorded (act_cur).
  void predict0(int wp, int n, bool alone, bool nostore, int last_n, const Hist &h, bool cur,
                int &pk, int &pcalc) const {
    const std::vector<int> &prevw = cur ? act_cur : act_prev;
    pk = -1;
    pcalc = 0;
    if (!spec_ok) return;
    if (!alone) return;
    const bool can_stop = spec_stop_ok && wp + 1 < warps;
    const bool can_cont = !nostore && n < iterations;
    if (can_stop && (n >= iterations || (n == 2 && last_n == 2))) {
      pk = 0;
      return;
    }
    const int ap = wp >= 2 && n < (int)prevw.size() ? prevw[n] : -2;
    if (ap == 0 && can_stop) {
      pk = 0;
      return;
    }
    if (ap > 0 && can_cont) {
      pk = ap >> 1;
      pcalc = ap & 1;
      return;
    }
    const double r = extrapolate(h, n, wp);
    if (r <= 1.0 && can_stop) {
      pk = 0;
    } else if (can_cont) {
      const int a = act_of(std::max(r, 1.0 + 1e-9) * scaledEps, n);
      pk = a >> 1;
      pcalc = a & 1;
    } else if (can_stop) {
      pk = 0;
    }
  }
  // a predicted 2-iteration continuation after a warp's first check is left to the host,
  // which may run it as a mid-check pass (less GPU work than the pass enqueued ahead)
  void predict(int wp, int n, bool alone, bool nostore, int last_n, const Hist &h, bool cur, int &pk,
               int &pcalc) const {
    predict0(wp, n, alone, nostore, last_n, h, cur, pk, pcalc);
    if (mid && pk == 2 && pcalc && n > 2) pk = -1;
  }
};

}  // namespace tvl1k
