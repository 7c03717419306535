// tvl1_batch_walk.hpp — the control flow of one pyramid level of one chunk of the batched solve
// (tvl1_calc_batch) as plain C++17: the pair selection the batched kernels take by value
// (BatchMask, BatchSel) and walk_batch_level, the warp loop over a small launch interface --
// the median, the fused first pass and its store-constants rule, the re-gather after a wrong
// store guess, and the rounds of passes grouped by their length.
//
// No HIP header, like tvl1_plan.hpp and tvl1_walk.hpp (the single-pair walker, whose WarpSched
// every pair of a chunk keeps here).  This loop decides, per pair, which u / p set a launch
// reads, whether p is still zero, whether the constants exist, which partials a reduce sums and
// when a residual may be read: a slip changes bits or reads a stale residual.  The engine is
// one backend (BatchOps); tests/batch_walk_model.cpp is the other, a symbolic device that
// follows every pair's buffer sets through scripted residuals on the CPU
// (tests/test_batch_walk_cpu.py).
#pragma once

#include <cstddef>

#include "tvl1_walk.hpp"

namespace tvl1k {

constexpr int kBatchMax = 256;

struct BatchMask {           // one bit per pair of a chunk
  uint64_t w[kBatchMax / 64];
  TVL1_HD int test(int b) const { return (int)((w[b >> 6] >> (b & 63)) & 1u); }
  TVL1_HD void set(int b) { w[b >> 6] |= 1ull << (b & 63); }
  TVL1_HD void clear(int b) { w[b >> 6] &= ~(1ull << (b & 63)); }
  TVL1_HD void flip(int b) { w[b >> 6] ^= 1ull << (b & 63); }
};

struct BatchSel {            // the pairs a launch works on, passed by value
  int n;                     // number of entries in idx
  uint8_t idx[kBatchMax];    // pair indices
  BatchMask ubit, pbit;      // per pair: current u set / p set (0 or 1)
  BatchMask cerr, pzero;     // per pair: the pass ends in a residual check / p == 0
  BatchMask storec;          // kb_warp_iter: per pair, store the warp constants to HBM
};

// the kernels read these from their argument block: the layout is part of every launch
static_assert(kBatchMax - 1 <= UINT8_MAX, "a pair index fits idx");
static_assert(sizeof(BatchMask) == 32, "BatchMask layout");
static_assert(sizeof(BatchSel) == 424, "BatchSel layout");
static_assert(offsetof(BatchSel, n) == 0 && offsetof(BatchSel, idx) == 4, "BatchSel layout");
static_assert(offsetof(BatchSel, ubit) == 264 && offsetof(BatchSel, pbit) == 296, "BatchSel layout");
static_assert(offsetof(BatchSel, cerr) == 328 && offsetof(BatchSel, pzero) == 360, "BatchSel layout");
static_assert(offsetof(BatchSel, storec) == 392, "BatchSel layout");

struct BatchWalkLevel {
  int n;   // pairs of the chunk
  int warps, iterations, kmax;
  double scaledEps;
  int eps_pos;
  bool fuse;         // warpBackward fused into every pair's first pass (2 iterations ending in the
                     // first check: needs eps_pos, kmax >= 2, iterations >= 2)
  bool median;       // the flow is median-filtered before every warp
  bool group;        // pairs grouped by their pass length, one launch per group; off:
                     // lock step, one launch of the shortest pass any active pair allows
  bool store_pred;   // a fused pass stores its constants only for pairs predicted to go on
};

// What a chunk carries from level to level, and the per-pair scratch of the current warp
// (allocated once per chunk: nothing is allocated inside a level).
struct BatchWalkState {
  explicit BatchWalkState(int n) : stopped_first(n, 0), sch(n), nx(n), act(n, 0) {
    all.n = n;
    for (int b = 0; b < n; ++b) all.idx[b] = (uint8_t)b;
  }
  BatchSel all{};            // every pair, no bit set
  BatchMask ubit{}, pbit{};  // per pair: the current u / p set
  BatchSel current() const {   // every pair, with its current u set
    BatchSel cur = all;
    cur.ubit = ubit;
    return cur;
  }
  void flip_u() {   // every pair's flow went to its other set (the median, the upsample)
    for (int b = 0; b < all.n; ++b) ubit.flip(b);
  }
  // per pair: its previous warp stopped at the first check, so this warp's fused pass is
  // predicted to stop there too and its constants are not stored (k_warp_iter's store_c rule,
  // DESIGN 4.5).  Consulted for a level's warps > 0 only, so the value a level leaves is never read.
  std::vector<char> stopped_first;
  std::vector<WarpSched> sch;        // each pair's procOneScale state in the current warp
  std::vector<WarpSched::Next> nx;   // ... and its next pass
  std::vector<char> act;             // ... and whether it is still in the warp's loop
};

struct BatchWalkCounts {   // per pair
  explicit BatchWalkCounts(int n) : checks(n, 0), regathers(n, 0), level_iters(n, 0) {}
  std::vector<int64_t> checks;
  std::vector<int64_t> regathers;     // constants not stored, then needed (re-gathered)
  std::vector<int64_t> level_iters;   // iterations of the level walked last
};

#define TVL1_WALK_TRY(expr)            \
  do {                                 \
    const tvl1_status r_ = (expr);     \
    if (r_ != TVL1_OK) return r_;      \
  } while (0)

// Ops, the backend: launches name pairs, buffer sets and flags only, through a BatchSel (each
// returns a tvl1_status):
//   median(sel)                   every pair's flow (set sel.ubit), median-filtered, into its other set
//   gather(sel)                   warpBackward of the pairs of sel: their constants from the flow sel.ubit
//   fused(sel, nstore, &blocks)   gather + the first 2 iterations + residual partials of every pair;
//                                 the nstore pairs of sel.storec store their constants
//   pass(K, sel, &blocks)         K iterations of the pairs of sel; those of sel.cerr leave `blocks`
//                                 residual partials each
//   reduce(sel, blocks, fused)    sums the partials of the pairs of sel (of the fused pass, or of
//                                 a pass) into their residual slots
//   sync(&residuals)              waits for everything enqueued; residuals (an Ops::Residuals)[b]:
//                                 pair b's slot
//   warp_done(b, wp, n)           pair b ran n iterations in warp wp
template <class Ops>
class BatchLevelWalk {
 public:
  BatchLevelWalk(Ops &ops, const BatchWalkLevel &lv, BatchWalkState &st, BatchWalkCounts &ct)
      : ops_(ops), lv_(lv), st_(st), ct_(ct) {
    for (int b = 0; b < lv.n; ++b) {
      pzero_.set(b);   // p = 0 at every level start
      ct.level_iters[b] = 0;
    }
  }

  tvl1_status run() {
    for (int wp = 0; wp < lv_.warps; ++wp) TVL1_WALK_TRY(warp(wp));
    return TVL1_OK;
  }

 private:
  Ops &ops_;
  const BatchWalkLevel &lv_;
  BatchWalkState &st_;
  BatchWalkCounts &ct_;
  BatchMask pzero_{};
  int nact_ = 0;   // pairs still in the current warp's loop

  void flip(int b) {   // a pass wrote pair b's other sets
    st_.ubit.flip(b);
    st_.pbit.flip(b);
    pzero_.clear(b);
  }
  // the pairs still in the loop after a pass (and its check)
  void count_active() {
    nact_ = 0;
    for (int b = 0; b < lv_.n; ++b) {
      if (!st_.act[b]) continue;
      st_.act[b] = st_.sch[b].active(lv_.scaledEps, lv_.iterations);
      nact_ += st_.act[b];
    }
  }

  tvl1_status warp(int wp) {
    const int n = lv_.n;
    BatchSel cur = st_.current();   // every pair, with its current buffer sets
    if (lv_.median) {
      TVL1_WALK_TRY(ops_.median(cur));
      st_.flip_u();
      cur.ubit = st_.ubit;
    }
    for (int b = 0; b < n; ++b) {
      st_.sch[b] = WarpSched{};
      st_.act[b] = lv_.iterations > 0;
    }
    if (lv_.fuse) {
      TVL1_WALK_TRY(fused_first(wp, cur));
    } else {
      TVL1_WALK_TRY(ops_.gather(cur));
      for (int b = 0; b < n; ++b) st_.stopped_first[b] = 0;
      nact_ = lv_.iterations > 0 ? n : 0;
    }
    while (nact_ > 0) TVL1_WALK_TRY(round());
    for (int b = 0; b < n; ++b) {
      ct_.level_iters[b] += st_.sch[b].n;
      ops_.warp_done(b, wp, st_.sch[b].n);
    }
    return TVL1_OK;
  }

  // warpBackward fused with the warp's first pass, which is 2 iterations ending in the first
  // check for every pair (procOneScale with epsilon > 0, iterations >= 2).  A pair stores its
  // constants unless its previous warp stopped at the first check; one that continues without
  // them is re-gathered from the flow the fused pass read.
  tvl1_status fused_first(int wp, BatchSel &cur) {
    const int n = lv_.n;
    auto stores = [&](int b) { return wp == 0 || !st_.stopped_first[b] || !lv_.store_pred; };
    cur.pbit = st_.pbit;
    cur.pzero = pzero_;
    int nstore = 0;
    for (int b = 0; b < n; ++b)
      if (stores(b)) {
        cur.storec.set(b);
        ++nstore;
      }
    int blocks = 0;
    TVL1_WALK_TRY(ops_.fused(cur, nstore, &blocks));
    TVL1_WALK_TRY(ops_.reduce(st_.all, blocks, true));
    typename Ops::Residuals res{};
    TVL1_WALK_TRY(ops_.sync(&res));
    BatchSel regather{};         // pairs that continue without stored constants
    regather.ubit = st_.ubit;    // the set the fused pass read
    for (int b = 0; b < n; ++b) {
      st_.sch[b].n = 2;
      flip(b);
      st_.sch[b].read(res[b]);
      ++ct_.checks[b];
    }
    count_active();
    for (int b = 0; b < n; ++b) {
      const bool stored = cur.storec.test(b) != 0;
      st_.stopped_first[b] = !st_.act[b];
      if (st_.act[b] && !stored) regather.idx[regather.n++] = (uint8_t)b;
    }
    if (regather.n > 0) {   // a wrong guess: gather the constants (k_warp_ring's body)
      TVL1_WALK_TRY(ops_.gather(regather));
      for (int j = 0; j < regather.n; ++j) ++ct_.regathers[regather.idx[j]];
    }
    return TVL1_OK;
  }

  // One round: each active pair's next pass (the single-pair rule, WarpSched: k iterations up to
  // and including its next check, at most kmax), one launch per pass length, then the checks.
  tvl1_status round() {
    const int n = lv_.n;
    int kmin = lv_.kmax;
    for (int b = 0; b < n; ++b) {
      st_.nx[b] = WarpSched::Next{0, false, 0.0};
      if (!st_.act[b]) continue;
      st_.nx[b] = st_.sch[b].next(lv_.scaledEps, lv_.iterations, lv_.kmax, lv_.eps_pos);
      kmin = std::min(kmin, st_.nx[b].k);
    }
    // lock step: the others split their pass (their schedule clipped to kmin iterations: no check)
    if (!lv_.group)
      for (int b = 0; b < n; ++b)
        if (st_.act[b] && st_.nx[b].k > kmin)
          st_.nx[b] = st_.sch[b].next(lv_.scaledEps, lv_.iterations, kmin, lv_.eps_pos);
    for (int K = 1; K <= lv_.kmax; ++K) {
      BatchSel sel{};
      BatchSel chk{};
      for (int b = 0; b < n; ++b) {
        if (!st_.act[b] || st_.nx[b].k != K) continue;
        sel.idx[sel.n++] = (uint8_t)b;
        if (st_.nx[b].calc_end) {
          sel.cerr.set(b);
          chk.idx[chk.n++] = (uint8_t)b;
        }
      }
      if (sel.n == 0) continue;
      sel.ubit = st_.ubit;
      sel.pbit = st_.pbit;
      sel.pzero = pzero_;
      int blocks = 0;
      TVL1_WALK_TRY(ops_.pass(K, sel, &blocks));
      if (chk.n > 0) TVL1_WALK_TRY(ops_.reduce(chk, blocks, false));
    }
    bool any_check = false;
    for (int b = 0; b < n; ++b) {
      if (!st_.act[b]) continue;
      st_.sch[b].ran(st_.nx[b]);
      flip(b);
      any_check = any_check || st_.nx[b].calc_end;
    }
    if (any_check) {
      typename Ops::Residuals res{};
      TVL1_WALK_TRY(ops_.sync(&res));
      for (int b = 0; b < n; ++b) {
        if (!st_.act[b] || !st_.nx[b].calc_end) continue;
        st_.sch[b].read(res[b]);
        ++ct_.checks[b];
      }
    }
    count_active();
    return TVL1_OK;
  }
};

// Every warp of one level of a chunk: from each pair's flow in its set st.ubit (p = 0) to the
// level's flow in st.ubit.
template <class Ops>
tvl1_status walk_batch_level(Ops &ops, const BatchWalkLevel &lv, BatchWalkState &st, BatchWalkCounts &ct) {
  return BatchLevelWalk<Ops>(ops, lv, st, ct).run();
}

#undef TVL1_WALK_TRY

}  // namespace tvl1k
