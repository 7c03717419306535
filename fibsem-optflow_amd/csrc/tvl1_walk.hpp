// tvl1_walk.hpp — the control flow of one pyramid level of a single-pair solve as plain C++17:
// procOneScale's per-warp state (WarpSched) and walk_level, the warp loop over a small launch
// interface -- the fused first pass and its store-constants rule, the mid-check pass, and
// speculation: the launch enqueued behind a check, its own check behind that, and
// the reconciliation after the read.  (The batched solve's level walker, which keeps one
// WarpSched per pair and shares nothing else, is tvl1_batch_walk.hpp.)
//
// No HIP header, like tvl1_plan.hpp.  Unlike the plan, this loop decides which buffer sets a
// launch reads, which constants are current and which check the host waits for: a slip here
// changes bits or hangs.  The engine is one backend; tests/walk_model.cpp is the other, a
// symbolic device that follows every buffer set through scripted residuals on the CPU
// (tests/test_walk_cpu.py).
#pragma once

#include <cstdio>

#include "tvl1_plan.hpp"

namespace tvl1k {

// procOneScale's loop state of one warp of one pair: for (n = 0; error > thr && n < iterations;)
struct WarpSched {
  int n = 0;
  double error = DBL_MAX, prevError = 0.0;
  // the iterations up to and including the next check (sched_after), at most kmax
  struct Next {
    int k;
    bool calc_end;
    double prev_end;   // prevError after them
  };
  bool active(double thr, int iterations) const { return error > thr && n < iterations; }
  Next next(double thr, int iterations, int kmax, int eps_pos) const {
    Next p{0, false, prevError};
    p.k = sched_after(prevError, thr, n, iterations, kmax, eps_pos, &p.calc_end, &p.prev_end);
    return p;
  }
  // the pass ran; one without a check leaves no residual (one with: read() follows)
  void ran(const Next &p) {
    n += p.k;
    if (p.calc_end) return;
    error = DBL_MAX;
    prevError = p.prev_end;
  }
  void read(double e) { error = prevError = e; }   // the check at n read e
};

// One iteration pass: k iterations (ending in a check if calc_end) from the buffer sets
// (ui, pi) into (ui ^ 1, pi ^ 1), with the constants of set cb.  witer: the warp's first pass
// with warpBackward fused in, which stores the constants it computes only with store_c; mid:
// a mid-check pass (4 iterations, the residuals after 2 and after 4, the input sets left as
// they were); gated: a speculative launch, which runs only if the check gseq found its
// prediction right.
struct PassReq {
  int k;
  bool calc_end;
  int ui, pi, cb;
  bool p_zero, witer, store_c, mid, gated;
  unsigned long long gseq;
};

// One residual check over the `blocks` partials from `first` on, at iteration count n.
// gated_in: enqueued behind the check in_seq, and runs only if that one's prediction held;
// gate_out: evaluates the prediction (pk, pcalc) for the launch enqueued behind it (gate_holds).
struct CheckReq {
  int blocks, first;
  bool gated_in;
  unsigned long long in_seq;
  bool gate_out;
  int n, pk, pcalc;
};

struct WalkLevel {
  int level;   // (for the trace)
  int warps, iterations, kmax;
  double scaledEps;
  int eps_pos;
  bool fuse;     // warpBackward fused into a warp's first pass (2 iterations ending in a check:
                 // needs eps_pos, kmax >= 2, iterations >= 2)
  bool median;   // the flow is median-filtered before every warp
  bool spec;     // launches may be enqueued behind a check (needs eps_pos, kmax >= 2)
  bool mid;      // 2-iteration continuations may run as mid-check passes (needs eps_pos, kmax >= 4)
  double mid_min;   // ... when the check before them read at least this, in units of scaledEps
  bool spec_trace;
};

// what a solve carries from level to level
struct WalkState {
  int ui, pi;   // ping-pong indices of the u and p buffer sets
  int cb;       // constants buffer (I1wx, I1wy, rho) of the current warp
  double w0_hint;   // speculation: residual / (eps^2 W H) at a level's first check
};

struct WalkCounts {
  int64_t checks = 0;
  int32_t spec_misses = 0;   // speculative launches that ran empty
  int mid_passes = 0, mid_taken = 0;   // mid-check passes; of those, ended on the mid state
  int64_t level_iters = 0;
};

#define TVL1_WALK_TRY(expr)            \
  do {                                 \
    const tvl1_status r_ = (expr);     \
    if (r_ != TVL1_OK) return r_;      \
  } while (0)

// Ops, the backend (each launch returns a tvl1_status):
//   median(ui)                    the flow of set ui, median-filtered, into set ui ^ 1
//   gather(ui, cb, wp)            warpBackward of warp wp: the constants cb from the flow ui
//   pass(req, wp, n, &blocks)     a pass at iteration count n; blocks: its partials (per check)
//   check(req, &seq)              enqueues a check, seq: its sequence number
//   wait(seq, &e)                 the residual of check seq, once it is there
//   mark() / rollback(mark)       forget the bookkeeping of launches that ran empty
//   alone()                       no other solve shares the device (speculation pays)
//   trace(line), warp_done(wp, n)
template <class Ops>
class LevelWalk {
 public:
  LevelWalk(Ops &ops, const WalkLevel &lv, WalkState &st, WalkCounts &ct)
      : ops_(ops), lv_(lv), st_(st), ct_(ct),
        pred_(lv.iterations, lv.kmax, lv.scaledEps, lv.warps, lv.spec,
              lv.spec && !lv.median && lv.iterations >= 2, lv.mid, st.w0_hint) {}

  tvl1_status run() {
    for (int wp = 0; wp < lv_.warps; ++wp) TVL1_WALK_TRY(warp(wp));
    return TVL1_OK;
  }

 private:
  using Hist = Predictor::Hist;
  // a check enqueued and not yet read, with the prediction its gate evaluates
  struct Check {
    unsigned long long seq = 0;
    int pk = -1, pcalc = 0;
  };

  Ops &ops_;
  const WalkLevel &lv_;
  WalkState &st_;
  WalkCounts &ct_;
  Predictor pred_;
  bool p_zero_ = true;     // p = 0 at the start of every level (setTo(0) in procOneScale)
  int last_warp_n_ = -1;   // iterations of the level's previous warp
  // a warp whose first pass (and check) the previous warp enqueued speculatively
  bool pre_ = false, pre_nostore_ = false;
  Check pre_chk_;
  // the current warp
  int wp_ = 0;
  WarpSched w_;
  Hist h_;
  bool fused_nostore_ = false;   // its fused first pass ran without storing the constants
  bool pending_ = false;
  Check pend_;

  void flip() {   // a pass (or the median) wrote the other sets
    st_.ui ^= 1;
    st_.pi ^= 1;
    p_zero_ = false;
  }

  tvl1_status warp(int wp) {
    wp_ = wp;
    w_ = WarpSched{};
    h_ = Hist{};
    fused_nostore_ = pending_ = false;
    if (pre_) {
      w_.n = 2;
      fused_nostore_ = pre_nostore_;
      pending_ = true;
      pend_ = pre_chk_;
      pre_ = false;
    } else {
      if (lv_.median) {
        TVL1_WALK_TRY(ops_.median(st_.ui));
        st_.ui ^= 1;
      }
      if (!lv_.fuse) TVL1_WALK_TRY(ops_.gather(st_.ui, st_.cb, wp));
    }
    // (pre_: this warp stopped where predicted, and the next warp has begun)
    while (!pre_ && (pending_ || w_.active(lv_.scaledEps, lv_.iterations))) {
      if (!pending_) {
        const WarpSched::Next nx = w_.next(lv_.scaledEps, lv_.iterations, lv_.kmax, lv_.eps_pos);
        if (mid_applies(nx))
          TVL1_WALK_TRY(mid_pass());
        else
          TVL1_WALK_TRY(own_pass(nx));
        if (!pending_) continue;
      }
      TVL1_WALK_TRY(read_check());
    }
    ct_.level_iters += w_.n;
    last_warp_n_ = w_.n;
    ops_.warp_done(wp, w_.n);
    st_.cb ^= 1;   // every warp gets the other constants buffer
    pred_.next_warp();
    return TVL1_OK;
  }

  // the warp's next pass as the schedule has it, and its check (with a prediction to gate)
  tvl1_status own_pass(const WarpSched::Next &nx) {
    const bool witer = lv_.fuse && w_.n == 0 && nx.k == 2 && nx.calc_end;
    // the constants go to HBM only when the warp may run further passes: always for a level's
    // first warp, else when the previous warp did not stop at its first check (a wrong guess
    // recomputes them with the warp kernel after the check)
    const bool store_c = wp_ == 0 || last_warp_n_ != 2;
    int blocks = 0;
    TVL1_WALK_TRY(ops_.pass(PassReq{nx.k, nx.calc_end, st_.ui, st_.pi, st_.cb, p_zero_, witer,
                                    witer && store_c, false, false, 0},
                            wp_, w_.n, &blocks));
    if (witer) fused_nostore_ = !store_c;
    flip();
    w_.ran(nx);
    if (!nx.calc_end) return TVL1_OK;
    pred_.predict(wp_, w_.n, ops_.alone(), fused_nostore_, last_warp_n_, h_, false, pend_.pk, pend_.pcalc);
    TVL1_WALK_TRY(ops_.check(CheckReq{blocks, 0, false, 0, pend_.pk >= 0, w_.n, pend_.pk, pend_.pcalc},
                             &pend_.seq));
    pending_ = true;
    return TVL1_OK;
  }

  // A converging warp (a check every second iteration, the error just above eps^2 W H) runs
  // its next two 2-iteration passes as one mid-check pass: both checks' residuals and the
  // state after 4 iterations in the usual set.  Not for a warp's first check (n = 2: its
  // error drops the most).
  bool mid_applies(const WarpSched::Next &nx) const {
    return lv_.mid && nx.k == 2 && nx.calc_end && w_.n > 2 && w_.n + 4 <= lv_.iterations &&
           w_.prevError >= lv_.mid_min * lv_.scaledEps;
  }
  // The host reads the first check as procOneScale does; if the warp stops there (or its
  // schedule is not a second 2-iteration pass) a 2-iteration pass from the same input set,
  // which the mid-check pass leaves as it was, recomputes the state at that check (DESIGN.md
  // §4.1 of r6).
  tvl1_status mid_pass() {
    int blocks = 0;
    TVL1_WALK_TRY(ops_.pass(PassReq{4, true, st_.ui, st_.pi, st_.cb, p_zero_, false, false, true, false, 0},
                            wp_, w_.n, &blocks));
    unsigned long long seq_mid = 0, seq_end = 0;
    TVL1_WALK_TRY(ops_.check(CheckReq{blocks, blocks, false, 0, false, 0, -1, 0}, &seq_mid));
    TVL1_WALK_TRY(ops_.check(CheckReq{blocks, 0, false, 0, false, 0, -1, 0}, &seq_end));
    double e = 0.0;
    TVL1_WALK_TRY(ops_.wait(seq_mid, &e));
    w_.n += 2;
    w_.read(e);
    ++ct_.checks;
    pred_.note(h_, e, w_.n);
    ++ct_.mid_passes;
    const WarpSched::Next nx = w_.next(lv_.scaledEps, lv_.iterations, lv_.kmax, 1);
    if (w_.active(lv_.scaledEps, lv_.iterations) && nx.k == 2 && nx.calc_end) {
      TVL1_WALK_TRY(ops_.wait(seq_end, &e));   // the second check: the next pass's own
      w_.n += 2;
      w_.read(e);
      ++ct_.checks;
      pred_.note(h_, e, w_.n);
    } else {   // the state at the first check: its 2 iterations again, no residual
      ++ct_.mid_taken;
      TVL1_WALK_TRY(ops_.pass(PassReq{2, false, st_.ui, st_.pi, st_.cb, false, false, false, false, false, 0},
                              wp_, w_.n - 2, &blocks));
    }
    flip();
    return TVL1_OK;
  }

  // The launch(es) predicted to follow the check chk of this warp at w_.n, gated on it: the
  // next warp's first pass and check (pk = 0) or this warp's next pass (and check).  next: the
  // check enqueued behind, with its own prediction; nostore: a next warp's fused pass that
  // does not store its constants.
  tvl1_status speculate(const Check &chk, Check &next, bool &nostore) {
    int blocks = 0;
    if (chk.pk == 0) {
      const int w2 = wp_ + 1, cb2 = st_.cb ^ 1;
      const bool store2 = w_.n != 2;   // the fused pass's store rule, if this warp stops here
      // the gather is not gated (a gate check costs k_warp_ring 34 VGPRs): after a wrong
      // guess it has only filled the constants set the next warp recomputes anyway
      if (!lv_.fuse) TVL1_WALK_TRY(ops_.gather(st_.ui, cb2, w2));
      TVL1_WALK_TRY(ops_.pass(PassReq{2, true, st_.ui, st_.pi, cb2, false, lv_.fuse, lv_.fuse && store2,
                                      false, true, chk.seq},
                              w2, 0, &blocks));
      nostore = lv_.fuse && !store2;
      pred_.note_stop_guess(w_.n);   // (as guessed; recorded after the read)
      pred_.predict(w2, 2, ops_.alone(), nostore, w_.n, Hist{}, true, next.pk, next.pcalc);
      TVL1_WALK_TRY(ops_.check(CheckReq{blocks, 0, true, chk.seq, next.pk >= 0, 2, next.pk, next.pcalc},
                               &next.seq));
    } else if (chk.pk > 0) {
      TVL1_WALK_TRY(ops_.pass(PassReq{chk.pk, chk.pcalc != 0, st_.ui, st_.pi, st_.cb, false, false, false,
                                      false, true, chk.seq},
                              wp_, w_.n, &blocks));
      if (chk.pcalc) {
        Hist h2;   // with this check's residual extrapolated
        h2.r0 = h_.r1;
        h2.n0 = h_.n_last;
        h2.r1 = h_.r1 < 0 ? -1.0 : pred_.extrapolate(h_, w_.n, wp_);
        h2.n_last = w_.n;
        const int n2 = w_.n + chk.pk;
        pred_.predict(wp_, n2, ops_.alone(), false, last_warp_n_, h2, false, next.pk, next.pcalc);
        TVL1_WALK_TRY(ops_.check(CheckReq{blocks, 0, true, chk.seq, next.pk >= 0, n2, next.pk, next.pcalc},
                                 &next.seq));
      }
    }
    return TVL1_OK;
  }

  // The pending check: enqueue what is predicted to follow it, read it (the cuda::sum -> host
  // read of procOneScale), and take up the speculative work if the guess was right.
  tvl1_status read_check() {
    pending_ = false;
    const Check chk = pend_;
    const auto mark = ops_.mark();
    Check next;
    bool nostore = false;
    TVL1_WALK_TRY(speculate(chk, next, nostore));
    double e = 0.0;
    TVL1_WALK_TRY(ops_.wait(chk.seq, &e));
    w_.read(e);
    ++ct_.checks;
    const bool ends = !w_.active(lv_.scaledEps, lv_.iterations);
    if (wp_ == 0 && h_.r1 < 0) st_.w0_hint = pred_.w0_hint = e / lv_.scaledEps;
    pred_.note(h_, e, w_.n);
    const bool right =
        chk.pk >= 0 && gate_holds(e, lv_.scaledEps, w_.n, lv_.iterations, lv_.kmax, 1, chk.pk, chk.pcalc);
    if (lv_.spec_trace) {
      char line[160];
      snprintf(line, sizeof line, "spec level %d warp %d n %d E/thr %.3f guess %d/%d %s\n", lv_.level, wp_,
               w_.n, e / lv_.scaledEps, chk.pk, chk.pcalc, chk.pk < 0 ? "-" : right ? "hit" : "miss");
      ops_.trace(line);
    }
    if (chk.pk >= 0 && !right) {   // the gated launches ran empty: forget them
      ++ct_.spec_misses;
      ops_.rollback(mark);
    }
    if (right && chk.pk == 0) {   // the next warp's first pass is done, its check pending
      flip();
      pre_ = true;
      pre_nostore_ = nostore;
      pre_chk_ = next;
      return TVL1_OK;
    }
    if (right) {   // the warp's next pass is done
      flip();
      w_.ran(w_.next(lv_.scaledEps, lv_.iterations, lv_.kmax, 1));
      if (chk.pcalc) {
        pending_ = true;
        pend_ = next;
      }
      return TVL1_OK;
    }
    // the fused pass guessed that this warp stops here; it continues: compute its constants
    // (from its input u, the set the pass just read) before the next pass
    if (fused_nostore_ && !ends) TVL1_WALK_TRY(ops_.gather(st_.ui ^ 1, st_.cb, wp_));
    fused_nostore_ = false;
    return TVL1_OK;
  }
};

// Every warp of one level: from the flow in set st.ui (p = 0) to the level's flow in st.ui.
template <class Ops>
tvl1_status walk_level(Ops &ops, const WalkLevel &lv, WalkState &st, WalkCounts &ct) {
  return LevelWalk<Ops>(ops, lv, st, ct).run();
}

#undef TVL1_WALK_TRY

}  // namespace tvl1k
