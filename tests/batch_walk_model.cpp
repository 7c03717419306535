// batch_walk_model: walk_batch_level (csrc/tvl1_batch_walk.hpp) over a symbolic device, one result
// line per `run` line of a case file (tests/test_batch_walk_cpu.py builds it with g++ and the host
// sanitizers; no GPU).  The device holds no pixels, only what each pair's buffers stand for:
//   u / p set     its position on the level's chain: the iterations of the pair's completed warps
//                 plus those into the current one (u also: how often it was median-filtered)
//   constants     the flow they were gathered from
//   partials      the launch that wrote them, at which iteration count, how many, packed or not
//   residual slot the reduce that filled it, whether a sync followed, whether it was read
// Every launch must name each pair once, read that pair's current sets, carry a pzero bit that
// says "level start", find the warp's constants, and stay within kmax and `iterations`; a reduce
// must follow exactly the passes that end in a check and sum what they wrote; a residual is read
// once, after the sync that followed its reduce.  Anything else ends the program with a message
// and a non-zero status.
//   script THR NS NW LEN r...   NS pair scripts of NW warps' residuals in units of THR by iteration
//                               count 1..LEN (pair b reads script b % NS, warp wp of level l reads
//                               warp (l * WARPS + wp) % NW); LEN is the runs' `iterations`
//   run N WARPS EPS_POS FUSE MEDIAN GROUP STORE   two levels of N pairs, one state carried across
//     -> what the device saw: store guesses that held, re-gathers, rounds of two or more pass
//        lengths, rounds without a check, passes during which a pair of the chunk sat idle,
//        non-fused gathers, medians
//        ; then per pair: each (level, warp)'s iterations | level.warp:n of every residual read
//        (as run-length coded steps) | the passes of each (level, warp), run-length coded: k, c =
//        ends in a check | the walker's checks, regathers and iterations of the last level
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tvl1_batch_walk.hpp"

using namespace tvl1k;

[[noreturn]] static void fail(const std::string &line, const char *what, long a = 0, long b = 0) {
  fprintf(stderr, "batch_walk_model: %s (%ld, %ld) in: %s\n", what, a, b, line.c_str());
  exit(1);
}

struct Script {
  double thr = 1.0;
  int ns = 0, nw = 0, len = 0;
  std::vector<double> r;   // ns x nw x len, in units of thr
  double at(int b, int w, int n) const { return r.at(((size_t)(b % ns) * nw + w % nw) * len + (n - 1)) * thr; }
};

// run-length coded list: tok or tokxN, comma separated
struct Rle {
  std::string out, last;
  int rep = 0;
  void flush() {
    if (!rep) return;
    out += (out.empty() ? "" : ",") + last + (rep > 1 ? "x" + std::to_string(rep) : "");
    rep = 0;
  }
  void add(const std::string &tok) {
    if (rep && tok == last) {
      ++rep;
      return;
    }
    flush();
    last = tok;
    rep = 1;
  }
  std::string str() {
    flush();
    return out.empty() ? "-" : out;
  }
};

struct Device {
  const BatchWalkLevel &lv;
  const Script &sc;
  const std::string &line;
  const int n;
  int level = 0;

  struct Flow {
    long tag = -1;
    int med = 0;
  };
  struct Part {
    long launch = -1;
    int n = -1, blocks = 0;
    bool fused = false, fresh = false;
  };
  struct Slot {
    bool filled = false, synced = false, read = false;
    int n = -1;
    double e = 0.0;
  };
  struct Pair {
    Flow u[2], C;
    long p[2] = {-1, -1};
    Part part;
    Slot slot;
    long cur = 0, start = 0;   // the chain's position, and where the current warp began
    int wp = 0;                // the current warp
    long last_pass = -1;       // the last launch that iterated the pair
    long round = -1;           // the round of that launch
    double err = DBL_MAX;      // procOneScale's error: DBL_MAX, or the residual read last
    bool nostore = false;      // the warp's fused pass did not store the constants
    bool regathered = false;
    int last_read_n = 0;
    std::vector<int> iters;
    std::vector<Rle> passes;
    Rle read_steps;
    std::vector<std::string> read_log;
  };
  std::vector<Pair> pr;
  long launches = 0, round = 0;
  int last_k = 0;                      // of the open round (0: none open)
  int round_launches = 0;
  bool round_check = false;
  std::vector<int> owed;               // the pairs the next call must reduce
  int owed_blocks = 0;
  bool owed_fused = false;
  long ev[7] = {};
  enum { kHeld, kRegather, kMultiK, kNoCheck, kIdle, kGather, kMedian };
  static constexpr int kFusedBlocks = 5, kPassBlocks = 7;

  Device(const BatchWalkLevel &lv_, const Script &sc_, const BatchWalkState &st, const std::string &line_)
      : lv(lv_), sc(sc_), line(line_), n(lv_.n), pr(lv_.n) {
    for (int b = 0; b < n; ++b) pr[b].u[st.ubit.test(b)].tag = 0;
  }
  // the next level: every pair's flow, upsampled into its other set (the caller flips ubit); p = 0
  void next_level(const BatchWalkState &st) {
    close_round();
    ++level;
    for (int b = 0; b < n; ++b) {
      Pair &q = pr[b];
      if (q.wp != lv.warps) fail(line, "level left before its last warp", b, q.wp);
      const int us = st.ubit.test(b);
      if (q.u[us].tag != q.cur) fail(line, "the level's flow is not the chain's end", q.u[us].tag, q.cur);
      q.u[us ^ 1] = Flow{0, 0};
      q.u[us] = Flow{};
      q.p[0] = q.p[1] = -1;
      q.C = Flow{};
      q.cur = q.start = 0;
      q.wp = 0;
    }
  }
  bool active(const Pair &q) const { return q.err > lv.scaledEps && q.cur - q.start < lv.iterations; }
  int med_of(const Pair &q) const { return lv.median ? q.wp + 1 : 0; }

  void settle(const char *what) const {
    if (!owed.empty()) fail(line, what, owed[0], (long)owed.size());
  }
  void close_round() {
    if (last_k) {
      ev[kMultiK] += round_launches >= 2;
      ev[kNoCheck] += !round_check;
    }
    last_k = round_launches = 0;
    round_check = false;
  }
  // the pairs of a launch: 1..n entries, each a pair of the chunk, none twice
  std::vector<int> pairs_of(const BatchSel &sel, bool every) {
    if (sel.n < 1 || sel.n > n) fail(line, "sel.n outside 1..n", sel.n, n);
    std::vector<char> seen(n, 0);
    std::vector<int> out;
    for (int j = 0; j < sel.n; ++j) {
      const int b = sel.idx[j];
      if (b >= n) fail(line, "a pair outside the chunk", b, n);
      if (seen[b]) fail(line, "a pair listed twice in one sel", b);
      seen[b] = 1;
      out.push_back(b);
    }
    if (every && sel.n != n) fail(line, "a launch of every pair that leaves one out", sel.n, n);
    return out;
  }
  static int count(const BatchMask &m) {
    int c = 0;
    for (uint64_t w : m.w) c += __builtin_popcountll(w);
    return c;
  }
  const Flow &current_u(const BatchSel &sel, int b, const char *what) {
    const Pair &q = pr[b];
    const Flow &in = q.u[sel.ubit.test(b)];
    if (in.tag != q.cur) fail(line, what, in.tag, q.cur);
    return in;
  }

  tvl1_status median(const BatchSel &sel) {
    settle("median before the reduce that was due");
    close_round();
    if (!lv.median) fail(line, "median on a level without one");
    if (count(sel.storec) || count(sel.cerr)) fail(line, "storec / cerr bit on a median");
    for (int b : pairs_of(sel, true)) {
      Pair &q = pr[b];
      if (q.cur != q.start) fail(line, "median inside a warp", b, q.cur - q.start);
      const Flow in = current_u(sel, b, "median of a stale flow");
      if (in.med != q.wp) fail(line, "median of a flow filtered for another warp", in.med, q.wp);
      q.u[sel.ubit.test(b) ^ 1] = Flow{in.tag, in.med + 1};
    }
    ++ev[kMedian];
    return TVL1_OK;
  }
  tvl1_status gather(const BatchSel &sel) {
    settle("gather before the reduce that was due");
    close_round();
    if (count(sel.storec) || count(sel.cerr)) fail(line, "storec / cerr bit on a gather");
    bool first = false, again = false;
    for (int b : pairs_of(sel, false)) {
      Pair &q = pr[b];
      const Flow &in = q.u[sel.ubit.test(b)];
      if (q.cur == q.start) {   // the warp's gather: the current flow
        if (lv.fuse) fail(line, "gather before a fused pass", b);
        current_u(sel, b, "gather from a stale flow");
        first = true;
      } else {   // a re-gather: the flow the fused pass read, for a pair that goes on without constants
        if (!q.nostore || q.regathered || q.cur != q.start + 2) fail(line, "re-gather of stored constants", b);
        if (q.slot.filled && !q.slot.read) fail(line, "re-gather before the first check was read", b);
        if (!active(q)) fail(line, "re-gather for a pair that stopped", b);
        if (in.tag != q.start) fail(line, "re-gather from another flow than the fused pass read", in.tag, q.start);
        q.regathered = true;
        again = true;
        ++ev[kRegather];
      }
      if (in.med != med_of(q)) fail(line, "gather from a flow filtered for another warp", in.med, q.wp);
      q.C = in;
    }
    if (first && (again || sel.n != n)) fail(line, "a warp's gather that leaves pairs out", sel.n, n);
    ev[kGather] += first;
    return TVL1_OK;
  }
  // one pair's pass of k iterations from its current sets into the others
  void iterate(const BatchSel &sel, int b, int k, bool check, bool fused, int blocks) {
    Pair &q = pr[b];
    if (q.slot.filled && !q.slot.read) fail(line, "pass before the pair's residual was read", b);
    if (q.part.fresh) fail(line, "pass over partials nobody summed", b);
    if (!active(q)) fail(line, "pass of a pair whose warp has ended", b, q.cur - q.start);
    const Flow in = current_u(sel, b, "pass reads a stale flow");
    if (in.med != med_of(q)) fail(line, "pass reads a flow filtered for another warp", in.med, q.wp);
    if (sel.pzero.test(b) != (q.cur == 0)) fail(line, "pzero disagrees with level start", b, q.cur);
    const int ps = sel.pbit.test(b);
    if (q.cur != 0 && q.p[ps] != q.cur) fail(line, "pass reads a stale p", q.p[ps], q.cur);
    const int nw = (int)(q.cur - q.start);
    if (k < 1 || k > lv.kmax || nw + k > lv.iterations) fail(line, "pass length", k, nw);
    if (fused) {
      if (nw != 0 || k != 2 || !check) fail(line, "fused pass that is no first pass", b, nw);
      q.nostore = !sel.storec.test(b);
      q.regathered = false;
      if (!q.nostore) q.C = in;
    } else if (q.C.tag != q.start || q.C.med != in.med) {
      fail(line, "pass before the warp's constants exist", q.C.tag, q.start);
    }
    q.u[sel.ubit.test(b) ^ 1] = Flow{q.cur + k, in.med};
    q.p[ps ^ 1] = q.cur + k;
    q.cur += k;
    q.err = DBL_MAX;
    q.last_pass = launches;
    q.round = round;
    if (check) q.part = Part{launches, nw + k, blocks, fused, true};
    q.passes.back().add(std::to_string(k) + (check ? "c" : ""));
  }
  tvl1_status fused(const BatchSel &sel, int nstore, int *blocks) {
    settle("fused pass before the reduce that was due");
    close_round();
    if (!lv.fuse) fail(line, "fused pass on a level without fusion");
    if (count(sel.cerr)) fail(line, "cerr bit on a fused pass");
    if (nstore != count(sel.storec)) fail(line, "nstore is not the number of storec bits", nstore);
    ++launches;
    ++round;
    *blocks = kFusedBlocks;
    owed = pairs_of(sel, true);
    for (int b : owed) iterate(sel, b, 2, true, true, kFusedBlocks);
    owed_blocks = kFusedBlocks;
    owed_fused = true;
    return TVL1_OK;
  }
  tvl1_status pass(int K, const BatchSel &sel, int *blocks) {
    settle("pass before the reduce that was due");
    if (count(sel.storec)) fail(line, "storec bit on a launch that is not the fused pass");
    const std::vector<int> ps = pairs_of(sel, false);
    // A round is one launch per pass length, ascending, and runs each pair once: a launch that
    // breaks either opens the next round.  (A pair put into two groups of one round therefore
    // shows as a stale read: its bits still name the sets its first pass read.)
    bool again = K <= last_k;
    for (int b : ps) again = again || pr[b].round == round;
    if (again) close_round();
    if (!last_k) ++round;
    last_k = K;
    ++round_launches;
    ++launches;
    *blocks = kPassBlocks;
    int idle = 0;
    for (int b = 0; b < n; ++b) idle += !active(pr[b]) && pr[b].round != round;
    ev[kIdle] += idle > 0;
    for (int b : ps) {
      iterate(sel, b, K, sel.cerr.test(b) != 0, false, kPassBlocks);
      if (sel.cerr.test(b)) owed.push_back(b);
    }
    if (count(sel.cerr) != (int)owed.size()) fail(line, "cerr bit of a pair outside the launch", count(sel.cerr));
    owed_blocks = kPassBlocks;
    owed_fused = false;
    round_check = round_check || !owed.empty();
    return TVL1_OK;
  }
  tvl1_status reduce(const BatchSel &sel, int blocks, bool fused) {
    if (owed.empty()) fail(line, "reduce after a pass without a check");
    std::vector<int> ps = pairs_of(sel, false);
    if (count(sel.storec)) fail(line, "storec bit on a reduce");
    if (ps.size() != owed.size()) fail(line, "cerr differs from the reduce's selection", (long)ps.size(), (long)owed.size());
    for (int b : ps) {
      Pair &q = pr[b];
      if (!q.part.fresh || q.part.launch != launches || q.part.launch != q.last_pass)
        fail(line, "reduce over partials the pair's last pass did not write", b, q.part.launch);
      if (blocks != q.part.blocks || blocks != owed_blocks || fused != q.part.fused || fused != owed_fused)
        fail(line, "reduce of other partials than the pass left", blocks, fused);
      if (q.slot.filled && !q.slot.read) fail(line, "residual overwritten before it was read", b);
      q.part.fresh = false;
      q.slot = Slot{true, false, false, q.part.n, sc.at(b, level * lv.warps + q.wp, q.part.n)};
    }
    owed.clear();
    return TVL1_OK;
  }
  // the residual slots as the host sees them: a read is checked and recorded
  struct Residuals {
    Device *dev = nullptr;
    double operator[](int b) const { return dev->read(b); }
  };
  tvl1_status sync(Residuals *res) {
    settle("sync before the reduce that was due");
    close_round();
    for (Pair &q : pr)
      if (q.slot.filled) q.slot.synced = true;
    res->dev = this;
    return TVL1_OK;
  }
  double read(int b) {
    Pair &q = pr.at(b);
    if (!q.slot.filled) fail(line, "read of a residual no reduce filled", b);
    if (!q.slot.synced) fail(line, "read of a residual before the sync after its reduce", b);
    if (q.slot.read) fail(line, "residual read twice", b, q.slot.n);
    q.slot.read = true;
    q.err = q.slot.e;
    q.read_steps.add(std::to_string(q.slot.n - q.last_read_n));   // the step from the warp's last read
    q.last_read_n = q.slot.n;
    return q.slot.e;
  }
  void warp_done(int b, int wp, int iters) {
    settle("warp_done before the reduce that was due");
    close_round();
    Pair &q = pr.at(b);
    if (wp != q.wp || wp >= lv.warps) fail(line, "warp_done out of turn", wp, q.wp);
    if (iters != q.cur - q.start) fail(line, "warp_done with another iteration count", iters, q.cur - q.start);
    if (q.slot.filled && !q.slot.read) fail(line, "warp left with a residual unread", b);
    if (active(q)) fail(line, "warp left while the pair is active", b, iters);
    ev[kHeld] += q.nostore && !q.regathered;
    q.iters.push_back(iters);
    q.read_log.push_back(q.read_steps.str());
    q.read_steps = Rle{};
    q.last_read_n = 0;
    q.passes.emplace_back();
    ++q.wp;
    q.start = q.cur;
    q.err = DBL_MAX;
    q.nostore = q.regathered = false;
  }
};

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  Script sc;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string cmd, tok;
    if (!(ss >> cmd)) continue;
    if (cmd == "script") {
      ss >> tok >> sc.ns >> sc.nw >> sc.len;
      sc.thr = strtod(tok.c_str(), nullptr);
      sc.r.clear();
      while (ss >> tok) sc.r.push_back(strtod(tok.c_str(), nullptr));
      if (sc.ns < 1 || sc.nw < 1 || sc.r.size() != (size_t)sc.ns * sc.nw * sc.len)
        fail(line, "script size", (long)sc.r.size());
      continue;
    }
    if (cmd != "run") fail(line, "unknown command");
    int fuse, median, group, store;
    BatchWalkLevel lv{};
    ss >> lv.n >> lv.warps >> lv.eps_pos >> fuse >> median >> group >> store;
    if (lv.n < 1 || lv.n > kBatchMax) fail(line, "chunk size", lv.n);
    lv.iterations = sc.len;
    lv.kmax = kTbMax;
    lv.scaledEps = sc.thr;
    // the engine's own precondition (solve_batch_chunk): the fused first pass is 2 iterations
    // ending in a check
    lv.fuse = fuse && lv.eps_pos && lv.iterations >= 2;
    lv.median = median != 0;
    lv.group = group != 0;
    lv.store_pred = store != 0;
    BatchWalkState st(lv.n);
    for (int b = 0; b < lv.n; ++b) {   // some pairs arrive in set 1
      if (b % 3 == 1) st.ubit.set(b);
      if (b % 5 >= 3) st.pbit.set(b);
    }
    BatchWalkCounts ct(lv.n);
    Device dev(lv, sc, st, line);
    for (Device::Pair &q : dev.pr) q.passes.emplace_back();
    for (int level = 0; level < 2; ++level) {
      if (level) {
        dev.next_level(st);
        st.flip_u();   // the upsample
      }
      if (walk_batch_level(dev, lv, st, ct) != TVL1_OK) fail(line, "walk_batch_level failed");
      dev.settle("level left before the reduce that was due");
    }
    dev.close_round();
    for (long e : dev.ev) printf("%ld ", e);
    for (int b = 0; b < lv.n; ++b) {
      Device::Pair &q = dev.pr[b];
      long last = 0;
      if ((int)q.iters.size() != 2 * lv.warps || q.u[st.ubit.test(b)].tag != q.cur)
        fail(line, "the level's flow is not the chain's end", b, q.cur);
      for (int w = lv.warps; w < 2 * lv.warps; ++w) last += q.iters[w];
      if (last != q.cur || ct.level_iters[b] != last) fail(line, "level_iters", b, (long)ct.level_iters[b]);
      printf(";");
      for (int i : q.iters) printf(" %d", i);
      printf(" |");
      for (const std::string &r : q.read_log) printf(" %s", r.c_str());
      printf(" |");
      for (size_t w = 0; w + 1 < q.passes.size(); ++w) printf(" %s", q.passes[w].str().c_str());
      printf(" | %lld %lld", (long long)ct.checks[b], (long long)ct.regathers[b]);
    }
    printf("\n");
  }
  return 0;
}
