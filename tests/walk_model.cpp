// walk_model: walk_level (csrc/tvl1_walk.hpp) over a symbolic device, one result line per `run`
// line of a case file (tests/test_walk_cpu.py builds it with g++ and the host sanitizers; no
// GPU).  The device holds no pixels, only what each buffer set stands for:
//   u / p set     its position on the level's chain: the iterations of the completed warps plus
//                 those into the current one (u also: how often it was median-filtered)
//   constants     the flow they were gathered from
//   partials      (warp, n) of the pass that wrote them, until a check has read them
// A pass must read the chain's current state, its warp's constants and a p_zero flag that says
// "level start"; a check must read the partials of the pass it follows; gates behave as on the
// device (gate_holds over the scripted residual); a wait must name a check that ran, once and in
// order; every missed guess must be rolled back exactly once.  Anything else ends the program
// with a message and a non-zero status.
//   script THR NW LEN r...     NW warps' residuals in units of THR by iteration count 1..LEN
//                              (warp wp reads script wp % NW); LEN is the runs' `iterations`
//   run WARPS KMAX EPS_POS FUSE MEDIAN SPEC MID MID_MIN    SPEC: 0 off, 1 alone, 2 not alone
//     -> spec mid | each warp's iterations | warp:n of every residual read | the final chain
//        position | the walker's checks, misses, mid passes, ended on the mid state | the passes
//        that ran, per warp: k, c = ends in a check, m = mid-check | what the device saw: right
//        and wrong stop guesses, re-gathers after a wrong stop guess, right and wrong continue
//        guesses, waited chained checks of the same and of the next warp, mid passes, of those
//        continued, retaken, and in a run that speculates
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tvl1_walk.hpp"

using namespace tvl1k;

[[noreturn]] static void fail(const std::string &line, const char *what, long a = 0, long b = 0) {
  fprintf(stderr, "walk_model: %s (%ld, %ld) in: %s\n", what, a, b, line.c_str());
  exit(1);
}

struct Script {
  double thr = 1.0;
  int nw = 0, len = 0;
  std::vector<double> r;   // nw x len, in units of thr
  double at(int wp, int n) const { return r.at((size_t)(wp % nw) * len + (n - 1)) * thr; }
};

struct Device {
  const WalkLevel &lv;
  const Script &sc;
  const bool alone_;
  const std::string &line;

  struct Flow {
    long tag = -1;
    int med = 0;
  };
  struct Part {
    int wp = -1, n = -1;
    bool fresh = false;
  };
  struct Chk {
    bool ran = false, waited = false, gated_in = false, gate_out = false, held = false, mid_end = false;
    int pk = -1, wp = -1, n = -1;
    double e = 0.0;
  };
  struct Mark {
    unsigned long long seq;
  };
  static constexpr int kBlocks = 7;

  Flow u[2], C[2];
  long p[2] = {-1, -1};
  Part part[2];
  std::vector<Chk> chk{1};
  unsigned long long seq = 0, gate = 0, slot[2] = {0, 0}, last_waited = 0;
  long cur = 0;                // the chain's current position
  std::vector<long> start;     // ... where each warp began
  long mid_in = -1;            // the input of a mid pass, while its retake may follow
  int owed = 0;                // missed guesses not yet rolled back
  int last_read_wp = -1;
  bool wrong_stop = false;     // the last check read was a wrong stop guess
  bool guessed = false;        // a check of this run has evaluated a guess: a speculating run
  std::vector<int> iters;
  std::vector<std::pair<int, int>> reads;
  std::vector<std::string> passes;
  long ev[11] = {};
  enum { kStopRight, kStopWrong, kStopRegather, kContRight, kContWrong, kChainSame, kChainNext, kMid,
         kMidCont, kMidRetake, kMidSpec };

  Device(const WalkLevel &lv_, const Script &sc_, bool alone, int ui, const std::string &line_)
      : lv(lv_), sc(sc_), alone_(alone), line(line_) {
    u[ui].tag = 0;
  }
  void settle() const {
    if (owed) fail(line, "a missed guess was not rolled back");
  }
  int wp_now() const { return (int)start.size() - 1; }

  tvl1_status median(int ui) {
    settle();
    if (u[ui].tag != cur) fail(line, "median of a stale flow", u[ui].tag, cur);
    u[ui ^ 1] = Flow{u[ui].tag, u[ui].med + 1};
    return TVL1_OK;
  }
  tvl1_status gather(int ui, int cb, int wp) {
    settle();
    if (u[ui].tag < 0) fail(line, "gather from an unwritten flow", ui, wp);
    if (wp == wp_now() && cur > start.back()) ev[kStopRegather] += wrong_stop;
    C[cb] = u[ui];
    return TVL1_OK;
  }
  tvl1_status pass(const PassReq &q, int wp, int n, int *blocks) {
    settle();
    *blocks = kBlocks;
    const long retake_of = mid_in;
    if (q.gated && gate != q.gseq) return TVL1_OK;   // ran empty
    if (q.gated && (q.gseq == 0 || q.gseq > seq)) fail(line, "pass gated on no check", (long)q.gseq);
    mid_in = -1;
    const Flow in = u[q.ui];
    if (wp == wp_now() + 1 && n == 0) {
      start.push_back(cur);
      passes.emplace_back();
    } else if (wp != wp_now()) {
      fail(line, "pass of a warp that is not the current one", wp, wp_now());
    }
    const long at = start.back() + n;
    if (retake_of >= 0 && in.tag == retake_of && at == retake_of && q.k == 2 && !q.calc_end && !q.mid) {
      cur = retake_of;   // the state at the mid check, from the mid pass's untouched input
      ++ev[kMidRetake];
    }
    if (in.tag != cur || at != cur) fail(line, "pass reads a stale flow", in.tag, cur);
    if (in.med != (lv.median ? wp + 1 : 0)) fail(line, "pass reads a flow filtered for another warp", in.med, wp);
    if (q.p_zero != (cur == 0)) fail(line, "p_zero disagrees with level start", q.p_zero, cur);
    if (!q.p_zero && p[q.pi] != cur) fail(line, "pass reads a stale p", p[q.pi], cur);
    if (q.witer) {
      if (n != 0 || q.k != 2 || !q.calc_end || q.mid) fail(line, "fused pass that is no first pass", n, q.k);
      if (q.store_c) C[q.cb] = in;
    } else if (C[q.cb].tag != start.back() || C[q.cb].med != in.med) {
      fail(line, "constants not gathered from the warp's starting flow", C[q.cb].tag, start.back());
    }
    if (q.mid && (q.k != 4 || !q.calc_end || q.gated)) fail(line, "malformed mid pass", q.k);
    if (q.k < 1 || q.k > lv.kmax || n + q.k > lv.iterations) fail(line, "pass length", q.k, n);
    u[q.ui ^ 1] = Flow{cur + q.k, in.med};
    p[q.pi ^ 1] = cur + q.k;
    part[0].fresh = part[1].fresh = false;
    if (q.mid) {
      part[0] = Part{wp, n + 4, true};
      part[1] = Part{wp, n + 2, true};
      mid_in = cur;
      ++ev[kMid];
      ev[kMidSpec] += guessed;
    } else if (q.calc_end) {
      part[0] = Part{wp, n + q.k, true};
    }
    cur += q.k;
    passes.back() += (passes.back().empty() ? "" : ",") + std::to_string(q.k) + (q.calc_end ? "c" : "") +
                     (q.mid ? "m" : "");
    return TVL1_OK;
  }
  tvl1_status check(const CheckReq &q, unsigned long long *seq_out) {
    settle();
    *seq_out = ++seq;
    chk.resize(seq + 1);
    Chk &c = chk[seq] = Chk{};
    c.gated_in = q.gated_in;
    c.gate_out = q.gate_out;
    c.pk = q.pk;
    if (q.gated_in && (q.in_seq == 0 || q.in_seq >= seq)) fail(line, "check gated on no check", (long)q.in_seq);
    if (q.gated_in && gate != q.in_seq) return TVL1_OK;   // ran empty
    if (q.blocks != kBlocks || (q.first != 0 && q.first != kBlocks)) fail(line, "check of other partials", q.first);
    Part &pt = part[q.first ? 1 : 0];
    if (!pt.fresh) fail(line, "check reads partials its pass did not write", pt.wp, pt.n);
    pt.fresh = false;
    if (q.gate_out && (q.n != pt.n || q.pk < 0)) fail(line, "gate of another iteration count", q.n, pt.n);
    c.ran = true;
    c.wp = pt.wp;
    c.n = pt.n;
    c.e = sc.at(pt.wp, pt.n);
    c.mid_end = mid_in >= 0 && q.first == 0;
    slot[seq & 1] = seq;
    if (q.gate_out) {
      c.held = gate_holds(c.e, lv.scaledEps, q.n, lv.iterations, lv.kmax, 1, q.pk, q.pcalc);
      gate = c.held ? seq : 0;
      guessed = true;
    }
    return TVL1_OK;
  }
  tvl1_status wait(unsigned long long s, double *e) {
    settle();
    if (s == 0 || s > seq) fail(line, "wait for a check never enqueued", (long)s, (long)seq);
    Chk &c = chk[s];
    if (!c.ran) fail(line, "wait for a check that was gated off", (long)s);
    if (c.waited || s <= last_waited) fail(line, "check consumed twice or out of order", (long)s, (long)last_waited);
    if (slot[s & 1] != s) fail(line, "residual overwritten before it was read", (long)s, (long)slot[s & 1]);
    c.waited = true;
    last_waited = s;
    reads.emplace_back(c.wp, c.n);
    *e = c.e;
    wrong_stop = false;
    if (c.gate_out) {
      ++ev[c.pk == 0 ? (c.held ? kStopRight : kStopWrong) : (c.held ? kContRight : kContWrong)];
      wrong_stop = c.pk == 0 && !c.held;
      if (!c.held) owed = 1;
    }
    if (c.gated_in) ++ev[c.wp == last_read_wp ? kChainSame : kChainNext];
    if (c.mid_end) ++ev[kMidCont];
    last_read_wp = c.wp;
    return TVL1_OK;
  }
  Mark mark() const { return Mark{seq}; }
  void rollback(const Mark &m) {
    if (owed != 1) fail(line, "rollback without a missed guess");
    owed = 0;
    for (unsigned long long s = m.seq + 1; s <= seq; ++s)
      if (chk[s].ran) fail(line, "rollback of a check that ran", (long)s);
    seq = m.seq;
    last_waited = std::min(last_waited, seq);
    chk.resize(seq + 1);
  }
  bool alone() const { return alone_; }
  void trace(const char *) {}
  void warp_done(int wp, int n) {
    settle();
    if (wp != (int)iters.size() || wp > wp_now()) fail(line, "warp_done out of turn", wp, wp_now());
    const long end = wp + 1 < (int)start.size() ? start[wp + 1] : cur;
    if (start[wp] + n != end) fail(line, "warp_done with another iteration count", n, end - start[wp]);
    iters.push_back(n);
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
      ss >> tok >> sc.nw >> sc.len;
      sc.thr = strtod(tok.c_str(), nullptr);
      sc.r.clear();
      while (ss >> tok) sc.r.push_back(strtod(tok.c_str(), nullptr));
      if (sc.nw < 1 || sc.r.size() != (size_t)sc.nw * sc.len) fail(line, "script size", (long)sc.r.size());
      continue;
    }
    if (cmd != "run") fail(line, "unknown command");
    int fuse, median, spec, mid;
    WalkLevel lv{};
    ss >> lv.warps >> lv.kmax >> lv.eps_pos >> fuse >> median >> spec >> mid >> tok;
    lv.level = 0;
    lv.iterations = sc.len;
    lv.scaledEps = sc.thr;
    lv.mid_min = strtod(tok.c_str(), nullptr);
    // the engine's own preconditions (solve()): nothing fused, speculated or mid-checked with
    // epsilon = 0; a fused or speculative first pass is 2 iterations; a mid-check pass is 4
    lv.fuse = fuse && lv.eps_pos && lv.kmax >= 2 && lv.iterations >= 2;
    lv.median = median != 0;
    lv.spec = spec && lv.eps_pos && lv.kmax >= 2;
    lv.mid = mid && lv.eps_pos && lv.kmax >= 4;
    lv.spec_trace = true;
    WalkState st{1, 0, 1, 50.0};
    WalkCounts ct;
    Device dev(lv, sc, spec == 1, st.ui, line);
    if (walk_level(dev, lv, st, ct) != TVL1_OK) fail(line, "walk_level failed");
    dev.settle();
    long total = 0;
    for (int n : dev.iters) total += n;
    if ((int)dev.iters.size() != lv.warps || total != dev.cur || dev.u[st.ui].tag != dev.cur ||
        ct.level_iters != total)
      fail(line, "the level's flow is not the chain's end", dev.u[st.ui].tag, dev.cur);
    if (st.cb != (1 ^ (lv.warps & 1))) fail(line, "constants set after the level", st.cb);
    printf("%d %d |", lv.spec && spec == 1, (int)lv.mid);
    for (int n : dev.iters) printf(" %d", n);
    printf(" |");
    for (const auto &r : dev.reads) printf(" %d:%d", r.first, r.second);
    printf(" | %ld | %lld %d %d %d |", dev.cur, (long long)ct.checks, (int)ct.spec_misses, ct.mid_passes,
           ct.mid_taken);
    for (const std::string &p : dev.passes) printf(" %s", p.c_str());
    printf(" |");
    for (long e : dev.ev) printf(" %ld", e);
    printf("\n");
  }
  return 0;
}
