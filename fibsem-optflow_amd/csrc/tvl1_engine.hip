// tvl1_engine.hip — host side of the MI355X TV-L1 engine + the C-ABI of include/tvl1.h.
//
// Replaces the reference's solver boundary /root/reference/src/optflow.cpp:516-520
// (TVL1_solve -> cv::cuda::OpticalFlowDual_TVL1::create(...)->calc(...)).  The
// host loop below restates OpenCV 3.4.1 calcImpl/procOneScale
// and launches the gfx950 kernels of tvl1_kernels.hpp.  There is no CPU path:
// every stage runs on the device; the only device->host traffic inside a solve is
// the residual of "check" iterations, read exactly where OpenCV reads it.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <atomic>
#include <chrono>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tvl1.h"
#include "tvl1_plan.hpp"
#include "tvl1_walk.hpp"
#include "tvl1_arena.hpp"
#include "tvl1_kernels.hpp"
#include "tvl1_batch.hpp"
#include "tvl1_align_plan.hpp"
#include "tvl1_planes.hpp"
#include "tvl1_align.hpp"
#include "tvl1_stack.hpp"
#include "tvl1_shift.hpp"
#include "tvl1_fbcheck.hpp"
#include "tvl1_compose.hpp"
#include "tvl1_invert.hpp"
#include "tvl1_score.hpp"

// the iteration passes are compiled in tvl1_passes.hip (another instruction scheduler)
namespace tvl1k {
#define TVL1_PASS_INSTANCE(...) extern template __global__ void __VA_ARGS__;
#include "tvl1_passes.inc"
#undef TVL1_PASS_INSTANCE
}  // namespace tvl1k

using namespace tvl1k;

namespace {

thread_local std::string g_create_error;

#ifndef TVL1_WI_M
#define TVL1_WI_M 6
#endif
// k_warp_iter's window margin (px): flows within about +-(M - 1) px gather from its LDS
// window ring, larger ones from HBM (the same taps)
constexpr int kWiMargin = TVL1_WI_M;
// Batched passes on levels at most this wide use 64-px bands, kb_iterate_roll<K, 1> (95
// VGPRs, 5 wavefronts per SIMD, against 3 for the LDS-staged <4, 2>): the production strips'
// levels of 515-1573 x 17-51 px give a batch too few 128-px bands to fill the SIMDs, so twice
// the wavefronts with half the work each finish sooner.  Measured on the strip workload (with
// the register-ring <4, 2>): cut-off 1700 +2.4 %, 1100 +1.2 %, 2500 +1.8 %, every level -3 %;
// with the LDS-staged one 1700 and 1100 +1.3 %, 2500 +0.2 %.
constexpr int kBatchPx1W = 1700;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Geometry {
  int W = 0, H = 0, L = 0;
  int ws[TVL1_MAX_LEVELS], hs[TVL1_MAX_LEVELS], ps[TVL1_MAX_LEVELS];
  bool gamma = false;
};

// tvl1_arena.hpp's backend: the HIP calls the memory lifecycle makes
struct HipDev {
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  int malloc(char **p, size_t n) { return hipMalloc((void **)p, n); }
  int free(char *p) { return hipFree(p); }
  int memset_async(char *p, int v, size_t n, Stream s) { return hipMemsetAsync(p, v, n, s); }
  int event_create(Event *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
  int event_record(Event e, Stream s) { return hipEventRecord(e, s); }
  int event_query(Event e) { return hipEventQuery(e); }
  int event_sync(Event e) { return hipEventSynchronize(e); }
  int event_destroy(Event e) { return e ? hipEventDestroy(e) : hipSuccess; }
  int stream_wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0); }
  void clear_error() { (void)hipGetLastError(); }
  const char *error_string(int e) { return hipGetErrorString((hipError_t)e); }
};

// Per-kernel-class HIP-event timing (tvl1_set_profiling): a pool of events, two per mark.
struct MarkPool {
  struct Mark {
    int cls;
    size_t a, b;
    double bytes;      // SURVEY 8(d) algorithmic bytes
    double hbm_bytes;  // compulsory bytes of this implementation
  };
  const size_t grow;        // events created when the pool runs short
  const size_t max_marks;   // marks held; later ones are dropped (0: no bound)
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  std::vector<Mark> marks;

  // the token of end(), 0 = not recording
  size_t begin(bool profiling, hipStream_t st) {
    if (!profiling || (max_marks && marks.size() >= max_marks)) return 0;
    for (size_t i = 0; used + 2 > ev.size() && i < grow; ++i) {
      hipEvent_t e;
      // timing-only events: no system-scope fence (cache writeback + invalidate) at each
      // record, which slowed the kernel after it and inflated the per-launch times ~6 %
      // against the rocprofv3 kernel trace (r3)
      if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) break;
      ev.push_back(e);
    }
    if (used + 2 > ev.size()) return 0;
    (void)hipEventRecord(ev[used], st);
    return ++used;
  }
  void end(hipStream_t st, size_t tok, int cls, double bytes, double hbm_bytes = -1.0) {
    if (tok == 0) return;
    const size_t b = used++;
    (void)hipEventRecord(ev[b], st);
    marks.push_back({cls, tok - 1, b, bytes, hbm_bytes < 0 ? bytes : hbm_bytes});
  }
  void reset() {
    marks.clear();
    used = 0;
  }
  void destroy() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

}  // namespace

struct tvl1_ctx {
  int device = 0;
  tvl1_params prm{};
  std::string err;
  // device memory (tvl1_arena.hpp): the lifecycle state and the own stream, then the blocks
  Arena<HipDev> mem;
  Block arena;                          // a single-pair solve's planes (ensure_geometry)
  Geometry geo;
  bool geo_valid = false;

  float *I0s[TVL1_MAX_LEVELS] = {};
  float *I1s[TVL1_MAX_LEVELS] = {};
  float4 *G = nullptr;
  float *U[2][3] = {};   // u1, u2, u3
  float *Pd[2][6] = {};  // p11, p12, p21, p22, p31, p32
  float *C[2][3] = {};   // two sets of warp constants I1wx, I1wy, rho_c (speculation)
  uint8_t *in0 = nullptr, *in1 = nullptr;   // staging for tvl1_calc_host
  float *outu = nullptr, *outv = nullptr;
  double *partials = nullptr;
  int partials_cap = 0;
  double *pinned = nullptr;      // host-pinned residual landing slot (coherent, mapped)
  double *pinned_dev = nullptr;  // its device address: k_reduce stores the residual there
  hipEvent_t ev_check[2] = {};   // recorded after each residual check (by sequence parity)
  unsigned long long *gate = nullptr;   // device word: the speculation gate
  int spec = 1;                   // TVL1_SPEC: 0 no launches enqueued behind a check, 1 when the
                                  // solve is alone on its device (this process), 2 always
  int spec_trace = 0;             // TVL1_SPEC_TRACE=1: one stderr line per check and guess
  unsigned long long check_seq = 0;  // sequence number of the last residual check
  int poll = 1;                      // TVL1_POLL: wait for a residual by polling its
                                     // sequence number in host memory (0: event sync)
  // dispatch: the defaults are the measured best; the environment knobs are
  // for tests (named in tests/test_gpu_parity.py) and diagnostics
  int roll_seg = 0;          // TVL1_ROLL_SEG: k_iterate_roll rows per segment (0 = auto)
  long roll_px4_min = 5000000;   // TVL1_ROLL_PX4_MIN: 2-iteration passes take 4 px per lane on
                                 // levels of at least this many px (2 px below: more waves)
  int roll_slots[kRollMax + 1][2][5] = {};   // resident k_iterate_roll<G, K, PX> wavefronts
  int fill = 100;            // TVL1_FILL: % of the resident slots a single-pair streaming launch
                             // is sized for while the solve is alone on its device, and
  int fill_shared = 60;      // TVL1_FILL_SHARED: ... while other solves of this process share
                             // the device (their blocks take the rest; DESIGN 9: 3 in flight
                             // +1.8 % at 60 %, and a pair alone keeps its 100 % latency)
                             // is sized for (segment rows)
  long roll_long_min = 0;    // >= 3-iteration passes stream (k_iterate_roll) on levels of at
                             // least this many 56 x 32 tiles, else k_iterate_tb
  int warp_ring_slots = 0;   // resident k_warp_ring<6, 2> blocks per device
  size_t buf_limit = ((size_t)1 << 31) - 4096;   // TVL1_BUF_LIMIT: plane bytes the
                             // buffer-addressed kernels take (tests force the fallbacks)
  int fuse = 1;              // TVL1_FUSE=0: no k_warp_iter (warp + first pass as two kernels)
  int tb4 = 1;               // TVL1_TB4=0: blocked passes (gamma = 0) in 64 x 32 regions
                             // (k_iterate_tb) instead of 64 x 48 (k_iterate_tb4)
  long fuse_min = 4000000;   // TVL1_FUSE_MIN: k_warp_iter on levels of >= this many px; smaller
                             // levels: k_warp_ring + the pass (as fast, and their warps mostly
                             // run past the first check).  4 M since the two-consumer form
                             // (C2's 4.2 Mpx level 4: one pair alone -3.7 %, in flight +0.3 %)
  int witer_slots = 0;       // resident k_warp_iter<6, -, 128, 1, wi_nc> blocks per device
  int mid = 1;               // TVL1_MID=0: no mid-check passes (k_iterate_roll_mid, DESIGN.md
                             // §4.1 of r6): two 2-iteration passes of a converging warp as one
                             // (C2 in flight +2.5 %, profiles/r6/final_mid/)
  double mid_min = 1.1;      // TVL1_MID_MIN: ... when the check before them read at least this
                             // many eps^2 W H (the first of the two checks then rarely stops)
  int mid_slots = 0;         // resident k_iterate_roll_mid wavefronts
  int wi_nc = 2;             // TVL1_WI_NC: k_warp_iter consumer wavefronts (2: one per
                             // iteration of the pass; 1: both on one wave)
  int stages = 1;            // TVL1_STAGES: k_iterate_stages (a wavefront per iteration).  1: the
                             // 4-iteration passes k_iterate_tb4 would take; 2: every gamma = 0
                             // pass of 2 or 4 iterations on every level (tests); 0: never
  int stage_slots[kRollMax + 1] = {};   // resident k_iterate_stages<-, K> blocks per device
  int stages_fill = 0;       // TVL1_STAGES_FILL: % of its resident blocks a k_iterate_stages launch
                             // is sized for.  0: TVL1_FILL alone on the device, kStagesFillShared
                             // while other solves share it (longer segments than the other
                             // streaming launches take: a block's run-in is 3 K - 1 steps)
  // batch arena (tvl1_calc_batch): per logical plane, kBatchMax pairs' copies
  Block barena;
  int bW = 0, bH = 0, bL = 0, bn = 0;   // geometry it is laid out for
  int bws[TVL1_MAX_LEVELS] = {}, bhs[TVL1_MAX_LEVELS] = {};   // ... and its level sizes
  float *bI0s[TVL1_MAX_LEVELS] = {}, *bI1s[TVL1_MAX_LEVELS] = {};
  size_t bips[TVL1_MAX_LEVELS] = {};    // pair stride of level s image planes (floats)
  float *bU[2][2] = {}, *bP[2][4] = {}, *bC[3] = {};
  size_t bps = 0;                       // pair stride of the level-0-sized planes (floats)
  double *bpartials = nullptr;
  int batch_fuse = 1;                   // TVL1_BATCH_FUSE=0: no fused warp + first pass
  int batch_group = 1;                  // TVL1_BATCH_GROUP=0: r3's lock-step passes (the
                                        // shortest pass any pair allows, for all)
  int batch_store_pred = 1;             // TVL1_BATCH_STORE=1: kb_warp_iter always stores the
                                        // warp constants (r3); default: only predicted pairs
  int batch_px1_w = kBatchPx1W;         // TVL1_BATCH_PX1_W: batched passes on levels at most
                                        // this wide run 64-px bands (1 px per lane)
  int kb1_slots[kRollMax + 1] = {};     // resident kb_iterate_roll<K, 1> wavefronts
  int batch_seg_min = 128;              // TVL1_BATCH_SEG_MIN: batched passes never split a
                                        // level into segments shorter than min(rows, this)
                                        // (0: roll_segment alone)
  int probe_lds = 0;                    // TVL1_PROBE_ROLL_LDS: dynamic LDS per k_iterate_roll
                                        // block (occupancy probe only; with the LDS-staged
                                        // passes' 40 KiB, at most 120 KiB)
  int probe_wi_lds = 0;                 // TVL1_PROBE_WI_LDS: the same for k_warp_iter (< 64 KiB)
  Block gather_scratch;                 // tvl1_gather_flow's offsets and values
  int batch_small = 1;                  // TVL1_BATCH_SMALL=0: the coarsest level of a batch
                                        // streams like the others (no kb_small_level)
  Block small_scratch;                  // kb_small_level's per-warp iteration counts
  Block map_scratch;                    // tvl1_postprocess_affine's staged map planes
  Block align_scratch;                  // tvl1_find_alignment's pyramid, keys, descriptors
  int4 *align_pat = nullptr;            // the rBRIEF pair pattern (device, set once)
  Block shift_scratch;                  // tvl1_estimate_shift's pyramids, tables and records
  Block seed_scratch;                   // tvl1_calc_batch_const_init / _auto_init: every pair's
                                        // constants (then two planes for pairs solved alone)
  Block count_scratch;                  // the counted utility calls' per-pair counters (zero_above, compose,
                                        // invert): one block, no solver scratch, sized once for a chunk of
                                        // the largest record.  Shared safely: a counted call synchronises
                                        // its stream before it returns, and a ctx is used from one thread
  bool invert_window = true;            // TVL1_INVERT_WINDOW: k_invert_flow's LDS-window arm (the default:
                                        // 1.9-2.1 x the global arm's rate at K = 8); 0: global gathers
  int bnblk = 0;                        // partials per pair
  int check = 0;             // TVL1_CHECK=1: synchronise + check after every launch (diagnostics)

  // optional per-kernel-class HIP-event timing (tvl1_set_profiling).  A solve's marks are
  // reset when it starts.  The slice-list and utility calls (tvl1_blend6_u8, tvl1_half_u8,
  // tvl1_remap_flow_u8, run_chunks) run outside a solve, so their marks (class 2) wait in a
  // pool of their own for the next solve's totals (sum_marks): at most kStackMarks of them; a
  // caller that never solves loses the later ones, not memory.
  bool profiling = false;
  static constexpr size_t kStackMarks = 1024;
  MarkPool prof{64, 0}, xprof{2, kStackMarks};
};

static tvl1_status set_err(tvl1_ctx *c, tvl1_status st, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c)
    c->err = buf;
  else
    g_create_error = buf;
  return st;
}

#define HIP_TRY(ctx, expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return set_err((ctx), TVL1_EHIP, "%s failed: %s (%s:%d)", #expr,                 \
                     hipGetErrorString(e_), __FILE__, __LINE__);                        \
  } while (0)

#define TVL1_TRY(expr)                 \
  do {                                 \
    tvl1_status r_ = (expr);           \
    if (r_ != TVL1_OK) return r_;      \
  } while (0)

static tvl1_status check_params(tvl1_ctx *c, const tvl1_params *p) {
  if (!p) return set_err(c, TVL1_EINVAL, "params is NULL");
  // CV_Assert(nscales_ > 0) in calcImpl
  if (p->nscales <= 0) return set_err(c, TVL1_EINVAL, "nscales must be > 0 (got %d)", p->nscales);
  if (p->warps < 0) return set_err(c, TVL1_EINVAL, "warps must be >= 0");
  if (p->iterations < 0) return set_err(c, TVL1_EINVAL, "iterations must be >= 0");
  if (!(p->theta != 0.0)) return set_err(c, TVL1_EINVAL, "theta must be non-zero (tau/theta)");
  if (!(p->scale_step > 0.0 && p->scale_step <= 1.0))
    return set_err(c, TVL1_EINVAL, "scaleStep must be in (0, 1]");
  if (p->median_filtering > 1 && p->median_filtering != 3 && p->median_filtering != 5)
    return set_err(c, TVL1_EINVAL, "medianFiltering must be 1 (off), 3 or 5");
  if (p->fast_math < 0 || p->fast_math > 2)
    return set_err(c, TVL1_EINVAL, "fastMath must be 0 (IEEE), 1 (fast) or 2 (fma) (got %d)",
                   p->fast_math);
  if (p->profile != 0 && p->profile != 1)
    return set_err(c, TVL1_EINVAL, "profile must be 0 (CUDA OpticalFlowDual_TVL1) or 1 (CPU DualTVL1) (got %d)",
                   p->profile);
  if (p->inner_iterations < 0 || p->outer_iterations < 0)
    return set_err(c, TVL1_EINVAL, "innerIterations / outerIterations must be >= 0");
  return TVL1_OK;
}

// Arithmetic mode of a solve (kIEEE / kFast / kFma, tvl1_kernels.hpp): tvl1_params.fast_math
// for the gamma = 0 path with 0 <= tau/theta < inf; gamma != 0 and taut < 0 solves run the
// IEEE kernels.
static int math_of(const tvl1_params &p) {
  const float taut = (float)(p.tau / p.theta);
  const bool exact_div = !(taut >= 0.0f && taut <= FLT_MAX);
  return p.gamma != 0.0 || exact_div ? kIEEE : p.fast_math;
}

// Grow a block of the ctx (tvl1_arena.hpp); the reason of a failure goes to the ctx's error text.
static tvl1_status reserve(tvl1_ctx *c, Block &b, size_t need, hipStream_t st, size_t floor = 0) {
  const tvl1_status r = c->mem.reserve(b, need, st, floor);
  return r == TVL1_OK ? r : set_err(c, r, "%s", c->mem.err);
}

// Carve the arena for a geometry; grows (never shrinks) the device allocation.  The
// calls's work goes to stream st.
static tvl1_status ensure_geometry(tvl1_ctx *c, int W, int H, hipStream_t st) {
  c->mem.enter(st);
  Geometry g;
  g.W = W;
  g.H = H;
  g.gamma = c->prm.gamma != 0.0;
  g.L = pyramid_sizes(W, H, c->prm.nscales, c->prm.scale_step, g.ws, g.hs);
  for (int s = 0; s < g.L; ++s) g.ps[s] = (int)align_up((size_t)g.ws[s], 64);
  if (c->geo_valid && g.W == c->geo.W && g.H == c->geo.H && g.L == c->geo.L &&
      g.gamma == c->geo.gamma && !memcmp(g.ws, c->geo.ws, sizeof(int) * g.L) &&
      !memcmp(g.hs, c->geo.hs, sizeof(int) * g.L))
    return TVL1_OK;

  const size_t P0 = (size_t)g.ps[0];
  const size_t plane = P0 * (size_t)H * sizeof(float);
  size_t bytes = 0;
  for (int s = 0; s < g.L; ++s) bytes += 2 * (size_t)g.ps[s] * g.hs[s] * sizeof(float);
  bytes += 4 * plane;                       // G (float4)
  bytes += 2 * 3 * plane;                   // U[2][3]
  bytes += 2 * 6 * plane;                   // Pd[2][6]
  bytes += 2 * 3 * plane;                   // C[2]
  bytes += 2 * align_up(P0 * H, 256);       // in0, in1 (u8)
  bytes += 2 * plane;                       // outu, outv
  const int nblk = partials_capacity(W, H);   // residual partials
  bytes += align_up((size_t)nblk * sizeof(double), 256);
  bytes += 4096;                            // alignment slack

  if (bytes > c->arena.bytes) c->geo_valid = false;
  TVL1_TRY(reserve(c, c->arena, bytes, st));
  char *p = c->arena.p;
  auto take = [&](size_t n) {
    char *r = p;
    p += align_up(n, 256);
    return r;
  };
  for (int s = 0; s < TVL1_MAX_LEVELS; ++s) c->I0s[s] = c->I1s[s] = nullptr;
  for (int s = 0; s < g.L; ++s) {
    const size_t n = (size_t)g.ps[s] * g.hs[s] * sizeof(float);
    c->I0s[s] = (float *)take(n);
    c->I1s[s] = (float *)take(n);
  }
  c->G = (float4 *)take(4 * plane);
  for (int b = 0; b < 2; ++b)
    for (int k = 0; k < 3; ++k) c->U[b][k] = (float *)take(plane);
  for (int b = 0; b < 2; ++b)
    for (int k = 0; k < 6; ++k) c->Pd[b][k] = (float *)take(plane);
  for (int b = 0; b < 2; ++b)
    for (int k = 0; k < 3; ++k) c->C[b][k] = (float *)take(plane);
  c->in0 = (uint8_t *)take(P0 * H);
  c->in1 = (uint8_t *)take(P0 * H);
  c->outu = (float *)take(plane);
  c->outv = (float *)take(plane);
  c->partials = (double *)take((size_t)nblk * sizeof(double));
  c->partials_cap = nblk;
  c->geo = g;
  c->geo_valid = true;
  return TVL1_OK;
}

// Diagnostics (TVL1_CHECK=1): after every launch, synchronise and report which
// kernel at which level / warp / iteration failed.
#define DIAG(ctx, st, what, lev, warp, it)                                                   \
  do {                                                                                     \
    if ((ctx)->check) {                                                                    \
      hipError_t e_ = hipStreamSynchronize(st);                                            \
      if (e_ == hipSuccess) e_ = hipGetLastError();                                        \
      if (e_ != hipSuccess)                                                                \
        return set_err((ctx), TVL1_EHIP, "%s failed at level %d warp %d n %d: %s", what,    \
                       (int)(lev), (int)(warp), (int)(it), hipGetErrorString(e_));         \
    }                                                                                      \
  } while (0)

// Launch the kernel instance of a runtime arithmetic mode (tvl1_params.fast_math):
// LAUNCH(FM) expands to the launch of the FM instantiation.
#define MATH_SWITCH(m, LAUNCH) \
  if ((m) == kFast) {          \
    LAUNCH(kFast)              \
  } else if ((m) == kFma) {    \
    LAUNCH(kFma)               \
  } else {                     \
    LAUNCH(kIEEE)              \
  }

static inline dim3 grid2(int w, int h, int z = 1) {
  return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)z);
}
static const dim3 kBlk2(64, 4, 1);

// ---- fills shared by the solve paths
// IterArgs scalars of a level: its sizes, the solver's float parameters and where the residual
// partials go (plane pointers and flags are set per pass)
static IterArgs iter_args(const tvl1_params &prm, int lw, int lh, int P, double *partials) {
  IterArgs a{};
  a.W = lw;
  a.H = lh;
  a.P = P;
  a.segs = (lw + kSegPx - 1) / kSegPx;
  a.strip_rows = kStripRows;
  a.l_t = (float)(prm.lambda * prm.theta);
  a.theta = (float)prm.theta;
  a.gamma = (float)prm.gamma;
  a.taut = (float)(prm.tau / prm.theta);
  a.taut_small = taut_small(a.taut);
  a.partials = partials;
  return a;
}

// source and destination planes of the buffer sets (ui, pi), warp constants of set cb
static void set_planes(const tvl1_ctx *c, IterArgs &a, int ui, int pi, int cb) {
  a.u1s = c->U[ui][0]; a.u2s = c->U[ui][1]; a.u3s = c->U[ui][2];
  a.u1d = c->U[ui ^ 1][0]; a.u2d = c->U[ui ^ 1][1]; a.u3d = c->U[ui ^ 1][2];
  a.p11s = c->Pd[pi][0]; a.p12s = c->Pd[pi][1]; a.p21s = c->Pd[pi][2];
  a.p22s = c->Pd[pi][3]; a.p31s = c->Pd[pi][4]; a.p32s = c->Pd[pi][5];
  a.p11d = c->Pd[pi ^ 1][0]; a.p12d = c->Pd[pi ^ 1][1]; a.p21d = c->Pd[pi ^ 1][2];
  a.p22d = c->Pd[pi ^ 1][3]; a.p31d = c->Pd[pi ^ 1][4]; a.p32d = c->Pd[pi ^ 1][5];
  a.I1wx = c->C[cb][0];
  a.I1wy = c->C[cb][1];
  a.rho = c->C[cb][2];
}

// the u / p / constants plane tables of the batch arena (every batched argument block has them)
template <class T>
static void set_batch_u(const tvl1_ctx *c, T &t) {
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 2; ++j) t.U[k][j] = c->bU[k][j];
}
template <class T>
static void set_batch_uc(const tvl1_ctx *c, T &t) {
  set_batch_u(c, t);
  for (int j = 0; j < 3; ++j) t.C[j] = c->bC[j];
}
template <class T>
static void set_batch_upc(const tvl1_ctx *c, T &t) {
  set_batch_uc(c, t);
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 4; ++j) t.Pp[k][j] = c->bP[k][j];
}

// Stats epilogue of a solve: levels, iteration counts, checks and misses (SURVEY 8(d) bytes
// with the executed iterations); the per-kernel-class figures start at zero (put_class_totals)
static void fill_stats(tvl1_stats *s, const Geometry &g, int warps, const int64_t *level_iters,
                       int64_t checks, int32_t misses) {
  s->levels = g.L;
  int64_t tot = 0;
  for (int l = 0; l < TVL1_MAX_LEVELS; ++l) {
    s->level_width[l] = l < g.L ? g.ws[l] : 0;
    s->level_height[l] = l < g.L ? g.hs[l] : 0;
    s->level_iterations[l] = l < g.L ? level_iters[l] : 0;
    tot += l < g.L ? level_iters[l] : 0;
  }
  s->iterations_total = tot;
  s->checks_total = checks;
  s->speculation_misses = misses;
  s->algorithmic_bytes = survey_bytes(g.L, g.ws, g.hs, warps, level_iters);
  for (int k = 0; k < 4; ++k) {
    s->kernel_ms[k] = 0.0;
    s->kernel_launches[k] = 0;
    s->kernel_bytes[k] = 0.0;
    s->kernel_hbm_bytes[k] = 0.0;
  }
}

// Per-kernel-class totals of the profiling marks of a solve (tvl1_set_profiling): waits for
// the last mark's event
struct ClassTotals {
  double ms[4] = {}, bytes[4] = {}, hbm[4] = {};
  int64_t launches[4] = {};
};
// each: wait for every mark's event (marks of several streams), not for the last one's only
static tvl1_status add_marks(tvl1_ctx *c, const MarkPool &p, bool each, ClassTotals &t) {
  if (!c->profiling || p.marks.empty()) return TVL1_OK;
  if (!each) HIP_TRY(c, hipEventSynchronize(p.ev[p.marks.back().b]));
  for (const auto &m : p.marks) {
    float ms = 0.f;
    if (each) HIP_TRY(c, hipEventSynchronize(p.ev[m.b]));
    HIP_TRY(c, hipEventElapsedTime(&ms, p.ev[m.a], p.ev[m.b]));
    t.ms[m.cls] += ms;
    t.launches[m.cls] += 1;
    t.bytes[m.cls] += m.bytes;
    t.hbm[m.cls] += m.hbm_bytes;
  }
  return TVL1_OK;
}
static tvl1_status sum_marks(tvl1_ctx *c, ClassTotals &t) {
  TVL1_TRY(add_marks(c, c->xprof, true, t));   // slice-list calls since the last solve
  if (c->profiling) c->xprof.reset();
  return add_marks(c, c->prof, false, t);
}
static void put_class_totals(tvl1_stats *s, const ClassTotals &t) {
  for (int k = 0; k < 4; ++k) {
    s->kernel_ms[k] = t.ms[k];
    s->kernel_launches[k] = t.launches[k];
    s->kernel_bytes[k] = t.bytes[k];
    s->kernel_hbm_bytes[k] = t.hbm[k];
  }
}

// calcImpl + procOneScale on device inputs already in the arena
// or caller memory.  Result left in caller's u, v.
//
// Host schedule.  procOneScale's inner loop
//     for (n = 0; error > eps^2*W*H && n < iterations; ++n)
//         calcError = eps > 0 && (n & 1) && prevError < eps^2*W*H
// is known on the host for every iteration up to and including the next check,
// so those iterations run as ONE temporally blocked pass (<= kTbMax iterations);
// the residual of the check is then read exactly where OpenCV reads it.
//
// One residual check: k_reduce sums the per-block partials in a fixed order into coherent
// host memory, and the host reads it once the kernel is done -- by polling the check's
// sequence number, which k_reduce stores after the residual (a few us sooner than an event
// wait), or with c->poll = 0 by an event.  The poll gives up on a stream error.
//
// Checks are split in two so that work can be enqueued behind a check before the host reads
// it (speculation): launch_check enqueues k_reduce (residual slot and event by the
// parity of its sequence number, so the next check cannot overwrite a residual the host has
// not read yet), wait_check reads it.
// (first: the partials start there: a mid-check pass's first check, k_iterate_roll_mid)
static tvl1_status launch_check(tvl1_ctx *c, hipStream_t st, int nparts, const CheckGate &g,
                                unsigned long long *seq_out, int first = 0) {
  unsigned long long *seq_dev = (unsigned long long *)(c->pinned_dev + 1);
  const unsigned long long seq = ++c->check_seq;
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(kBlock), 0, st, c->partials + first, nparts,
                     c->pinned_dev + ((seq & 1) ? 2 : 0), c->poll ? seq_dev : nullptr, seq, g);
  HIP_TRY(c, hipGetLastError());
  if (!c->poll) HIP_TRY(c, hipEventRecord(c->ev_check[seq & 1], st));
  *seq_out = seq;
  return TVL1_OK;
}

static tvl1_status wait_check(tvl1_ctx *c, hipStream_t st, unsigned long long seq, double *out) {
  unsigned long long *seq_host = (unsigned long long *)(c->pinned + 1);
  if (!c->poll) {
    HIP_TRY(c, hipEventSynchronize(c->ev_check[seq & 1]));
  } else {
    // a later (speculative) check may already have stored its own, larger number
    for (unsigned spins = 1;; ++spins) {
      if (__atomic_load_n(seq_host, __ATOMIC_ACQUIRE) >= seq) break;
      if ((spins & 4095) == 0) {   // now and then: has the stream failed or finished?
        const hipError_t e = hipStreamQuery(st);
        if (e != hipSuccess && e != hipErrorNotReady)
          return set_err(c, TVL1_EHIP, "residual check: %s", hipGetErrorString(e));
        if (e == hipSuccess && __atomic_load_n(seq_host, __ATOMIC_ACQUIRE) < seq)
          return set_err(c, TVL1_EHIP, "residual check: stream idle without the residual");
      }
      // spin briefly, then give the core away between reads (a caller may run many
      // contexts and other host work, e.g. the CLI's decode threads)
      if (spins < 2048)
        __builtin_ia32_pause();
      else
        sched_yield();
    }
  }
  *out = *(volatile double *)(c->pinned + ((seq & 1) ? 2 : 0));
  return TVL1_OK;
}

static tvl1_status read_residual(tvl1_ctx *c, hipStream_t st, int nparts, double *out) {
  CheckGate g{};
  unsigned long long seq = 0;
  const tvl1_status r = launch_check(c, st, nparts, g, &seq);
  if (r != TVL1_OK) return r;
  return wait_check(c, st, seq, out);
}

// Profile 1 (tvl1_params.profile): the schedule of OpenCV's CPU
// cv::DualTVL1OpticalFlow::calc / procOneScale, restated in oracle/tvl1_oracle_dualtvl1.c.
// Per warp: remap (k_remap_cubic), then up to outerIterations rounds, each starting with
// medianFiltering, of up to innerIterations primal-dual iterations, every one of which
// evaluates the residual (one k_iterate launch + k_reduce + one host read each).  This is
// a compatibility mode, not the benchmark path: it keeps OpenCV's per-iteration check.
// The two input frames of a solve: u8 (tvl1_calc) or f32 (tvl1_calc_f32), device pointers,
// row pitches in bytes.
struct Frames {
  const void *I0, *I1;
  size_t pitch0, pitch1;
  bool f32;
};

// The initial flow of a solve (tvl1_calc_init): device planes of the frame's
// size, row pitch and pair stride in floats (stride 0: one seed for every pair of a batch).
// A batch may instead be seeded by one constant per pair and component (cst: device, pair b's
// at cst[2 b], cst[2 b + 1]; the planes exist nowhere then and u0 = v0 = NULL).
struct Seed {
  const float *u0, *v0;
  size_t pitch, stride;
  const float *cst;
};

// [A.1] I0f = convertTo(CV_32F, u8 ? 1 : 255) into the level-0 planes
static void convert_frames(tvl1_ctx *c, const Frames &in, int W, int H, hipStream_t st) {
  if (in.f32)
    hipLaunchKernelGGL(k_convert_f32, grid2(W, H, 2), kBlk2, 0, st, (const float *)in.I0,
                       in.pitch0, (const float *)in.I1, in.pitch1, c->I0s[0], c->I1s[0], W, H,
                       c->geo.ps[0]);
  else
    hipLaunchKernelGGL(k_convert_u8, grid2(W, H, 2), kBlk2, 0, st, (const uint8_t *)in.I0,
                       in.pitch0, (const uint8_t *)in.I1, in.pitch1, c->I0s[0], c->I1s[0], W, H,
                       c->geo.ps[0]);
}

static tvl1_status solve_dualtvl1(tvl1_ctx *c, const Frames &in, int W, int H, float *u,
                                  float *v, size_t fpitch, tvl1_stats *stats, hipStream_t st) {
  const tvl1_params &prm = c->prm;
  const Geometry &g = c->geo;
  const int L = g.L;
  const bool gam = g.gamma;
  const bool median = prm.median_filtering > 1;
  convert_frames(c, in, W, H, st);
  const double dscale = 1. / prm.scale_step;
  const int afast = area_fast_of(dscale, dscale);
  for (int s = 1; s < L; ++s)
    hipLaunchKernelGGL(k_resize_hp, grid2(g.ws[s], g.hs[s], 2), kBlk2, 0, st, c->I0s[s - 1],
                       c->I1s[s - 1], nullptr, g.ws[s - 1], g.hs[s - 1], g.ps[s - 1], c->I0s[s],
                       c->I1s[s], nullptr, g.ws[s], g.hs[s], g.ps[s], dscale, dscale, afast, 0,
                       1.0f);
  HIP_TRY(c, hipGetLastError());
  int ui = 0, pi = 0;
  {
    const size_t n = (size_t)g.ps[L - 1] * g.hs[L - 1] * sizeof(float);
    for (int k = 0; k < (gam ? 3 : 2); ++k) HIP_TRY(c, hipMemsetAsync(c->U[ui][k], 0, n, st));
  }
  const float taut = (float)(prm.tau / prm.theta);
  const bool exact_div = !(taut >= 0.0f && taut <= FLT_MAX);
  const float upmul = (float)(1.0 / prm.scale_step);
  int64_t level_iters[TVL1_MAX_LEVELS] = {};
  for (int s = L - 1; s >= 0; --s) {
    const int lw = g.ws[s], lh = g.hs[s], P = g.ps[s];
    const float scaledEps = (float)(prm.epsilon * prm.epsilon * (double)(lw * lh));
    hipLaunchKernelGGL(k_gradient, grid2(lw, lh), kBlk2, 0, st, c->I1s[s], lw, lh, P, c->G);
    IterArgs a = iter_args(prm, lw, lh, P, c->partials);
    a.calc_err = 1;
    const int nblk = iterate_blocks(lw, lh);
    bool p_zero = true;
    for (int wp = 0; wp < prm.warps; ++wp) {
      hipLaunchKernelGGL(k_remap_cubic, grid2(lw, lh), kBlk2, 0, st, c->I0s[s], c->G,
                         c->U[ui][0], c->U[ui][1], lw, lh, P, c->C[0][0], c->C[0][1],
                         c->C[0][2]);
      float error = FLT_MAX;
      int n = 0;
      for (int no = 0; error > scaledEps && no < prm.outer_iterations; ++no) {
        if (median) {
          hipLaunchKernelGGL(k_median, grid2(lw, lh, 2), kBlk2, 0, st, c->U[ui][0], c->U[ui][1],
                             lw, lh, P, prm.median_filtering, c->U[ui ^ 1][0], c->U[ui ^ 1][1]);
          if (gam)
            HIP_TRY(c, hipMemcpyAsync(c->U[ui ^ 1][2], c->U[ui][2], (size_t)P * lh * sizeof(float),
                                      hipMemcpyDeviceToDevice, st));
          ui ^= 1;
        }
        for (int ni = 0; error > scaledEps && ni < prm.inner_iterations; ++ni) {
          set_planes(c, a, ui, pi, 0);
          a.p_zero = p_zero ? 1 : 0;
          if (gam && exact_div)
            hipLaunchKernelGGL((k_iterate<true, true, true>), dim3(nblk), dim3(kBlock), 0, st, a);
          else if (exact_div)
            hipLaunchKernelGGL((k_iterate<false, true, true>), dim3(nblk), dim3(kBlock), 0, st, a);
          else if (gam)
            hipLaunchKernelGGL((k_iterate<true, false, true>), dim3(nblk), dim3(kBlock), 0, st, a);
          else
            hipLaunchKernelGGL((k_iterate<false, false, true>), dim3(nblk), dim3(kBlock), 0, st, a);
          double e = 0.0;
          {
            const tvl1_status r = read_residual(c, st, nblk, &e);
            if (r != TVL1_OK) return r;
          }
          error = (float)e;
          p_zero = false;
          ui ^= 1;
          pi ^= 1;
          ++n;
        }
      }
      level_iters[s] += n;
      if (stats && stats->warp_iterations && s * prm.warps + wp < stats->warp_iterations_capacity)
        stats->warp_iterations[s * prm.warps + wp] = n;
    }
    HIP_TRY(c, hipGetLastError());
    if (s == 0) break;
    // resize(u, .., I0s[s-1].size()), then multiply u1, u2 (not u3) by 1/scaleStep
    const int dw = g.ws[s - 1], dh = g.hs[s - 1];
    const double sxu = 1. / ((double)dw / lw), syu = 1. / ((double)dh / lh);
    hipLaunchKernelGGL(k_resize_hp, grid2(dw, dh, gam ? 3 : 2), kBlk2, 0, st, c->U[ui][0],
                       c->U[ui][1], c->U[ui][2], lw, lh, P, c->U[ui ^ 1][0], c->U[ui ^ 1][1],
                       c->U[ui ^ 1][2], dw, dh, g.ps[s - 1], sxu, syu, area_fast_of(sxu, syu), 2,
                       upmul);
    ui ^= 1;
  }
  hipLaunchKernelGGL(k_output, grid2(W, H), kBlk2, 0, st, c->U[ui][0], c->U[ui][1], W, H,
                     g.ps[0], u, v, fpitch);
  HIP_TRY(c, hipGetLastError());
  if (stats) {
    fill_stats(stats, g, prm.warps, level_iters, 0, 0);
    stats->checks_total = stats->iterations_total;   // every iteration evaluates the residual
  }
  return TVL1_OK;
}

// Solves in progress per device in this process.  Speculation pays only for a
// solve alone on its device: with other pairs in flight their kernels already fill the
// check round trips, and a wrong guess would cost them GPU time.
static std::atomic<int> g_solving[64];
struct SolveCount {
  int d;
  explicit SolveCount(int dev) : d(dev & 63) { g_solving[d].fetch_add(1, std::memory_order_relaxed); }
  ~SolveCount() { g_solving[d].fetch_sub(1, std::memory_order_relaxed); }
};

// share of the resident slots a streaming launch is sized for: all of them for a solve
// alone on its device, fill_shared while other solves are in progress (their blocks fill
// the rest instead of waiting for this launch's last round).  Segmentation never changes
// a result (tests/test_gpu_parity.py TVL1_ROLL_SEG cases)
static int fill_now(const tvl1_ctx *c) {
  return g_solving[c->device & 63].load(std::memory_order_relaxed) > 1 ? c->fill_shared : c->fill;
}

// ---------------------------------------------------------------- single-pair launchers
// The streaming kernels (k_iterate_roll, k_warp_ring, k_warp_iter) take 32-bit buffer
// byte offsets, and the iteration passes address a whole plane group (RollBufs: up to 6
// planes at the level-0 plane stride) through one descriptor: a level whose largest group
// reaches c->buf_limit bytes uses the 64-bit-addressed kernels (k_warp_img, k_iterate_tb).
static size_t plane_stride(const tvl1_ctx *c) {   // arena plane stride
  return (size_t)c->geo.ps[0] * c->geo.H * sizeof(float);
}
static size_t group_bytes(const tvl1_ctx *c, int s, int planes) {
  return (size_t)(planes - 1) * plane_stride(c) + (size_t)c->geo.ps[s] * c->geo.hs[s] * sizeof(float);
}
static bool buffer_ok(const tvl1_ctx *c, int s) {
  return group_bytes(c, s, c->geo.gamma ? 6 : 4) < c->buf_limit;
}
// the planes of a pass as RollBufs groups (the arena keeps each set's planes contiguous)
static RollBufs roll_bufs(const tvl1_ctx *c, int s, int uset, int pset, int cbuf) {
  const bool gam = c->geo.gamma;
  RollBufs b;
  b.c = c->C[cbuf][0];
  b.us = c->U[uset][0];
  b.ud = c->U[uset ^ 1][0];
  b.ps = c->Pd[pset][0];
  b.pd = c->Pd[pset ^ 1][0];
  b.pstride = (unsigned)plane_stride(c);
  b.cb = (unsigned)group_bytes(c, s, 3);
  b.ub = (unsigned)group_bytes(c, s, gam ? 3 : 2);
  b.pb = (unsigned)group_bytes(c, s, gam ? 6 : 4);
  return b;
}

// What the launchers need of one pyramid level of a single-pair solve
struct Level {
  tvl1_ctx *c;
  hipStream_t st;
  int s, lw, lh, P;
  IterArgs a;        // the level's scalars (iter_args); planes and flags are set per pass
  int math;          // kIEEE / kFast / kFma (math_of)
  bool gam, exact_div;
  bool roll_ok;      // the level's planes fit 32-bit buffer offsets (the streaming kernels)
  bool roll_long;    // ... and passes of >= 3 iterations stream too
};

// K5 warpBackward of warp wp: the constants of set cbuf from the flow of set uset
static tvl1_status gather(const Level &lv, int uset, int cbuf, int wp) {
  tvl1_ctx *c = lv.c;
  hipStream_t st = lv.st;
  const int s = lv.s, lw = lv.lw, lh = lv.lh, P = lv.P;
  size_t t0 = c->prof.begin(c->profiling, st);
  if (!lv.roll_ok) {
    const int tx = (lw + kWarpTW - 1) / kWarpTW, ty = (lh + kWarpTH - 1) / kWarpTH;
#define WARP_IMG(FM)                                                                           \
  hipLaunchKernelGGL(k_warp_img<FM>, dim3(tx * ty), dim3(256), 0, st, c->I0s[s], c->I1s[s],    \
                     c->U[uset][0], c->U[uset][1], lw, lh, P, tx, c->C[cbuf][0], c->C[cbuf][1], \
                     c->C[cbuf][2]);
    MATH_SWITCH(lv.math, WARP_IMG)
#undef WARP_IMG
  } else {
    WarpRingArgs wa;
    wa.I0 = c->I0s[s];
    wa.I1 = c->I1s[s];
    wa.u1 = c->U[uset][0];
    wa.u2 = c->U[uset][1];
    wa.I1wx = c->C[cbuf][0];
    wa.I1wy = c->C[cbuf][1];
    wa.rho = c->C[cbuf][2];
    wa.W = lw;
    wa.H = lh;
    wa.P = P;
    const StreamPlan sp = plan_warp_ring(lw, lh, 6, fill_slots(c->warp_ring_slots, fill_now(c)), c->roll_seg);
    wa.bands = sp.bands;
    wa.seg_rows = sp.seg_rows;
    wa.waves = sp.waves;
#define WARP_RING(FM) \
  hipLaunchKernelGGL((k_warp_ring<6, 2, FM>), dim3(wa.waves), dim3(128), 0, st, wa);
    MATH_SWITCH(lv.math, WARP_RING)
#undef WARP_RING
  }
  // algorithmic: 40 B/px per warp; compulsory here ~28 B/px (I1 x 1 + 2M/64)
  c->prof.end(st, t0, 1, (double)lw * lh * 40.0, (double)lw * lh * 28.0);
  DIAG(c, st, "warp kernel", s, wp, -1);
  return TVL1_OK;
}

// the flow of level s (set uset) zoomed to level s-1 (set uset^1), scaled by 1/scaleStep
static tvl1_status upsample(const Level &lv, int uset) {
  tvl1_ctx *c = lv.c;
  hipStream_t st = lv.st;
  const Geometry &g = c->geo;
  const int s = lv.s, lw = lv.lw, lh = lv.lh;
  const int dw = g.ws[s - 1], dh = g.hs[s - 1];
  const float fxu = (float)(1.0 / ((double)dw / lw));
  const float fyu = (float)(1.0 / ((double)dh / lh));
  const float upmul = (float)(1.0 / c->prm.scale_step);
  size_t t0 = c->prof.begin(c->profiling, st);
  if (contracts(lv.math))
    hipLaunchKernelGGL(k_upsample<true>, grid2(dw, dh, lv.gam ? 3 : 2), kBlk2, 0, st, c->U[uset][0],
                       c->U[uset][1], c->U[uset][2], lw, lh, g.ps[s], c->U[uset ^ 1][0],
                       c->U[uset ^ 1][1], c->U[uset ^ 1][2], dw, dh, g.ps[s - 1], fxu, fyu, upmul);
  else
    hipLaunchKernelGGL(k_upsample<false>, grid2(dw, dh, lv.gam ? 3 : 2), kBlk2, 0, st, c->U[uset][0],
                       c->U[uset][1], c->U[uset][2], lw, lh, g.ps[s], c->U[uset ^ 1][0],
                       c->U[uset ^ 1][1], c->U[uset ^ 1][2], dw, dh, g.ps[s - 1], fxu, fyu, upmul);
  c->prof.end(st, t0, 2, (double)lw * lh * 8.0 + (double)dw * dh * 8.0);
  DIAG(c, st, "k_upsample", s, -1, -1);
  return TVL1_OK;
}

// (One iteration pass: PassReq, tvl1_walk.hpp.)
// Each launcher takes the pass's IterArgs (planes and flags set), launches its kernel family
// and returns the number of residual partials the pass wrote (-1: the ctx's error is set, a
// TVL1_EHIP), with the compulsory HBM bytes of the launch in *hbm.
static int partials_fit(tvl1_ctx *c, int need, int blocks, const char *what) {
  if (need <= c->partials_cap) return blocks;
  (void)set_err(c, TVL1_EHIP, "internal: %d %s > partials capacity %d", blocks, what, c->partials_cap);
  return -1;
}

// the warp's first pass with warpBackward fused in (k_warp_iter), storing the constants if store_c
static int launch_warp_iter(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  tvl1_ctx *c = lv.c;
  WarpIterArgs w;
  w.ra.b = roll_bufs(c, lv.s, p.ui, p.pi, p.cb);
  w.ra.it = a;
  w.I0 = c->I0s[lv.s];
  w.I1 = c->I1s[lv.s];
  w.store_c = p.store_c ? 1 : 0;
  constexpr int M = kWiMargin, BW = 128;
  const StreamPlan sp = plan_warp_iter(lv.lw, lv.lh, BW, M, fill_slots(c->witer_slots, fill_now(c)), c->roll_seg);
  w.ra.bands = sp.bands;
  w.ra.seg_rows = sp.seg_rows;
  w.ra.waves = sp.waves;
  if (partials_fit(c, sp.waves, sp.waves, "blocks") < 0) return -1;
#define WITER(FM)                                                                           \
  if (c->wi_nc == 2)                                                                       \
    hipLaunchKernelGGL((k_warp_iter<M, FM, BW, 1, 2>), dim3(w.ra.waves), dim3(128 + BW),    \
                       c->probe_wi_lds, lv.st, w);                                          \
  else                                                                                     \
    hipLaunchKernelGGL((k_warp_iter<M, FM, BW, 1, 1>), dim3(w.ra.waves), dim3(64 + BW), 0, lv.st, w);
  MATH_SWITCH(lv.math, WITER)
#undef WITER
  *hbm = warp_iter_hbm(sp, lv.lh, BW, wi_ww<M, BW>(), (double)lv.lw * lv.lh, p.p_zero, p.store_c);
  return sp.waves;
}

// taut < 0 or not finite: one iteration per launch, IEEE divisions (k_iterate)
static int launch_iterate(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  const int nblk = iterate_blocks(lv.lw, lv.lh);
  if (lv.gam)
    hipLaunchKernelGGL((k_iterate<true, true>), dim3(nblk), dim3(kBlock), 0, lv.st, a);
  else
    hipLaunchKernelGGL((k_iterate<false, true>), dim3(nblk), dim3(kBlock), 0, lv.st, a);
  *hbm = iterate_hbm((double)lv.lw * lv.lh, p.k, pass_planes(lv.gam, p.p_zero));
  return nblk;
}

// the streaming pass (k_iterate_roll<G, K, PX>); p.mid: a 4-iteration pass that also keeps the
// residual after 2 (k_iterate_roll_mid: two partials per wavefront)
static int launch_roll(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  const bool midp = p.mid;
  tvl1_ctx *c = lv.c;
  hipStream_t st = lv.st;
  const int k = p.k, math = lv.math;
  const bool gam = lv.gam;
  RollArgs ra;
  ra.b = roll_bufs(c, lv.s, p.ui, p.pi, p.cb);
  ra.it = a;
  const int px = k <= 2 && (long)lv.lw * lv.lh >= c->roll_px4_min ? 4 : 2;
  const int slots = midp ? c->mid_slots : c->roll_slots[k][gam][px];
  const StreamPlan sp = plan_roll(lv.lw, lv.lh, k, px, fill_slots(slots, fill_now(c)), c->roll_seg);
  ra.bands = sp.bands;
  ra.seg_rows = sp.seg_rows;
  ra.waves = sp.waves;   // one residual partial per wavefront (two for the mid pass)
  if (partials_fit(c, (midp ? 2 : 1) * sp.waves, sp.waves, "wavefronts") < 0) return -1;
  if (midp && (k != 4 || px != 2 || gam || !p.calc_end)) {
    (void)set_err(c, TVL1_EHIP, "internal: mid-check pass of k = %d, px = %d", k, px);
    return -1;
  }
  const dim3 grid((ra.waves + 3) / 4);
#define ROLL_G(K, PX) \
  hipLaunchKernelGGL((k_iterate_roll<true, K, PX>), grid, dim3(256), 0, st, ra);
#define ROLL_M(FM, K, PX)                                                                  \
  if (c->probe_lds > 0)                                                                    \
    (void)hipFuncSetAttribute((const void *)k_iterate_roll<false, K, PX, FM>,              \
                              hipFuncAttributeMaxDynamicSharedMemorySize, c->probe_lds);   \
  hipLaunchKernelGGL((k_iterate_roll<false, K, PX, FM>), grid, dim3(256), c->probe_lds, st, ra);
#define ROLL(K, PX)                     \
  if (gam) {                            \
    ROLL_G(K, PX)                       \
  } else if (math == kFast) {           \
    ROLL_M(kFast, K, PX)                \
  } else if (math == kFma) {            \
    ROLL_M(kFma, K, PX)                 \
  } else {                              \
    ROLL_M(kIEEE, K, PX)                \
  }
#define MID_M(FM) hipLaunchKernelGGL((k_iterate_roll_mid<FM>), grid, dim3(256), 0, st, ra);
  if (midp) {
    MATH_SWITCH(math, MID_M)
  } else if (px == 4) {   // k <= 2
    if (k == 1) {
      ROLL(1, 4)
    } else {
      ROLL(2, 4)
    }
  } else {
    switch (k) {
      case 1: ROLL(1, 2) break;
      case 2: ROLL(2, 2) break;
      case 3: ROLL(3, 2) break;
      default: ROLL(4, 2) break;
    }
  }
#undef MID_M
#undef ROLL
#undef ROLL_M
#undef ROLL_G
  *hbm = roll_hbm(sp, lv.lh, k, px, (double)lv.lw * lv.lh, pass_planes(gam, p.p_zero));
  return sp.waves;
}

// the 2- or 4-iteration pass with a wavefront per iteration (k_iterate_stages, gamma = 0)
static bool stages_take(const Level &lv, const PassReq &p) {
  const tvl1_ctx *c = lv.c;
  if (!c->stages || lv.gam || !lv.roll_ok || p.mid || (p.k != 2 && p.k != 4)) return false;
  return c->stages == 2 || (p.k == 4 && !lv.roll_long && c->tb4);
}
static int launch_stages(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  tvl1_ctx *c = lv.c;
  RollArgs ra;
  ra.b = roll_bufs(c, lv.s, p.ui, p.pi, p.cb);
  ra.it = a;
  const StreamPlan sp =
      plan_stages(lv.lw, lv.lh, p.k,
                  fill_slots(c->stage_slots[p.k], c->stages_fill > 0       ? c->stages_fill
                                                  : fill_now(c) == c->fill ? c->fill
                                                                           : kStagesFillShared),
                  c->roll_seg);
  ra.bands = sp.bands;
  ra.seg_rows = sp.seg_rows;
  ra.waves = sp.waves;   // blocks: one residual partial each
  if (partials_fit(c, sp.waves, sp.waves, "blocks") < 0) return -1;
#define STAGES_M(FM)                                                                        \
  if (p.k == 2)                                                                             \
    hipLaunchKernelGGL((k_iterate_stages<FM, 2>), dim3(sp.waves), dim3(128), 0, lv.st, ra);  \
  else                                                                                      \
    hipLaunchKernelGGL((k_iterate_stages<FM, 4>), dim3(sp.waves), dim3(256), 0, lv.st, ra);
  MATH_SWITCH(lv.math, STAGES_M)
#undef STAGES_M
  *hbm = stages_hbm(sp, lv.lh, p.k, (double)lv.lw * lv.lh, pass_planes(false, p.p_zero));
  return sp.waves;
}

// blocked pass in 64 x 48 regions, 3 rows x 2 px per thread (k_iterate_tb4, gamma = 0)
static int launch_tb4(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  const BlockedPlan bp = tb4_plan(lv.lw, lv.lh, p.k);
  TBArgs t;
  t.it = a;
  t.niter = p.k;
  t.tiles_x = bp.tiles_x;
  t.out_h = bp.out_h;
  const int blocks = bp.blocks;
  if (partials_fit(lv.c, blocks, blocks, "blocks") < 0) return -1;
#define TB4_M(FM) \
  hipLaunchKernelGGL((k_iterate_tb4<FM>), dim3(blocks), dim3(32 * kTb4Groups), 0, lv.st, t);
  MATH_SWITCH(lv.math, TB4_M)
#undef TB4_M
  *hbm = blocked_hbm(blocks, kTb4Groups * kTb4RowsPerThread, (double)lv.lw * lv.lh,
                     pass_planes(lv.gam, p.p_zero));
  return blocks;
}

// blocked pass in 64 x 32 regions, 2 px per lane (k_iterate_tb)
static int launch_tb(const Level &lv, const IterArgs &a, const PassReq &p, double *hbm) {
  const BlockedPlan bp = tb_plan(lv.lw, lv.lh, p.k);
  TBArgs t;
  t.it = a;
  t.niter = p.k;
  t.tiles_x = bp.tiles_x;
  t.out_h = bp.out_h;
  const int blocks = bp.blocks;
  if (partials_fit(lv.c, blocks, blocks, "blocks") < 0) return -1;
  constexpr int rh = kTbRows;
#define TB(G, FM) \
  hipLaunchKernelGGL((k_iterate_tb<G, rh, 1, 2, FM>), dim3(blocks), dim3(32 * rh), 0, lv.st, t);
#define TB_M(FM) TB(false, FM)
  if (lv.gam) {
    TB(true, kIEEE)
  } else {
    MATH_SWITCH(lv.math, TB_M)
  }
#undef TB_M
#undef TB
  *hbm = blocked_hbm(blocks, rh, (double)lv.lw * lv.lh, pass_planes(lv.gam, p.p_zero));
  return blocks;
}

// Pass kernels: 2-iteration passes (HBM-bound) stream through k_iterate_roll's x-only
// halo; passes of >= 3 iterations are VALU-bound, where the streaming kernel wins only
// while the level has enough rows for one round of >= 32-row segments (short segments
// repeat the 2K-row halo) and k_iterate_tb (64 x 32 regions, 2 px/lane) wins below.
// Planes beyond 32-bit buffer offsets take k_iterate_tb for every pass.
// p.witer: the warp's first pass as k_warp_iter (storing the constants if p.store_c); p.mid: a
// mid-check pass.  blocks_out: the residual partials of the pass (per check of a mid pass).
static tvl1_status launch_pass(const Level &lv, const PassReq &p, int wp, int n, int &blocks_out) {
  tvl1_ctx *c = lv.c;
  IterArgs a = lv.a;
  set_planes(c, a, p.ui, p.pi, p.cb);
  a.calc_err = p.calc_end ? 1 : 0;
  a.p_zero = p.p_zero ? 1 : 0;
  a.gate = p.gated ? c->gate : nullptr;
  a.gate_seq = p.gseq;
  const size_t tkp = c->prof.begin(c->profiling, lv.st);
  const double Nl = (double)lv.lw * lv.lh;
  double hbm = 0.0;
  int blocks;
  if (p.witer)
    blocks = launch_warp_iter(lv, a, p, &hbm);
  else if (lv.exact_div)
    blocks = launch_iterate(lv, a, p, &hbm);
  else if (stages_take(lv, p))
    blocks = launch_stages(lv, a, p, &hbm);
  else if (lv.roll_ok && (p.k <= 2 || lv.roll_long))
    blocks = launch_roll(lv, a, p, &hbm);
  else if (c->tb4 && !lv.gam)
    blocks = launch_tb4(lv, a, p, &hbm);
  else
    blocks = launch_tb(lv, a, p, &hbm);
  if (blocks < 0) return TVL1_EHIP;
  // algorithmic: 64 B/px per executed iteration (+ 40 B/px for a fused
  // warpBackward)
  c->prof.end(lv.st, tkp, 0, Nl * 64.0 * p.k + (p.witer ? Nl * 40.0 : 0.0), hbm);
  DIAG(c, lv.st, "iteration pass", lv.s, wp, n);
  blocks_out = blocks;
  return TVL1_OK;
}

// walk_level's backend (tvl1_walk.hpp): the launches of one level of a single-pair solve
struct LevelOps {
  const Level &lv;
  const WalkLevel &wl;
  tvl1_stats *stats;
  // profiling marks and check numbers taken so far: launches that ran empty give theirs back
  struct Mark {
    size_t marks, ev_used;
    unsigned long long check_seq;
  };

  // build-only median of u before a warp
  tvl1_status median(int ui) {
    tvl1_ctx *c = lv.c;
    hipLaunchKernelGGL(k_median, grid2(lv.lw, lv.lh, 2), kBlk2, 0, lv.st, c->U[ui][0], c->U[ui][1], lv.lw,
                       lv.lh, lv.P, c->prm.median_filtering, c->U[ui ^ 1][0], c->U[ui ^ 1][1]);
    if (lv.gam) {
      const size_t n = (size_t)lv.P * lv.lh * sizeof(float);
      HIP_TRY(c, hipMemcpyAsync(c->U[ui ^ 1][2], c->U[ui][2], n, hipMemcpyDeviceToDevice, lv.st));
    }
    return TVL1_OK;
  }
  tvl1_status gather(int ui, int cb, int wp) { return ::gather(lv, ui, cb, wp); }
  tvl1_status pass(const PassReq &p, int wp, int n, int *blocks) { return launch_pass(lv, p, wp, n, *blocks); }
  // the check's speculation gate: the device word, and the level's stopping rule for gate_holds
  tvl1_status check(const CheckReq &q, unsigned long long *seq) {
    CheckGate gt{};
    if (q.gated_in) {
      gt.in = lv.c->gate;
      gt.in_seq = q.in_seq;
    }
    if (q.gate_out) {
      gt.out = lv.c->gate;
      gt.thr = wl.scaledEps;
      gt.n = q.n;
      gt.iters = wl.iterations;
      gt.kmax = wl.kmax;
      gt.eps_pos = 1;
      gt.pk = q.pk;
      gt.pcalc = q.pcalc;
    }
    return launch_check(lv.c, lv.st, q.blocks, gt, seq, q.first);
  }
  tvl1_status wait(unsigned long long seq, double *e) { return wait_check(lv.c, lv.st, seq, e); }
  Mark mark() const { return Mark{lv.c->prof.marks.size(), lv.c->prof.used, lv.c->check_seq}; }
  void rollback(const Mark &m) {
    lv.c->prof.marks.resize(m.marks);
    lv.c->prof.used = m.ev_used;
    lv.c->check_seq = m.check_seq;
  }
  // speculates only a solve alone on its device (TVL1_SPEC=2: always)
  bool alone() const {
    return !(lv.c->spec == 1 && g_solving[lv.c->device & 63].load(std::memory_order_relaxed) > 1);
  }
  void trace(const char *line) { fputs(line, stderr); }
  void warp_done(int wp, int n) {
    const int i = lv.s * wl.warps + wp;
    if (stats && stats->warp_iterations && i < stats->warp_iterations_capacity) stats->warp_iterations[i] = n;
  }
};

// [A.1] convertTo + [A.2] pyramid, kernel step = float(1/scaleStep)
static tvl1_status build_pyramid(tvl1_ctx *c, const Frames &in, int W, int H, hipStream_t st) {
  const Geometry &g = c->geo;
  const size_t tk = c->prof.begin(c->profiling, st);
  convert_frames(c, in, W, H, st);
  const float fdown = (float)(1.0 / c->prm.scale_step);
  const bool contract_pyr = contracts(math_of(c->prm));
  for (int s = 1; s < g.L; ++s) {
    if (contract_pyr)
      hipLaunchKernelGGL(k_resize_down2<true>, grid2(g.ws[s], g.hs[s], 2), kBlk2, 0, st,
                         c->I0s[s - 1], c->I1s[s - 1], g.ws[s - 1], g.hs[s - 1], g.ps[s - 1],
                         c->I0s[s], c->I1s[s], g.ws[s], g.hs[s], g.ps[s], fdown, fdown);
    else
      hipLaunchKernelGGL(k_resize_down2<false>, grid2(g.ws[s], g.hs[s], 2), kBlk2, 0, st,
                         c->I0s[s - 1], c->I1s[s - 1], g.ws[s - 1], g.hs[s - 1], g.ps[s - 1],
                         c->I0s[s], c->I1s[s], g.ws[s], g.hs[s], g.ps[s], fdown, fdown);
  }
  double b = (double)W * H * (2 + 8);
  for (int s = 1; s < g.L; ++s) b += (double)g.ws[s] * g.hs[s] * 8 + (double)g.ws[s - 1] * g.hs[s - 1] * 8;
  c->prof.end(st, tk, 2, b);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

// The flow the coarsest level starts from, in the u set *ui: 0, or the seed's coarsest level.
// [A.2b] the seed's pyramid: u[s] = resize(u[s-1]) * scaleStep, a chain of rounded levels.
// Only its coarsest level reaches the solver (every upsample overwrites the finer one), so
// the first step reads the caller's planes and the steps ping-pong between the two u sets;
// a one-level pyramid takes the seed as it is.  u3 = 0 at the coarsest level either way.
static tvl1_status initial_flow(tvl1_ctx *c, const Seed *seed, int W, int H, hipStream_t st, int *ui_out) {
  const Geometry &g = c->geo;
  const int L = g.L;
  const bool gam = g.gamma;
  int ui = 0;
  if (!seed) {         // u = 0 at the coarsest level (no initial flow)
    const size_t n = (size_t)g.ps[L - 1] * g.hs[L - 1] * sizeof(float);
    HIP_TRY(c, hipMemsetAsync(c->U[ui][0], 0, n, st));
    HIP_TRY(c, hipMemsetAsync(c->U[ui][1], 0, n, st));
    if (gam) HIP_TRY(c, hipMemsetAsync(c->U[ui][2], 0, n, st));
    *ui_out = ui;
    return TVL1_OK;
  }
  const float fdown = (float)(1.0 / c->prm.scale_step);
  const float fmul = (float)c->prm.scale_step;
  const bool contract_pyr = contracts(math_of(c->prm));
  const size_t tk = c->prof.begin(c->profiling, st);
  double b = 0.0;
  if (L == 1) {
    hipLaunchKernelGGL(kb_flow_copy, grid2(W, H, 2), kBlk2, 0, st, seed->u0, seed->v0,
                       (int)seed->pitch, (size_t)0, c->U[ui][0], c->U[ui][1], W, H, g.ps[0],
                       (size_t)0);
    b = (double)W * H * 16.0;
  }
  for (int s = 1; s < L; ++s) {
    const float *s1 = s == 1 ? seed->u0 : c->U[ui][0], *s2 = s == 1 ? seed->v0 : c->U[ui][1];
    const int sp = s == 1 ? (int)seed->pitch : g.ps[s - 1];
    if (s > 1) ui ^= 1;
    if (contract_pyr)
      hipLaunchKernelGGL(k_flow_down<true>, grid2(g.ws[s], g.hs[s], 2), kBlk2, 0, st, s1, s2,
                         g.ws[s - 1], g.hs[s - 1], sp, c->U[ui][0], c->U[ui][1], g.ws[s],
                         g.hs[s], g.ps[s], fdown, fdown, fmul);
    else
      hipLaunchKernelGGL(k_flow_down<false>, grid2(g.ws[s], g.hs[s], 2), kBlk2, 0, st, s1, s2,
                         g.ws[s - 1], g.hs[s - 1], sp, c->U[ui][0], c->U[ui][1], g.ws[s],
                         g.hs[s], g.ps[s], fdown, fdown, fmul);
    b += (double)g.ws[s] * g.hs[s] * 8 + (double)g.ws[s - 1] * g.hs[s - 1] * 8;
  }
  c->prof.end(st, tk, 2, b);
  if (gam)
    HIP_TRY(c, hipMemsetAsync(c->U[ui][2], 0, (size_t)g.ps[L - 1] * g.hs[L - 1] * sizeof(float), st));
  HIP_TRY(c, hipGetLastError());
  *ui_out = ui;
  return TVL1_OK;
}

// seed: the initial flow (tvl1_calc_init), or null for u = 0 at the coarsest level
static tvl1_status solve(tvl1_ctx *c, const Frames &in, const Seed *seed, int W, int H, float *u,
                         float *v, size_t fpitch, tvl1_stats *stats, hipStream_t st) {
  const tvl1_params &prm = c->prm;
  if (prm.profile == 1) {
    if (seed) return set_err(c, TVL1_EINVAL, "profile 1 takes no initial flow");
    return solve_dualtvl1(c, in, W, H, u, v, fpitch, stats, st);
  }
  const SolveCount active(c->device);
  const Geometry &g = c->geo;
  const int L = g.L;
  const bool gam = g.gamma;
  const bool median = prm.median_filtering > 1;
  if (c->profiling) c->prof.reset();

  TVL1_TRY(build_pyramid(c, in, W, H, st));
  WalkState ws{0, 0, 0, 50.0};   // the buffer sets in use (u, p, constants), and w0_hint
  TVL1_TRY(initial_flow(c, seed, W, H, st, &ws.ui));

  const float taut = (float)(prm.tau / prm.theta);
  // The projection's shared-reciprocal division (dual_px) needs ng = 1 + taut*|grad u| >= 1;
  // other parameters take the one-iteration kernel with plain IEEE divisions.
  const bool exact_div = !(taut >= 0.0f && taut <= FLT_MAX);

  int64_t level_iters[TVL1_MAX_LEVELS] = {};
  WalkCounts ct;
  for (int s = L - 1; s >= 0; --s) {
    const int lw = g.ws[s], lh = g.hs[s], P = g.ps[s];
    const double scaledEps = prm.epsilon * prm.epsilon * (double)lw * (double)lh;
    Level lv{};
    lv.c = c;
    lv.st = st;
    lv.s = s;
    lv.lw = lw;
    lv.lh = lh;
    lv.P = P;
    lv.a = iter_args(prm, lw, lh, P, c->partials);
    // arithmetic mode of the gamma = 0 kernels (kIEEE / kFast / kFma, tvl1_kernels.hpp);
    // gamma != 0 and taut < 0 solves run IEEE
    lv.math = math_of(prm);
    lv.gam = gam;
    lv.exact_div = exact_div;
    lv.roll_ok = buffer_ok(c, s);
    lv.roll_long = lv.roll_ok && (long)((lw + 55) / 56) * ((lh + 31) / 32) >= c->roll_long_min;
    const bool roll_ok = lv.roll_ok;

    WalkLevel wl{};
    wl.level = s;
    wl.warps = prm.warps;
    wl.iterations = prm.iterations;
    wl.kmax = exact_div ? 1 : roll_ok ? kRollMax : kTbMax;
    wl.scaledEps = scaledEps;
    wl.eps_pos = prm.epsilon > 0;
    // warpBackward fused into the warp's first pass (2 iterations ending in the first
    // check) when that pass would stream through k_iterate_roll anyway
    wl.fuse = c->fuse && !gam && !exact_div && roll_ok && prm.epsilon > 0 && prm.iterations >= 2 &&
              (long)lw * lh >= c->fuse_min;
    wl.median = median;
    // Speculation: behind each residual check the host enqueues the launch it
    // expects to follow, gated on the device by the check's own evaluation of the stopping
    // rule, and only then waits for the residual.  A right guess hides the host round trip;
    // a wrong one costs an empty launch, and the host enqueues the right work as before.
    wl.spec = c->spec && !exact_div && roll_ok && prm.epsilon > 0;
    // the mid-check pass (k_iterate_roll_mid) where a 4-iteration pass streams
    wl.mid = c->mid && !gam && !exact_div && lv.roll_long && prm.epsilon > 0 && kRollMax >= 4;
    wl.mid_min = c->mid_min;
    wl.spec_trace = c->spec_trace != 0;
    LevelOps ops{lv, wl, stats};
    ct.level_iters = 0;
    TVL1_TRY(walk_level(ops, wl, ws, ct));
    level_iters[s] = ct.level_iters;
    HIP_TRY(c, hipGetLastError());
    if (s == 0) break;
    TVL1_TRY(upsample(lv, ws.ui));  // zoom the flow to level s-1, scale by 1/scaleStep
    ws.ui ^= 1;
  }
  const size_t tk = c->prof.begin(c->profiling, st);
  hipLaunchKernelGGL(k_output, grid2(W, H), kBlk2, 0, st, c->U[ws.ui][0], c->U[ws.ui][1], W, H,
                     g.ps[0], u, v, fpitch);
  c->prof.end(st, tk, 2, (double)W * H * 16.0);
  HIP_TRY(c, hipGetLastError());

  ClassTotals tot;
  if (stats) fill_stats(stats, g, prm.warps, level_iters, ct.checks, ct.spec_misses);
  TVL1_TRY(sum_marks(c, tot));
  if (stats) put_class_totals(stats, tot);
  if (c->spec_trace && ct.mid_passes)
    fprintf(stderr, "mid-check passes %d, ended on the mid state %d\n", ct.mid_passes, ct.mid_taken);
  return TVL1_OK;
}


// ---------------------------------------------------------------- batched solve
// tvl1_calc_batch: n pairs of one size through the batched kernels (tvl1_batch.hpp), in
// chunks of kBatchMax.  The pairs of a chunk walk the levels and warps in lock step; inside
// a warp each pair keeps its own iteration count, stopping-rule state and u / p buffer set,
// and a pass runs the smallest number of iterations any active pair may fuse before its
// next check (<= kTbMax), so every pair sees exactly the single-pair schedule.
static tvl1_status ensure_batch(tvl1_ctx *c, int W, int H, int n, hipStream_t st) {
  const Geometry &g = c->geo;   // pyramid sizes of (W, H) (ensure_geometry ran)
  // reuse only for the same level sizes: a new scaleStep with the same level count changes
  // every level's plane stride (c->bips), and the kernels would write past each pair's slot
  if (c->barena.p && c->bW == W && c->bH == H && c->bL == g.L && c->bn >= n &&
      !memcmp(c->bws, g.ws, sizeof(int) * g.L) && !memcmp(c->bhs, g.hs, sizeof(int) * g.L))
    return TVL1_OK;
  const size_t P0 = (size_t)g.ps[0];
  const size_t ps = align_up(P0 * H, 64);
  const int tb_blocks = batch_partials_capacity(W, H);   // residual partials per pair
  size_t bytes = 0;
  size_t ips[TVL1_MAX_LEVELS];
  for (int s = 0; s < g.L; ++s) {
    ips[s] = align_up((size_t)g.ps[s] * g.hs[s], 64);
    bytes += 2 * ips[s] * n * sizeof(float) + 512;
  }
  bytes += (ps * n * sizeof(float) + 256) * (4 + 8 + 3);   // U + P + C
  bytes += (size_t)tb_blocks * n * sizeof(double) + 4096;
  c->bW = c->bH = c->bL = c->bn = 0;
  // a layout that fits re-lays the existing arena (stream-ordered like ensure_geometry's):
  // only growth allocates, so alternating batch geometries hold one arena
  TVL1_TRY(reserve(c, c->barena, bytes, st));   // TVL1_ENOMEM: the caller retries a smaller chunk
  char *p = c->barena.p;
  auto take = [&](size_t nbytes) {
    char *r = p;
    p += align_up(nbytes, 256);
    return r;
  };
  for (int s = 0; s < TVL1_MAX_LEVELS; ++s) c->bI0s[s] = c->bI1s[s] = nullptr;
  for (int s = 0; s < g.L; ++s) {
    c->bips[s] = ips[s];
    c->bI0s[s] = (float *)take(ips[s] * n * sizeof(float));
    c->bI1s[s] = (float *)take(ips[s] * n * sizeof(float));
  }
  c->bps = ps;
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 2; ++j) c->bU[k][j] = (float *)take(ps * n * sizeof(float));
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 4; ++j) c->bP[k][j] = (float *)take(ps * n * sizeof(float));
  for (int j = 0; j < 3; ++j) c->bC[j] = (float *)take(ps * n * sizeof(float));
  c->bpartials = (double *)take((size_t)tb_blocks * n * sizeof(double));
  c->bnblk = tb_blocks;
  c->bW = W;
  c->bH = H;
  c->bL = g.L;
  c->bn = n;
  memcpy(c->bws, g.ws, sizeof(int) * g.L);
  memcpy(c->bhs, g.hs, sizeof(int) * g.L);
  return TVL1_OK;
}

// ---- batched launchers
// What the batched launchers need of one level of a chunk of n pairs
struct BatchLevel {
  tvl1_ctx *c;
  hipStream_t st;
  int n;
  int s, lw, lh, P;
  int math;
  size_t ps;         // pair stride of the level-0-sized planes (floats)
  RollBufs bufs;     // RollBufs geometry of the batch arena (the kernels point it at each pair's planes)
  IterArgs it;       // pass geometry and scalars (plane pointers are set per pair)
};

// [A.1] convertTo + [A.2] pyramid of every pair
static void batch_pyramid(tvl1_ctx *c, int n, const uint8_t *I0, size_t pitch0, size_t stride0,
                          const uint8_t *I1, size_t pitch1, size_t stride1, int W, int H, hipStream_t st) {
  const Geometry &g = c->geo;
  hipLaunchKernelGGL(kb_convert, grid2(W, H, 2 * n), kBlk2, 0, st, I0, pitch0, stride0, I1,
                     pitch1, stride1, c->bI0s[0], c->bI1s[0], W, H, g.ps[0], c->bips[0]);
  const float fdown = (float)(1.0 / c->prm.scale_step);
  const bool contract = contracts(math_of(c->prm));
  for (int s = 1; s < g.L; ++s) {
#define KB_DOWN(C)                                                                             \
  hipLaunchKernelGGL(kb_resize_down2<C>, grid2(g.ws[s], g.hs[s], 2 * n), kBlk2, 0, st,         \
                     c->bI0s[s - 1], c->bI1s[s - 1], g.ws[s - 1], g.hs[s - 1], g.ps[s - 1],    \
                     c->bips[s - 1], c->bI0s[s], c->bI1s[s], g.ws[s], g.hs[s], g.ps[s],       \
                     c->bips[s], fdown, fdown);
    if (contract) {
      KB_DOWN(true)
    } else {
      KB_DOWN(false)
    }
#undef KB_DOWN
  }
}

// The flow the coarsest level starts from, in set 0 of every pair: 0, or
// [A.2b] every pair's seed pyramid (solve()'s chain): the first step reads the caller's
// planes, the steps alternate between the u sets and the last one writes set 0
static tvl1_status batch_initial_flow(tvl1_ctx *c, int n, const Seed *seed, int W, int H, hipStream_t st) {
  const Geometry &g = c->geo;
  const int L = g.L;
  const size_t ps = c->bps;
  if (!seed) {   // u = 0 at the coarsest level, set 0 of every pair
    for (int k = 0; k < 2; ++k)
      HIP_TRY(c, hipMemsetAsync(c->bU[0][k], 0, ps * n * sizeof(float), st));
    return TVL1_OK;
  }
  const float fdown = (float)(1.0 / c->prm.scale_step);
  const float fmul = (float)c->prm.scale_step;
  const bool contract = contracts(math_of(c->prm));
  const size_t tkf = c->prof.begin(c->profiling, st);
  double fb = 0.0;
  if (L == 1 && seed->cst) {
    hipLaunchKernelGGL(kb_flow_fill, grid2(W, H, 2 * n), kBlk2, 0, st, seed->cst, c->bU[0][0],
                       c->bU[0][1], W, H, g.ps[0], ps);
    fb = (double)n * W * H * 8.0;
  } else if (L == 1) {
    hipLaunchKernelGGL(kb_flow_copy, grid2(W, H, 2 * n), kBlk2, 0, st, seed->u0, seed->v0,
                       (int)seed->pitch, seed->stride, c->bU[0][0], c->bU[0][1], W, H, g.ps[0], ps);
    fb = (double)n * W * H * 16.0;
  }
  int set = L & 1;   // L - 1 steps end in set 0
  for (int s = 1; s < L; ++s, set ^= 1) {
    if (s == 1 && seed->cst) {   // per-pair constants: level 1 from a level 0 that is not stored
      if (contract)
        hipLaunchKernelGGL(kb_flow_down_const<true>, grid2(g.ws[1], g.hs[1], 2 * n), kBlk2, 0, st,
                           seed->cst, c->bU[set][0], c->bU[set][1], g.ws[1], g.hs[1], g.ps[1], ps,
                           fdown, fdown, fmul);
      else
        hipLaunchKernelGGL(kb_flow_down_const<false>, grid2(g.ws[1], g.hs[1], 2 * n), kBlk2, 0, st,
                           seed->cst, c->bU[set][0], c->bU[set][1], g.ws[1], g.hs[1], g.ps[1], ps,
                           fdown, fdown, fmul);
      fb += (double)n * g.ws[1] * g.hs[1] * 8;
      continue;
    }
    const float *s1 = s == 1 ? seed->u0 : c->bU[set ^ 1][0], *s2 = s == 1 ? seed->v0 : c->bU[set ^ 1][1];
    const int sp = s == 1 ? (int)seed->pitch : g.ps[s - 1];
    const size_t sps = s == 1 ? seed->stride : ps;
#define KB_FLOW(C)                                                                             \
  hipLaunchKernelGGL(kb_flow_down<C>, grid2(g.ws[s], g.hs[s], 2 * n), kBlk2, 0, st, s1, s2,    \
                     g.ws[s - 1], g.hs[s - 1], sp, sps, c->bU[set][0], c->bU[set][1], g.ws[s], \
                     g.hs[s], g.ps[s], ps, fdown, fdown, fmul);
    if (contract) {
      KB_FLOW(true)
    } else {
      KB_FLOW(false)
    }
#undef KB_FLOW
    fb += (double)n * ((double)g.ws[s] * g.hs[s] * 8 + (double)g.ws[s - 1] * g.hs[s - 1] * 8);
  }
  c->prof.end(st, tkf, 2, fb);
  return TVL1_OK;
}

// The coarsest level on chip (kb_small_level, one workgroup per pair: every warp's gather,
// iterations, residuals and stopping rule without leaving the workgroup); u enters as 0 (or,
// seeded, as set 0's planes: <FM, true>) and leaves in set 0.  Reads back every pair's
// iterations per warp and checks: hw[b * warps + wp], then hw[n * warps + b].
static tvl1_status batch_small_level(const BatchLevel &bl, const BatchSel &all, bool seeded,
                                     double scaledEps, std::vector<int> &hw) {
  tvl1_ctx *c = bl.c;
  hipStream_t st = bl.st;
  const tvl1_params &prm = c->prm;
  const int n = bl.n, lw = bl.lw, lh = bl.lh;
  const size_t need = (size_t)n * (prm.warps + 1) * sizeof(int);
  TVL1_TRY(reserve(c, c->small_scratch, need, st, 64 << 10));
  BatchSmall sm{};
  sm.I0 = c->bI0s[bl.s];
  sm.I1 = c->bI1s[bl.s];
  sm.u1 = c->bU[0][0];
  sm.u2 = c->bU[0][1];
  sm.ips = c->bips[bl.s];
  sm.ps = bl.ps;
  sm.W = lw;
  sm.H = lh;
  sm.P = bl.P;
  sm.warps = prm.warps;
  sm.iterations = prm.iterations;
  sm.eps_pos = prm.epsilon > 0;
  sm.thr = scaledEps;
  sm.it = bl.it;
  sm.warp_iters = c->small_scratch.as<int>();
  sm.checks = sm.warp_iters + (size_t)n * prm.warps;
  sm.sel = all;
  const size_t tks = c->prof.begin(c->profiling, st);
#define KB_SMALL(FM)                                                                               \
  if (seeded)                                                                                     \
    hipLaunchKernelGGL((kb_small_level<FM, true>), dim3(n), dim3(64 * ((lw + 63) / 64)), 0, st, sm); \
  else                                                                                            \
    hipLaunchKernelGGL((kb_small_level<FM>), dim3(n), dim3(64 * ((lw + 63) / 64)), 0, st, sm);
  MATH_SWITCH(bl.math, KB_SMALL)
#undef KB_SMALL
  HIP_TRY(c, hipGetLastError());
  hw.resize((size_t)n * (prm.warps + 1));
  HIP_TRY(c, hipMemcpyAsync(hw.data(), c->small_scratch.p, need, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  int64_t it_sum = 0;
  for (size_t i = 0; i < (size_t)n * prm.warps; ++i) it_sum += hw[i];
  // its own class (3): SURVEY 8(d)'s bytes of every iteration and warp it ran, but from HBM
  // it only reads I0, I1 and writes u once, so it would skew class 0's HBM roofline
  c->prof.end(st, tks, 3, (double)lw * lh * (64.0 * it_sum + 40.0 * n * prm.warps),
           (double)lw * lh * 16.0 * n);
  return TVL1_OK;
}

static int batch_partials_fit(tvl1_ctx *c, int blocks, const char *what) {
  if (blocks <= c->bnblk) return blocks;
  (void)set_err(c, TVL1_EHIP, "internal: %d %s > batch partials %d", blocks, what, c->bnblk);
  return -1;
}

// warpBackward fused with the warp's first pass (kb_warp_iter) for the pairs of sel, nstore
// of which store their constants.  Returns the residual partials per pair (-1: error set).
static int launch_batch_warp_iter(const BatchLevel &bl, const BatchSel &sel, int nstore) {
  tvl1_ctx *c = bl.c;
  hipStream_t st = bl.st;
  const int n = bl.n;
  const StreamPlan sp = plan_warp_iter(bl.lw, bl.lh, 128, 6, c->witer_slots, 0, n);
  if (batch_partials_fit(c, sp.waves, "blocks") < 0) return -1;
  BatchWI wi{};
  wi.w.ra.b = bl.bufs;
  wi.w.ra.it = bl.it;
  wi.w.ra.bands = sp.bands;
  wi.w.ra.seg_rows = sp.seg_rows;
  wi.w.ra.waves = sp.waves;
  wi.I0 = c->bI0s[bl.s];
  wi.I1 = c->bI1s[bl.s];
  set_batch_upc(c, wi);
  wi.ips = c->bips[bl.s];
  wi.ps = bl.ps;
  wi.partials = c->bpartials;
  wi.nblk = sp.waves;
  wi.sel = sel;
  const size_t tkw = c->prof.begin(c->profiling, st);
#define KB_WITER(FM)                                                                             \
  if (c->wi_nc == 2)                                                                            \
    hipLaunchKernelGGL((kb_warp_iter<6, FM, 2>), dim3(wi.w.ra.waves, n), dim3(256), 0, st, wi); \
  else                                                                                          \
    hipLaunchKernelGGL((kb_warp_iter<6, FM, 1>), dim3(wi.w.ra.waves, n), dim3(192), 0, st, wi);
  MATH_SWITCH(bl.math, KB_WITER)
#undef KB_WITER
  if (tkw) {   // k_warp_iter's accounting per pair (constants always stored), x n
    const double Nl = (double)bl.lw * bl.lh;
    int nz = 0;   // pairs whose p is zero (a level's first warp): p not loaded
    for (int b = 0; b < n; ++b) nz += sel.pzero.test(b) ? 1 : 0;
    c->prof.end(st, tkw, 0, (double)n * Nl * (64.0 * 2 + 40.0),
             batch_warp_iter_hbm(sp, bl.lh, wi_ww<6, 128>(), Nl, n, nz, nstore));
  }
  return sp.waves;
}

// k_warp_ring's streaming LDS-ring gather for the pairs of sel (a warp's gather of every pair,
// or the regather of the pairs whose fused pass did not store the constants they now need)
static void launch_batch_ring(const BatchLevel &bl, const BatchSel &sel) {
  tvl1_ctx *c = bl.c;
  hipStream_t st = bl.st;
  const int lw = bl.lw, lh = bl.lh;
  const StreamPlan sp = plan_warp_ring(lw, lh, 6, c->warp_ring_slots, 0, sel.n);
  BatchRing br{};
  br.wa.W = lw;
  br.wa.H = lh;
  br.wa.P = bl.P;
  br.wa.bands = sp.bands;
  br.wa.seg_rows = sp.seg_rows;
  br.wa.waves = sp.waves;
  br.I0 = c->bI0s[bl.s];
  br.I1 = c->bI1s[bl.s];
  set_batch_uc(c, br);
  br.ips = c->bips[bl.s];
  br.ps = bl.ps;
  br.sel = sel;
  const size_t tkr = c->prof.begin(c->profiling, st);
#define KB_RING(FM) \
  hipLaunchKernelGGL((kb_warp_ring<6, 2, FM>), dim3(br.wa.waves, sel.n), dim3(128), 0, st, br);
  MATH_SWITCH(bl.math, KB_RING)
#undef KB_RING
  c->prof.end(st, tkr, 1, (double)sel.n * lw * lh * 40.0, (double)sel.n * lw * lh * 28.0);
}

// One pass group: K iterations for the pairs of sel (kb_iterate_roll: wavefront pipelines,
// 64*PX-px bands down the whole level, one per wave).  Returns the residual partials per pair
// (pair stride c->bnblk; -1: error set).
static int launch_batch_roll(const BatchLevel &bl, int K, const BatchSel &sel) {
  tvl1_ctx *c = bl.c;
  hipStream_t st = bl.st;
  const int lw = bl.lw, lh = bl.lh, math = bl.math;
  // PX = 1 (64-px bands) on narrow levels when TVL1_BATCH_PX1_W asks for it
  const int px = lw <= c->batch_px1_w ? 1 : 2;
  // segments sized so the launch's wavefronts fill whole rounds of resident slots,
  // but never shorter than min(rows, batch_seg_min): a pass group of a few pairs (or
  // a tiny level) would otherwise be cut into short segments that repeat the 2K-row
  // halo to fill slots the other batch in flight fills anyway (r5: one segment per
  // band on the strips' <= 100-row levels, +1.7 % strip solves/s,
  // profiles/r5/ab/strips_seg/)
  const StreamPlan sp = plan_roll(lw, lh, K, px, px == 1 ? c->kb1_slots[K] : c->roll_slots[K][0][2],
                                  c->roll_seg, std::min(lh, c->batch_seg_min), sel.n);
  if (batch_partials_fit(c, sp.waves, "waves") < 0) return -1;
  BatchRoll br{};
  br.ra.b = bl.bufs;
  br.ra.it = bl.it;
  br.ra.bands = sp.bands;
  br.ra.seg_rows = sp.seg_rows;
  br.ra.waves = sp.waves;
  set_batch_upc(c, br);
  br.ps = bl.ps;
  br.partials = c->bpartials;
  br.nblk = c->bnblk;
  br.sel = sel;
  const dim3 grid((br.ra.waves + 3) / 4, sel.n);
  const size_t tkp = c->prof.begin(c->profiling, st);
#define KB_ROLL_M(FM)                                                                       \
  if (px == 1)                                                                            \
    hipLaunchKernelGGL((kb_iterate_roll<KK, 1, FM>), grid, dim3(256), 0, st, br);         \
  else                                                                                    \
    hipLaunchKernelGGL((kb_iterate_roll<KK, 2, FM>), grid, dim3(256), 0, st, br);
#define KB_ROLL(K_)                 \
  {                                 \
    constexpr int KK = K_;          \
    MATH_SWITCH(math, KB_ROLL_M)    \
  }
  switch (K) {
    case 1: KB_ROLL(1) break;
    case 2: KB_ROLL(2) break;
    case 3: KB_ROLL(3) break;
    default: KB_ROLL(4) break;
  }
#undef KB_ROLL
#undef KB_ROLL_M
  if (tkp) {   // k_iterate_roll's accounting (64*PX-px bands) per pair of the launch
    const double Nl = (double)lw * lh;
    int nz = 0;
    for (int j = 0; j < sel.n; ++j) nz += sel.pzero.test(sel.idx[j]) ? 1 : 0;
    c->prof.end(st, tkp, 0, (double)sel.n * Nl * 64.0 * K, batch_roll_hbm(sp, lh, K, px, Nl, sel.n, nz));
  }
  return sp.waves;
}

// every pair's flow of level s (its current u set) zoomed to level s-1 (the other set)
static void batch_upsample(const BatchLevel &bl, BatchSel sel) {
  tvl1_ctx *c = bl.c;
  const Geometry &g = c->geo;
  BatchUp up{};
  set_batch_u(c, up);
  up.ps = bl.ps;
  up.sw = bl.lw;
  up.sh = bl.lh;
  up.sp = bl.P;
  up.dw = g.ws[bl.s - 1];
  up.dh = g.hs[bl.s - 1];
  up.dp = g.ps[bl.s - 1];
  up.fx = (float)(1.0 / ((double)up.dw / bl.lw));
  up.fy = (float)(1.0 / ((double)up.dh / bl.lh));
  up.mul = (float)(1.0 / c->prm.scale_step);
  up.sel = sel;
  if (contracts(bl.math))
    hipLaunchKernelGGL(kb_upsample<true>, grid2(up.dw, up.dh, 2 * bl.n), kBlk2, 0, bl.st, up);
  else
    hipLaunchKernelGGL(kb_upsample<false>, grid2(up.dw, up.dh, 2 * bl.n), kBlk2, 0, bl.st, up);
}

static void batch_output(tvl1_ctx *c, int n, int W, int H, float *u, float *v, size_t fpitch,
                         size_t fstride, BatchSel sel, hipStream_t st) {
  BatchOut bo{};
  set_batch_u(c, bo);
  bo.ps = c->bps;
  bo.W = W;
  bo.H = H;
  bo.P = c->geo.ps[0];
  bo.u = u;
  bo.v = v;
  bo.fpitch = fpitch;
  bo.fstride = fstride;
  bo.sel = sel;
  hipLaunchKernelGGL(kb_output, grid2(W, H, n), kBlk2, 0, st, bo);
}

// walk_batch_level's backend (tvl1_batch_walk.hpp): the launches of one level of a chunk
struct BatchOps {
  const BatchLevel &bl;
  tvl1_stats *stats;   // per pair, or null

  // build-only median of u before a warp
  tvl1_status median(const BatchSel &sel) {
    tvl1_ctx *c = bl.c;
    BatchMedian md{};
    set_batch_u(c, md);
    md.ps = bl.ps;
    md.W = bl.lw;
    md.H = bl.lh;
    md.P = bl.P;
    md.ksize = c->prm.median_filtering;
    md.sel = sel;
    hipLaunchKernelGGL(kb_median, grid2(bl.lw, bl.lh, 2 * bl.n), kBlk2, 0, bl.st, md);
    return TVL1_OK;
  }
  tvl1_status gather(const BatchSel &sel) {
    launch_batch_ring(bl, sel);
    return TVL1_OK;
  }
  tvl1_status fused(const BatchSel &sel, int nstore, int *blocks) {
    return (*blocks = launch_batch_warp_iter(bl, sel, nstore)) < 0 ? TVL1_EHIP : TVL1_OK;
  }
  tvl1_status pass(int K, const BatchSel &sel, int *blocks) {
    return (*blocks = launch_batch_roll(bl, K, sel)) < 0 ? TVL1_EHIP : TVL1_OK;
  }
  // the fused pass packs each pair's partials (pair stride = their number); a pass leaves
  // them at the arena's pair stride
  tvl1_status reduce(const BatchSel &sel, int blocks, bool fused) {
    tvl1_ctx *c = bl.c;
    hipLaunchKernelGGL(kb_reduce, dim3(sel.n), dim3(kBlock), 0, bl.st, c->bpartials,
                       fused ? (size_t)blocks : (size_t)c->bnblk, blocks, sel, c->pinned_dev + 8);
    return TVL1_OK;
  }
  using Residuals = const double *;
  tvl1_status sync(Residuals *residuals) {
    tvl1_ctx *c = bl.c;
    HIP_TRY(c, hipEventRecord(c->ev_check[0], bl.st));
    HIP_TRY(c, hipEventSynchronize(c->ev_check[0]));
    *residuals = c->pinned + 8;
    return TVL1_OK;
  }
  void warp_done(int b, int wp, int iters) {
    const int i = bl.s * bl.c->prm.warps + wp;
    if (stats && stats[b].warp_iterations && i < stats[b].warp_iterations_capacity)
      stats[b].warp_iterations[i] = iters;
  }
};

static tvl1_status solve_batch_chunk(tvl1_ctx *c, int n, const uint8_t *I0, size_t pitch0,
                                     size_t stride0, const uint8_t *I1, size_t pitch1,
                                     size_t stride1, const Seed *seed, int W, int H, float *u,
                                     float *v, size_t fpitch, size_t fstride, tvl1_stats *stats,
                                     hipStream_t st) {
  const tvl1_params &prm = c->prm;
  const Geometry &g = c->geo;
  const int L = g.L;
  TVL1_TRY(ensure_batch(c, W, H, n, st));
  const size_t ps = c->bps;
  // counted as a solve in progress (single-pair solves speculate and size their launches
  // by this count); the batched launches themselves are sized for every resident slot (the
  // shared share measured neutral here: 2925 / 2901 against 2919 / 2928 strip solves/s,
  // profiles/r3/ab_batch_fill.txt)
  const SolveCount active(c->device);
  if (c->profiling) c->prof.reset();   // per-class HIP events of this chunk's launches (shared by its pairs)

  batch_pyramid(c, n, I0, pitch0, stride0, I1, pitch1, stride1, W, H, st);
  TVL1_TRY(batch_initial_flow(c, n, seed, W, H, st));
  HIP_TRY(c, hipGetLastError());

  BatchWalkState ws(n);   // every pair's buffer sets in use, and the walker's per-pair scratch
  BatchWalkCounts ct(n);
  std::vector<int64_t> level_iters((size_t)n * TVL1_MAX_LEVELS, 0);
  std::vector<int> hw;
  for (int s = L - 1; s >= 0; --s) {
    const int lw = g.ws[s], lh = g.hs[s], P = g.ps[s];
    const double scaledEps = prm.epsilon * prm.epsilon * (double)lw * (double)lh;
    BatchLevel bl{};
    bl.c = c;
    bl.st = st;
    bl.n = n;
    bl.s = s;
    bl.lw = lw;
    bl.lh = lh;
    bl.P = P;
    bl.math = math_of(prm);
    bl.ps = ps;
    {
      const size_t bstride = (size_t)(c->bC[1] - c->bC[0]) * sizeof(float);
      const size_t lvl = (size_t)P * lh * sizeof(float);
      bl.bufs.pstride = (unsigned)bstride;
      bl.bufs.cb = (unsigned)(2 * bstride + lvl);
      bl.bufs.ub = (unsigned)(bstride + lvl);
      bl.bufs.pb = (unsigned)(3 * bstride + lvl);
    }
    bl.it = iter_args(prm, lw, lh, P, nullptr);   // (each pair's partials are set on the device)
    bl.it.gamma = 0.0f;                           // the batched kernels are the gamma = 0 ones
    BatchOps ops{bl, stats};
    // the coarsest level runs on chip when it fits one workgroup's registers and LDS (p is
    // reset at every level anyway)
    const bool small = c->batch_small && s == L - 1 && prm.median_filtering <= 1 &&
                       lw <= 64 * kSmallWaves && lh <= kSmallR && lw * lh <= kSmallPx;
    if (small) {
      TVL1_TRY(batch_small_level(bl, ws.all, seed != nullptr, scaledEps, hw));
      for (int b = 0; b < n; ++b) {
        ct.level_iters[b] = 0;
        for (int wp = 0; wp < prm.warps; ++wp) {
          ops.warp_done(b, wp, hw[(size_t)b * prm.warps + wp]);
          ct.level_iters[b] += hw[(size_t)b * prm.warps + wp];
        }
        ct.checks[b] += hw[(size_t)n * prm.warps + b];
      }
    } else {
      BatchWalkLevel wl{};
      wl.n = n;
      wl.warps = prm.warps;
      wl.iterations = prm.iterations;
      wl.kmax = kTbMax;
      wl.scaledEps = scaledEps;
      wl.eps_pos = prm.epsilon > 0;
      // warpBackward fused with the warp's first pass, which is 2 iterations ending in the
      // first check for every pair (procOneScale with epsilon > 0, iterations >= 2)
      wl.fuse = c->batch_fuse && prm.epsilon > 0 && prm.iterations >= 2;
      wl.median = prm.median_filtering > 1;
      // r4: pairs grouped by their pass length, one launch per group, so every pair runs
      // its whole pass.  TVL1_BATCH_GROUP=0 keeps r3's lock step
      wl.group = c->batch_group != 0;
      wl.store_pred = c->batch_store_pred != 0;
      TVL1_TRY(walk_batch_level(ops, wl, ws, ct));
    }
    for (int b = 0; b < n; ++b) level_iters[(size_t)b * TVL1_MAX_LEVELS + s] = ct.level_iters[b];
    HIP_TRY(c, hipGetLastError());
    if (s == 0) break;
    batch_upsample(bl, ws.current());
    ws.flip_u();
  }
  batch_output(c, n, W, H, u, v, fpitch, fstride, ws.current(), st);
  HIP_TRY(c, hipGetLastError());
  if (stats)
    for (int b = 0; b < n; ++b)   // misses: constants not stored, then needed (re-gathered)
      fill_stats(&stats[b], g, prm.warps, &level_iters[(size_t)b * TVL1_MAX_LEVELS], ct.checks[b],
                 (int32_t)ct.regathers[b]);
  // with tvl1_set_profiling: every pair of the chunk reports the chunk's launches (each
  // launch serves all its pairs; bytes are summed over them)
  ClassTotals tot;
  TVL1_TRY(sum_marks(c, tot));
  if (stats && c->profiling && !c->prof.marks.empty())
    for (int b = 0; b < n; ++b) put_class_totals(&stats[b], tot);
  return TVL1_OK;
}


// ---------------------------------------------------------------- feature pre-alignment
// find_alignment (features.cpp:46-167) on the GPU + host (tvl1_align.hpp).
namespace {
struct OrbSet {
  std::vector<OrbKp> kps;     // level coordinates (angle filled when asked, orb_detect)
  std::vector<Pt> pts;        // level-0 coordinates
  std::vector<float> resp;    // Harris responses
  uint32_t *desc = nullptr;   // device, 8 words per keypoint (in the ctx's align scratch)
};

// The pyramid geometry, the quotas and the scratch layout are planned in
// tvl1_align_plan.hpp (HIP-free); here the layout's offsets become pointers.
static OrbGeom orb_geom(int W, int H, const tvl1_align_params &ap) {
  return tvl1k::orb_geom(W, H, ap.nfeatures, ap.scale_factor, ap.nlevels, ap.first_level);
}

struct AlignPtrs {
  float *lev = nullptr, *blur = nullptr, *score = nullptr;
  uint64_t *keys = nullptr, *sel = nullptr;
  unsigned *cnt = nullptr, *nsel = nullptr;
  SelLevel *lv = nullptr;
  float **dlev = nullptr;
  int *dlp = nullptr;
  OrbKp *kps = nullptr;
  uint32_t *desc[2] = {nullptr, nullptr};
  int2 *best = nullptr, *dist = nullptr;
  Top2 *part = nullptr;
};
static_assert(sizeof(int2) == 2 * sizeof(int32_t), "int2 layout");

static AlignPtrs align_ptrs(char *base, const AlignCarve &a) {
  AlignPtrs cv;
  cv.kps = (OrbKp *)(base + a.kps);
  cv.desc[0] = (uint32_t *)(base + a.desc[0]);
  cv.desc[1] = (uint32_t *)(base + a.desc[1]);
  cv.best = (int2 *)(base + a.best);
  cv.dist = (int2 *)(base + a.dist);
  cv.part = (Top2 *)(base + a.part);
  cv.lev = (float *)(base + a.lev);
  cv.blur = a.blur != AlignCarve::kNone ? (float *)(base + a.blur) : nullptr;
  cv.score = (float *)(base + a.score);
  cv.keys = (uint64_t *)(base + a.keys);
  cv.cnt = (unsigned *)(base + a.cnt);
  cv.sel = (uint64_t *)(base + a.sel);
  cv.nsel = (unsigned *)(base + a.nsel);
  cv.lv = (SelLevel *)(base + a.lv);
  cv.dlev = (float **)(base + a.dlev);
  cv.dlp = (int *)(base + a.dlp);
  return cv;
}

// ORB detect + describe of one frame (cv::cuda::ORB::detectAndCompute, features.cpp:60-61)
// into out; descriptors go to desc.  All levels are queued back to back: one host sync for
// the selected keys, one for the descriptors.
static tvl1_status orb_detect(tvl1_ctx *c, const uint8_t *img, size_t pitch, const OrbGeom &g,
                              const tvl1_align_params &ap, const AlignPtrs &cv, uint32_t *desc,
                              OrbSet &out, hipStream_t st, bool angles = false) {
  const int L = g.L, W = g.w[0], H = g.h[0];
  std::vector<float *> lev(L);
  {
    size_t o = 0;
    for (int l = 0; l < L; ++l) {
      lev[l] = cv.lev + o;
      o += align_up((size_t)g.p[l] * g.h[l], 64);
    }
  }
  hipLaunchKernelGGL(k_convert_u8, grid2(W, H, 1), kBlk2, 0, st, img, pitch, img, pitch, lev[0],
                     lev[0], W, H, g.p[0]);
  for (int l = 1; l < L; ++l)
    hipLaunchKernelGGL(k_resize_hp, grid2(g.w[l], g.h[l], 1), kBlk2, 0, st, lev[l - 1], nullptr,
                       nullptr, g.w[l - 1], g.h[l - 1], g.p[l - 1], lev[l], nullptr, nullptr,
                       g.w[l], g.h[l], g.p[l], (double)g.w[l - 1] / g.w[l],
                       (double)g.h[l - 1] / g.h[l], 0, 0, 1.0f);
  const int border = orb_border(ap.edge_threshold);
  std::vector<SelLevel> lv(L);
  HIP_TRY(c, hipMemsetAsync(cv.cnt, 0, L * sizeof(unsigned), st));
  for (int l = 0; l < L; ++l) {
    lv[l] = SelLevel{g.off[l], g.cap[l], (unsigned)g.quota[l]};
    if (orb_level_skipped(g, l, border)) {
      lv[l].quota = 0;
      lv[l].cap = 0;
      continue;
    }
    hipLaunchKernelGGL(ka_fast_harris, dim3((g.w[l] + kFhW - 1) / kFhW, (g.h[l] + kFhH - 1) / kFhH),
                       dim3(256), 0, st, lev[l], g.w[l], g.h[l], g.p[l], border,
                       (float)ap.fast_threshold, cv.score);
    hipLaunchKernelGGL(ka_nms, dim3((g.w[l] + 63) / 64, (g.h[l] + kNmsRows - 1) / kNmsRows),
                       dim3(256), 0, st, cv.score, g.w[l], g.h[l], cv.keys + g.off[l],
                       cv.cnt + l, g.cap[l]);
  }
  HIP_TRY(c, hipMemcpyAsync(cv.lv, lv.data(), L * sizeof(SelLevel), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ka_select, dim3(L), dim3(1024), 0, st, cv.keys, cv.cnt, cv.lv, cv.sel,
                     g.kmax, cv.nsel);
  std::vector<unsigned> nsel(L);
  std::vector<uint64_t> sel((size_t)L * g.kmax);
  HIP_TRY(c, hipMemcpyAsync(nsel.data(), cv.nsel, L * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(sel.data(), cv.sel, sel.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int l = 0; l < L; ++l) {
    const unsigned n = std::min(nsel[l], (unsigned)g.quota[l]);
    uint64_t *k = sel.data() + (size_t)l * g.kmax;
    std::sort(k, k + n, [](uint64_t a, uint64_t b) { return a > b; });   // best first
    const double scale = std::pow(ap.scale_factor, l - ap.first_level);
    for (unsigned i = 0; i < n; ++i) {
      const unsigned pos = 0xFFFFFFFFu - (unsigned)(k[i] & 0xFFFFFFFFu);
      const float x = (float)(pos % (unsigned)g.w[l]), y = (float)(pos / (unsigned)g.w[l]);
      out.kps.push_back(OrbKp{x, y, 0.0f, l});
      out.pts.push_back(Pt{x * scale, y * scale});
      const uint32_t rb = (uint32_t)(k[i] >> 32);   // the key's score bits
      float rf;
      memcpy(&rf, &rb, sizeof rf);
      out.resp.push_back(rf);
    }
  }
  if (ap.blur_for_descriptor) {
    size_t o = 0;
    for (int l = 0; l < L; ++l) {
      float *b = cv.blur + o;
      o += align_up((size_t)g.p[l] * g.h[l], 64);
      hipLaunchKernelGGL(ka_blur7, grid2(g.w[l], g.h[l]), kBlk2, 0, st, lev[l], g.w[l], g.h[l],
                         g.p[l], b);
      lev[l] = b;
    }
  }
  const int nk = (int)out.kps.size();
  out.desc = desc;
  if (nk > 0) {
    HIP_TRY(c, hipMemcpyAsync(cv.kps, out.kps.data(), nk * sizeof(OrbKp), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(cv.dlev, lev.data(), L * sizeof(float *), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(cv.dlp, g.p.data(), L * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ka_describe, dim3((nk + 63) / 64), dim3(64), 0, st,
                       (const float *const *)cv.dlev, cv.dlp, cv.kps, nk, c->align_pat, desc);
    HIP_TRY(c, hipGetLastError());
    if (angles)
      HIP_TRY(c, hipMemcpyAsync(out.kps.data(), cv.kps, nk * sizeof(OrbKp), hipMemcpyDeviceToHost, st));
    // the host vectors above are the copy sources: they must outlive the copies
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  return TVL1_OK;
}

// the rBRIEF pair pattern on the device (set once per ctx)
static tvl1_status ensure_pattern(tvl1_ctx *c) {
  if (c->align_pat) return TVL1_OK;
  static const std::vector<int> pat = orb_pattern();
  HIP_TRY(c, hipMalloc((void **)&c->align_pat, pat.size() * sizeof(int)));
  HIP_TRY(c, hipMemcpy(c->align_pat, pat.data(), pat.size() * sizeof(int), hipMemcpyHostToDevice));
  return TVL1_OK;
}

static tvl1_status check_orb_params(tvl1_ctx *c, const tvl1_align_params *ap) {
  if (ap->nlevels <= 0 || !(ap->scale_factor > 1.0f) || ap->nfeatures <= 0)
    return set_err(c, TVL1_EINVAL, "bad ORB parameters");
  if (ap->wta_k != 2 || ap->patch_size != 31)
    return set_err(c, TVL1_EINVAL, "only WTA_K = 2 and patchSize = 31 are supported");
  return TVL1_OK;
}

static void affine_inverse(const float M[6], Affine &iM) {
  const double a = M[0], b = M[1], cc = M[2], d = M[3], e = M[4], f = M[5];
  double D = a * e - b * d;
  D = D != 0 ? 1.0 / D : 0.0;
  const double A11 = e * D, A22 = a * D, A12 = -b * D, A21 = -d * D;
  iM.m[0] = (float)A11;
  iM.m[1] = (float)A12;
  iM.m[2] = (float)(-A11 * cc - A12 * f);
  iM.m[3] = (float)A21;
  iM.m[4] = (float)A22;
  iM.m[5] = (float)(-A21 * cc - A22 * f);
}
}  // namespace

extern "C" {

void tvl1_params_default(tvl1_params *p) {
  if (!p) return;
  // generate_TV_args, optflow.cpp:503-512
  p->tau = 0.25;
  p->lambda = 0.05;
  p->theta = 0.3;
  p->nscales = 10;
  p->warps = 5;
  p->epsilon = 0.01;
  p->iterations = 300;
  p->scale_step = 0.8;
  p->gamma = 0.0;
  p->use_initial_flow = 0;
  p->median_filtering = 1;
  p->fast_math = 0;
  p->profile = 0;
  p->inner_iterations = 30;   // cv::DualTVL1OpticalFlow defaults (profile 1)
  p->outer_iterations = 10;
}

int32_t tvl1_abi_version(void) { return TVL1_ABI_VERSION; }

int32_t tvl1_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

tvl1_status tvl1_create(tvl1_ctx **out, int device, const tvl1_params *params) {
  if (!out) return set_err(nullptr, TVL1_EINVAL, "out is NULL");
  *out = nullptr;
  tvl1_status s = check_params(nullptr, params);
  if (s != TVL1_OK) return s;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return set_err(nullptr, TVL1_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n)
    return set_err(nullptr, TVL1_ENODEV, "device %d out of range (have %d)", device, n);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return set_err(nullptr, TVL1_ENODEV, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(nullptr, TVL1_ENODEV, "device %d is %s; this build targets gfx950 only",
                   device, prop.gcnArchName);
  tvl1_ctx *c = new (std::nothrow) tvl1_ctx();
  if (!c) return set_err(nullptr, TVL1_ENOMEM, "out of host memory");
  c->device = device;
  c->prm = *params;
  // test / diagnostic knobs (tests/test_gpu_parity.py names what each one reaches)
  if (const char *m = getenv("TVL1_ROLL_SEG")) c->roll_seg = atoi(m);
  if (const char *m = getenv("TVL1_ROLL_PX4_MIN")) c->roll_px4_min = atol(m);
  if (const char *m = getenv("TVL1_FUSE")) c->fuse = atoi(m) != 0;
  if (const char *m = getenv("TVL1_MID")) c->mid = atoi(m) != 0;
  if (const char *m = getenv("TVL1_MID_MIN")) c->mid_min = atof(m);
  if (const char *m = getenv("TVL1_WI_NC")) c->wi_nc = atoi(m) == 1 ? 1 : 2;
  if (const char *m = getenv("TVL1_TB4")) c->tb4 = atoi(m) != 0;
  if (const char *m = getenv("TVL1_INVERT_WINDOW")) c->invert_window = atoi(m) != 0;
  if (const char *m = getenv("TVL1_STAGES")) c->stages = std::min(std::max(atoi(m), 0), 2);
  if (const char *m = getenv("TVL1_STAGES_FILL")) c->stages_fill = std::max(0, atoi(m));
  if (const char *m = getenv("TVL1_POLL")) c->poll = atoi(m);
  if (const char *m = getenv("TVL1_SPEC")) c->spec = atoi(m);
  if (const char *m = getenv("TVL1_SPEC_TRACE")) c->spec_trace = atoi(m);
  if (const char *m = getenv("TVL1_FUSE_MIN")) c->fuse_min = atol(m);
  if (const char *m = getenv("TVL1_BATCH_FUSE")) c->batch_fuse = atoi(m) != 0;
  if (const char *m = getenv("TVL1_BATCH_STORE")) c->batch_store_pred = atoi(m) == 0;
  if (const char *m = getenv("TVL1_BATCH_GROUP")) c->batch_group = atoi(m) != 0;
  if (const char *m = getenv("TVL1_BATCH_PX1_W")) c->batch_px1_w = atoi(m);
  if (const char *m = getenv("TVL1_BATCH_SEG_MIN")) c->batch_seg_min = atoi(m);
  if (const char *m = getenv("TVL1_BATCH_SMALL")) c->batch_small = atoi(m) != 0;
  if (const char *m = getenv("TVL1_PROBE_ROLL_LDS")) c->probe_lds = atoi(m);
  if (const char *m = getenv("TVL1_PROBE_WI_LDS")) c->probe_wi_lds = std::min(atoi(m), 32768);
  if (const char *m = getenv("TVL1_BUF_LIMIT"))   // force the 64-bit-addressed kernels
    c->buf_limit = std::min(c->buf_limit, (size_t)std::max(0LL, atoll(m)));
  if (const char *m = getenv("TVL1_CHECK")) c->check = atoi(m);
  if (const char *m = getenv("TVL1_FILL")) c->fill = std::max(10, atoi(m));
  if (const char *m = getenv("TVL1_FILL_SHARED")) c->fill_shared = std::max(10, atoi(m));
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->mem.own, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc((void **)&c->pinned, sizeof(double) * (8 + kBatchMax),
                    hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void **)&c->pinned_dev, c->pinned, 0) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_check[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_check[1], hipEventDisableTiming) != hipSuccess ||
      hipMalloc((void **)&c->gate, 256) != hipSuccess ||
      hipMemset(c->gate, 0, 256) != hipSuccess ||
      !c->mem.init()) {
    delete c;
    return set_err(nullptr, TVL1_EHIP, "HIP initialisation failed on device %d", device);
  }
  // hipHostMalloc does not promise zeroed memory: a stale sequence word >= the first check's
  // would let the residual poll return before k_reduce wrote
  memset(c->pinned, 0, sizeof(double) * (8 + kBatchMax));
  // resident wavefronts / blocks of the streaming kernels, for their segment sizing
  {
    auto blocks_of = [&](const void *fn, int threads) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, 0) != hipSuccess) nb = 0;
      return nb * prop.multiProcessorCount;
    };
#define ROLL_SLOTS(G, K, PX) \
  c->roll_slots[K][G][PX] = 4 * blocks_of((const void *)k_iterate_roll<G, K, PX>, 256);
    ROLL_SLOTS(false, 1, 2) ROLL_SLOTS(false, 2, 2) ROLL_SLOTS(false, 3, 2) ROLL_SLOTS(false, 4, 2)
    ROLL_SLOTS(true, 1, 2) ROLL_SLOTS(true, 2, 2) ROLL_SLOTS(true, 3, 2) ROLL_SLOTS(true, 4, 2)
    ROLL_SLOTS(false, 1, 4) ROLL_SLOTS(false, 2, 4) ROLL_SLOTS(true, 1, 4) ROLL_SLOTS(true, 2, 4)
#undef ROLL_SLOTS
    c->mid_slots = 4 * blocks_of((const void *)k_iterate_roll_mid<kIEEE>, 256);
    c->kb1_slots[1] = 4 * blocks_of((const void *)kb_iterate_roll<1, 1, kIEEE>, 256);
    c->kb1_slots[2] = 4 * blocks_of((const void *)kb_iterate_roll<2, 1, kIEEE>, 256);
    c->kb1_slots[3] = 4 * blocks_of((const void *)kb_iterate_roll<3, 1, kIEEE>, 256);
    c->kb1_slots[4] = 4 * blocks_of((const void *)kb_iterate_roll<4, 1, kIEEE>, 256);
    c->stage_slots[2] = blocks_of((const void *)k_iterate_stages<kIEEE, 2>, 128);
    c->stage_slots[4] = blocks_of((const void *)k_iterate_stages<kIEEE, 4>, 256);
    c->warp_ring_slots = blocks_of((const void *)k_warp_ring<6, 2>, 128);
    c->witer_slots = c->wi_nc == 2 ? blocks_of((const void *)k_warp_iter<kWiMargin, 0, 128, 1, 2>, 256)
                                   : blocks_of((const void *)k_warp_iter<kWiMargin, 0, 128, 1, 1>, 192);
    if (c->probe_wi_lds > 0 && c->wi_nc == 2) {   // the probe's segments fill its own residency
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_warp_iter<kWiMargin, 0, 128, 1, 2>,
                                                       256, c->probe_wi_lds) == hipSuccess && nb > 0)
        c->witer_slots = nb * prop.multiProcessorCount;
      (void)hipGetLastError();
    }
    // >= 3-iteration passes stream when the level has at least 4 wavefronts' worth of 56 x 32
    // tiles per SIMD (the measured crossover against 64 x 32 blocked regions)
    c->roll_long_min = 16L * prop.multiProcessorCount;
    if (const char *m = getenv("TVL1_ROLL_LONG_MIN")) c->roll_long_min = atol(m);   // tests
    (void)hipGetLastError();
  }
  *out = c;
  return TVL1_OK;
}

tvl1_status tvl1_set_params(tvl1_ctx *c, const tvl1_params *params) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  tvl1_status s = check_params(c, params);
  if (s != TVL1_OK) return s;
  c->prm = *params;
  c->geo_valid = false;  // pyramid depth may change
  return TVL1_OK;
}

static tvl1_status check_call(tvl1_ctx *c, const void *I0, size_t p0, const void *I1, size_t p1,
                              int W, int H, const void *u, const void *v, size_t fp) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!I0 || !I1 || !u || !v) return set_err(c, TVL1_EINVAL, "null image or flow pointer");
  if (W <= 0 || H <= 0) return set_err(c, TVL1_ESIZE, "bad size %dx%d", W, H);
  if ((size_t)W * (size_t)H > (size_t)1 << 31)
    return set_err(c, TVL1_ESIZE, "image %dx%d too large", W, H);
  if (p0 < (size_t)W || p1 < (size_t)W) return set_err(c, TVL1_EINVAL, "input pitch < width");
  if (fp < sizeof(float) * (size_t)W || fp % sizeof(float))
    return set_err(c, TVL1_EINVAL, "flow pitch must be >= 4*width and a multiple of 4");
  return TVL1_OK;
}

tvl1_status tvl1_calc(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                      size_t pitch1, int32_t W, int32_t H, float *u, float *v, size_t fpitch,
                      tvl1_stats *stats, void *stream) {
  tvl1_status s = check_call(c, I0, pitch0, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  HIP_TRY(c, hipSetDevice(c->device));
  s = ensure_geometry(c, W, H, (hipStream_t)stream);
  if (s != TVL1_OK) return s;
  return solve(c, Frames{I0, I1, pitch0, pitch1, false}, nullptr, W, H, u, v, fpitch, stats,
               (hipStream_t)stream);
}

// The seed arguments of the tvl1_calc_*_init calls, checked before anything is launched
// (and before the ctx: a NULL ctx reports the error through tvl1_last_error(NULL)).
static tvl1_status check_seed(tvl1_ctx *c, const float *u0, const float *v0, size_t ipitch,
                              int W) {
  if (!u0 || !v0) return set_err(c, TVL1_EINVAL, "null initial flow pointer");
  if (W > 0 && (ipitch < sizeof(float) * (size_t)W || ipitch % sizeof(float) ||
                ipitch / sizeof(float) > (size_t)INT32_MAX))
    return set_err(c, TVL1_EINVAL, "initial flow pitch must be >= 4*width and a multiple of 4");
  if (c && c->prm.profile == 1)
    return set_err(c, TVL1_EINVAL, "profile 1 takes no initial flow (tvl1_calc_init)");
  return TVL1_OK;
}

tvl1_status tvl1_calc_init(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                           size_t pitch1, int32_t W, int32_t H, const float *u0, const float *v0,
                           size_t init_pitch, float *u, float *v, size_t fpitch,
                           tvl1_stats *stats, void *stream) {
  tvl1_status s = check_seed(c, u0, v0, init_pitch, W);
  if (s != TVL1_OK) return s;
  s = check_call(c, I0, pitch0, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  HIP_TRY(c, hipSetDevice(c->device));
  s = ensure_geometry(c, W, H, (hipStream_t)stream);
  if (s != TVL1_OK) return s;
  const Seed seed{u0, v0, init_pitch / sizeof(float), 0, nullptr};
  return solve(c, Frames{I0, I1, pitch0, pitch1, false}, &seed, W, H, u, v, fpitch, stats,
               (hipStream_t)stream);
}

tvl1_status tvl1_find_homography(const float *src_xy, const float *dst_xy, int32_t n,
                                 int32_t method, double thresh, double H[9], uint8_t *mask) {
  if (!src_xy || !dst_xy || !H || n < 4 || !(method == 0 || method == 4 || method == 8))
    return set_err(nullptr, TVL1_EINVAL, "find_homography: need n >= 4 points and method 0, 4 or 8");
  std::vector<Pt> a(n), b(n);
  for (int i = 0; i < n; ++i) {
    a[i] = Pt{src_xy[2 * i], src_xy[2 * i + 1]};
    b[i] = Pt{dst_xy[2 * i], dst_xy[2 * i + 1]};
  }
  if (method == 0) {   // all points: the least-squares fit, then the LM refinement
    if (!dlt_homography(a, b, H))
      return set_err(nullptr, TVL1_ESIZE, "find_homography: degenerate points");
    lm_refine(a, b, H, 10);
    if (mask) std::fill(mask, mask + n, (uint8_t)1);
    return TVL1_OK;
  }
  if (!find_homography(a, b, method, thresh, H, mask))
    return set_err(nullptr, TVL1_ESIZE, "find_homography: no model found");
  return TVL1_OK;
}

tvl1_status tvl1_calc_f32(tvl1_ctx *c, const float *I0, size_t pitch0, const float *I1,
                          size_t pitch1, int32_t W, int32_t H, float *u, float *v, size_t fpitch,
                          tvl1_stats *stats, void *stream) {
  tvl1_status s = check_call(c, I0, pitch0, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  if (pitch0 < sizeof(float) * (size_t)W || pitch1 < sizeof(float) * (size_t)W ||
      pitch0 % sizeof(float) || pitch1 % sizeof(float))
    return set_err(c, TVL1_EINVAL, "f32 input pitch must be >= 4*width and a multiple of 4");
  HIP_TRY(c, hipSetDevice(c->device));
  s = ensure_geometry(c, W, H, (hipStream_t)stream);
  if (s != TVL1_OK) return s;
  return solve(c, Frames{I0, I1, pitch0, pitch1, true}, nullptr, W, H, u, v, fpitch, stats,
               (hipStream_t)stream);
}


// The arguments of the tvl1_calc_batch* calls, checked before anything is launched
static tvl1_status check_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                               size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                               size_t pair_stride1, int32_t W, int32_t H, float *u, float *v,
                               size_t fpitch, size_t flow_pair_stride) {
  if (n <= 0) return set_err(c, TVL1_EINVAL, "batch size must be > 0 (got %d)", n);
  tvl1_status s = check_call(c, I0, pitch0, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  // an input stride of 0 gives every pair the same frame (e.g. one reference slice)
  if (n > 1 && ((pair_stride0 != 0 && pair_stride0 < pitch0 * (size_t)H) ||
                (pair_stride1 != 0 && pair_stride1 < pitch1 * (size_t)H) ||
                flow_pair_stride < fpitch * (size_t)H))
    return set_err(c, TVL1_EINVAL, "pair strides must be 0 or cover one image; the flow stride one field");
  return TVL1_OK;
}

// The most pairs the batched kernels take in one chunk of the ctx's geometry (ensure_geometry
// ran), or 0: the pairs are solved one by one
static int batch_chunk_max(const tvl1_ctx *c, int H) {
  const tvl1_params &prm = c->prm;
  const float taut = (float)(prm.tau / prm.theta);
  // the batched kernels cover the reference's path with gamma = 0 (every production
  // config); other parameter sets solve the pairs one by one, same results
  if (!(prm.profile == 0 && prm.gamma == 0.0 && taut >= 0.0f && taut <= FLT_MAX)) return 0;
  // the batched passes address the 4 p planes of every pair of a chunk through one buffer
  // descriptor (RollBufs): that group must stay below 2 GiB
  const double pplane = (double)align_up((size_t)c->geo.ps[0] * H, 64) * sizeof(float);
  const int nmax = (int)((double)(((size_t)1 << 31) - 8192) / (4.0 * pplane));
  // (nmax < 1: frames this large solve one by one, tvl1_calc's fallbacks)
  return std::min(kBatchMax, std::max(nmax, 0));
}

// tvl1_calc_batch (seed null) and tvl1_calc_batch_init (seed of pair 0, stride to the next)
static tvl1_status calc_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                              size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                              size_t pair_stride1, const Seed *seed, int32_t W, int32_t H,
                              float *u, float *v, size_t fpitch, size_t flow_pair_stride,
                              tvl1_stats *stats, void *stream) {
  tvl1_status s = check_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W, H, u, v,
                              fpitch, flow_pair_stride);
  if (s != TVL1_OK) return s;
  HIP_TRY(c, hipSetDevice(c->device));
  s = ensure_geometry(c, W, H, (hipStream_t)stream);
  if (s != TVL1_OK) return s;
  // chunk size: kBatchMax pairs, fewer when their batch arena would not fit in half of
  // the device memory free now (large frames: one chunk of 256 6144x4096 pairs is 0.7 TB)
  int chunk = batch_chunk_max(c, H);
  const bool batched = chunk > 0;
  if (batched) {
    const Geometry &g = c->geo;
    double per_pair = 15.0 * align_up((size_t)g.ps[0] * H, 64) * sizeof(float);
    for (int l = 0; l < g.L; ++l) per_pair += 2.0 * (double)g.ps[l] * g.hs[l] * sizeof(float);
    per_pair += (((W + 55) / 56) * ((H + 23) / 24) + 64) * sizeof(double);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
      const double avail = 0.5 * (double)free_b + (double)c->barena.bytes;
      chunk = (int)std::max(1.0, std::min((double)chunk, avail / per_pair));
    }
  }
  // other contexts on the device may take memory between hipMemGetInfo and the arena's
  // hipMalloc: a chunk whose arena does not fit is retried at half the size
  for (int b0 = 0; b0 < n;) {
    const int m = batched ? std::min(chunk, n - b0) : 1;
    const uint8_t *i0 = I0 + (size_t)b0 * pair_stride0, *i1 = I1 + (size_t)b0 * pair_stride1;
    float *ub = reinterpret_cast<float *>(reinterpret_cast<char *>(u) + (size_t)b0 * flow_pair_stride);
    float *vb = reinterpret_cast<float *>(reinterpret_cast<char *>(v) + (size_t)b0 * flow_pair_stride);
    Seed sb{};
    if (seed && seed->cst) {
      // constants: the chunk's first pair's; a pair solved alone takes the two planes behind
      // the constants (calc_batch_const), filled here, as tvl1_calc_init's seed
      sb = Seed{nullptr, nullptr, 0, 0, seed->cst + 2 * (size_t)b0};
      if (!batched) {
        hipLaunchKernelGGL(kb_flow_fill, grid2(W, H, 2), kBlk2, 0, (hipStream_t)stream, sb.cst,
                           const_cast<float *>(seed->u0), const_cast<float *>(seed->v0), W, H, W,
                           (size_t)0);
        sb = Seed{seed->u0, seed->v0, (size_t)W, 0, nullptr};
      }
    } else if (seed) {
      sb = Seed{seed->u0 + (size_t)b0 * seed->stride, seed->v0 + (size_t)b0 * seed->stride,
                seed->pitch, seed->stride, nullptr};
    }
    const Seed *sd = seed ? &sb : nullptr;
    s = batched ? solve_batch_chunk(c, m, i0, pitch0, pair_stride0, i1, pitch1, pair_stride1, sd, W,
                                    H, ub, vb, fpitch, flow_pair_stride, stats ? stats + b0 : nullptr,
                                    (hipStream_t)stream)
                : solve(c, Frames{i0, i1, pitch0, pitch1, false}, sd, W, H, ub, vb, fpitch,
                        stats ? stats + b0 : nullptr, (hipStream_t)stream);
    if (s == TVL1_ENOMEM && batched && m > 1) {
      chunk = m / 2;
      continue;
    }
    if (s != TVL1_OK) return s;
    b0 += m;
  }
  return TVL1_OK;
}

tvl1_status tvl1_calc_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                            size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                            size_t pair_stride1, int32_t W, int32_t H, float *u, float *v,
                            size_t fpitch, size_t flow_pair_stride, tvl1_stats *stats,
                            void *stream) {
  return calc_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, nullptr, W, H, u, v,
                    fpitch, flow_pair_stride, stats, stream);
}

tvl1_status tvl1_calc_batch_init(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                                 size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                                 size_t pair_stride1, int32_t W, int32_t H, const float *u0,
                                 const float *v0, size_t init_pitch, size_t init_pair_stride,
                                 float *u, float *v, size_t fpitch, size_t flow_pair_stride,
                                 tvl1_stats *stats, void *stream) {
  tvl1_status s = check_seed(c, u0, v0, init_pitch, W);
  if (s != TVL1_OK) return s;
  if (init_pair_stride % sizeof(float) ||
      (n > 1 && H > 0 && init_pair_stride != 0 && init_pair_stride < init_pitch * (size_t)H))
    return set_err(c, TVL1_EINVAL, "initial flow pair stride must be 0 or cover one field, in whole floats");
  const Seed seed{u0, v0, init_pitch / sizeof(float), init_pair_stride / sizeof(float), nullptr};
  return calc_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, &seed, W, H, u, v,
                    fpitch, flow_pair_stride, stats, stream);
}


void tvl1_align_params_default(tvl1_align_params *p) {
  if (!p) return;
  // orb_defaults (features.cpp:19-31), the ratio test (:109), findHomography (:133)
  p->nfeatures = 5000;
  p->scale_factor = 1.2f;
  p->nlevels = 8;
  p->edge_threshold = 31;
  p->first_level = 0;
  p->wta_k = 2;
  p->patch_size = 31;
  p->fast_threshold = 20;
  p->blur_for_descriptor = 0;
  p->ratio = 0.8f;
  p->method = 8;   // cv::RANSAC
  p->ransac_threshold = 5.0;
}

tvl1_status tvl1_find_alignment(tvl1_ctx *c, const uint8_t *frame1, size_t pitch1, int32_t w1,
                                int32_t h1, const uint8_t *frame0, size_t pitch0, int32_t w0,
                                int32_t h0, const tvl1_align_params *ap, float affine[6],
                                int32_t *n_good, int32_t *outcome, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!frame1 || !frame0 || !ap || !affine) return set_err(c, TVL1_EINVAL, "null argument");
  if (w1 <= 0 || h1 <= 0 || w0 <= 0 || h0 <= 0) return set_err(c, TVL1_ESIZE, "bad frame size");
  {
    const tvl1_status r = check_orb_params(c, ap);
    if (r != TVL1_OK) return r;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  {
    const tvl1_status r = ensure_pattern(c);
    if (r != TVL1_OK) return r;
  }
  const OrbGeom g1 = orb_geom(w1, h1, *ap), g0 = orb_geom(w0, h0, *ap);
  const bool blur = ap->blur_for_descriptor != 0;
  // one per-keypoint capacity for both frames (the quota sum can exceed nfeatures)
  const int kcap = std::max(g1.kcap, g0.kcap);
  const AlignCarve a1 = align_carve(g1, blur, kcap), a0 = align_carve(g0, blur, kcap);
  TVL1_TRY(reserve(c, c->align_scratch, std::max(a1.bytes, a0.bytes), st));
  static const bool timing = getenv("TVL1_ALIGN_TIMING") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  // query = frame1, train = frame0 (find_alignment(frame1_GPU, frame0_GPU)); the two frames
  // share the scratch's pyramid and keys and keep their descriptors apart
  OrbSet q, t;
  const AlignPtrs cv = align_ptrs(c->align_scratch.p, a1);
  tvl1_status s = orb_detect(c, frame1, pitch1, g1, *ap, cv, cv.desc[0], q, st);
  const auto t1 = now();
  const AlignPtrs cv0 = align_ptrs(c->align_scratch.p, a0);
  if (s == TVL1_OK) s = orb_detect(c, frame0, pitch0, g0, *ap, cv0, cv0.desc[1], t, st);
  const auto t2 = now();
  if (s != TVL1_OK) return s;
  std::vector<int2> best, dist;
  const int nq = (int)q.kps.size(), nt = (int)t.kps.size();
  if (nq > 0 && nt > 0) {
    const MatchPlan mp = match_plan(nt);
    hipLaunchKernelGGL(ka_match2, dim3((nq + 63) / 64, mp.nseg), dim3(64), 0, st, q.desc, nq,
                       t.desc, nt, mp.seg, cv.part);
    hipLaunchKernelGGL(ka_match2_merge, dim3((nq + 255) / 256), dim3(256), 0, st, cv.part, nq,
                       mp.nseg, cv.best, cv.dist);
    best.resize(nq);
    dist.resize(nq);
    HIP_TRY(c, hipMemcpyAsync(best.data(), cv.best, nq * sizeof(int2), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(dist.data(), cv.dist, nq * sizeof(int2), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  const auto t3 = now();
  // the ratio test over the first min(train rows - 1, queries) queries (features.cpp:105-112)
  struct Good {
    int qi, ti, d;
  };
  std::vector<Good> good;
  for (int i = 0; i < std::min(nt - 1, nq); ++i)
    if (best[i].y >= 0 && dist[i].x < ap->ratio * dist[i].y) good.push_back(Good{i, best[i].x, dist[i].x});
  std::stable_sort(good.begin(), good.end(), [](const Good &a, const Good &b) { return a.d < b.d; });
  if (n_good) *n_good = (int32_t)good.size();
  const float ident[6] = {1, 0, 0, 0, 1, 0};
  int oc = 0;
  if (good.size() > 10) {
    std::vector<Pt> p0, p1;
    for (auto &g : good) {
      p0.push_back(q.pts[g.qi]);
      p1.push_back(t.pts[g.ti]);
    }
    double H[9];
    const bool ok = find_homography(p0, p1, ap->method, ap->ransac_threshold, H);
    if (!ok || std::fabs(1 - H[0]) > 0.20 || std::fabs(1 - H[4]) > 0.20) {
      std::copy(ident, ident + 6, affine);
      oc = 2;
    } else {
      for (int k = 0; k < 6; ++k) affine[k] = (float)H[k];
    }
  } else {
    std::copy(ident, ident + 6, affine);
    oc = 1;
  }
  if (outcome) *outcome = oc;
  if (timing)
    fprintf(stderr, "[align] detect1 %.2f ms, detect0 %.2f ms, match %.2f ms, model %.2f ms "
                    "(%d / %d keypoints, %zu good)\n",
            ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, now()), nq, nt, good.size());
  return TVL1_OK;
}

tvl1_status tvl1_orb_detect(tvl1_ctx *c, const uint8_t *frame, size_t pitch, int32_t w, int32_t h,
                            const tvl1_align_params *ap, float *kp, uint8_t *desc, int32_t cap,
                            int32_t *n, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!frame || !ap || !n || cap < 0 || (cap > 0 && (!kp || !desc)))
    return set_err(c, TVL1_EINVAL, "null argument");
  if (w <= 0 || h <= 0 || pitch < (size_t)w) return set_err(c, TVL1_ESIZE, "bad frame size");
  {
    const tvl1_status r = check_orb_params(c, ap);
    if (r != TVL1_OK) return r;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  {
    const tvl1_status r = ensure_pattern(c);
    if (r != TVL1_OK) return r;
  }
  const OrbGeom g = orb_geom(w, h, *ap);
  const bool blur = ap->blur_for_descriptor != 0;
  const AlignCarve ac = align_carve(g, blur, g.kcap);
  TVL1_TRY(reserve(c, c->align_scratch, ac.bytes, st));
  const AlignPtrs cv = align_ptrs(c->align_scratch.p, ac);
  OrbSet q;
  {
    const tvl1_status r = orb_detect(c, frame, pitch, g, *ap, cv, cv.desc[0], q, st, true);
    if (r != TVL1_OK) return r;
  }
  const int nk = (int)q.kps.size(), m = std::min(nk, cap);
  *n = nk;
  if (m > 0) {
    HIP_TRY(c, hipMemcpyAsync(desc, cv.desc[0], (size_t)m * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int i = 0; i < m; ++i) {
      float deg = q.kps[i].angle * (float)(180.0 / M_PI);   // cv::KeyPoint::angle
      if (deg < 0.f) deg += 360.f;
      if (deg >= 360.f) deg = 0.f;   // -tiny + 360 rounds to 360
      kp[5 * i + 0] = (float)q.pts[i].x;
      kp[5 * i + 1] = (float)q.pts[i].y;
      kp[5 * i + 2] = (float)q.kps[i].level;
      kp[5 * i + 3] = deg;
      kp[5 * i + 4] = q.resp[i];
    }
  }
  return TVL1_OK;
}

tvl1_status tvl1_match_knn2(tvl1_ctx *c, const uint8_t *query, int32_t nq, const uint8_t *train,
                            int32_t nt, int32_t *idx, int32_t *dist, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (nq < 0 || nt < 0 || (nq > 0 && (!query || !idx || !dist)) || (nt > 0 && !train))
    return set_err(c, TVL1_EINVAL, "bad argument");
  if (nq == 0) return TVL1_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  const MatchPlan mp = match_plan(nt);
  const int nseg = mp.nseg, seg = mp.seg;
  // scratch: query and train descriptors, the per-segment top-2, the merged top-2
  const size_t oq = 0, ot = align_up((size_t)nq * 32, 256);
  const size_t op = ot + align_up((size_t)std::max(nt, 1) * 32, 256);
  const size_t ob = op + align_up((size_t)nq * nseg * sizeof(Top2), 256);
  const size_t od = ob + align_up((size_t)nq * sizeof(int2), 256);
  const size_t need = od + align_up((size_t)nq * sizeof(int2), 256);
  TVL1_TRY(reserve(c, c->align_scratch, need, st));
  char *b = c->align_scratch.p;
  uint32_t *dq = (uint32_t *)(b + oq), *dt = (uint32_t *)(b + ot);
  Top2 *part = (Top2 *)(b + op);
  int2 *best = (int2 *)(b + ob), *dd = (int2 *)(b + od);
  HIP_TRY(c, hipMemcpyAsync(dq, query, (size_t)nq * 32, hipMemcpyHostToDevice, st));
  if (nt > 0) HIP_TRY(c, hipMemcpyAsync(dt, train, (size_t)nt * 32, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ka_match2, dim3((nq + 63) / 64, nseg), dim3(64), 0, st, dq, nq, dt, nt, seg, part);
  hipLaunchKernelGGL(ka_match2_merge, dim3((nq + 255) / 256), dim3(256), 0, st, part, nq, nseg, best, dd);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(idx, best, (size_t)nq * sizeof(int2), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(dist, dd, (size_t)nq * sizeof(int2), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}

tvl1_status tvl1_warp_affine_u8(tvl1_ctx *c, const uint8_t *src, size_t sp, int32_t sw, int32_t sh,
                                uint8_t *dst, size_t dp, int32_t dw, int32_t dh,
                                const float affine[6], void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!src || !dst || !affine) return set_err(c, TVL1_EINVAL, "null argument");
  if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0) return set_err(c, TVL1_ESIZE, "bad size");
  HIP_TRY(c, hipSetDevice(c->device));
  Affine iM;
  affine_inverse(affine, iM);
  hipLaunchKernelGGL(ka_warp_u8, grid2(dw, dh), kBlk2, 0, (hipStream_t)stream, src, sp, sw, sh,
                     dst, dp, dw, dh, iM);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

tvl1_status tvl1_postprocess_affine(tvl1_ctx *c, float *u, float *v, size_t fp, const uint8_t *I1,
                                    size_t p1, int32_t W, int32_t H, int32_t flow_output,
                                    const float affine[6], void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!u || !v || !I1 || !affine) return set_err(c, TVL1_EINVAL, "null argument");
  if (W <= 0 || H <= 0) return set_err(c, TVL1_ESIZE, "bad size");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  TVL1_TRY(reserve(c, c->map_scratch, 2 * (size_t)W * H * sizeof(float), st));
  float *m1 = c->map_scratch.as<float>(), *m2 = m1 + (size_t)W * H;
  Affine iM;
  affine_inverse(affine, iM);
  hipLaunchKernelGGL(ka_map_stage, grid2(W, H), kBlk2, 0, st, u, v, fp, W, H, m1, m2);
  hipLaunchKernelGGL(ka_map_warp, grid2(W, H), kBlk2, 0, st, m1, m2, W, H, iM, flow_output ? 1 : 0,
                     I1, p1, u, v, fp);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

// ---- Average-flow alignment of a slice list (added under ABI 9; kernels in tvl1_stack.hpp) ----
// Profiling marks of these calls: class 2, in the ctx's xprof pool.
static inline dim3 grid_lanes(int w, int h, int px) {
  return dim3(((w + px - 1) / px + 63) / 64, (h + 3) / 4, 1);
}

void tvl1_blend6_weights(float w[6]) {
  if (!w) return;
  const float k[6] = {kBlendW0, kBlendW1, kBlendW2, kBlendW2, kBlendW1, kBlendW0};
  for (int i = 0; i < 6; ++i) w[i] = k[i];
}

tvl1_status tvl1_blend6_u8(tvl1_ctx *c, const uint8_t *const frames[6], const size_t pitches[6],
                           int32_t W, int32_t H, uint8_t *dst, size_t dp, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!frames || !pitches || !dst) return set_err(c, TVL1_EINVAL, "null argument");
  if (W <= 0 || H <= 0) return set_err(c, TVL1_ESIZE, "bad size %dx%d", W, H);
  Blend6Args a;
  for (int k = 0; k < 6; ++k) {
    if (!frames[k]) return set_err(c, TVL1_EINVAL, "frame %d is NULL", k);
    if (pitches[k] < (size_t)W) return set_err(c, TVL1_EINVAL, "pitch %d below the row size", k);
    a.f[k] = frames[k];
    a.pitch[k] = pitches[k];
  }
  if (dp < (size_t)W) return set_err(c, TVL1_EINVAL, "dst pitch below the row size");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t tok = c->xprof.begin(c->profiling, st);
  hipLaunchKernelGGL(k_blend6_u8, grid_lanes(W, H, kStackPx), kBlk2, 0, st, a, W, H, dst, dp);
  c->xprof.end(st, tok, 2,7.0 * W * H);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

tvl1_status tvl1_half_u8(tvl1_ctx *c, const uint8_t *src, size_t sp, int32_t W, int32_t H,
                         uint8_t *dst, size_t dp, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!src || !dst) return set_err(c, TVL1_EINVAL, "null argument");
  if (W <= 0 || H <= 0) return set_err(c, TVL1_ESIZE, "bad size %dx%d", W, H);
  if ((W | H) & 1) return set_err(c, TVL1_EINVAL, "tvl1_half_u8 takes even sizes (got %dx%d)", W, H);
  if (sp < (size_t)W || dp < (size_t)(W / 2)) return set_err(c, TVL1_EINVAL, "pitch below the row size");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t tok = c->xprof.begin(c->profiling, st);
  hipLaunchKernelGGL(k_half_u8, grid_lanes(W / 2, H / 2, kStackPx), kBlk2, 0, st, src, sp, W / 2,
                     H / 2, dst, dp);
  c->xprof.end(st, tok, 2,1.25 * W * H);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

tvl1_status tvl1_remap_flow_u8(tvl1_ctx *c, const uint8_t *frame, size_t pitch, int32_t W, int32_t H,
                               const float *u, const float *v, size_t fpitch, int32_t fw,
                               int32_t fh, double gain, int32_t border, uint8_t *dst, size_t dp,
                               void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!frame || !u || !v || !dst) return set_err(c, TVL1_EINVAL, "null argument");
  if (W <= 0 || H <= 0) return set_err(c, TVL1_ESIZE, "bad size %dx%d", W, H);
  if (border < 0) return set_err(c, TVL1_EINVAL, "border must be >= 0 (got %d)", border);
  if (fw < 1 || fh < 1) return set_err(c, TVL1_EINVAL, "bad flow size %dx%d", fw, fh);
  // cv::remap's coordinates saturate to short
  if ((int64_t)W + 2 * (int64_t)border > 32767 || (int64_t)H + 2 * (int64_t)border > 32767)
    return set_err(c, TVL1_ESIZE, "canvas %lldx%lld above 32767", (long long)W + 2LL * border,
                   (long long)H + 2LL * border);
  const int CW = W + 2 * border, CH = H + 2 * border;
  if (pitch < (size_t)W || dp < (size_t)CW) return set_err(c, TVL1_EINVAL, "pitch below the row size");
  if (fpitch % 4 || fpitch < (size_t)fw * sizeof(float))
    return set_err(c, TVL1_EINVAL, "flow pitch must be a multiple of 4 and >= 4 * fw");
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(frame), f1 = f0 + pitch * (size_t)(H - 1) + W;
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + dp * (size_t)(CH - 1) + CW;
  if (f0 < d1 && d0 < f1) return set_err(c, TVL1_EINVAL, "dst overlaps frame");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  RemapArgs a;
  a.frame = frame, a.pitch = pitch, a.W = W, a.H = H;
  a.u = u, a.v = v, a.fpitch = fpitch / sizeof(float), a.fw = fw, a.fh = fh;
  a.gain = gain, a.scale_x = (double)fw / W, a.scale_y = (double)fh / H;
  a.border = border, a.dst = dst, a.dpitch = dp, a.CW = CW, a.CH = CH;
  const size_t tok = c->xprof.begin(c->profiling, st);
  hipLaunchKernelGGL(k_remap_flow_u8, grid_lanes(CW, CH, kRemapPx), kBlk2, 0, st, a);
  c->xprof.end(st, tok, 2,(double)W * H + (double)CW * CH + 8.0 * fw * fh);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

// ---- Integer drift estimate (added under ABI 9; kernels in tvl1_shift.hpp) ----
static constexpr int kShiftLevels = 8;    // max_shift <= 128: L <= 5
static constexpr int kShiftChunk = 256;   // pairs per launch

// I0 rows per wavefront of k_sad_shifts: long segments (the 2r halo rows of I1 are read again
// by the next segment) unless the launch would leave the device short of wavefronts
static int shift_seg(int w, int h, int n) {
  const long bands = (w + kShiftBand - 1) / kShiftBand;
  int seg = 64;
  while (seg > 8 && bands * n * ((h + seg - 1) / seg) < 8192) seg >>= 1;
  return seg;
}

static void launch_sad_shifts(const ShiftSadArgs &a, int n, int r, bool zero, hipStream_t st) {
  const int segs = (a.h + a.seg - 1) / a.seg;
  const dim3 grid((unsigned)((a.w + kShiftBand - 1) / kShiftBand), (unsigned)n, (unsigned)((segs + 3) / 4));
#define SHIFT_LAUNCH(R)                                                                    \
  case R:                                                                                  \
    if (zero) hipLaunchKernelGGL((k_sad_shifts<R, true>), grid, kBlk2, 0, st, a);          \
    else hipLaunchKernelGGL((k_sad_shifts<R, false>), grid, kBlk2, 0, st, a);              \
    break;
  switch (r) {
    SHIFT_LAUNCH(1)
    SHIFT_LAUNCH(2)
    SHIFT_LAUNCH(3)
    SHIFT_LAUNCH(4)
  }
#undef SHIFT_LAUNCH
}

static tvl1_status check_shift_frames(tvl1_ctx *c, const uint8_t *I0, size_t p0, const uint8_t *I1,
                                      size_t p1, int32_t w, int32_t h, const void *out) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (!I0) return set_err(c, TVL1_EINVAL, "I0 is NULL");
  if (!I1) return set_err(c, TVL1_EINVAL, "I1 is NULL");
  if (!out) return set_err(c, TVL1_EINVAL, "out is NULL");
  if (w <= 0 || h <= 0) return set_err(c, TVL1_ESIZE, "bad size %dx%d", w, h);
  if ((int64_t)w * h > ((int64_t)1 << 26))
    return set_err(c, TVL1_ESIZE, "w*h = %lld above 2^26", (long long)w * h);
  if (p0 < (size_t)w) return set_err(c, TVL1_EINVAL, "pitch0 below the row size");
  if (p1 < (size_t)w) return set_err(c, TVL1_EINVAL, "pitch1 below the row size");
  return TVL1_OK;
}

tvl1_status tvl1_sad_shifts_u8(tvl1_ctx *c, const uint8_t *I0, size_t p0, const uint8_t *I1, size_t p1,
                               int32_t w, int32_t h, int32_t cx, int32_t cy, int32_t radius,
                               uint64_t *sad, void *stream) {
  tvl1_status s = check_shift_frames(c, I0, p0, I1, p1, w, h, sad);
  if (s != TVL1_OK) return s;
  if (radius < 1 || radius > kShiftMaxR)
    return set_err(c, TVL1_EINVAL, "radius must be in 1..4 (got %d)", radius);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  TVL1_TRY(reserve(c, c->shift_scratch, kShiftSlots * sizeof(uint64_t), st, 64 << 10));
  unsigned long long *table = c->shift_scratch.as<unsigned long long>();
  HIP_TRY(c, hipMemsetAsync(table, 0, kShiftSlots * sizeof(uint64_t), st));
  // a centre further out than the frame has no overlap at any of its shifts; so has this one
  ShiftSadArgs a{I0, I1, p0, p1, 0, 0, w, h, nullptr, std::max(-(w + 8), std::min(w + 8, cx)),
                 std::max(-(h + 8), std::min(h + 8, cy)), shift_seg(w, h, 1), table};
  launch_sad_shifts(a, 1, radius, false, st);
  HIP_TRY(c, hipGetLastError());
  const int D = 2 * radius + 1;
  HIP_TRY(c, hipMemcpyAsync(sad, table, (size_t)D * D * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}

// One chunk of pairs: pyramid, then per level table and selection, all enqueued on st
static tvl1_status shift_chunk(tvl1_ctx *c, int n, const uint8_t *I0, size_t p0, size_t s0,
                               const uint8_t *I1, size_t p1, size_t s1, int w, int h, int R,
                               tvl1_shift *out, float *seed_out, hipStream_t st) {
  int L = 0;
  while (((R + (1 << L) - 1) >> L) > kShiftMaxR) ++L;
  int ws[kShiftLevels], hs[kShiftLevels];
  size_t lp[kShiftLevels], off[kShiftLevels], one = 0;   // level planes of one frame of one pair
  ws[0] = w, hs[0] = h;
  for (int l = 1; l <= L; ++l) {
    ws[l] = ws[l - 1] / 2, hs[l] = hs[l - 1] / 2;
    lp[l] = align_up((size_t)ws[l], 16);
    off[l] = one;
    one += align_up(lp[l] * hs[l], 256);
  }
  const int n0 = s0 ? n : 1, n1 = s1 ? n : 1;   // a frame shared by every pair has one pyramid
  const size_t tab_b = align_up((size_t)(L + 1) * n * kShiftSlots * sizeof(uint64_t), 256);
  const size_t base_b = align_up((size_t)(L + 1) * n * sizeof(int2), 256);
  const size_t rec_b = align_up((size_t)n * sizeof(tvl1_shift), 256);
  TVL1_TRY(reserve(c, c->shift_scratch, tab_b + base_b + rec_b + one * (size_t)(n0 + n1), st, 64 << 10));
  char *p = c->shift_scratch.p;
  unsigned long long *tables = reinterpret_cast<unsigned long long *>(p);
  int2 *bases = reinterpret_cast<int2 *>(p + tab_b);
  tvl1_shift *recs = reinterpret_cast<tvl1_shift *>(p + tab_b + base_b);
  uint8_t *pyr0 = reinterpret_cast<uint8_t *>(p + tab_b + base_b + rec_b), *pyr1 = pyr0 + one * n0;
  HIP_TRY(c, hipMemsetAsync(tables, 0, tab_b, st));
  // level l of frame f: plane, pitch and pair stride
  auto plane = [&](int f, int l, const uint8_t *&q, size_t &pitch, size_t &stride) {
    if (l == 0) q = f ? I1 : I0, pitch = f ? p1 : p0, stride = f ? s1 : s0;
    else q = (f ? pyr1 : pyr0) + off[l], pitch = lp[l], stride = (f ? s1 : s0) ? one : 0;
  };
  for (int l = 1; l <= L; ++l)
    for (int f = 0; f < 2; ++f) {
      const uint8_t *src, *dst;
      size_t sp, ss, dp, ds;
      plane(f, l - 1, src, sp, ss);
      plane(f, l, dst, dp, ds);
      const dim3 grid((unsigned)(((ws[l] + kStackPx - 1) / kStackPx + 63) / 64), (unsigned)(f ? n1 : n0),
                      (unsigned)((hs[l] + 3) / 4));
      hipLaunchKernelGGL(k_shift_half, grid, kBlk2, 0, st, src, sp, ss, ws[l], hs[l],
                         const_cast<uint8_t *>(dst), dp, ds);
    }
  for (int l = L; l >= 0; --l) {
    const int r = l == L ? (R + (1 << L) - 1) >> L : 1;
    unsigned long long *table = tables + (size_t)l * n * kShiftSlots;
    const int2 *base = l == L ? nullptr : bases + (size_t)l * n;
    ShiftSadArgs a{};
    plane(0, l, a.I0, a.p0, a.s0);
    plane(1, l, a.I1, a.p1, a.s1);
    a.w = ws[l], a.h = hs[l], a.base = base, a.cx = 0, a.cy = 0;
    a.seg = shift_seg(ws[l], hs[l], n), a.table = table;
    launch_sad_shifts(a, n, r, l == 0, st);
    ShiftSelArgs b{table, base, ws[l], hs[l], r, (R + (1 << l) - 1) >> l, l == 0, L + 1,
                   l > 0 ? bases + (size_t)(l - 1) * n : nullptr, recs};
    hipLaunchKernelGGL(k_shift_select, dim3(1, (unsigned)n), dim3(64), 0, st, b);
  }
  // a seeded batch takes its constants from the records here, before the next chunk (or the
  // next call) re-lays the workspace
  if (seed_out)
    hipLaunchKernelGGL(k_shift_seed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, recs, n, seed_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, recs, (size_t)n * sizeof(tvl1_shift), hipMemcpyDeviceToHost, st));
  return TVL1_OK;
}

// The arguments of tvl1_estimate_shift_batch, checked before anything is launched
static tvl1_status check_shift_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t p0, size_t s0,
                                     const uint8_t *I1, size_t p1, size_t s1, int32_t w, int32_t h,
                                     int32_t R, const tvl1_shift *out) {
  tvl1_status s = check_shift_frames(c, I0, p0, I1, p1, w, h, out);
  if (s != TVL1_OK) return s;
  if (n < 1) return set_err(c, TVL1_EINVAL, "n must be >= 1 (got %d)", n);
  if (R < 1 || R > 128) return set_err(c, TVL1_EINVAL, "max_shift must be in 1..128 (got %d)", R);
  if (4 * R > std::min(w, h))
    return set_err(c, TVL1_EINVAL, "4 * max_shift = %d above min(w, h) = %d", 4 * R, std::min(w, h));
  if (n > 1 && ((s0 != 0 && s0 < p0 * (size_t)(h - 1) + w) || (s1 != 0 && s1 < p1 * (size_t)(h - 1) + w)))
    return set_err(c, TVL1_EINVAL, "pair_stride0 / pair_stride1 must be 0 or cover one image");
  return TVL1_OK;
}

// The estimate of n pairs enqueued on st, kShiftChunk at a time: records to out (host), and,
// for a seeded batch, every pair's constants to seed_out (device, 2 n floats)
static tvl1_status shift_chunks(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t p0, size_t s0,
                                const uint8_t *I1, size_t p1, size_t s1, int32_t w, int32_t h,
                                int32_t R, tvl1_shift *out, float *seed_out, hipStream_t st) {
  for (int32_t b = 0; b < n; b += kShiftChunk) {
    // the next chunk re-lays the workspace: in stream order behind this one's record copy
    const int m = std::min(kShiftChunk, n - b);
    TVL1_TRY(shift_chunk(c, m, I0 + (size_t)b * s0, p0, s0, I1 + (size_t)b * s1, p1, s1, w, h, R,
                         out + b, seed_out ? seed_out + 2 * (size_t)b : nullptr, st));
  }
  return TVL1_OK;
}

tvl1_status tvl1_estimate_shift_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t p0, size_t s0,
                                      const uint8_t *I1, size_t p1, size_t s1, int32_t w, int32_t h,
                                      int32_t R, tvl1_shift *out, void *stream) {
  tvl1_status s = check_shift_batch(c, n, I0, p0, s0, I1, p1, s1, w, h, R, out);
  if (s != TVL1_OK) return s;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  TVL1_TRY(shift_chunks(c, n, I0, p0, s0, I1, p1, s1, w, h, R, out, nullptr, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}

// ---- Batched solves seeded by one constant per pair (added under ABI 9) ----
// seed_xy (host, 2 n floats) or, when it is NULL, the drift estimate of every pair (records to
// shifts): the constants go to a block of their own, which lives through every chunk of the
// solve -- the shift workspace is re-laid per 256 pairs, the batch arena per chunk
static tvl1_status calc_batch_const(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                                    size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                                    size_t pair_stride1, int32_t W, int32_t H, const float *seed_xy,
                                    int32_t R, tvl1_shift *shifts, float *u, float *v,
                                    size_t fpitch, size_t flow_pair_stride, tvl1_stats *stats,
                                    void *stream) {
  tvl1_status s = check_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W, H, u, v,
                              fpitch, flow_pair_stride);
  if (s != TVL1_OK) return s;
  if (c->prm.profile == 1)
    return set_err(c, TVL1_EINVAL, "profile 1 takes no initial flow (tvl1_calc_init)");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  s = ensure_geometry(c, W, H, st);
  if (s != TVL1_OK) return s;
  // pairs solved one by one (gamma != 0) take their constant as planes, one pair's at a time
  const size_t cst_b = align_up((size_t)2 * n * sizeof(float), 256);
  const size_t plane_b = batch_chunk_max(c, H) > 0 ? 0 : align_up((size_t)W * H * sizeof(float), 256);
  TVL1_TRY(reserve(c, c->seed_scratch, cst_b + 2 * plane_b, st, 64 << 10));
  float *cst = c->seed_scratch.as<float>();
  if (seed_xy)
    HIP_TRY(c, hipMemcpyAsync(cst, seed_xy, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, st));
  else
    TVL1_TRY(shift_chunks(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W, H, R, shifts,
                          cst, st));
  const Seed seed{plane_b ? c->seed_scratch.as<float>(cst_b) : nullptr,
                  plane_b ? c->seed_scratch.as<float>(cst_b + plane_b) : nullptr,
                  (size_t)W, 0, cst};
  s = calc_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, &seed, W, H, u, v, fpitch,
                 flow_pair_stride, stats, stream);
  if (s != TVL1_OK) return s;
  // the records are on the host when the call returns (the solve has waited at its residual
  // checks: this wait is for its last launches)
  if (!seed_xy) HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}

tvl1_status tvl1_calc_batch_const_init(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                                       size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                                       size_t pair_stride1, int32_t W, int32_t H,
                                       const float *seed_xy, float *u, float *v, size_t fpitch,
                                       size_t flow_pair_stride, tvl1_stats *stats, void *stream) {
  if (!seed_xy) return set_err(c, TVL1_EINVAL, "null initial flow constants");
  for (int64_t i = 0; i < 2 * (int64_t)std::max(n, 0); ++i)
    if (!std::isfinite(seed_xy[i]))
      return set_err(c, TVL1_EINVAL, "initial flow constant %lld of pair %lld is not finite",
                     (long long)(i & 1), (long long)(i >> 1));
  return calc_batch_const(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W, H, seed_xy, 0,
                          nullptr, u, v, fpitch, flow_pair_stride, stats, stream);
}

tvl1_status tvl1_calc_batch_auto_init(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                                      size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                                      size_t pair_stride1, int32_t W, int32_t H, int32_t max_shift,
                                      tvl1_shift *shifts, float *u, float *v, size_t fpitch,
                                      size_t flow_pair_stride, tvl1_stats *stats, void *stream) {
  const tvl1_status s = check_shift_batch(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W,
                                          H, max_shift, shifts);
  if (s != TVL1_OK) return s;
  return calc_batch_const(c, n, I0, pitch0, pair_stride0, I1, pitch1, pair_stride1, W, H, nullptr,
                          max_shift, shifts, u, v, fpitch, flow_pair_stride, stats, stream);
}

tvl1_status tvl1_estimate_shift(tvl1_ctx *c, const uint8_t *I0, size_t p0, const uint8_t *I1, size_t p1,
                                int32_t w, int32_t h, int32_t R, tvl1_shift *out, void *stream) {
  return tvl1_estimate_shift_batch(c, 1, I0, p0, 0, I1, p1, 0, w, h, R, out, stream);
}

// tvl1_calc_host, and tvl1_calc_host_init with a host seed (u0, v0, row pitch ipitch bytes):
// the seed is uploaded into the output staging planes, which the solve reads before its
// last kernel writes them (the in/out flow of tvl1_calc_init)
static tvl1_status calc_host(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                             size_t pitch1, int32_t W, int32_t H, const float *u0, const float *v0,
                             size_t ipitch, float *u, float *v, size_t fpitch, tvl1_stats *stats) {
  tvl1_status s = check_call(c, I0, pitch0, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->mem.own;
  s = ensure_geometry(c, W, H, st);
  if (s != TVL1_OK) return s;
  const size_t P0 = (size_t)c->geo.ps[0];
  // GpuMat::upload (optflow.cpp:315-316)
  HIP_TRY(c, hipMemcpy2DAsync(c->in0, P0, I0, pitch0, W, H, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpy2DAsync(c->in1, P0, I1, pitch1, W, H, hipMemcpyHostToDevice, st));
  const Seed seed{c->outu, c->outv, P0, 0};
  if (u0) {
    HIP_TRY(c, hipMemcpy2DAsync(c->outu, P0 * sizeof(float), u0, ipitch, W * sizeof(float), H,
                                hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpy2DAsync(c->outv, P0 * sizeof(float), v0, ipitch, W * sizeof(float), H,
                                hipMemcpyHostToDevice, st));
  }
  s = solve(c, Frames{c->in0, c->in1, P0, P0, false}, u0 ? &seed : nullptr, W, H, c->outu, c->outv,
            P0 * sizeof(float), stats, st);
  if (s != TVL1_OK) return s;
  // download (optflow.cpp:475-476)
  HIP_TRY(c, hipMemcpy2DAsync(u, fpitch, c->outu, P0 * sizeof(float), W * sizeof(float), H,
                              hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpy2DAsync(v, fpitch, c->outv, P0 * sizeof(float), W * sizeof(float), H,
                              hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}

tvl1_status tvl1_calc_host(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                           size_t pitch1, int32_t W, int32_t H, float *u, float *v,
                           size_t fpitch, tvl1_stats *stats) {
  return calc_host(c, I0, pitch0, I1, pitch1, W, H, nullptr, nullptr, 0, u, v, fpitch, stats);
}

tvl1_status tvl1_calc_host_init(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                                size_t pitch1, int32_t W, int32_t H, const float *u0,
                                const float *v0, size_t init_pitch, float *u, float *v,
                                size_t fpitch, tvl1_stats *stats) {
  const tvl1_status s = check_seed(c, u0, v0, init_pitch, W);
  if (s != TVL1_OK) return s;
  return calc_host(c, I0, pitch0, I1, pitch1, W, H, u0, v0, init_pitch, u, v, fpitch, stats);
}

tvl1_status tvl1_postprocess_batch(tvl1_ctx *c, int32_t n, float *u, float *v, size_t fpitch,
                                   size_t fstride, const uint8_t *I1, size_t pitch1,
                                   size_t stride1, int32_t W, int32_t H, int32_t mode,
                                   void *stream) {
  if (n < 0) return set_err(c, TVL1_EINVAL, "n must be >= 0");
  if (n == 0) return c ? TVL1_OK : set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  tvl1_status s = check_call(c, I1, pitch1, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  if (mode < 0 || mode > 2)
    return set_err(c, TVL1_EINVAL, "mode must be 0 (flow), 1 (map) or 2 (map - grid)");
  if (n > 1 && (fstride < fpitch * (size_t)H || fstride % 4 || stride1 < pitch1 * (size_t)(H - 1) + W))
    return set_err(c, TVL1_EINVAL, "pair strides overlap the pairs");
  if (n > 65535) return set_err(c, TVL1_EINVAL, "at most 65535 pairs per call");
  HIP_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_postprocess_batch, grid2(W, H, n), kBlk2, 0, (hipStream_t)stream, u, v,
                     fpitch, fstride, I1, pitch1, stride1, W, H, mode);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

tvl1_status tvl1_gather_flow(tvl1_ctx *c, const float *u, const float *v, int64_t plane_elems,
                             const int64_t *offsets, int32_t n, float *out_u, float *out_v,
                             void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  if (n < 0 || (n > 0 && (!u || !v || !offsets || !out_u || !out_v)))
    return set_err(c, TVL1_EINVAL, "bad argument");
  if (n == 0) return TVL1_OK;
  for (int32_t i = 0; i < n; ++i)
    if (offsets[i] < 0 || offsets[i] >= plane_elems)   // never an out-of-range device read
      return set_err(c, TVL1_EINVAL, "offset %lld at %d outside [0, %lld)",
                     (long long)offsets[i], i, (long long)plane_elems);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  c->mem.enter(st);
  const size_t off_b = align_up((size_t)n * sizeof(int64_t), 256);
  TVL1_TRY(reserve(c, c->gather_scratch, off_b + (size_t)n * sizeof(float2), st, 64 << 10));
  int64_t *doff = c->gather_scratch.as<int64_t>();
  float2 *dout = c->gather_scratch.as<float2>(off_b);
  std::vector<float2> host((size_t)n);
  HIP_TRY(c, hipMemcpyAsync(doff, offsets, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_gather_flow, dim3((n + 255) / 256), dim3(256), 0, st, u, v, doff, n, dout);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(host.data(), dout, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int32_t i = 0; i < n; ++i) {
    out_u[i] = host[i].x;
    out_v[i] = host[i].y;
  }
  return TVL1_OK;
}

tvl1_status tvl1_postprocess(tvl1_ctx *c, float *u, float *v, size_t fpitch, const uint8_t *I1,
                             size_t pitch1, int32_t W, int32_t H, int32_t mode, void *stream) {
  tvl1_status s = check_call(c, I1, pitch1, I1, pitch1, W, H, u, v, fpitch);
  if (s != TVL1_OK) return s;
  if (mode < 0 || mode > 2)
    return set_err(c, TVL1_EINVAL, "mode must be 0 (flow), 1 (map) or 2 (map - grid)");
  HIP_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_postprocess, grid2(W, H), kBlk2, 0, (hipStream_t)stream, u, v, fpitch, I1,
                     pitch1, W, H, mode);
  HIP_TRY(c, hipGetLastError());
  return TVL1_OK;
}

// ---- Forward-backward consistency score (added under ABI 9; kernels in tvl1_fbcheck.hpp,
// DESIGN 13) ----
// The utility calls below (this section and DESIGN 14-16) share their argument rules
// (tvl1_planes.hpp: each states a plane table and an overlap table), pair_at and run_chunks.
static constexpr int kFbChunk = 256;              // pairs per launch

// A tvl1_planes.hpp verdict into the ctx's error text
static tvl1_status planes_try(tvl1_ctx *c, tvl1_status s, const std::string &msg) {
  return s == TVL1_OK ? s : set_err(c, s, "%s", msg.c_str());
}

extern "C++" {
// The plane of pair b: p advanced by b pair strides (bytes)
template <class T>
static inline T *pair_at(T *p, int32_t b, size_t stride) {
  return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + (size_t)b * stride);
}

// What every batched utility call does around its launches: n pairs in chunks of kFbChunk on
// `stream`, as one class-2 mark of `bytes` moved.  launch(first pair, pairs in the chunk, the device
// counters or null) fills the kernel's Args and launches.  With `counts` (HOST, n records of `rec`
// bytes) each chunk's counters are zeroed before and copied out after its launch, in the ctx's
// count scratch, and the call returns once they have arrived.
template <class Launch>
static tvl1_status run_chunks(tvl1_ctx *c, void *stream, int32_t n, double bytes, void *counts,
                              size_t rec, Launch launch) {
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *cnt = nullptr;
  if (counts) {
    c->mem.enter(st);
    const size_t need = kFbChunk * sizeof(tvl1_invert_counts);   // the largest record
    TVL1_TRY(reserve(c, c->count_scratch, need, st));
    cnt = c->count_scratch.as<unsigned long long>();
  }
  const size_t tok = c->xprof.begin(c->profiling, st);
  for (int32_t b = 0; b < n; b += kFbChunk) {
    const int m = std::min(kFbChunk, n - b);
    // the next chunk's zero fill is in stream order behind this one's copy
    if (cnt) HIP_TRY(c, hipMemsetAsync(cnt, 0, (size_t)m * rec, st));
    launch(b, m, cnt);
    if (cnt)
      HIP_TRY(c, hipMemcpyAsync(pair_at(static_cast<char *>(counts), b, rec), cnt, (size_t)m * rec,
                                hipMemcpyDeviceToHost, st));
  }
  c->xprof.end(st, tok, 2,bytes);
  HIP_TRY(c, hipGetLastError());
  if (cnt) HIP_TRY(c, hipStreamSynchronize(st));
  return TVL1_OK;
}
}  // extern "C++"

static inline dim3 fb_grid(int w, int h, int n) {
  return dim3((unsigned)((w + 64 * kFbPx - 1) / (64 * kFbPx)), (unsigned)n,
              (unsigned)std::min((h + 3) / 4, kFbMaxRowGroups));
}

tvl1_status tvl1_fb_score_batch(tvl1_ctx *c, int32_t n, const float *uf, const float *vf,
                                size_t fpitch, size_t fstride, const float *ub, const float *vb,
                                size_t bpitch, size_t bstride, int32_t w, int32_t h, float alpha,
                                float *score, size_t spitch, size_t sstride, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[5] = {{"uf", uf, fpitch, fstride}, {"vf", vf, fpitch, fstride},
                       {"ub", ub, bpitch, bstride}, {"vb", vb, bpitch, bstride},
                       {"score", score, spitch, sstride}};
  // score off every flow plane, the backward flow off the forward
  static constexpr Overlap ov[8] = {{4, 0}, {4, 1}, {4, 2}, {4, 3}, {2, 0}, {3, 0}, {2, 1}, {3, 1}};
  const PlaneSet ps = {n, w, h, pl, 5, -1};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kFloatXLimit, &msg), msg));
  if (std::isnan(alpha)) return set_err(c, TVL1_EINVAL, "alpha is NaN");
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 8, false, &msg), msg));
  return run_chunks(c, stream, n, 20.0 * w * h * n, nullptr, 0, [&](int32_t b, int m, unsigned long long *) {
    FbScoreArgs a;
    a.uf = pair_at(uf, b, fstride), a.vf = pair_at(vf, b, fstride);
    a.ub = pair_at(ub, b, bstride), a.vb = pair_at(vb, b, bstride);
    a.score = pair_at(score, b, sstride);
    a.fp = fpitch, a.fs = fstride, a.bp = bpitch, a.bs = bstride, a.sp = spitch, a.ss = sstride;
    a.w = w, a.h = h, a.alpha = alpha;
    hipLaunchKernelGGL(k_fb_score, fb_grid(w, h, m), kBlk2, 0, (hipStream_t)stream, a);
  });
}

tvl1_status tvl1_fb_score(tvl1_ctx *c, const float *uf, const float *vf, size_t fpitch,
                          const float *ub, const float *vb, size_t bpitch, int32_t w, int32_t h,
                          float alpha, float *score, size_t spitch, void *stream) {
  return tvl1_fb_score_batch(c, 1, uf, vf, fpitch, 0, ub, vb, bpitch, 0, w, h, alpha, score, spitch, 0,
                             stream);
}

tvl1_status tvl1_zero_above_batch(tvl1_ctx *c, int32_t n, float *u, float *v, size_t fpitch,
                                  size_t fstride, const float *score, size_t spitch, size_t sstride,
                                  int32_t w, int32_t h, float beta, uint64_t *rejected,
                                  void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[3] = {{"u", u, fpitch, fstride}, {"v", v, fpitch, fstride}, {"score", score, spitch, sstride}};
  static constexpr Overlap ov[2] = {{2, 0}, {2, 1}};
  const PlaneSet ps = {n, w, h, pl, 3, -1};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kFloatXLimit, &msg), msg));
  if (std::isnan(beta)) return set_err(c, TVL1_EINVAL, "beta is NaN");
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 2, false, &msg), msg));
  return run_chunks(c, stream, n, 12.0 * w * h * n, rejected, sizeof(uint64_t),
                    [&](int32_t b, int m, unsigned long long *cnt) {
    ZeroAboveArgs a;
    a.u = pair_at(u, b, fstride), a.v = pair_at(v, b, fstride), a.score = pair_at(score, b, sstride);
    a.fp = fpitch, a.fs = fstride, a.sp = spitch, a.ss = sstride;
    a.w = w, a.h = h, a.beta = beta, a.count = cnt;
    hipLaunchKernelGGL(k_zero_above, fb_grid(w, h, m), kBlk2, 0, (hipStream_t)stream, a);
  });
}

tvl1_status tvl1_zero_above(tvl1_ctx *c, float *u, float *v, size_t fpitch, const float *score,
                            size_t spitch, int32_t w, int32_t h, float beta, uint64_t *rejected,
                            void *stream) {
  return tvl1_zero_above_batch(c, 1, u, v, fpitch, 0, score, spitch, 0, w, h, beta, rejected, stream);
}

// ---- Flow composition (added under ABI 9; kernel in tvl1_compose.hpp) ----
tvl1_status tvl1_compose_flow_batch(tvl1_ctx *c, int32_t n, const float *ua, const float *va,
                                    size_t apitch, size_t astride, const float *ub, const float *vb,
                                    size_t bpitch, size_t bstride, int32_t w, int32_t h, float *uc,
                                    float *vc, size_t cpitch, size_t cstride, uint64_t *outside,
                                    void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[6] = {{"ua", ua, apitch, astride}, {"va", va, apitch, astride},
                       {"ub", ub, bpitch, bstride}, {"vb", vb, bpitch, bstride},
                       {"uc", uc, cpitch, cstride}, {"vc", vc, cpitch, cstride}};
  // c off b; c off a too, unless it runs in place on a: a px reads its own a and nobody else's
  static constexpr Overlap ov[8] = {{4, 2}, {4, 3}, {5, 2}, {5, 3},
                                    {4, 0, true}, {4, 1, true}, {5, 0, true}, {5, 1, true}};
  const bool in_place = uc == ua && vc == va && cpitch == apitch && cstride == astride;
  const PlaneSet ps = {n, w, h, pl, 6, -1};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kFloatXLimit, &msg), msg));
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 8, in_place, &msg), msg));
  return run_chunks(c, stream, n, 24.0 * w * h * n, outside, sizeof(uint64_t),
                    [&](int32_t b, int m, unsigned long long *cnt) {
    ComposeArgs a;
    a.ua = pair_at(ua, b, astride), a.va = pair_at(va, b, astride);
    a.ub = pair_at(ub, b, bstride), a.vb = pair_at(vb, b, bstride);
    a.uc = pair_at(uc, b, cstride), a.vc = pair_at(vc, b, cstride);
    a.ap = apitch, a.as = astride, a.bp = bpitch, a.bs = bstride, a.cp = cpitch, a.cs = cstride;
    a.w = w, a.h = h, a.count = cnt;
    hipLaunchKernelGGL(k_compose_flow, fb_grid(w, h, m), kBlk2, 0, (hipStream_t)stream, a);
  });
}

tvl1_status tvl1_compose_flow(tvl1_ctx *c, const float *ua, const float *va, size_t apitch,
                              const float *ub, const float *vb, size_t bpitch, int32_t w, int32_t h,
                              float *uc, float *vc, size_t cpitch, uint64_t *outside, void *stream) {
  return tvl1_compose_flow_batch(c, 1, ua, va, apitch, 0, ub, vb, bpitch, 0, w, h, uc, vc, cpitch, 0,
                                 outside, stream);
}

// ---- Flow inversion (added under ABI 9; kernel in tvl1_invert.hpp) ----
static_assert(sizeof(tvl1_invert_counts) == 2 * sizeof(unsigned long long), "the kernel's record");
tvl1_status tvl1_invert_flow_batch(tvl1_ctx *c, int32_t n, const float *uf, const float *vf,
                                   size_t fpitch, size_t fstride, int32_t iterations, float tol,
                                   float *ug, float *vg, size_t gpitch, size_t gstride, float *resid,
                                   size_t rpitch, size_t rstride, int32_t w, int32_t h,
                                   tvl1_invert_counts *counts, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[5] = {{"uf", uf, fpitch, fstride}, {"vf", vf, fpitch, fstride},
                       {"ug", ug, gpitch, gstride}, {"vg", vg, gpitch, gstride},
                       {"resid", resid, rpitch, rstride}};
  // a px reads f at other px: nothing runs in place, every output off every plane before it
  static constexpr Overlap ov[9] = {{2, 0}, {2, 1}, {3, 0}, {3, 1}, {3, 2}, {4, 0}, {4, 1}, {4, 2}, {4, 3}};
  const PlaneSet ps = {n, w, h, pl, 5, resid ? -1 : 4};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kFloatXLimit, &msg), msg));
  if (iterations < 1 || iterations > kInvMaxIter)
    return set_err(c, TVL1_EINVAL, "iterations must be 1..%d (got %d)", kInvMaxIter, iterations);
  if (std::isnan(tol)) return set_err(c, TVL1_EINVAL, "tol is NaN");
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 9, false, &msg), msg));
  return run_chunks(c, stream, n, 20.0 * w * h * n, counts, sizeof(tvl1_invert_counts),
                    [&](int32_t b, int m, unsigned long long *cnt) {
    InvertArgs a;
    a.uf = pair_at(uf, b, fstride), a.vf = pair_at(vf, b, fstride);
    a.ug = pair_at(ug, b, gstride), a.vg = pair_at(vg, b, gstride);
    a.resid = resid ? pair_at(resid, b, rstride) : nullptr;
    a.fp = fpitch, a.fs = fstride, a.gp = gpitch, a.gs = gstride, a.rp = rpitch, a.rs = rstride;
    a.w = w, a.h = h, a.iters = iterations, a.tol = tol, a.count = cnt;
    if (c->invert_window)
      hipLaunchKernelGGL(k_invert_flow<true>, fb_grid(w, h, m), kBlk2, 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(k_invert_flow<false>, fb_grid(w, h, m), kBlk2, 0, (hipStream_t)stream, a);
  });
}

tvl1_status tvl1_invert_flow(tvl1_ctx *c, const float *uf, const float *vf, size_t fpitch,
                             int32_t iterations, float tol, float *ug, float *vg, size_t gpitch,
                             float *resid, size_t rpitch, int32_t w, int32_t h,
                             tvl1_invert_counts *counts, void *stream) {
  return tvl1_invert_flow_batch(c, 1, uf, vf, fpitch, 0, iterations, tol, ug, vg, gpitch, 0, resid, rpitch,
                                0, w, h, counts, stream);
}

// ---- Photometric (ZNCC) score of a flow (added under ABI 9; kernels in tvl1_score.hpp,
// DESIGN 14) ----
static void launch_zncc(const ZnccArgs &a, int radius, int m, hipStream_t st) {
  const int bw = 64 - 2 * radius, bands = (a.w + bw - 1) / bw;   // a band's output columns
  const dim3 grid((unsigned)((bands + 3) / 4), (unsigned)((a.h + kZnSegRows - 1) / kZnSegRows), (unsigned)m);
  switch (radius) {
    case 1: hipLaunchKernelGGL(k_zncc_score<1>, grid, kBlk2, 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_zncc_score<2>, grid, kBlk2, 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_zncc_score<3>, grid, kBlk2, 0, st, a); break;
    default: hipLaunchKernelGGL(k_zncc_score<4>, grid, kBlk2, 0, st, a); break;
  }
}

tvl1_status tvl1_zncc_score_batch(tvl1_ctx *c, int32_t n, const uint8_t *I0, size_t pitch0,
                                  size_t stride0, const uint8_t *I1, size_t pitch1, size_t stride1,
                                  const float *u, const float *v, size_t fpitch, size_t fstride,
                                  int32_t w, int32_t h, int32_t radius, float *score, size_t spitch,
                                  size_t sstride, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[5] = {{"I0", I0, pitch0, stride0, 1, true}, {"I1", I1, pitch1, stride1, 1, true},
                       {"u", u, fpitch, fstride}, {"v", v, fpitch, fstride},
                       {"score", score, spitch, sstride}};
  static constexpr Overlap ov[4] = {{4, 0}, {4, 1}, {4, 2}, {4, 3}};
  const PlaneSet ps = {n, w, h, pl, 5, -1};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kMap32Limit, &msg), msg));
  if (radius < 1 || radius > 4) return set_err(c, TVL1_EINVAL, "radius must be 1..4 (got %d)", radius);
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 4, false, &msg), msg));
  return run_chunks(c, stream, n, 14.0 * w * h * n, nullptr, 0, [&](int32_t b, int m, unsigned long long *) {
    ZnccArgs a;
    a.I0 = pair_at(I0, b, stride0), a.I1 = pair_at(I1, b, stride1);
    a.u = pair_at(u, b, fstride), a.v = pair_at(v, b, fstride), a.score = pair_at(score, b, sstride);
    a.p0 = pitch0, a.s0 = stride0, a.p1 = pitch1, a.s1 = stride1;
    a.fp = fpitch, a.fs = fstride, a.sp = spitch, a.ss = sstride;
    a.w = w, a.h = h;
    launch_zncc(a, radius, m, (hipStream_t)stream);
  });
}

tvl1_status tvl1_zncc_score(tvl1_ctx *c, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                            size_t pitch1, const float *u, const float *v, size_t fpitch, int32_t w,
                            int32_t h, int32_t radius, float *score, size_t spitch, void *stream) {
  return tvl1_zncc_score_batch(c, 1, I0, pitch0, 0, I1, pitch1, 0, u, v, fpitch, 0, w, h, radius, score,
                               spitch, 0, stream);
}

tvl1_status tvl1_warp_by_flow_u8(tvl1_ctx *c, const uint8_t *I1, size_t pitch1, const float *u,
                                 const float *v, size_t fpitch, int32_t w, int32_t h, uint8_t *dst,
                                 size_t dpitch, uint8_t *valid, size_t vpitch, void *stream) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  const Plane pl[5] = {{"I1", I1, pitch1, 0, 1}, {"dst", dst, dpitch, 0, 1},
                       {"valid", valid, vpitch, 0, 1},   // left out where it is not given
                       {"u", u, fpitch, 0}, {"v", v, fpitch, 0}};
  // each output off each input, then off each other
  static constexpr Overlap ov[7] = {{1, 0}, {1, 3}, {1, 4}, {2, 0}, {2, 3}, {2, 4}, {2, 1}};
  const PlaneSet ps = {1, w, h, pl, 5, valid ? -1 : 2};
  std::string msg;
  TVL1_TRY(planes_try(c, check_planes(ps, kMap32Limit, &msg), msg));
  TVL1_TRY(planes_try(c, check_overlaps(ps, ov, 7, false, &msg), msg));
  return run_chunks(c, stream, 1, (valid ? 11.0 : 10.0) * w * h, nullptr, 0, [&](int32_t, int, unsigned long long *) {
    WarpFlowArgs a;
    a.I1 = I1, a.p1 = pitch1, a.u = u, a.v = v, a.fp = fpitch, a.w = w, a.h = h;
    a.dst = dst, a.dp = dpitch, a.valid = valid, a.vp = vpitch;
    const dim3 grid((unsigned)((w + 64 * kFbPx - 1) / (64 * kFbPx)), 1u,
                    (unsigned)std::min((h + 3) / 4, kZnMaxRowGroups));
    hipLaunchKernelGGL(k_warp_flow_u8, grid, kBlk2, 0, (hipStream_t)stream, a);
  });
}

void *tvl1_stream(tvl1_ctx *c) { return c ? (void *)c->mem.own : nullptr; }

tvl1_status tvl1_set_profiling(tvl1_ctx *c, int32_t enable) {
  if (!c) return set_err(nullptr, TVL1_EINVAL, "ctx is NULL");
  c->profiling = enable != 0;
  if (!c->profiling) c->xprof.reset();   // marks still waiting for a solve do not outlive the switch
  return TVL1_OK;
}

void tvl1_destroy(tvl1_ctx *c) {
  if (!c) return;
  c->prof.destroy();
  c->xprof.destroy();
  (void)hipSetDevice(c->device);
  if (c->mem.own) (void)hipStreamSynchronize(c->mem.own);
  // hipFree waits for the device: callers' streams included
  c->mem.release_all(c->arena, c->barena, c->align_scratch, c->map_scratch, c->gather_scratch,
                     c->small_scratch, c->shift_scratch, c->seed_scratch, c->count_scratch);
  if (c->align_pat) (void)hipFree(c->align_pat);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->mem.own) (void)hipStreamDestroy(c->mem.own);
  for (hipEvent_t e : c->ev_check)
    if (e) (void)hipEventDestroy(e);
  if (c->gate) (void)hipFree(c->gate);
  delete c;
}

const char *tvl1_last_error(const tvl1_ctx *c) {
  return c ? c->err.c_str() : g_create_error.c_str();
}

}  // extern "C"
