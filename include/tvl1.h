/*
 * tvl1.h — C-ABI boundary of the MI355X-native dense TV-L1 optical-flow engine.
 *
 * This header is the drop-in replacement for the reference's single solver
 * call site:
 *
 *   reference  src/optflow.h:31 / src/optflow.cpp:516-520
 *     void TVL1_solve(cv::cuda::GpuMat& frame0, cv::cuda::GpuMat& frame1,
 *                     cv::cuda::GpuMat& output, const Json::Value& args);
 *   which does
 *     cv::cuda::OpticalFlowDual_TVL1::create(tau, lambda, theta, nscales, warps,
 *                                            epsilon, iterations, scaleStep, gamma)
 *       ->calc(frame0, frame1, output);                 (OpenCV 3.4.1, not vendored)
 *
 * Mapping (one row per reference concept):
 *   OpticalFlowDual_TVL1::create(...)       -> tvl1_create(&ctx, device, &params)
 *   solver->calc(I0, I1, flow) on GpuMats   -> tvl1_calc(ctx, dI0, pitch0, dI1, pitch1, w, h,
 *                                                       du, dv, flow_pitch, &stats, stream)
 *   cuda::split(flow) (optflow.cpp:404)     -> outputs are already planar (u, v)
 *   solver destruction                      -> tvl1_destroy(ctx)
 *   cv::Exception (CV_Assert)               -> tvl1_status return code + tvl1_last_error(ctx)
 *   post-ops optflow.cpp:445-473            -> tvl1_postprocess(...) (map grid add + I1<=1 mask)
 *   generate_TV_args defaults :500-514      -> tvl1_params_default(&params)
 *
 * Conventions
 *   - Plain pointers and sizes only; no HIP, torch or OpenCV types.  `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream).
 *   - All pitches are in BYTES (OpenCV GpuMat::step convention).
 *   - Inputs are 8-bit unsigned grayscale (CV_8UC1, IMREAD_GRAYSCALE, optflow.cpp:106);
 *     outputs are planar float32 u (x displacement) and v (y displacement) such
 *     that I1(x+u, y+v) ~= I0(x, y)  (flow points from frame0=p to frame1=q).
 *   - Errors never throw across the ABI: every entry point returns tvl1_status.
 *   - A ctx is not thread-safe.  Distinct ctxs (one per device per host thread)
 *     are independent.  tvl1_calc is asynchronous w.r.t. the host only where the
 *     stats say so: the convergence test reads the residual on the host exactly
 *     where OpenCV does (a device->host read on "check" iterations), so the call
 *     returns after the solve has been fully enqueued; outputs are valid after a
 *     stream synchronize (tvl1_calc_host synchronizes for you).
 */
#ifndef FIBSEM_OPTFLOW_AMD_TVL1_H
#define FIBSEM_OPTFLOW_AMD_TVL1_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVL1_ABI_VERSION 9
#define TVL1_MAX_LEVELS 32

typedef enum tvl1_status {
  TVL1_OK = 0,
  TVL1_EINVAL = 1, /* bad argument (null pointer, nscales <= 0, bad pitch ...)  */
  TVL1_ESIZE = 2,  /* size mismatch / image smaller than 1x1 / too large       */
  TVL1_EHIP = 3,   /* a HIP runtime call failed (message in tvl1_last_error)    */
  TVL1_ENOMEM = 4, /* device or host allocation failed                          */
  TVL1_ENODEV = 5  /* no usable gfx950 device / extension not built             */
} tvl1_status;

/* The nine cv::cuda::OpticalFlowDual_TVL1::create() arguments (optflow.cpp:518)
 * plus the two build-only additions listed in SURVEY Appendix B. */
typedef struct tvl1_params {
  double tau;          /* 0.25  optflow.cpp:503 */
  double lambda;       /* 0.05  optflow.cpp:504 */
  double theta;        /* 0.3   optflow.cpp:505 */
  int32_t nscales;     /* 10    optflow.cpp:506 */
  int32_t warps;       /* 5     optflow.cpp:507 */
  double epsilon;      /* 0.01  optflow.cpp:508 */
  int32_t iterations;  /* 300   optflow.cpp:509 */
  double scale_step;   /* 0.8   optflow.cpp:510 */
  double gamma;        /* 0.0   optflow.cpp:511 */
  int32_t use_initial_flow; /* read at optflow.cpp:512 but NOT passed to create() (:518): ignored by every
                               entry point, as in the reference; a solve that starts from a flow is a call
                               of its own, tvl1_calc_init */
  int32_t median_filtering; /* build-only: 1 = off (reference behaviour); 3 or 5 = median of u,v before each warp */
  int32_t fast_math;   /* build-only arithmetic mode:
                          0 = IEEE float32, no contraction: bit-identical to oracle/ (default);
                          1 = the reference build's CUDA_FAST_MATH semantics (singularity/optflow.def:33-34):
                              a*b + c contracted as nvcc does, approximate division and sqrt.  Held to
                              the tolerance of DESIGN.md 2 against oracle/, not to bit identity;
                          2 = nvcc's default -fmad=true contraction alone, IEEE division and sqrt:
                              bit-identical to oracle/'s fma mode.
                          gamma != 0 and tau/theta < 0 solves stay IEEE. */
  int32_t profile;     /* build-only: 0 = cv::cuda::OpticalFlowDual_TVL1,
                          the reference's path (default); 1 = the schedule of OpenCV's CPU
                          cv::DualTVL1OpticalFlow: half-pixel pyramid/upsample, remap INTER_CUBIC
                          (a = -0.75, 1/32 px map, BORDER_CONSTANT), outer iterations each starting
                          with medianFiltering, inner iterations each checking the residual.
                          `iterations` is unused there; fast_math is ignored. */
  int32_t inner_iterations; /* profile 1: innerIterations (cv::DualTVL1OpticalFlow default 30) */
  int32_t outer_iterations; /* profile 1: outerIterations (default 10) */
} tvl1_params;

/* Per-call statistics.  Valid after tvl1_calc returns (host-side counters). */
typedef struct tvl1_stats {
  int32_t levels;                           /* effective pyramid depth (OpenCV mutates nscales_) */
  int32_t level_width[TVL1_MAX_LEVELS];
  int32_t level_height[TVL1_MAX_LEVELS];
  int64_t level_iterations[TVL1_MAX_LEVELS]; /* executed iterations summed over warps */
  int64_t iterations_total;
  int64_t checks_total;                     /* iterations that evaluated the residual (cuda::sum) */
  double algorithmic_bytes;                 /* SURVEY 8(d) byte model with executed counts */
  /* Optional caller-owned buffer: executed iterations per (level, warp), indexed
   * [level * warps + warp], level 0 = finest.  Left untouched when NULL. */
  int32_t *warp_iterations;
  int32_t warp_iterations_capacity;         /* number of int32 slots in warp_iterations */
  int32_t speculation_misses;               /* tvl1_calc: launches enqueued behind a residual check
                                             * that ran empty (a wrong guess);
                                             * tvl1_calc_batch: warps whose constants were not
                                             * stored but needed (re-gathered) */
  /* Filled only when profiling is enabled (tvl1_set_profiling): HIP-event time,
   * launch count and algorithmic bytes per kernel class, on the solve's stream.
   * Class 0 = fused primal-dual iteration (K6+K8+K7 partials), 1 = warpBackward
   * (K5), 2 = everything else (convert, pyramid, gradient, upsample, output), 3 = a batch's
   * coarsest level solved on chip in one launch (warps, iterations and stopping rule; bound
   * on chip, so it stays out of class 0's HBM roofline). */
  double kernel_ms[4];
  int64_t kernel_launches[4];
  double kernel_bytes[4];      /* SURVEY 8(d) algorithmic bytes (64 B/px per iteration for class 0) */
  double kernel_hbm_bytes[4];  /* compulsory HBM bytes of THIS implementation's tiling */
} tvl1_stats;

typedef struct tvl1_ctx tvl1_ctx;

/* Fill params with the reference defaults of generate_TV_args (optflow.cpp:500-514). */
void tvl1_params_default(tvl1_params *params);

/* Create a solver bound to HIP device `device` (ordinal).  Replaces
 * OpticalFlowDual_TVL1::create (optflow.cpp:518).  Scratch grows on demand. */
tvl1_status tvl1_create(tvl1_ctx **out, int device, const tvl1_params *params);

/* Replace the solver parameters of an existing ctx (the reference re-creates the
 * solver per call, optflow.cpp:518; this avoids re-allocating scratch). */
tvl1_status tvl1_set_params(tvl1_ctx *ctx, const tvl1_params *params);

/* Solve I0 -> I1 on DEVICE memory.  Replaces solver->calc(frame0, frame1, flow)
 * (optflow.cpp:519) followed by cuda::split (optflow.cpp:404).
 *   I0, I1 : device u8 images, row pitch pitch0/pitch1 bytes (ROI views allowed)
 *   u, v   : device f32 outputs, row pitch flow_pitch bytes
 *   stats  : may be NULL
 *   stream : hipStream_t as void*, NULL = default stream            */
tvl1_status tvl1_calc(tvl1_ctx *ctx,
                      const uint8_t *I0, size_t pitch0,
                      const uint8_t *I1, size_t pitch1,
                      int32_t width, int32_t height,
                      float *u, float *v, size_t flow_pitch,
                      tvl1_stats *stats, void *stream);

/* CV_32FC1 frames: calc converts f32 inputs with convertTo(CV_32F, 255), so
 * pixel values are expected in [0, 1]; everything else as tvl1_calc.  Device pointers,
 * pitches in bytes (>= 4 * width, multiples of 4). */
tvl1_status tvl1_calc_f32(tvl1_ctx *ctx, const float *I0, size_t pitch0, const float *I1,
                          size_t pitch1, int32_t width, int32_t height, float *u, float *v,
                          size_t flow_pitch, tvl1_stats *stats, void *stream);

/* Batched solve (build addition for the production workload, SURVEY 3.2: two 3072x100
 * ROI strips per slice pair, each a solve of ~400 tiny launches): n pairs of one size,
 * pair b at I0 + b*pair_stride0, I1 + b*pair_stride1 (bytes; 0 = the same frame for every
 * pair; device pointers, as in
 * tvl1_calc), flow of pair b at u / v + b*flow_pair_stride.  Up to 256 pairs share every
 * kernel launch; each pair's flow and per-warp iteration counts are those of tvl1_calc
 * (bit-identical; with fast_math = 1 within the same tolerance as tvl1_calc's).  stats: NULL
 * or an array of n.  gamma != 0 and profile 1 solve the pairs one by one.  Asynchronous on
 * `stream` like tvl1_calc, but the host waits at residual checks. */
tvl1_status tvl1_calc_batch(tvl1_ctx *ctx, int32_t n,
                            const uint8_t *I0, size_t pitch0, size_t pair_stride0,
                            const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                            int32_t width, int32_t height,
                            float *u, float *v, size_t flow_pitch, size_t flow_pair_stride,
                            tvl1_stats *stats, void *stream);

/* ---- Solves that start from a caller-supplied flow (added under ABI 9) ----
 * cv::cuda::OpticalFlowDual_TVL1::calc with useInitialFlow = true: level 0 of the flow
 * pyramid is the seed (u0, v0), each coarser level is cuda::resize(INTER_LINEAR) of the one
 * before times scaleStep, and the coarsest level of that chain replaces the zero flow the
 * solve otherwise starts from (u3 stays zero there for gamma != 0).  Everything else is
 * tvl1_calc.  u0, v0: device f32 planes of the frame's size, row pitch init_pitch bytes
 * (>= 4 * width, a multiple of 4).  u0 == u and v0 == v are allowed (OpenCV's in/out flow):
 * the seed is read before the flow is written, on the same stream.  A null seed or a bad
 * pitch is TVL1_EINVAL before anything is launched; so is a ctx with profile = 1. */
tvl1_status tvl1_calc_init(tvl1_ctx *ctx,
                           const uint8_t *I0, size_t pitch0,
                           const uint8_t *I1, size_t pitch1,
                           int32_t width, int32_t height,
                           const float *u0, const float *v0, size_t init_pitch,
                           float *u, float *v, size_t flow_pitch,
                           tvl1_stats *stats, void *stream);

/* tvl1_calc_init on HOST memory (frames, seed and flow; as tvl1_calc_host). */
tvl1_status tvl1_calc_host_init(tvl1_ctx *ctx,
                                const uint8_t *I0, size_t pitch0,
                                const uint8_t *I1, size_t pitch1,
                                int32_t width, int32_t height,
                                const float *u0, const float *v0, size_t init_pitch,
                                float *u, float *v, size_t flow_pitch,
                                tvl1_stats *stats);

/* tvl1_calc_batch from per-pair seeds: pair b's seed at u0 / v0 + b*init_pair_stride bytes
 * (a multiple of 4; 0 = one seed for every pair).  Each pair's flow and per-warp iteration
 * counts are those of tvl1_calc_init.  gamma != 0 solves the pairs one by one through
 * tvl1_calc_init's path; in/out flow (u0 == u) then needs init_pair_stride ==
 * flow_pair_stride and init_pitch == flow_pitch. */
tvl1_status tvl1_calc_batch_init(tvl1_ctx *ctx, int32_t n,
                                 const uint8_t *I0, size_t pitch0, size_t pair_stride0,
                                 const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                                 int32_t width, int32_t height,
                                 const float *u0, const float *v0, size_t init_pitch,
                                 size_t init_pair_stride,
                                 float *u, float *v, size_t flow_pitch, size_t flow_pair_stride,
                                 tvl1_stats *stats, void *stream);

/* ---- Feature pre-alignment (features.cpp:46-167, optflow.cpp:366-377) ----
 * find_alignment(frame1, frame0): ORB keypoints and descriptors on the GPU, brute-force
 * Hamming 2-NN + ratio test, RANSAC / LMEDS homography on the host; affine = its top 2x3
 * (maps frame1 coordinates onto frame0), or the identity when <= 10 matches survive the
 * ratio test (outcome 1) or the homography is missing or zooms by more than 20 % (outcome
 * 2).  SURF (features = 2) is served by the ORB path.  Parity with OpenCV unpinned (see
 * fibsem-optflow_amd/csrc/tvl1_align.hpp).  Inputs are device pointers; synchronous. */
typedef struct tvl1_align_params {
  int32_t nfeatures;           /* 5000 features.cpp:22 */
  float scale_factor;          /* 1.2  :23 */
  int32_t nlevels;             /* 8    :24 */
  int32_t edge_threshold;      /* 31   :25 */
  int32_t first_level;         /* 0    :26 */
  int32_t wta_k;               /* 2    :27 (only 2 is supported) */
  int32_t patch_size;          /* 31   :28 (only 31 is supported) */
  int32_t fast_threshold;      /* 20   :29 */
  int32_t blur_for_descriptor; /* 0    :30 */
  float ratio;                 /* 0.8  :109 */
  int32_t method;              /* homo: 8 = RANSAC (default, :133), 4 = LMEDS */
  double ransac_threshold;     /* ransac: 5 (:133) */
} tvl1_align_params;

void tvl1_align_params_default(tvl1_align_params *p);

tvl1_status tvl1_find_alignment(tvl1_ctx *ctx,
                                const uint8_t *frame1, size_t pitch1, int32_t w1, int32_t h1,
                                const uint8_t *frame0, size_t pitch0, int32_t w0, int32_t h0,
                                const tvl1_align_params *params, float affine[6],
                                int32_t *n_good, int32_t *outcome, void *stream);

/* The two stages of tvl1_find_alignment as calls of their own (ABI 7):
 *
 * cv::cuda::ORB::detectAndCompute(frame, noArray(), keypoints, descriptors)
 * (features.cpp:56-61) of one device u8 frame: the keypoints tvl1_find_alignment uses, levels
 * in order, best response first within a level.  kp: 5 floats per keypoint -- x, y (level-0
 * px, cv::KeyPoint::pt), octave (the pyramid level), angle (degrees in [0, 360)), response;
 * desc: 32 bytes per keypoint (rBRIEF, 256 bits, bit j of byte k = test 8k + j).  Host
 * outputs for up to cap keypoints; *n = how many were found (may exceed cap: the first cap
 * are written).  *n can exceed params->nfeatures: the budget is split over the levels by
 * ORB's quota rule, each level's share rounded to an integer and the last level given the
 * remainder if any, so the shares can add up to a few more (16 levels at scale 1.1 and
 * nfeatures 16 give 17; 12 levels at 1.2 and 24 give 25).  Synchronous on stream. */
tvl1_status tvl1_orb_detect(tvl1_ctx *ctx, const uint8_t *frame, size_t pitch, int32_t w,
                            int32_t h, const tvl1_align_params *params, float *kp,
                            uint8_t *desc, int32_t cap, int32_t *n, void *stream);

/* cv::cuda::DescriptorMatcher::createBFMatcher(NORM_HAMMING)->knnMatch(query, train, k = 2)
 * (features.cpp:97-104) on host descriptor lists (32 bytes each), on the GPU: for query i,
 * idx[2i], idx[2i+1] = the nearest and second-nearest train index (ties: the lower index;
 * -1, with distance 2^30, where the train set has no such descriptor), dist[2i], dist[2i+1]
 * = their Hamming distances.  Synchronous on stream. */
tvl1_status tvl1_match_knn2(tvl1_ctx *ctx, const uint8_t *query, int32_t nq,
                            const uint8_t *train, int32_t nt, int32_t *idx, int32_t *dist,
                            void *stream);

/* cv::findHomography(src, dst, method, ransacReprojThreshold) on host point lists
 * (features.cpp:131-133; the model tvl1_find_alignment fits): method 8 = RANSAC, 4 = LMEDS,
 * 0 = all points; a normalised DLT refit on the inliers, then 10 Levenberg-Marquardt steps
 * on their reprojection error.  src / dst: n (x, y) pairs; H: row-major 3x3, H[8] = 1;
 * inlier_mask: n bytes or NULL.  Host only (no GPU work, ctx not needed).  TVL1_EINVAL for
 * n < 4 or a bad method; TVL1_ESIZE when no model is found (all hypotheses degenerate). */
tvl1_status tvl1_find_homography(const float *src_xy, const float *dst_xy, int32_t n,
                                 int32_t method, double ransac_threshold, double H[9],
                                 uint8_t *inlier_mask);

/* cv::cuda::warpAffine(src, dst, M, dsize, INTER_LINEAR, BORDER_CONSTANT, 0) on u8
 * (optflow.cpp:370): dst(x, y) = src(M^-1 (x, y)).  Device pointers, async on stream. */
tvl1_status tvl1_warp_affine_u8(tvl1_ctx *ctx, const uint8_t *src, size_t src_pitch,
                                int32_t sw, int32_t sh, uint8_t *dst, size_t dst_pitch,
                                int32_t dw, int32_t dh, const float affine[6], void *stream);

/* solve_wrapper's features branch with the alignment's affine (optflow.cpp:411-443,
 * 468-473): map = flow + grid, warpAffine(map, M), then flow = map' - grid (flow_output 1)
 * or map' (0), and 0 where I1 <= 1.  Device pointers, async on stream. */
tvl1_status tvl1_postprocess_affine(tvl1_ctx *ctx, float *u, float *v, size_t flow_pitch,
                                    const uint8_t *I1, size_t pitch1, int32_t width,
                                    int32_t height, int32_t flow_output, const float affine[6],
                                    void *stream);

/* ---- Average-flow alignment of a slice list (added under ABI 9; the reference's disabled
 * average_flow / remap_and_save, optflow.cpp:180-226, 263-300; CLI "style": 2) ----
 * For slice i: B = blend6 of slices i-3 .. i+3 without i, flow = tvl1_calc(F_i, B) on the
 * pre-scaled pair, aligned = remap(F_i, flow).  All pointers are device pointers, all pitches
 * bytes, every call asynchronous on `stream`; none touches the solver's scratch.  With
 * profiling on they count into class 2 of the ctx's next solve: whichever solve that is, so
 * a caller that wants a solve's own totals issues these calls on the ctx that solves next.
 * At most 1024 such marks wait for a solve (later ones are dropped), and
 * tvl1_set_profiling(ctx, 0) discards the ones still waiting.
 *
 * The blend's six weights, in neighbour order (i-3, i-2, i-1, i+1, i+2, i+3):
 * float(float(exp(-d^2 / 4)) * s) with s = 0.5 / (exp(-9/4) + exp(-1) + exp(-1/4)) in double
 * (cv::Vec6f times a double).  Their double sum is exactly 1.  Host only, no GPU. */
void tvl1_blend6_weights(float w[6]);

/* dst = saturate_u8(round-half-to-even(sum_k double(w_k) * frames[k])): the six neighbours'
 * weighted mean with a double accumulator (exact: every weight is a multiple of 2^-28), then
 * convertTo(CV_8U).  w x h planes. */
tvl1_status tvl1_blend6_u8(tvl1_ctx *ctx, const uint8_t *const frames[6], const size_t pitches[6],
                           int32_t w, int32_t h, uint8_t *dst, size_t dst_pitch, void *stream);

/* cv::resize of a u8 plane at an exact 1/2 scale: dst = (a + b + c + d + 2) >> 2 over each
 * 2x2 block.  w, h: the SOURCE size, both even (odd: TVL1_EINVAL); dst is w/2 x h/2. */
tvl1_status tvl1_half_u8(tvl1_ctx *ctx, const uint8_t *src, size_t pitch, int32_t w, int32_t h,
                         uint8_t *dst, size_t dst_pitch, void *stream);

/* Warp a frame by a flow field onto a canvas of (w + 2 border) x (h + 2 border): canvas px
 * (X, Y) shows frame coordinate (x, y) = (X - border, Y - border) and samples the frame at
 * (x - U, y - V), where (U, V) is the flow at the nearest frame px: float(double(flow) * gain),
 * the fw x fh planes (u, v) brought to w x h by cv::resize INTER_LINEAR (half-pixel centres)
 * when the sizes differ.  The sample is cv::remap INTER_LINEAR on u8 with BORDER_CONSTANT 0:
 * the map rounded to 1/32 px, four taps, 5-bit weights, each tap outside the frame counting
 * 0; NaN or infinite flow gives 0.  Nothing of the frame's size is staged in memory.
 * TVL1_EINVAL: a null pointer, a pitch below its row, flow_pitch not a multiple of 4,
 * border < 0, fw or fh < 1, dst overlapping frame.  TVL1_ESIZE: w + 2 border or h + 2 border
 * above 32767 (the map's coordinates saturate to short there, as in OpenCV). */
tvl1_status tvl1_remap_flow_u8(tvl1_ctx *ctx, const uint8_t *frame, size_t pitch, int32_t w, int32_t h,
                               const float *u, const float *v, size_t flow_pitch,
                               int32_t fw, int32_t fh, double gain, int32_t border,
                               uint8_t *dst, size_t dst_pitch, void *stream);

/* ---- Integer drift estimate of a frame pair (added under ABI 9) ----
 * The integer translation d = (dx, dy) with I1(x + d) ~= I0(x) (the flow's convention), for
 * seeding tvl1_calc_init when a stage drift lies outside what the unseeded solve captures.
 * Cost of a shift on a level of w x h px: S(d) = sum |I0(x, y) - I1(x + dx, y + dy)| over the
 * overlap, N(d) = (w - |dx|)(h - |dy|) px; a is better than b iff S_a N_b < S_b N_a (the mean
 * absolute differences, compared exactly in 64-bit integers), then the smaller dx^2 + dy^2,
 * then dy, then dx.  Pyramid: L = the smallest integer with ceil(R / 2^L) <= 4, R = max_shift;
 * each level is the one before, cropped to even sizes, under tvl1_half_u8's 2x2 mean.  Search:
 * every shift of [-R_L, R_L]^2 on level L, R_l = ceil(R / 2^l); 2 d_(l+1) + {-1, 0, 1}^2 within
 * R_l on level l < L; level 0 also tries (0, 0).  No float anywhere: any profile, any
 * arithmetic mode.  A true shift outside max_shift returns some in-range shift whose mean
 * difference is barely below (0, 0)'s: compare sad / count with sad_zero / count_zero. */
typedef struct tvl1_shift {
  int32_t dx, dy, levels, reserved;   /* levels = L + 1 */
  uint64_t sad, count;                /* S and N of the result at level 0 */
  uint64_t sad_zero, count_zero;      /* S and N of (0, 0) at level 0 */
} tvl1_shift;

/* I0, I1: device u8 frames of w x h (ROI views allowed: any pointer, any pitch >= w); out: one
 * HOST record.  1 <= max_shift <= 128 and 4 max_shift <= min(w, h), else TVL1_EINVAL; w h >
 * 2^26 is TVL1_ESIZE.  The whole search is enqueued on `stream` without a host round trip; the
 * call returns once the record has arrived (it synchronizes the stream). */
tvl1_status tvl1_estimate_shift(tvl1_ctx *ctx, const uint8_t *I0, size_t pitch0,
                                const uint8_t *I1, size_t pitch1, int32_t w, int32_t h,
                                int32_t max_shift, tvl1_shift *out, void *stream);

/* n pairs of one size, laid out as tvl1_calc_batch's (pair b at I0 + b*pair_stride0, I1 +
 * b*pair_stride1 bytes; 0 = the same frame for every pair); out: n HOST records, each equal to
 * tvl1_estimate_shift's of that pair.  Up to 256 pairs share every launch. */
tvl1_status tvl1_estimate_shift_batch(tvl1_ctx *ctx, int32_t n, const uint8_t *I0, size_t pitch0,
                                      size_t pair_stride0, const uint8_t *I1, size_t pitch1,
                                      size_t pair_stride1, int32_t w, int32_t h,
                                      int32_t max_shift, tvl1_shift *out, void *stream);

/* ---- Batched solves seeded by one constant per pair (added under ABI 9) ----
 * tvl1_calc_batch whose pair b starts from the flow (dx_b, dy_b) everywhere: its flow and
 * per-warp iteration counts are those of tvl1_calc_init from two planes filled with (dx_b,
 * dy_b) (bit-identical, as tvl1_calc_batch_init's), but no such plane is stored or read: the
 * first step of the seed's pyramid is evaluated from the constant, per px (its bilinear
 * weights are rounded, so a level of that pyramid is not one value).  seed_xy: HOST, 2 n
 * floats (dx_0, dy_0, dx_1, ...), copied before the call returns.  NULL seed_xy, a value that
 * is not finite, or a ctx with profile = 1 is TVL1_EINVAL before anything is launched.
 * gamma != 0 solves the pairs one by one through tvl1_calc_init's path (the constant is
 * then written out as planes in scratch of one pair's size). */
tvl1_status tvl1_calc_batch_const_init(tvl1_ctx *ctx, int32_t n,
                                       const uint8_t *I0, size_t pitch0, size_t pair_stride0,
                                       const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                                       int32_t width, int32_t height, const float *seed_xy,
                                       float *u, float *v, size_t flow_pitch,
                                       size_t flow_pair_stride, tvl1_stats *stats, void *stream);

/* tvl1_estimate_shift_batch and tvl1_calc_batch_const_init in one call, the seeds handed over
 * on the device: shifts[b] (HOST, n records) is tvl1_estimate_shift of pair b, and pair b's
 * flow is tvl1_calc_batch_const_init's with ((float)dx_b, (float)dy_b).  The argument checks
 * of tvl1_estimate_shift_batch apply first and unchanged (max_shift, 4 max_shift <= min(w, h),
 * w h <= 2^26), then tvl1_calc_batch's; nothing is launched after an error.  The estimate is
 * enqueued ahead of the solve with no host wait between them; the records are on the host
 * when the call returns (it synchronizes the stream once the solve is enqueued). */
tvl1_status tvl1_calc_batch_auto_init(tvl1_ctx *ctx, int32_t n,
                                      const uint8_t *I0, size_t pitch0, size_t pair_stride0,
                                      const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                                      int32_t width, int32_t height, int32_t max_shift,
                                      tvl1_shift *shifts,
                                      float *u, float *v, size_t flow_pitch,
                                      size_t flow_pair_stride, tvl1_stats *stats, void *stream);

/* The estimate's cost kernel as a call of its own: sad[(dy + r) (2r + 1) + (dx + r)] =
 * S(cx + dx, cy + dy) for dx, dy in [-r, r], r = radius in 1 .. 4 (else TVL1_EINVAL), on one
 * level (no pyramid).  A shift whose overlap is empty reports 0.  sad: (2r + 1)^2 HOST values;
 * synchronous on stream. */
tvl1_status tvl1_sad_shifts_u8(tvl1_ctx *ctx, const uint8_t *I0, size_t pitch0, const uint8_t *I1,
                               size_t pitch1, int32_t w, int32_t h, int32_t cx, int32_t cy,
                               int32_t radius, uint64_t *sad, void *stream);

/* Same on HOST memory: upload, solve, download, synchronize.
 * (GpuMat::upload optflow.cpp:315-316 ... download :475-476) */
tvl1_status tvl1_calc_host(tvl1_ctx *ctx,
                           const uint8_t *I0, size_t pitch0,
                           const uint8_t *I1, size_t pitch1,
                           int32_t width, int32_t height,
                           float *u, float *v, size_t flow_pitch,
                           tvl1_stats *stats);

/* Output post-processing of solve_wrapper (optflow.cpp:411-473), in place on
 * device u, v:  mode 0 = "flow" (unchanged), 1 = "map" (u += x, v += y),
 * 2 = features branch with output_type "flow" under an identity alignment
 * (u = (u + x) - x, optflow.cpp:429-437); then u = v = 0 wherever I1 <= 1
 * (cuda::threshold THRESH_BINARY_INV + setTo). */
tvl1_status tvl1_postprocess(tvl1_ctx *ctx, float *u, float *v, size_t flow_pitch,
                             const uint8_t *I1, size_t pitch1,
                             int32_t width, int32_t height, int32_t mode, void *stream);

/* tvl1_postprocess on n same-size pairs of a batch in one launch (ABI 8; the CLI's batched
 * strip jobs, solve_wrapper optflow.cpp:411-473 per ROI): pair b's flow at u / v +
 * b*flow_pair_stride, its frame1 at I1 + b*pair_stride1 (bytes).  Device pointers, async. */
tvl1_status tvl1_postprocess_batch(tvl1_ctx *ctx, int32_t n, float *u, float *v,
                                   size_t flow_pitch, size_t flow_pair_stride,
                                   const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                                   int32_t width, int32_t height, int32_t mode, void *stream);

/* The flow values of a few chosen px (ABI 8; plane_elems since ABI 9): out_u[i] =
 * u[offsets[i]], out_v[i] = v[offsets[i]], offsets in floats from the device pointers u / v
 * (host array of n).  Every offset must lie in [0, plane_elems), the number of floats
 * addressable from u and from v (for a batch: pairs x pair stride); any other offset is
 * TVL1_EINVAL before anything is launched.  The point-match output draws npoints px per ROI
 * (random_points, optflow.cpp:522-572) and needs only their flow, not the whole field.
 * Host outputs; synchronous on stream. */
tvl1_status tvl1_gather_flow(tvl1_ctx *ctx, const float *u, const float *v, int64_t plane_elems,
                             const int64_t *offsets, int32_t n, float *out_u, float *out_v,
                             void *stream);

/* ---- Forward-backward consistency score (added under ABI 9) ----
 * Given the forward flow (uf, vf) of a pair I0 -> I1 and the backward flow (ub, vb) of I1 -> I0
 * (the same solve with the frames swapped), a px (x, y) follows its forward flow, reads the
 * backward flow where it lands and scores how far the two are from cancelling.  Per px, every
 * operation one IEEE f32 rounding in this order, never contracted, whatever the ctx's fast_math
 * or profile:
 *   X = float(x) + uf, Y = float(y) + vf;
 *   unless 0 <= X <= float(w - 1) and 0 <= Y <= float(h - 1) (false for NaN): score = +inf;
 *   x0 = int(floorf(X)), ax = X - float(x0), x1 = min(x0 + 1, w - 1); y0, ay, y1 likewise;
 *   for P = ub, vb:  t = P[y0][x0] + ax * (P[y0][x1] - P[y0][x0]),
 *                    b = P[y1][x0] + ax * (P[y1][x1] - P[y1][x0]),  s = t + ay * (b - t);
 *   ex = uf + ubs, ey = vf + vbs, err = ex * ex + ey * ey;
 *   mag = (uf * uf + vf * vf) + (ubs * ubs + vbs * vbs);  score = err - alpha * mag.
 * A px is consistent at beta iff score <= beta (NaN and +inf are not): the usual
 * |f + b(x + f)|^2 <= alpha (|f|^2 + |b(x + f)|^2) + beta with the threshold kept out of the
 * plane, so one score plane serves any beta and can be gathered at points (tvl1_gather_flow).
 *
 * All planes are device f32, w x h, ROI views allowed: any pointer and any pitch that are
 * multiples of 4.  Pair b's planes lie at base + b * pair stride (bytes); up to 256 pairs share
 * a launch, a larger n is chunked.  Asynchronous on `stream`; no solver scratch is touched; with
 * profiling on the calls count into class 2 of the ctx's next solve, as the slice-list calls do.
 * TVL1_EINVAL before anything is launched: a null plane, n < 1, w or h < 1, a pitch below 4 w or
 * not a multiple of 4, a pair stride that is not a multiple of 4 or (n > 1) does not cover one
 * plane, NaN alpha or beta, score overlapping a flow plane, ub / vb overlapping uf / vf (overlap
 * is judged on each plane's whole span over the n pairs).  TVL1_ESIZE: w or h above 2^24, where
 * float(x) is no longer exact. */
tvl1_status tvl1_fb_score_batch(tvl1_ctx *ctx, int32_t n,
                                const float *uf, const float *vf, size_t f_pitch, size_t f_pair_stride,
                                const float *ub, const float *vb, size_t b_pitch, size_t b_pair_stride,
                                int32_t w, int32_t h, float alpha,
                                float *score, size_t score_pitch, size_t score_pair_stride,
                                void *stream);

/* tvl1_fb_score_batch with n = 1. */
tvl1_status tvl1_fb_score(tvl1_ctx *ctx, const float *uf, const float *vf, size_t f_pitch,
                          const float *ub, const float *vb, size_t b_pitch, int32_t w, int32_t h,
                          float alpha, float *score, size_t score_pitch, void *stream);

/* u = v = 0 wherever !(score <= beta), in place: the I1 <= 1 mask's sibling, to run where that
 * mask runs (after tvl1_postprocess, so a rejected px is 0 in "map" output too).  rejected: NULL,
 * or n HOST values, the number of such px of each pair; the call then returns after the counts
 * have arrived (it synchronizes the stream).  The per-pair counters live in a ctx block of their
 * own. */
tvl1_status tvl1_zero_above_batch(tvl1_ctx *ctx, int32_t n,
                                  float *u, float *v, size_t flow_pitch, size_t flow_pair_stride,
                                  const float *score, size_t score_pitch, size_t score_pair_stride,
                                  int32_t w, int32_t h, float beta, uint64_t *rejected,
                                  void *stream);

/* tvl1_zero_above_batch with n = 1. */
tvl1_status tvl1_zero_above(tvl1_ctx *ctx, float *u, float *v, size_t flow_pitch,
                            const float *score, size_t score_pitch, int32_t w, int32_t h,
                            float beta, uint64_t *rejected, void *stream);

/* ---- Photometric (ZNCC) score of a flow (added under ABI 9) ----
 * Given the two u8 frames of a pair and its forward flow (u, v), I1(x + u, y + v) ~ I0(x, y),
 * frame1 is warped back along the flow and every px is scored by the zero-mean normalised
 * cross-correlation of a (2 radius + 1)^2 window of frame0 against the warped frame1, in one
 * pass and without a second solve.  Lower is better: score = 1 - ZNCC, so tvl1_zero_above and
 * the candidate rule of the forward-backward score apply as they are.
 *
 * Step 1, the warped frame J and its validity m.  Per px, every float operation one IEEE f32
 * rounding, never contracted:
 *   mx = float(x) + u, my = float(y) + v;
 *   m = mx >= 0 && mx <= float(w - 1) && my >= 0 && my <= float(h - 1)   (false for NaN);
 *   where !m nothing is converted and no tap is read; where m:
 *   ix = rint(mx * 32) (half to even), sx = ix >> 5, fx = ix & 31, x1 = min(sx + 1, w - 1);
 *   iy, sy, fy, y1 likewise;  s00 = I1[sy][sx], s01 = I1[sy][x1], s10 = I1[y1][sx], s11 = I1[y1][x1];
 *   J = (s00 (32 - fx)(32 - fy) + s01 fx (32 - fy) + s10 (32 - fx) fy + s11 fx fy + 512) >> 10
 *   (sx = w - 1 implies fx = 0: the clamped tap carries weight 0).
 * Step 2, over the window {(x + i, y + j) : |i|, |j| <= radius} cut to the frame and to px with
 * m, in integers: n = its px, Sa = sum I0, Sb = sum J, Saa = sum I0^2, Sbb = sum J^2, Sab = sum
 * I0 J;  A = n Sab - Sa Sb, B = n Saa - Sa^2, C = n Sbb - Sb^2 (all below 2^29 for n <= 81).
 * Step 3: score = +inf where the centre px has !m, or B == 0, or C == 0 (a flat window on either
 * side is no evidence); otherwise score = float(1.0 - double(A) / sqrt(double(B) * double(C))):
 * four IEEE f64 operations and one conversion, each rounded once whatever the ctx's fast_math
 * or profile.  Identical windows score exactly 0, J = 255 - I0 scores exactly 2; a px is
 * accepted at beta iff score <= beta, that is ZNCC >= 1 - beta.
 *
 * All pointers are device pointers, pitches and pair strides in bytes.  The frames may be ROI
 * views of any pointer and any pitch >= w; the f32 planes of any pointer and pitch that are
 * multiples of 4.  Pair b's planes lie at base + b * pair stride; a frame pair stride 0 is one
 * frame shared by every pair, as in tvl1_calc_batch.  Up to 256 pairs share a launch, a larger n
 * is chunked.  Nothing outside a row's w px or a plane's h rows is read or written.
 * Asynchronous on `stream`; no solver scratch is touched; with profiling on each call is one
 * class-2 mark of the ctx's next solve.
 * TVL1_EINVAL before anything is launched: a null plane, n < 1, w or h < 1, radius outside 1..4,
 * a frame pitch below w, a flow or score pitch below 4 w or not a multiple of 4, an f32 pair
 * stride that is not a multiple of 4, a pair stride (other than a frame's 0) that for n > 1 does
 * not cover one plane, score overlapping any input (judged on each plane's whole span over the
 * n pairs).  TVL1_ESIZE: w or h above 2^19 (below that mx * 32 is an exact integer under 2^24). */
tvl1_status tvl1_zncc_score_batch(tvl1_ctx *ctx, int32_t n,
                                  const uint8_t *I0, size_t pitch0, size_t pair_stride0,
                                  const uint8_t *I1, size_t pitch1, size_t pair_stride1,
                                  const float *u, const float *v, size_t flow_pitch, size_t flow_pair_stride,
                                  int32_t w, int32_t h, int32_t radius,
                                  float *score, size_t score_pitch, size_t score_pair_stride,
                                  void *stream);

/* tvl1_zncc_score_batch with n = 1. */
tvl1_status tvl1_zncc_score(tvl1_ctx *ctx, const uint8_t *I0, size_t pitch0,
                            const uint8_t *I1, size_t pitch1,
                            const float *u, const float *v, size_t flow_pitch,
                            int32_t w, int32_t h, int32_t radius,
                            float *score, size_t score_pitch, void *stream);

/* Step 1 as a call of its own: dst = J where m and 0 elsewhere (what frame1 looks like warped
 * onto frame0), and, where `valid` is not NULL, m as a 0/1 u8 plane.  The sample is the score's
 * own.  TVL1_EINVAL: a null plane (but `valid`), w or h < 1, a u8 pitch below w, a flow pitch
 * below 4 w or not a multiple of 4, dst or valid overlapping an input or each other.
 * TVL1_ESIZE as above. */
tvl1_status tvl1_warp_by_flow_u8(tvl1_ctx *ctx, const uint8_t *I1, size_t pitch1,
                                 const float *u, const float *v, size_t flow_pitch,
                                 int32_t w, int32_t h, uint8_t *dst, size_t dst_pitch,
                                 uint8_t *valid /* or NULL */, size_t valid_pitch, void *stream);

/* ---- Flow composition (added under ABI 9) ----
 * Given the flow a = (ua, va) of a pair A -> B and the flow b = (ub, vb) of B -> C, a px follows
 * a, reads b where it lands and adds the two: c(x) = a(x) + b(x + a(x)) is the flow A -> C.
 * Chained over the short links that connect two distant slices, it is a dense, sub-pixel seed for
 * their solve (tvl1_calc_init).  Per px, every float operation one IEEE f32 rounding in this
 * order, never contracted, whatever the ctx's fast_math or profile:
 *   X = float(x) + ua, Y = float(y) + va;
 *   inside = X >= 0 && X <= float(w - 1) && Y >= 0 && Y <= float(h - 1)   (false for NaN);
 *   Xc = X >= 0 ? (X <= float(w - 1) ? X : float(w - 1)) : 0   (NaN and -inf give 0, +inf gives
 *   w - 1), Yc likewise: no tap is ever read outside the plane, whatever the input;
 *   x0 = int(floorf(Xc)), ax = Xc - float(x0), x1 = min(x0 + 1, w - 1); y0, ay, y1 likewise;
 *   for P = ub, vb:  t = P[y0][x0] + ax * (P[y0][x1] - P[y0][x0]),
 *                    b = P[y1][x0] + ax * (P[y1][x1] - P[y1][x0]),  s = t + ay * (b - t);
 *   uc = ua + ubs, vc = va + vbs.
 * A NaN or an infinity in a or b propagates into c; it never becomes an address.
 * outside: NULL, or n HOST values, the number of px of each pair with !inside (clamped to the
 * frame's edge before b is read); the call then returns after the counts have arrived (it
 * synchronizes the stream).  The per-pair counters live in a ctx block of their own.
 *
 * All planes are device f32, w x h, ROI views allowed: any pointer and any pitch that are
 * multiples of 4.  Pair b's planes lie at base + b * pair stride (bytes); up to 256 pairs share
 * a launch, a larger n is chunked.  Asynchronous on `stream` (but for `outside`); no solver
 * scratch is touched; with profiling on each call is one class-2 mark of the ctx's next solve.
 * c may be a exactly (the same pointers, pitch and pair stride: a px reads its own a and nobody
 * else's, which is what a chain accumulates into).
 * TVL1_EINVAL before anything is launched: a null plane, n < 1, w or h < 1, a pitch below 4 w or
 * not a multiple of 4, a pair stride that is not a multiple of 4 or (n > 1) does not cover one
 * plane, uc / vc overlapping ub / vb, uc / vc overlapping ua / va in any way other than c being a
 * exactly (overlap is judged on each plane's whole span over the n pairs).  TVL1_ESIZE: w or h
 * above 2^24, where float(x) is no longer exact. */
tvl1_status tvl1_compose_flow_batch(tvl1_ctx *ctx, int32_t n,
                                    const float *ua, const float *va, size_t a_pitch, size_t a_pair_stride,
                                    const float *ub, const float *vb, size_t b_pitch, size_t b_pair_stride,
                                    int32_t w, int32_t h,
                                    float *uc, float *vc, size_t c_pitch, size_t c_pair_stride,
                                    uint64_t *outside, void *stream);

/* tvl1_compose_flow_batch with n = 1. */
tvl1_status tvl1_compose_flow(tvl1_ctx *ctx, const float *ua, const float *va, size_t a_pitch,
                              const float *ub, const float *vb, size_t b_pitch, int32_t w, int32_t h,
                              float *uc, float *vc, size_t c_pitch, uint64_t *outside, void *stream);

/* ---- Flow inversion (added under ABI 9) ----
 * Given the flow f = (uf, vf) of a pair A -> B, the flow g = (ug, vg) of B -> A on B's grid: the
 * fixed point of g(y) = -f(y + g(y)), started at -f(y) and iterated `iterations` (K) times.  It
 * seeds a solve in the opposite direction to the flows that exist (a reverse pair, or the
 * backward solve of a consistency check) where the negation -f is wrong by about |grad f| |f|.
 * Per px (x, y), every float operation one IEEE f32 rounding in this order, never contracted,
 * whatever the ctx's fast_math or profile:
 *   g_0 = (-uf[y][x], -vf[y][x]);
 *   for k = 0 .. K - 1:
 *     X = float(x) + ug_k, Y = float(y) + vg_k;
 *     Xc = X >= 0 ? (X <= float(w - 1) ? X : float(w - 1)) : 0   (NaN and -inf give 0, +inf gives
 *     w - 1), Yc likewise: no tap is ever read outside the plane, whatever the input;
 *     x0 = int(floorf(Xc)), ax = Xc - float(x0), x1 = min(x0 + 1, w - 1); y0, ay, y1 likewise;
 *     for P = uf, vf:  t = P[y0][x0] + ax * (P[y0][x1] - P[y0][x0]),
 *                      b = P[y1][x0] + ax * (P[y1][x1] - P[y1][x0]),  s = t + ay * (b - t);
 *     g_{k+1} = (-us, -vs);
 *   one more sample (us, vs) at g_K in the same way, with
 *     inside = X >= 0 && X <= float(w - 1) && Y >= 0 && Y <= float(h - 1)   (false for NaN);
 *     ex = ug_K + us, ey = vg_K + vs, resid = ex * ex + ey * ey;
 *   ug = ug_K, vg = vg_K.
 * A NaN or an infinity in f propagates into g; it never becomes an address.
 * resid: NULL, or a score-shaped plane (px^2; tvl1_zero_above and tvl1_gather_flow apply to it
 * as they are) of how far g is from a fixed point: where f folds, the iteration does not converge.
 * counts: NULL, or n HOST records: outside, the px of each pair with !inside at the last landing;
 * unconverged, the px with !(resid <= tol) (NaN counts).  The call then returns after the counts
 * have arrived (it synchronizes the stream).  The per-pair counters live in a ctx block of their
 * own.
 *
 * All planes are device f32, w x h, ROI views allowed: any pointer and any pitch that are
 * multiples of 4.  Pair b's planes lie at base + b * pair stride (bytes); up to 256 pairs share
 * a launch, a larger n is chunked.  Asynchronous on `stream` (but for `counts`); no solver
 * scratch is touched; with profiling on each call is one class-2 mark of the ctx's next solve.
 * Nothing runs in place: a px reads f at other px.
 * TVL1_EINVAL before anything is launched: a null plane (but resid), n < 1, w or h < 1, a pitch
 * below 4 w or not a multiple of 4, a pair stride that is not a multiple of 4 or (n > 1) does not
 * cover one plane, iterations outside 1..32, a NaN tol, ug / vg / resid overlapping uf / vf or
 * each other (overlap is judged on each plane's whole span over the n pairs).  TVL1_ESIZE: w or
 * h above 2^24, where float(x) is no longer exact. */
typedef struct {
    uint64_t outside, unconverged;
} tvl1_invert_counts;

tvl1_status tvl1_invert_flow_batch(tvl1_ctx *ctx, int32_t n,
                                   const float *uf, const float *vf, size_t f_pitch, size_t f_pair_stride,
                                   int32_t iterations, float tol,
                                   float *ug, float *vg, size_t g_pitch, size_t g_pair_stride,
                                   float *resid /* or NULL */, size_t resid_pitch, size_t resid_pair_stride,
                                   int32_t w, int32_t h,
                                   tvl1_invert_counts *counts /* HOST, n records, or NULL */, void *stream);

/* tvl1_invert_flow_batch with n = 1. */
tvl1_status tvl1_invert_flow(tvl1_ctx *ctx, const float *uf, const float *vf, size_t f_pitch,
                             int32_t iterations, float tol,
                             float *ug, float *vg, size_t g_pitch,
                             float *resid /* or NULL */, size_t resid_pitch,
                             int32_t w, int32_t h, tvl1_invert_counts *counts, void *stream);

/* The ctx's own non-blocking HIP stream (hipStream_t as void*): callers that keep
 * several pairs in flight on one device give each ctx its own stream this way. */
void *tvl1_stream(tvl1_ctx *ctx);

/* Enable (1) / disable (0) per-kernel-class HIP-event timing into tvl1_stats. */
tvl1_status tvl1_set_profiling(tvl1_ctx *ctx, int32_t enable);

/* Destroy a ctx and free its device scratch. */
void tvl1_destroy(tvl1_ctx *ctx);

/* Last error message of ctx (or of the last failed tvl1_create when ctx==NULL). */
const char *tvl1_last_error(const tvl1_ctx *ctx);

/* ABI version (TVL1_ABI_VERSION) — lets an FFI binding check what it loaded. */
int32_t tvl1_abi_version(void);

/* Number of visible HIP devices (0 when no GPU); never initialises a context. */
int32_t tvl1_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* FIBSEM_OPTFLOW_AMD_TVL1_H */
