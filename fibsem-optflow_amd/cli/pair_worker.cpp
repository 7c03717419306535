// pair_worker.cpp — the per-pair path of a style 1 job: a worker takes chunks of pairs, loads
// (and reuses) their slices, and solves each pair's ROIs one by one.
//
//   PairWorker      the pair loop of from_file (optflow.cpp:75-178 of the reference): p / q /
//                   scale, frame reuse, ROIs, output naming, retry on a rebuilt context
//   solve_rois      optflow.cpp:312-392  upload, features flag, sorted ROI loop
//   align_frame1    optflow.cpp:366-377  find_alignment + warpAffine
//   solve_wrapper   optflow.cpp:395-496  TVL1 solve + map/flow/mask + TIFF output
#include <cstring>

#include "job.hpp"
#include "points.hpp"

namespace ofcli {
namespace {

// two planes of `count` px filled with the constants (dx, dy): the seed is the flow buffers'
// own content (tvl1_calc_init's in/out flow)
bool fill_seed(DeviceCtx &dc, float *u, float *v, float dx, float dy, size_t count, std::string &err) {
  uint32_t bx, by;
  memcpy(&bx, &dx, 4);
  memcpy(&by, &dy, 4);
  if (hipMemsetD32Async((hipDeviceptr_t)u, (int)bx, count, dc.stream) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)v, (int)by, count, dc.stream) != hipSuccess)
    return dc.hip_error("initial flow fill failed", err);
  return true;
}

// One ROI's solve from I0 to I1 into (u, v), from the constant seed when there is one
struct RoiViews {
  const uint8_t *a, *b;   // frame0's and frame1's ROI on the device
  size_t pitch0, pitch1;
  int W, H;
  size_t fp;   // the flow planes' pitch in bytes
};
// false: err and dc.faulted say why
bool solve_seeded(DeviceCtx &dc, const uint8_t *I0, size_t p0, const uint8_t *I1, size_t p1, const RoiViews &r,
                  const InitFlow &seed, float sign, float *u, float *v, tvl1_stats *st, std::string &err) {
  if (!seed.on) return !dc.failed(tvl1_calc(dc.ctx, I0, p0, I1, p1, r.W, r.H, u, v, r.fp, st, dc.stream), err);
  // a chain's seed is in (u, v) already (load_chain)
  if (!seed.chained() && !fill_seed(dc, u, v, sign * seed.dx, sign * seed.dy, (size_t)r.W * r.H, err)) return false;
  return !dc.failed(tvl1_calc_init(dc.ctx, I0, p0, I1, p1, r.W, r.H, u, v, r.fp, u, v, r.fp, st, dc.stream), err);
}

// "initialFlow": {"chain": [...]}: the links' flow files of this ROI key, composed left to right
// on the device, in place on (dc.du, dc.dv); a link waits in (dc.dub, dc.dvb) while it is composed.
// A link that is missing, unreadable or of another size fails the pair with its file's name.
bool load_chain(DeviceCtx &dc, const Value &im, InitFlow &init, const RoiViews &r, std::string &err) {
  const std::string suffix = im["output_suffix"].asString();
  const size_t bytes = (size_t)r.W * r.H * sizeof(float);
  init.outside.clear();
  for (size_t k = 0; k < init.chain.size(); ++k) {
    float *dst[2] = {k ? dc.dub.f32() : dc.du.f32(), k ? dc.dvb.f32() : dc.dv.f32()};
    const char *axis[2] = {"_x.tiff", "_y.tiff"};
    for (int c = 0; c < 2; ++c) {
      const std::string path = init.chain[k] + suffix + axis[c];
      ofio::HostVec<float> plane;
      int w = 0, h = 0;
      std::string e;
      if (!ofio::read_tiff_f32(path, w, h, plane, e)) {
        err = "initialFlow chain, link " + std::to_string(k) + ": " + e;
        return false;
      }
      if (w != r.W || h != r.H) {
        err = "initialFlow chain, link " + std::to_string(k) + ": " + path + " is " + std::to_string(w) + "x" +
              std::to_string(h) + ", the ROI is " + std::to_string(r.W) + "x" + std::to_string(r.H);
        return false;
      }
      // the host plane goes back to its pool below: the copy is waited for
      if (hipMemcpyAsync(dst[c], plane.data(), bytes, hipMemcpyHostToDevice, dc.stream) != hipSuccess ||
          hipStreamSynchronize(dc.stream) != hipSuccess)
        return dc.hip_error("upload of a chain link failed", err);
    }
    if (!k) continue;
    uint64_t outside = 0;
    if (dc.failed(tvl1_compose_flow(dc.ctx, dc.du.f32(), dc.dv.f32(), r.fp, dst[0], dst[1], r.fp, r.W, r.H,
                                    dc.du.f32(), dc.dv.f32(), r.fp, &outside, dc.stream),
                  err, "initialFlow chain: "))
      return false;
    init.outside.push_back(outside);
  }
  return true;
}

// The chain's inverse (tvl1_invert_flow), where the config asks for one.  The composed
// chain c is in (dc.du, dc.dv); its inverse g goes to (dc.dub, dc.dvb), nothing runs in place.
//   "inverse": the forward seed is g: copied over c, or, when the backward solve of a
//     consistency check is seeded too, exchanged with c through dc.dsc (its seed is c itself);
//   "backward": "inverse" alone: c stays the forward seed and g waits in (dub, dvb), where the
//     backward solve runs in place.
bool invert_chain(DeviceCtx &dc, InitFlow &init, const RoiViews &r, bool seed_backward, std::string &err) {
  init.inverted = false;
  if (!init.inverse && !seed_backward) return true;
  const size_t bytes = (size_t)r.W * r.H * sizeof(float);
  if (dc.failed(tvl1_invert_flow(dc.ctx, dc.du.f32(), dc.dv.f32(), r.fp, init.inverse_iterations,
                                 init.inverse_tolerance, dc.dub.f32(), dc.dvb.f32(), r.fp, nullptr, 0, r.W, r.H,
                                 &init.inverse_counts, dc.stream),
                err, "initialFlow chain, inverse: "))
    return false;
  init.inverted = true;
  if (!init.inverse) return true;
  const auto copy = [&](float *dst, const float *src) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, dc.stream) == hipSuccess;
  };
  bool ok = true;
  float *fwd[2] = {dc.du.f32(), dc.dv.f32()}, *bwd[2] = {dc.dub.f32(), dc.dvb.f32()};
  for (int c = 0; c < 2 && ok; ++c) {
    if (seed_backward) ok = copy(dc.dsc.f32(), fwd[c]) && copy(fwd[c], bwd[c]) && copy(bwd[c], dc.dsc.f32());
    else ok = copy(fwd[c], bwd[c]);
  }
  return ok || dc.hip_error("copy of the inverted chain failed", err);
}

// random_points without the debug flag (points.hpp's sample_points): only the chosen px's flow
// (and a checked pair's score) crosses PCIe (tvl1_gather_flow: one upload, one gather, one
// download), synchronous.  Debug runs keep the exact shuffle so their output is reproducible.
bool random_points_sampled(DeviceCtx &dc, const RoiViews &v, const ofio::Image8 &f0, const ofio::Image8 &f1,
                           const Rect &r0, const Rect &r1, Value &im, const PairConfig &cfg, bool features,
                           PointCount &count, std::string &err) {
  uint64_t total = 0;
  Points pts = sample_points([&](int y) { return f0.row(r0.y + y) + r0.x; },
                             [&](int y) { return f1.row(r1.y + y) + r1.x; }, v.W, v.H, draw_count(cfg), &total);
  std::vector<float> vx(pts.size()), vy(pts.size()), sc, sc2;
  std::vector<int64_t> off(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) off[i] = (int64_t)(pts[i].second * (v.fp / 4) + pts[i].first);
  const int64_t plane = (int64_t)((size_t)(v.H - 1) * (v.fp / 4) + v.W);
  if (dc.failed(tvl1_gather_flow(dc.ctx, dc.du.f32(), dc.dv.f32(), plane, off.data(), (int32_t)off.size(), vx.data(),
                                 vy.data(), dc.stream),
                err, "flow read-back failed: "))
    return false;
  if (cfg.check.on) {   // the candidates' score: the same gather with the score plane as both planes
    sc.resize(pts.size()), sc2.resize(pts.size());
    if (dc.failed(tvl1_gather_flow(dc.ctx, dc.dsc.f32(), dc.dsc.f32(), plane, off.data(), (int32_t)off.size(),
                                   sc.data(), sc2.data(), dc.stream),
                  err, "score read-back failed: "))
      return false;
  }
  const float inv_scale = 1. / cfg.scale;
  count = report_points(std::move(pts), std::move(vx), std::move(vy), sc, cfg, total > 0, im, r0, r1, inv_scale,
                        features);
  return true;
}

// the solved ROI's planes on the host: points of the exact shuffle, then the TIFF outputs
bool download_and_write(DeviceCtx &dc, const RoiViews &v, const ofio::Image8 &f0, const ofio::Image8 &f1,
                        const Rect &r0, const Rect &r1, Value &im, const PairConfig &cfg, bool features,
                        const std::function<void(const PointCount *)> &record, std::string &err) {
  const int W = v.W, H = v.H;
  const FlowCheck &check = cfg.check;
  ofio::HostVec<float> fx((size_t)W * H), fy((size_t)W * H);   // pinned (PinnedPool)
  if (hipMemcpyAsync(fx.data(), dc.du.p, fx.size() * 4, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
      hipMemcpyAsync(fy.data(), dc.dv.p, fy.size() * 4, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
      hipStreamSynchronize(dc.stream) != hipSuccess)
    return dc.hip_error("flow download failed", err);
  // the score plane: the exact shuffle's candidates read it, the check's "...Output" writes it
  ofio::HostVec<float> fs(check.on && (check.output || cfg.random_points()) ? (size_t)W * H : 0);
  if (fs.size() && (hipMemcpyAsync(fs.data(), dc.dsc.p, fs.size() * 4, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
                    hipStreamSynchronize(dc.stream) != hipSuccess))
    return dc.hip_error("score download failed", err);
  if (!check.on) record(nullptr);
  PointCount count;
  if (cfg.random_points()) {
    // mask = (frame0 > 1) | (frame1 > 1) on the ROIs (optflow.cpp:486-494)
    std::vector<uint8_t> mask((size_t)W * H);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        mask[(size_t)y * W + x] = (f0.row(r0.y + y)[r0.x + x] > 1) | (f1.row(r1.y + y)[r1.x + x] > 1);
    count = random_points(fx.data(), fy.data(), fs.data(), W, H, im, cfg, r0, r1, mask, features);
  }
  if (check.on) record(cfg.random_points() ? &count : nullptr);   // with the candidates and the kept points
  const std::string base = im["output"].asString() + im["output_suffix"].asString();
  std::string e;
  if (((cfg.otype == "map" || cfg.otype == "flow") &&
       (!ofio::write_tiff_f32(base + "_x.tiff", fx.data(), W, H, v.fp, e) ||
        !ofio::write_tiff_f32(base + "_y.tiff", fy.data(), W, H, v.fp, e))) ||
      (check.on && check.output && !ofio::write_tiff_f32(base + check_suffix(check), fs.data(), W, H, v.fp, e))) {
    err = e;
    return false;
  }
  return true;
}

// solve_wrapper (optflow.cpp:395-496) for one ROI.
bool solve_wrapper(DeviceCtx &dc, const ofio::Image8 &f0, const ofio::Image8 &f1, const Rect &r0, const Rect &r1,
                   Value &im, const PairConfig &cfg, bool features, const float *affine, PairResult &res,
                   std::string &err) {
  const FlowCheck &check = cfg.check;
  if (cfg.check_error) {
    err = cfg.check_error;
    return false;
  }
  if (check.on && features) {
    err = check_features_error(check);
    return false;
  }
  if (dc.failed(tvl1_set_params(dc.ctx, &cfg.tv), err)) return false;
  // device frames are packed, pitch = width
  const RoiViews v{dc.d0.u8() + (size_t)r0.y * f0.width + r0.x, dc.d1.u8() + (size_t)r1.y * f1.width + r1.x,
                   (size_t)f0.width, (size_t)f1.width, r0.width, r0.height, (size_t)r0.width * sizeof(float)};
  const int W = v.W, H = v.H;
  // "initialFlow": "auto": the ROI's integer drift, on the views the solve sees
  InitFlow init = cfg.init;
  tvl1_shift shift;
  memset(&shift, 0, sizeof shift);
  int auto_R = 0;
  if (init.automatic) {
    auto_R = auto_seed_range(init.max_shift, W, H);
    if (auto_R < 1) {
      init.on = false;   // too small to search: solved unseeded
    } else {
      if (dc.failed(tvl1_estimate_shift(dc.ctx, v.a, v.pitch0, v.b, v.pitch1, W, H, auto_R, &shift, dc.stream), err))
        return false;
      init.dx = (float)shift.dx, init.dy = (float)shift.dy;
    }
  }
  tvl1_stats st;
  memset(&st, 0, sizeof st);
  // per-warp executed iterations (level-major), reported in stats_json beside the totals
  std::vector<int32_t> warp_iters((size_t)TVL1_MAX_LEVELS * std::max(1, cfg.tv.warps), -1);
  st.warp_iterations = warp_iters.data();
  st.warp_iterations_capacity = (int32_t)warp_iters.size();
  uint64_t rejected = 0;
  const auto t0 = Clock::now();
  const std::function<void(const PointCount *)> record = [&](const PointCount *points) {
    res.stats["solves"].append(solve_record(Rect{r0.x, r0.y, W, H}, secs_since(t0), st, cfg.tv.warps, init, auto_R,
                                            shift, check, rejected, points));
  };
  if (init.chained() &&
      (!dc.reserve_check((size_t)W * H * sizeof(float), err) || !load_chain(dc, im, init, v, err) ||
       !invert_chain(dc, init, v, init.backward_inverse && check.on && !check.zncc(), err)))
    return false;
  if (!solve_seeded(dc, v.a, v.pitch0, v.b, v.pitch1, v, init, 1.f, dc.du.f32(), dc.dv.f32(), &st, err)) return false;
  FlowSet fs;
  fs.I0 = v.a, fs.pitch0 = v.pitch0, fs.I1 = v.b, fs.pitch1 = v.pitch1;
  fs.u = dc.du.f32(), fs.v = dc.dv.f32(), fs.fpitch = v.fp, fs.W = W, fs.H = H;
  if (check.on) {
    if (!dc.reserve_check((size_t)W * H * sizeof(float), err)) return false;
    fs.ub = dc.dub.f32(), fs.vb = dc.dvb.f32(), fs.score = dc.dsc.f32();
    bool backward_ok = true;   // false: solve_seeded has reported it
    const tvl1_status s = score_flows(dc, fs, check, [&] {
      backward_ok = solve_seeded(dc, v.b, v.pitch1, v.a, v.pitch0, v, init, -1.f, fs.ub, fs.vb, nullptr, err);
      return backward_ok ? TVL1_OK : TVL1_EHIP;
    });
    if (!backward_ok || dc.failed(s, err)) return false;
  }
  // features: map = flow + grid -> warpAffine(identity) -> flow = map - grid (mode 2),
  // or the map itself (mode 1);
  // "map": flow + grid (mode 1); otherwise unchanged.  Then zero where I1 <= 1.
  const int mode = features ? (cfg.otype == "flow" ? 2 : 1) : (cfg.otype == "map" ? 1 : 0);
  tvl1_status s;
  if (features && affine)   // the features branch with the alignment's affine (:429-443)
    s = tvl1_postprocess_affine(dc.ctx, fs.u, fs.v, v.fp, v.b, v.pitch1, W, H, cfg.otype == "flow" ? 1 : 0, affine,
                                dc.stream);
  else
    s = tvl1_postprocess(dc.ctx, fs.u, fs.v, v.fp, v.b, v.pitch1, W, H, mode, dc.stream);
  if (dc.failed(s, err)) return false;
  if (check.on && dc.failed(reject_flows(dc, fs, check, &rejected), err)) return false;
  if (!cfg.sampled()) return download_and_write(dc, v, f0, f1, r0, r1, im, cfg, features, record, err);
  if (hipStreamSynchronize(dc.stream) != hipSuccess) return dc.hip_error("solve failed", err);
  if (!check.on) record(nullptr);
  PointCount count;
  const bool ok = random_points_sampled(dc, v, f0, f1, r0, r1, im, cfg, features, count, err);
  if (check.on) record(ok ? &count : nullptr);   // with the candidates and the kept points
  return ok;
}

bool in_bounds(const Rect &r, const ofio::Image8 &f) {
  return r.x >= 0 && r.y >= 0 && r.width > 0 && r.height > 0 && r.x + r.width <= f.width &&
         r.y + r.height <= f.height;
}

// find_alignment(frame1, frame0) + warpAffine(frame1 -> frame0 size) (optflow.cpp:372-376,
// features.cpp:46-167).  The aligned frame replaces frame1 on the device (and on the host,
// for the random_points mask), as frame1_GPU = new_frame1 does in the reference.
bool align_frame1(DeviceCtx &dc, const ofio::Image8 &f0, const ofio::Image8 &f1, ofio::Image8 &aligned,
                  const Value &im, const Value &args, float affine[6], std::string &err) {
  const int w1 = f1.width, h1 = f1.height;   // f1 may be `aligned` itself (a second key)
  const int feature_type = im.get("features", Value(args.get("features", Value(2)).asInt())).asInt();
  if (feature_type != 1)   // SURF_TYPE (features.h:9) and anything else
    fprintf(stderr, "SURF features are not part of this build; using ORB features for the "
                    "alignment of %s.\n", im["p"].asString().c_str());
  const tvl1_align_params p = align_params_of(im, args);
  int32_t n_good = 0, outcome = 0;
  if (dc.failed(tvl1_find_alignment(dc.ctx, dc.d1.u8(), (size_t)w1, w1, h1, dc.d0.u8(), (size_t)f0.width, f0.width,
                                    f0.height, &p, affine, &n_good, &outcome, dc.stream),
                err, "find_alignment: "))
    return false;
  if (args.get("debug", Value(false)).asBool())
    printf("Number of good features: %d\n", n_good);
  if (outcome == 1) printf("Not enough matches. Using no transformation\n");
  if (outcome == 2)
    printf("More than twenty percent variance in zoom or no homography found, this is probably "
           "an error, ignoring the transformation.\n");
  if (dc.failed(tvl1_warp_affine_u8(dc.ctx, dc.d1.u8(), (size_t)w1, w1, h1, dc.dw.u8(), (size_t)f0.width, f0.width,
                                    f0.height, affine, dc.stream),
                err, "warpAffine: "))
    return false;
  aligned.width = f0.width;
  aligned.height = f0.height;
  aligned.data.resize((size_t)f0.width * f0.height);
  if (hipMemcpyAsync(aligned.data.data(), dc.dw.p, aligned.data.size(), hipMemcpyDeviceToHost, dc.stream) !=
          hipSuccess ||
      hipStreamSynchronize(dc.stream) != hipSuccess)
    return dc.hip_error("download of the aligned frame failed", err);
  std::swap(dc.d1, dc.dw);
  dc.key1.clear();  // the device copy is the aligned frame, not the slice
  return true;
}

// solve_rois (optflow.cpp:312-392)
bool solve_rois(DeviceCtx &dc, const ofio::Image8 &f0, const ofio::Image8 &f1_in, bool f0_resident,
                bool f1_resident, const Value &rois, Value &im, const Value &args, const PairConfig &cfg,
                PairResult &res, std::string &err) {
  ofio::Image8 f1_aligned;               // frame1 after find_alignment + warpAffine
  const ofio::Image8 *f1p = &f1_in;      // the frame1 the ROIs read: the slice or f1_aligned
  bool features = cfg.features;
  // a seeded pair is not pre-aligned: the seed is a flow between the frames as they are; nor is
  // a pair whose flow is checked (against the backward solve, or on the frames as they are)
  if (const char *conflict = cfg.features_conflict()) {
    err = conflict;
    return false;
  }
  // cv::Mat affine(cv::Size(3,2), CV_32FC1) (optflow.cpp:319) is uninitialised until
  // find_alignment fills it; the identity stands in for that here.
  float affine[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  size_t img_bytes = std::max(f0.data.size(), f1p->data.size());
  size_t flow_bytes = 0;
  for (auto &k : rois.memberNames()) {
    const Rect r = roi_from_array(k == "custom_diff" ? rois[k]["0"] : rois[k]);
    flow_bytes = std::max(flow_bytes, (size_t)std::max(0, r.width) * std::max(0, r.height) * 4);
  }
  bool realloc = false;
  if (!dc.reserve(img_bytes, std::max<size_t>(flow_bytes, 4), realloc, err)) return false;
  // PinnedPool's invariant (cli/imageio.hpp): a host buffer goes back to the pool only after
  // the stream that reads it was synchronised.  Every successful path below ends in a
  // synchronising download; a failing one (an ROI outside the image, EINVAL / ESIZE, an
  // alignment error) may leave the uploads of f0 / f1 queued, so it waits here.
  struct SyncOnFailure {
    DeviceCtx &dc;
    bool ok = false;
    ~SyncOnFailure() {
      if (!ok && dc.stream) (void)hipStreamSynchronize(dc.stream);
    }
  } sync_guard{dc};
  if (realloc) f0_resident = f1_resident = false;
  // GpuMat::upload (optflow.cpp:315-316), skipped when the slice is already resident
  if (!f0_resident && hipMemcpyAsync(dc.d0.p, f0.data.data(), f0.data.size(), hipMemcpyHostToDevice, dc.stream) != hipSuccess)
    return dc.hip_error("upload failed", err);
  if (!f1_resident && hipMemcpyAsync(dc.d1.p, f1p->data.data(), f1p->data.size(), hipMemcpyHostToDevice, dc.stream) != hipSuccess)
    return dc.hip_error("upload failed", err);
  bool ok = true;
  for (const auto &key : rois.memberNames()) {  // sorted, like jsoncpp getMemberNames
    im["output_suffix"] = roi_suffix(key);
    Rect r0, r1;
    if (key == "custom_diff") {
      if (features) fprintf(stderr, "Features isn't compatible with different ROIs for each image.\n Ignoring features.\n");
      r0 = roi_from_array(rois[key]["0"]);
      r1 = roi_from_array(rois[key]["1"]);
      if (r0.width != r1.width || r0.height != r1.height) {
        err = "custom ROIs of the two frames must have the same size";
        ok = false;
        continue;
      }
    } else {
      const bool size_differs = f0.width != f1p->width || f0.height != f1p->height;
      if (features || size_differs || key == "default") {   // optflow.cpp:366-377
        if (size_differs || (key == "default" && !features))
          fprintf(stderr, "Rows or columns differ between frames no ROI selected, reverting to "
                          "features even though it wasn't selected.\n");
        if (cfg.init.on) {   // (no ROI, or frames of different sizes: the reference aligns these)
          err = kInitFlowFeatures;
          return false;
        }
        if (cfg.check.on) {
          err = check_features_error(cfg.check);
          return false;
        }
        if (!align_frame1(dc, f0, *f1p, f1_aligned, im, args, affine, err)) return false;
        f1p = &f1_aligned;
        features = true;
      }
      r0 = r1 = roi_from_array(rois[key]);
    }
    if (!in_bounds(r0, f0) || !in_bounds(r1, *f1p)) {
      err = "ROI '" + key + "' is outside the image";
      ok = false;
      continue;
    }
    if (!solve_wrapper(dc, f0, *f1p, r0, r1, im, cfg, features, affine, res, err)) ok = false;
  }
  if (cfg.random_points()) res.pms.push_back(move_pm(im));
  sync_guard.ok = ok;
  return ok;
}

// One worker thread's pairs: chunks of JobState::todo, the current one and the next both queued
// for decode.
struct PairWorker {
  JobState &job;
  const int device;
  DeviceCtx dc;
  std::map<std::string, LoadFuture> pending;   // slice key -> its decode
  ChunkWalk *walk = nullptr;

  PairWorker(JobState &j, int d) : job(j), device(d) { dc.device = d; }

  float scale_of(size_t i) const {
    return job.images[i].get("scale", job.args.get("scale", 0.5).asFloat()).asFloat();
  }
  static std::string key_of(const std::string &path, float scale) { return path + "|" + scale_string(scale); }

  void queue_chunk(size_t start) {
    for (size_t k = start; k < std::min(job.todo.size(), start + job.chunk); ++k) {
      const size_t i = job.todo[k];
      const float sc = scale_of(i);
      for (const char *side : {"p", "q"}) {
        const std::string path = job.images[i][side].asString(), key = key_of(path, sc);
        if (!pending.count(key)) pending.emplace(key, job.pool.load(path, sc));
      }
    }
  }
  // a pair after position kk of the current chunk, or one of the next chunk, names the slice
  bool needed_later(const std::string &k, size_t kk) const {
    auto names = [&](size_t from, size_t to) {
      for (size_t jj = from; jj < to; ++jj) {
        const size_t j = job.todo[jj];
        if (key_of(job.images[j]["p"].asString(), scale_of(j)) == k ||
            key_of(job.images[j]["q"].asString(), scale_of(j)) == k)
          return true;
      }
      return false;
    };
    return names(kk + 1, walk->end()) || names(walk->next_start, walk->next_end());
  }
  // a queued slice leaves `pending` after the last pair of the two queued chunks that names
  // it, whether or not it was decoded for nothing because the slice was already resident
  void retire(const std::string &k, size_t kk) {
    if (!needed_later(k, kk)) pending.erase(k);
  }
  // the pooled decode of a slice
  bool load(const std::string &name, float scale, size_t kk, ofio::Image8 &dst, std::string &err) {
    const std::string k = key_of(name, scale);
    auto it = pending.find(k);
    LoadFuture f = it != pending.end() ? it->second : job.pool.load(name, scale);
    const std::shared_ptr<Loaded> r = f.get();
    if (!r->ok) {
      err = r->err;
      return false;
    }
    if (needed_later(k, kk)) dst = r->img;   // a later pair reads it again: copy
    else dst = std::move(r->img);            // last use: nobody reads it after this
    return true;
  }

  // the pair's two slices into dc.h0 / dc.h1, reusing what is resident (r0 / r1: on the device
  // too); false: a slice could not be read, which is reported as the reference reports it
  bool load_pair(size_t i, size_t kk, const std::string &p, const std::string &q, float scale, bool &r0, bool &r1) {
    const std::string k0 = key_of(p, scale), k1 = key_of(q, scale);
    r0 = r1 = false;
    if (k0 == dc.key0) {
      r0 = true;
    } else if (k0 == dc.key1) {  // previous q is this p: swap roles
      std::swap(dc.d0, dc.d1);
      std::swap(dc.key0, dc.key1);
      std::swap(dc.h0, dc.h1);
      r0 = true;
    }
    r1 = (k1 == dc.key1);
    std::string err;
    const char *bad = nullptr;
    if (!r0 && !load(p, scale, kk, dc.h0, err)) {
      bad = p.c_str();
      dc.key0.clear();
    } else if (!r1 && !load(q, scale, kk, dc.h1, err)) {
      bad = q.c_str();
      dc.key1.clear();
    }
    if (bad) {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      printf("Error: %s \n", bad);
      job.results[i].done = true;
    } else {
      dc.key0 = k0;
      dc.key1 = k1;
    }
    retire(k0, kk);
    retire(k1, kk);
    return !bad;
  }

  // solve_rois, and after a device error once more on a rebuilt context; input errors (an ROI
  // outside the image) are reported as the reference reports them
  void solve_pair(size_t i, bool r0, bool r1, const Value &rois, Value &im, const PairConfig &cfg) {
    PairResult &res = job.results[i];
    const std::string p = im["p"].asString(), q = im["q"].asString();
    const std::string k0 = dc.key0, k1 = dc.key1;
    std::string err;
    if (inject_fault(i)) {
      res.ok = false;
      dc.faulted = true;
      err = "injected device fault";
    } else {
      res.ok = solve_rois(dc, dc.h0, dc.h1, r0, r1, rois, im, job.args, cfg, res, err);
    }
    if (!res.ok) {  // device contents are unknown after a failure
      dc.key0.clear();
      dc.key1.clear();
    }
    if (!res.ok && dc.faulted) {
      {
        std::lock_guard<std::mutex> lk(g_io_mutex);
        fprintf(stderr, "Warning: pair %zu (%s %s): %s; retrying on a fresh device context\n", i, p.c_str(),
                q.c_str(), err.c_str());
      }
      res = PairResult();
      if (rebuild_device(dc, device, err)) {
        err.clear();
        res.ok = solve_rois(dc, dc.h0, dc.h1, false, false, rois, im, job.args, cfg, res, err);
        if (res.ok) {
          dc.key0 = k0;
          dc.key1 = k1;
        } else {
          dc.key0.clear();
          dc.key1.clear();
        }
      }
    }
    res.done = true;
    if (!res.ok) {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      fprintf(stderr, "Error: pair %zu (%s %s): %s\n", i, p.c_str(), q.c_str(), err.c_str());
    }
  }

  void run_pair(size_t kk) {
    const size_t i = job.todo[kk];
    Value im = job.images[i];
    const PairConfig cfg = resolve_pair(im, job.args);
    const std::string p = im["p"].asString(), q = im["q"].asString();
    const float scale = scale_of(i);
    {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      printf("%s %s\n", p.c_str(), q.c_str());
      fflush(stdout);
    }
    fill_defaults(im, job.args, scale);
    bool r0, r1;
    if (!load_pair(i, kk, p, q, scale, r0, r1)) return;
    const int rows = std::min(dc.h0.height, dc.h1.height), cols = std::min(dc.h0.width, dc.h1.width);
    const Value rois = rois_of(im, job.args, rows, cols);
    PairResult &res = job.results[i];
    if (job.plan_only) {
      job.plans[i] = plan_entry(job, i, im, cfg, rois, dc.h0.width, dc.h0.height);
      res.done = res.ok = true;
      return;
    }
    if (job.skip_existing && !cfg.random_points() && outputs_exist(im["output"].asString(), rois.memberNames())) {
      res.done = res.ok = true;
      return;
    }
    solve_pair(i, r0, r1, rois, im, cfg);
  }

  void run() {
    if (!job.plan_only && !open_or_hard_error(dc, device, job)) return;
    auto queue = [this](size_t start) { queue_chunk(start); };
    ChunkWalk w(job.next, job.chunk, job.todo.size(), queue);
    walk = &w;
    while (w.advance(queue))
      for (size_t kk = w.start; kk < w.end(); ++kk) run_pair(kk);
    dc.close();
  }
};

}  // namespace

void run_pair_worker(JobState &job, int device) { PairWorker(job, device).run(); }

}  // namespace ofcli
