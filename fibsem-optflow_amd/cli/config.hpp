// config.hpp — what a style 1 job's JSON says about one pair, resolved once (no HIP here: this
// header and points.hpp compile without hip_runtime.h, tests/cli_units.cpp).
//
//   Rect, roi_from_array, get_rois      ROI geometry (optflow.cpp:228-261, 302-310 of the reference)
//   generate_TV_args .. align_params_of per-image value, else global, else default
//   InitFlow, FlowCheck                 the build-only seed and check keys
//   PairConfig, resolve_pair            all of it for one pair, handed down the solve path
//   roi_suffix .. auto_seed_range       the small rules both workers share
//   solve_record                        one stats_json "solves" entry
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/tvl1.h"
#include "json.hpp"

namespace ofcli {

using ofjson::Value;

struct Rect {
  int x = 0, y = 0, width = 0, height = 0;
};

// roi_from_array (optflow.cpp:302-310)
inline Rect roi_from_array(const Value &a) {
  Rect r;
  r.x = a[(size_t)0].asInt();
  r.y = a[(size_t)1].asInt();
  r.width = a[(size_t)2].asInt();
  r.height = a[(size_t)3].asInt();
  return r;
}

// get_rois (optflow.cpp:228-261)
inline void get_rois(Value &rois, const Value &args, int rows, int cols) {
  if (args.isMember("top")) {
    rois["top"][0] = 0;
    rois["top"][1] = 0;
    rois["top"][2] = cols;
    rois["top"][3] = args.get("top", 300).asInt();
  }
  if (args.isMember("bottom")) {
    const int bottom = args.get("bottom", 300).asInt();
    rois["bottom"][0] = 0;
    rois["bottom"][1] = rows - bottom;
    rois["bottom"][2] = cols;
    rois["bottom"][3] = bottom;
  }
  if (args.isMember("custom")) {
    if (args["custom"].isMember("0")) {
      rois["custom_diff"]["0"] = args["custom"]["0"];
      if (!args["custom"].isMember("1"))
        fprintf(stderr, "If you specify a custom for the first frame, you must specify a custom "
                        "for the second.\n");
      rois["custom_diff"]["1"] = args["custom"]["1"];
    } else {
      rois["custom"] = args["custom"];
    }
  }
}

// the ROIs of a pair whose two slices are rows x cols where they overlap: the image's "rois",
// else the job's, else the whole frame as "default" (optflow.cpp:136-154)
inline Value rois_of(const Value &im, const Value &args, int rows, int cols) {
  Value rois;
  if (im.isMember("rois")) {
    get_rois(rois, im["rois"], rows, cols);
  } else if (args.isMember("rois")) {
    get_rois(rois, args["rois"], rows, cols);
  } else {
    rois["default"][0] = 0;
    rois["default"][1] = 0;
    rois["default"][2] = cols;
    rois["default"][3] = rows;
  }
  return rois;
}

// generate_TV_args (optflow.cpp:500-514): per-image value, else global, else default.
inline tvl1_params generate_TV_args(const Value &im, const Value &args) {
  tvl1_params p;
  tvl1_params_default(&p);
  auto D = [&](const char *k, double d) { return im.get(k, args.get(k, d).asDouble()).asDouble(); };
  auto I = [&](const char *k, int d) { return im.get(k, args.get(k, d).asInt()).asInt(); };
  p.tau = D("tau", 0.25);
  p.lambda = D("lambda", 0.05);
  p.theta = D("theta", 0.3);
  p.nscales = I("nscales", 10);
  p.warps = I("warps", 5);
  p.epsilon = D("epsilon", 0.01);
  p.iterations = I("iterations", 300);
  p.scale_step = D("scaleStep", 0.8);
  p.gamma = D("gamma", 0.0);
  p.use_initial_flow = im.get("useInitialFlow", args.get("useInitialFlow", false).asBool()).asBool();
  p.median_filtering = I("medianFiltering", 1);
  p.fast_math = I("fastMath", 0);
  // build-only: OpenCV's CPU DualTVL1OpticalFlow schedule
  p.profile = I("profile", 0);
  p.inner_iterations = I("innerIterations", 30);
  p.outer_iterations = I("outerIterations", 10);
  return p;
}

inline std::string output_type_of(const Value &im, const Value &args) {
  return im.get("output_type", args.get("output_type", "map").asString()).asString();
}

// solve_rois' tri-state "features" resolution (optflow.cpp:323-338)
inline bool resolve_features(const Value &im, const Value &args) {
  if (im.isMember("features") && !im["features"].asBool()) return false;
  if (args.isMember("features") && !args["features"].asBool()) return false;
  if (im.get("features", false).asBool() || args.get("features", false).asBool()) return true;
  return false;
}

// build-only "initialFlow": [dx, dy] (px of the pre-scaled frame, flow from frame0 to frame1),
// per image or global, honoured only with "useInitialFlow": true: the pair's ROIs are solved
// by tvl1_calc_init from that constant flow.  "useInitialFlow" alone stays without effect,
// as in the reference (optflow.cpp:512, never passed to create()).  "initialFlow": "auto" is
// the same with a constant found per ROI (tvl1_estimate_shift within "initialFlowMaxShift" px,
// default 32, per image or global); any other value of the key stays inert.
//
// "initialFlow": {"chain": [prefix, ...]}, 1 to 64 links, each the "output" value of an earlier
// pair: the seed is the composition, left to right, of the flows those pairs wrote.
// For ROI key k a link is read from {prefix}{roi_suffix(k)}_x.tiff and _y.tiff, the links are
// composed on the device (tvl1_compose_flow, in place) and the ROI is solved by tvl1_calc_init
// from the result; a chain of one link is a seed read from a file.  The link files must have been
// written with "output_type": "flow", at this pair's scale and for the same ROI: a map cannot be
// told from a flow here.  Such pairs are solved one by one, never in a strip batch.
//
// Beside "chain", in the same object:
//   "inverse": true (default false): the links are the outputs of the pairs that walk from this
//     pair's frame1 to its frame0, and the seed is tvl1_invert_flow of their composition;
//   "inverseIterations" (1..32, default 8) and "inverseTolerance" (px^2, finite, default 0.01):
//     the inversion's K and the bound its unconverged count is taken at;
//   "backward": "inverse": allows the pair beside "consistency"; the backward solve is seeded by
//     the inverse of the forward seed (with "inverse": true that is the composed chain itself, so
//     no second inversion is computed).
struct InitFlow {
  bool on = false;
  float dx = 0.f, dy = 0.f;
  bool automatic = false;
  int max_shift = 0;
  std::vector<std::string> chain;        // the links' prefixes; empty: no chain
  const char *error = nullptr;           // the key cannot run as written
  int error_status = 2;                  // ... and the job's exit status for it (the inverse's keys: 1)
  std::vector<uint64_t> outside;         // per composition of a solve: px clamped at the frame edge
  bool inverse = false;                  // the seed is the inverse of the composed chain
  bool backward_inverse = false;         // "backward": "inverse"
  int inverse_iterations = 8;
  float inverse_tolerance = 0.01f;
  bool inverted = false;                 // a solve's inversion ran, with these counts
  tvl1_invert_counts inverse_counts = {0, 0};
  bool chained() const { return !chain.empty(); }
};
constexpr size_t kMaxChainLinks = 64;
inline const char *const kChainLinks = "initialFlow: \"chain\" must be a list of 1 to 64 output names";
inline const char *const kChainConsistency =
    "an initialFlow chain cannot be combined with consistency: the backward solve's seed would be the "
    "chain's inverse, not its negation";
inline const char *const kChainInverse = "initialFlow: \"inverse\" must be true or false";
inline const char *const kChainInverseIterations = "initialFlow: \"inverseIterations\" must be an integer from 1 to 32";
inline const char *const kChainInverseTolerance = "initialFlow: \"inverseTolerance\" must be a finite number (px^2)";
inline const char *const kChainBackward = "initialFlow: \"backward\" must be \"inverse\"";
inline const char *const kInitFlowFeatures =
    "initialFlow cannot be combined with feature alignment (features, a pair without ROIs, or "
    "frames of different sizes)";
inline InitFlow initial_flow_of(const Value &im, const Value &args) {
  InitFlow f;
  if (!im.get("useInitialFlow", args.get("useInitialFlow", false).asBool()).asBool()) return f;
  const Value &v = im.isMember("initialFlow") ? im["initialFlow"] : args["initialFlow"];
  if (v.isString() && v.asString() == "auto") {
    f.on = f.automatic = true;
    f.max_shift = im.get("initialFlowMaxShift", args.get("initialFlowMaxShift", 32).asInt()).asInt();
    return f;
  }
  if (v.isObject() && v.isMember("chain")) {
    const Value &c = v["chain"];
    bool good = c.isArray() && c.size() >= 1 && c.size() <= kMaxChainLinks;
    for (size_t i = 0; good && i < c.size(); ++i) good = c[i].isString() && !c[i].asString().empty();
    if (!good) {
      f.error = kChainLinks;
      return f;
    }
    if (const Value *x = v.find("inverse")) {
      if (x->type() != Value::Bool) return f.error = kChainInverse, f.error_status = 1, f;
      f.inverse = x->asBool();
    }
    if (const Value *x = v.find("inverseIterations")) {
      if (x->type() != Value::Int || x->asInt64() < 1 || x->asInt64() > 32)
        return f.error = kChainInverseIterations, f.error_status = 1, f;
      f.inverse_iterations = x->asInt();
    }
    if (const Value *x = v.find("inverseTolerance")) {
      if ((x->type() != Value::Int && x->type() != Value::Real) || !std::isfinite(x->asFloat()))
        return f.error = kChainInverseTolerance, f.error_status = 1, f;
      f.inverse_tolerance = x->asFloat();
    }
    if (const Value *x = v.find("backward")) {
      if (!x->isString() || x->asString() != "inverse") return f.error = kChainBackward, f.error_status = 1, f;
      f.backward_inverse = true;
    }
    f.on = true;
    for (size_t i = 0; i < c.size(); ++i) f.chain.push_back(c[i].asString());
    return f;
  }
  if (!v.isArray() || v.size() != 2) return f;
  f.on = true;
  f.dx = v[0].asFloat();
  f.dy = v[1].asFloat();
  return f;
}

// The search range of an "auto" seed on a W x H ROI: "initialFlowMaxShift", at most 128 and at
// most min(W, H) / 4; 0 = too small to search, the ROI is solved unseeded.
inline int auto_seed_range(int max_shift, int W, int H) {
  return std::max(0, std::min(std::min(max_shift, 128), std::min(W, H) / 4));
}

// The check of a pair's flows, one of two build-only keys (never both):
//
// "consistency": false (default), true (alpha 0.01, beta 0.5) or {"alpha": a, "beta": b}, per
// image or global: every ROI is also solved backward (the frame views swapped, a seed negated),
// the forward flow is scored against the backward one (tvl1_fb_score) and zeroed
// where !(score <= beta) after the post-process (tvl1_zero_above); random_points draws
// "consistencyOversample" times as many candidates (default 4) and emits the first npoints that
// are consistent; "consistencyOutput" writes the score plane as {output}{suffix}_fb.tiff.
//
// "zncc": false (default), true (radius 3, beta 0.25) or {"radius": r, "beta": b}: the one-solve
// check.  Every ROI's raw flow is scored by 1 - ZNCC of a (2r+1)^2 window of frame0 against
// frame1 warped back along the flow (tvl1_zncc_score), on the views the solve saw;
// from there on the score is used as "consistency" uses its own, with "znccOversample" and
// "znccOutput" ({output}{suffix}_zncc.tiff).
struct FlowCheck {
  enum Kind { kForwardBackward, kZncc };
  Kind kind = kForwardBackward;
  bool on = false;
  float alpha = 0.01f, beta = 0.5f;   // alpha: kForwardBackward only
  int radius = 0;                     // kZncc only, 1..4
  int oversample = 4;
  bool output = false;
  bool zncc() const { return kind == kZncc; }
};
inline const char *const kConsistencyFeatures =
    "consistency cannot be combined with feature alignment (features, a pair without ROIs, or "
    "frames of different sizes): the backward pair would need the inverse alignment";
inline const char *const kZnccFeatures =
    "zncc cannot be combined with feature alignment (features, a pair without ROIs, or frames of "
    "different sizes): the score plane would need the alignment's warp";
inline const char *const kZnccConsistency = "zncc cannot be combined with consistency";

inline FlowCheck consistency_of(const Value &im, const Value &args) {
  FlowCheck c;
  const Value &v = im.isMember("consistency") ? im["consistency"] : args["consistency"];
  if (v.isObject()) {
    c.on = true;
    c.alpha = v.get("alpha", 0.01).asFloat();
    c.beta = v.get("beta", 0.5).asFloat();
  } else if (v.isNumeric()) {   // true / false; any other value of the key stays inert
    c.on = v.asBool();
  }
  c.oversample = std::max(1, im.get("consistencyOversample", args.get("consistencyOversample", 4).asInt()).asInt());
  c.output = im.get("consistencyOutput", args.get("consistencyOutput", false).asBool()).asBool();
  return c;
}
inline FlowCheck zncc_of(const Value &im, const Value &args) {
  FlowCheck c;
  c.kind = FlowCheck::kZncc;
  c.radius = 3, c.beta = 0.25f;
  const Value &v = im.isMember("zncc") ? im["zncc"] : args["zncc"];
  if (v.isObject()) {
    c.on = true;
    c.radius = v.get("radius", 3).asInt();
    c.beta = v.get("beta", 0.25).asFloat();
  } else if (v.isNumeric()) {   // true / false; any other value of the key stays inert
    c.on = v.asBool();
  }
  c.oversample = std::max(1, im.get("znccOversample", args.get("znccOversample", 4).asInt()).asInt());
  c.output = im.get("znccOutput", args.get("znccOutput", false).asBool()).asBool();
  return c;
}
// "consistency", "zncc" or none; *err where the keys cannot run as written
inline FlowCheck check_of(const Value &im, const Value &args, const char **err = nullptr) {
  const FlowCheck fb = consistency_of(im, args), zn = zncc_of(im, args);
  if (err) *err = nullptr;
  if (!zn.on) return fb;
  if (err && fb.on) *err = kZnccConsistency;
  if (err && !*err && (zn.radius < 1 || zn.radius > 4)) *err = "zncc: radius must be 1..4";
  return zn;
}
inline const char *check_key(const FlowCheck &c) { return c.zncc() ? "zncc" : "consistency"; }
inline const char *check_suffix(const FlowCheck &c) { return c.zncc() ? "_zncc.tiff" : "_fb.tiff"; }
inline const char *check_features_error(const FlowCheck &c) { return c.zncc() ? kZnccFeatures : kConsistencyFeatures; }
inline void check_json(Value &dst, const FlowCheck &c) {
  if (c.zncc())
    dst["radius"] = c.radius;
  else
    dst["alpha"] = (double)c.alpha;
  dst["beta"] = (double)c.beta;
}
// how many candidates a check draws for npoints points
inline size_t candidates_of(int npoints, const FlowCheck &c) {
  return (size_t)std::max(npoints, 0) * (size_t)(c.on ? c.oversample : 1);
}

// orb_defaults (features.cpp:19-32) + the ratio / homo / ransac keys of find_alignment
// (:109, :133), each looked up in the image's args first, then the global args.
inline tvl1_align_params align_params_of(const Value &im, const Value &args) {
  tvl1_align_params p;
  tvl1_align_params_default(&p);
  auto i = [&](const char *k, int d) { return im.get(k, Value(args.get(k, Value(d)).asInt())).asInt(); };
  auto f = [&](const char *k, double d) {
    return im.get(k, Value(args.get(k, Value(d)).asDouble())).asDouble();
  };
  p.nfeatures = i("nfeatures", p.nfeatures);
  p.scale_factor = (float)f("scaleFactor", p.scale_factor);
  p.nlevels = i("nlevels", p.nlevels);
  p.edge_threshold = i("edgeThreshold", p.edge_threshold);
  p.first_level = i("firstLevel", p.first_level);
  p.wta_k = i("WTA_K", p.wta_k);
  p.patch_size = i("patchSize", p.patch_size);
  p.fast_threshold = i("fastThreshold", p.fast_threshold);
  p.blur_for_descriptor = im.get("blurForDescriptor", Value(args.get("blurForDescriptor", Value(false)).asBool())).asBool();
  p.ratio = (float)f("ratio", p.ratio);
  p.method = i("homo", p.method);
  p.ransac_threshold = f("ransac", p.ransac_threshold);
  return p;
}

// One pair's config, resolved once from its image entry and the job (per-image value, else
// global, else default) and handed down through solve_rois, solve_wrapper and the plan.
struct PairConfig {
  tvl1_params tv;
  std::string otype;        // "map" | "flow" | "random_points" | anything else: solved, not written
  bool features = false;
  InitFlow init;
  FlowCheck check;
  const char *check_error = nullptr;   // the check keys cannot run as written
  int npoints = 25;
  float scale = 0.5f;
  bool debug = false;
  bool random_points() const { return otype == "random_points"; }
  bool sampled() const { return random_points() && !debug; }   // time-seeded draw of npoints px
  // the config names feature alignment beside a seed or a check: nullptr, or why it cannot run
  const char *features_conflict() const {
    if (init.error) return init.error;
    if (init.on && features) return kInitFlowFeatures;
    if (check_error) return check_error;
    if (init.chained() && check.on && !check.zncc() && !init.backward_inverse) return kChainConsistency;
    if (check.on && features) return check_features_error(check);
    return nullptr;
  }
};
inline PairConfig resolve_pair(const Value &im, const Value &args) {
  PairConfig c;
  c.tv = generate_TV_args(im, args);
  c.otype = output_type_of(im, args);
  c.features = resolve_features(im, args);
  c.init = initial_flow_of(im, args);
  c.check = check_of(im, args, &c.check_error);
  c.npoints = im.get("npoints", args.get("npoints", 25).asInt()).asInt();
  c.scale = im.get("scale", args.get("scale", 0.5).asFloat()).asFloat();
  c.debug = args.get("debug", false).asBool();
  return c;
}

// "_top" / "_bottom" for those ROI keys, nothing for the others (optflow.cpp:343-350)
inline std::string roi_suffix(const std::string &key) {
  return (key == "top" || key == "bottom") ? "_" + key : std::string();
}
// the scale as output names and slice keys carry it (optflow.cpp:155-157)
inline std::string scale_string(float scale) {
  char b[32];
  snprintf(b, sizeof b, "%0.2f", scale);
  return b;
}
// a pair's working copy of its image entry: "scale" and "output" filled in where it has none
inline void fill_defaults(Value &im, const Value &args, float scale) {
  im["scale"] = im.get("scale", (double)scale).asDouble();
  im["output"] = im.get("output", args["output_dir"].asString() + "/" + im["output_name"].asString() + "_" +
                                      scale_string(scale));
}

// One stats_json "solves" entry.  `init` is the seed the solve ran from (on = false: unseeded);
// `shift` the estimate's record of an "auto" seed, searched within auto_R (0: not searched).
struct PointCount {
  size_t candidates = 0, kept = 0;
};
// a checked random_points solve: how many candidates were drawn and how many points kept
inline void record_points(Value &sv, const FlowCheck &check, const PointCount &n) {
  if (!check.on) return;
  sv[check_key(check)]["candidates"] = (int64_t)n.candidates;
  sv[check_key(check)]["kept"] = (int64_t)n.kept;
}
inline Value solve_record(const Rect &roi, double seconds, const tvl1_stats &st, int warps, const InitFlow &init,
                          int auto_R, const tvl1_shift &shift, const FlowCheck &check, uint64_t rejected_px,
                          const PointCount *points) {
  Value sv;
  sv["roi"][0] = roi.x;
  sv["roi"][1] = roi.y;
  sv["roi"][2] = roi.width;
  sv["roi"][3] = roi.height;
  sv["seconds"] = seconds;
  sv["levels"] = st.levels;
  sv["iterations"] = (int64_t)st.iterations_total;
  sv["checks"] = (int64_t)st.checks_total;
  // per-warp executed iterations (level-major), beside the totals
  const size_t nw = std::min((size_t)std::max(0, st.warp_iterations_capacity),
                             (size_t)std::max(0, st.levels) * std::max(1, warps));
  for (size_t k = 0; k < nw; ++k) sv["warp_iterations"][(int)k] = st.warp_iterations[k];
  if (init.chained()) {
    sv["initial_flow_chain"]["links"] = (int64_t)init.chain.size();
    sv["initial_flow_chain"]["outside"] = Value();
    for (size_t k = 0; k < init.outside.size(); ++k)
      sv["initial_flow_chain"]["outside"][(int)k] = (int64_t)init.outside[k];
    if (init.inverted) {
      Value &iv = sv["initial_flow_chain"]["inverse"];
      iv["iterations"] = init.inverse_iterations;
      iv["tolerance"] = (double)init.inverse_tolerance;
      iv["outside"] = (int64_t)init.inverse_counts.outside;
      iv["unconverged"] = (int64_t)init.inverse_counts.unconverged;
    }
  } else if (init.on) {
    sv["initial_flow"][0] = (double)init.dx;
    sv["initial_flow"][1] = (double)init.dy;
  }
  if (init.automatic) {
    sv["initial_flow_auto"]["max_shift"] = auto_R;
    if (auto_R) {
      sv["initial_flow_auto"]["sad"] = (int64_t)shift.sad;
      sv["initial_flow_auto"]["count"] = (int64_t)shift.count;
      sv["initial_flow_auto"]["sad_zero"] = (int64_t)shift.sad_zero;
      sv["initial_flow_auto"]["count_zero"] = (int64_t)shift.count_zero;
    }
  }
  if (check.on) {
    Value &cv = sv[check_key(check)];
    check_json(cv, check);
    cv["px"] = (int64_t)roi.width * roi.height;
    cv["rejected_px"] = (int64_t)rejected_px;
  }
  if (points) record_points(sv, check, *points);
  return sv;
}

}  // namespace ofcli
