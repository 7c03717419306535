// optflow.cpp — the `optflow` command-line driver, MI355X edition.
//
// Keeps the reference CLI/JSON surface (/root/reference/src/optflow.cpp) and calls
// the HIP engine through the C-ABI of include/tvl1.h.  The reference's functions, by their
// lines there, and where they live here:
//
//   main            optflow.cpp:29-72    argv, JSON (+gunzip), style dispatch      (this file)
//   from_file       optflow.cpp:75-178   config checks, devices, the split into batched and
//                                        per-pair pairs, workers, --plan, point-match
//                                        batching, timing_json, stats_json         (this file)
//                                        pair loop, p/q/scale, frame reuse, ROIs,
//                                        output naming              (pair_worker.cpp, PairWorker)
//   get_rois        optflow.cpp:228-261  top / bottom / custom / custom_diff       (config.hpp)
//   roi_from_array  optflow.cpp:302-310                                            (config.hpp)
//   solve_rois      optflow.cpp:312-392  upload, features flag, sorted ROI loop    (pair_worker.cpp)
//   solve_wrapper   optflow.cpp:395-496  TVL1 solve + map/flow/mask + TIFF output  (pair_worker.cpp)
//   generate_TV_args optflow.cpp:500-514                                           (config.hpp)
//   TVL1_solve      optflow.cpp:516-520  -> tvl1_calc (the drop-in boundary)
//   random_points   optflow.cpp:522-572                                            (points.hpp)
//   move_pm         optflow.cpp:574-593                                            (job.hpp)
//   upload_points   optflow.cpp:595-641  -> the render-ws payload is written to a
//                                           file (network upload is out of scope)  (this file)
//
// Not in the reference: the strip-batch worker (strip_worker.cpp), the decode-ahead pool
// (decode_pool.hpp), the device context, buffers and page-locked pool (device.hpp), the job
// state the workers share (job.hpp), and style 2 (from_list.cpp).
//
// Deliberate differences (documented in DESIGN.md):
//   * feature pre-alignment (features.cpp) runs on the engine's GPU ORB path; SURF
//     (features = 2, the default type) is served by ORB with a warning;
//   * per-image "rois" are honoured (the reference passes images["rois"], :140, so
//     they are silently ignored there);
//   * a malformed JSON file is an error (the reference ignores parse failure);
//   * build-only keys: "devices" (list of GPU ordinals, pairs sharded over them),
//     "inflight" (pairs in flight per GPU, default 3), "decode_threads" (slice decode-ahead
//     pool, default min(16, cores - 1)), "medianFiltering",
//     "matches_file", "stats_json", "timing_json" (per-stage host seconds of strip jobs),
//     "skip_existing", "pinned_host" (page-locked slices and
//     flows, default off), "initialFlow" ([dx, dy]: with "useInitialFlow", the pair's ROIs
//     are solved from that constant flow, tvl1_calc_init; or "auto": each ROI's constant is
//     the integer drift tvl1_estimate_shift finds on the ROI views the solve sees, searched
//     within "initialFlowMaxShift" px (default 32; per ROI at most min(W, H) / 4, and a ROI
//     too small for a search of 1 px is solved unseeded).  There is no gate on the estimate:
//     stats_json's "initial_flow_auto" carries sad / count, the summed and counted absolute
//     differences over the overlap at the estimate, and sad_zero / count_zero, the same at
//     (0, 0); a drift outside the search range shows as two means that barely differ; or
//     {"chain": [output of an earlier pair, ...]}, 1 to 64 links: each ROI's seed is the
//     composition, left to right, of the flows those pairs wrote for the same ROI key,
//     {link}{suffix}_x.tiff / _y.tiff, tvl1_compose_flow, DESIGN 15 -- the files must hold
//     "output_type": "flow" at this pair's scale, a map cannot be told from a flow; such pairs are
//     never batched, and combined with "consistency" only where the same object carries
//     "backward": "inverse" (the backward solve is seeded by tvl1_invert_flow of the forward
//     seed); "inverse": true beside "chain" takes the links of the opposite pair
//     (they walk from frame1 to frame0) and seeds the solve with the inverse of their
//     composition, by "inverseIterations" steps (1..32, default 8), counting the px whose
//     residual stays above "inverseTolerance" (px^2, default 0.01) into stats_json);
//     "seededStripBatch" (default false: a seeded pair leaves the strip batch and its ROIs are
//     solved one by one; true: a pair the *global* "useInitialFlow" / "initialFlow" seeds stays
//     in its tvl1_calc_batch chunk -- a numeric seed through tvl1_calc_batch_const_init,
//     "auto" through tvl1_calc_batch_auto_init on the packed strips of each ROI key, with the
//     per-pair path's range min(initialFlowMaxShift, 128, min(W, h) / 4), below 1 unseeded --
//     with the same flows, outputs and stats_json entries; per-image seed keys still send a
//     pair the per-pair way); "consistency" (false, true or {"alpha", "beta"}: style 1 only; each
//     ROI is also solved backward, the forward flow is scored against the backward one and
//     zeroed where the forward-backward check fails), "consistencyOversample"
//     (random_points candidates per point, default 4) and "consistencyOutput" (the score plane
//     as {output}{suffix}_fb.tiff); "zncc" (false, true or {"radius", "beta"}: style 1 only; the
//     one-solve check: each ROI's raw flow is scored by 1 - ZNCC of a window of frame0 against
//     frame1 warped back along the flow and zeroed where score > beta; not together
//     with "consistency"), "znccOversample" and "znccOutput" ({output}{suffix}_zncc.tiff);
//   * "style": 2 (from_list.cpp): the average-flow alignment of a slice list that the
//     reference declares and keeps disabled; keys "slices" | "file_list", "border",
//     "save_flow" (DESIGN 11, and 8 for where it departs from the disabled code).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "job.hpp"

using namespace ofcli;

namespace ofcli {

// --plan: one pair as the per-pair worker resolved it
Value plan_entry(const JobState &job, size_t i, const Value &im, const PairConfig &cfg, const Value &rois, int w0,
                 int h0) {
  Value pl;
  pl["index"] = (int64_t)i;
  pl["p"] = im["p"].asString();
  pl["q"] = im["q"].asString();
  pl["scale"] = (double)cfg.scale;
  pl["size0"][0] = w0;
  pl["size0"][1] = h0;
  pl["output"] = im["output"];
  pl["rois"] = rois;
  pl["output_type"] = cfg.otype;
  pl["features"] = cfg.features;
  pl["strip_batch"] = (bool)job.batch_ok[i];   // solved in a tvl1_calc_batch chunk
  if (cfg.init.automatic) {
    pl["initialFlow"] = "auto";   // tvl1_estimate_shift, then tvl1_calc_init, per ROI (or,
                                  // strip_batch: tvl1_calc_batch_auto_init per ROI key)
    pl["initialFlowMaxShift"] = cfg.init.max_shift;
  } else if (cfg.init.chained()) {   // the links' flow files composed (tvl1_compose_flow), then
                                     // tvl1_calc_init, per ROI; never in a strip batch
    for (const std::string &link : cfg.init.chain) pl["initialFlow"]["chain"].append(link);
    pl["initialFlow"]["links"] = (int64_t)cfg.init.chain.size();
    if (cfg.init.inverse || cfg.init.backward_inverse) {   // tvl1_invert_flow of the composed chain
      pl["initialFlow"]["inverse"] = cfg.init.inverse;
      pl["initialFlow"]["inverseIterations"] = cfg.init.inverse_iterations;
      pl["initialFlow"]["inverseTolerance"] = (double)cfg.init.inverse_tolerance;
      if (cfg.init.backward_inverse) pl["initialFlow"]["backward"] = "inverse";
    }
  } else if (cfg.init.on) {   // tvl1_calc_init per ROI
    pl["initialFlow"][0] = (double)cfg.init.dx;
    pl["initialFlow"][1] = (double)cfg.init.dy;
  }
  if (cfg.check.on) {   // (backward solve +) score
    Value &cv = pl[check_key(cfg.check)];
    check_json(cv, cfg.check);
    cv["oversample"] = cfg.check.oversample;
    cv["output"] = cfg.check.output;
  }
  const tvl1_params &tp = cfg.tv;
  pl["tv"]["tau"] = tp.tau;
  pl["tv"]["lambda"] = tp.lambda;
  pl["tv"]["theta"] = tp.theta;
  pl["tv"]["nscales"] = tp.nscales;
  pl["tv"]["warps"] = tp.warps;
  pl["tv"]["epsilon"] = tp.epsilon;
  pl["tv"]["iterations"] = tp.iterations;
  pl["tv"]["scaleStep"] = tp.scale_step;
  pl["tv"]["gamma"] = tp.gamma;
  pl["tv"]["medianFiltering"] = tp.median_filtering;
  pl["tv"]["fastMath"] = tp.fast_math;
  pl["tv"]["profile"] = tp.profile;
  pl["tv"]["innerIterations"] = tp.inner_iterations;
  pl["tv"]["outerIterations"] = tp.outer_iterations;
  for (auto &key : rois.memberNames()) pl["files"].append(im["output"].asString() + roi_suffix(key));
  return pl;
}

}  // namespace ofcli

namespace {

int fail(const std::string &what, int status = 2) {
  fprintf(stderr, "Error: %s\n", what.c_str());
  return status;
}

// a config that cannot run as written ends the job before any slice is read
int check_job(Value &images, const Value &args) {
  const size_t n = images.size();
  for (size_t i = 0; i < n; ++i) {
    const InitFlow f = initial_flow_of(images[i], args);
    if (f.error) return fail("pair " + std::to_string(i) + ": " + f.error, f.error_status);
    if (f.on && resolve_features(images[i], args))
      return fail("pair " + std::to_string(i) + ": " + kInitFlowFeatures);
  }
  for (size_t i = 0; i < n; ++i) {
    const char *ce = nullptr;
    const FlowCheck ck = check_of(images[i], args, &ce);
    if (ce) return fail("pair " + std::to_string(i) + ": " + ce);
    if (ck.on && resolve_features(images[i], args))
      return fail("pair " + std::to_string(i) + ": " + check_features_error(ck));
  }
  return 0;
}

// Strip jobs (every ROI "top" / "bottom", the production shape: two 100-row strips per pair)
bool is_strip_job(const Value &args) {
  bool strip_job = args.isMember("rois") && args["rois"].isObject() && args["rois"].size() > 0;
  if (strip_job)
    for (auto &k : args["rois"].memberNames()) strip_job = strip_job && (k == "top" || k == "bottom");
  return strip_job;
}

// build-only "strip_batch": strip pairs per tvl1_calc_batch (default 256; 0 or 1 = one
// tvl1_calc per strip, the r3 path).  A pair is batched when the job's ROIs are all top /
// bottom and its own keys are only the production ones (gen_cross_file_list.py:47-54);
// features, per-image ROIs / scales / TV parameters go the per-pair way.  So does a seeded
// pair, unless "seededStripBatch" keeps the pairs the global config seeds in the batch
// (per-image seed keys are not production keys).  Returns the pairs per batch, 0: no batching.
int split_pairs(JobState &job, bool strip_job) {
  Value &args = job.args;
  const int strip_batch = std::min(256, std::max(0, args.get("strip_batch", 256).asInt()));
  const std::string gotype = output_type_of(Value(), args);
  const bool seeded_batch = args.get("seededStripBatch", false).asBool();
  const bool batching = strip_job && strip_batch > 1 && !resolve_features(Value(), args) &&
                        (gotype == "map" || gotype == "flow" || gotype == "random_points");
  if (batching) {
    job.roi_keys = args["rois"].memberNames();
    job.roi_top = args["rois"].get("top", 300).asInt();
    job.roi_bottom = args["rois"].get("bottom", 300).asInt();
    static const char *kProd[] = {"p", "q", "pId", "qId", "pGroupId", "qGroupId", "output_name", "output"};
    for (size_t i = 0; i < job.n; ++i) {
      // a seeded pair's ROIs are solved one by one (tvl1_calc_init), or "seededStripBatch"
      // (a chained pair always: its seed is a plane per ROI, read from the links' files)
      const InitFlow seed = initial_flow_of(job.images[i], args);
      bool ok = job.images[i].isObject() && !seed.chained() && (seeded_batch || !seed.on);
      for (auto &k : job.images[i].memberNames())
        ok = ok && std::find_if(std::begin(kProd), std::end(kProd), [&](const char *x) { return k == x; }) !=
                       std::end(kProd);
      (ok ? job.batched : job.todo).push_back(i);
      job.batch_ok[i] = ok;
    }
  }
  if (!batching || job.plan_only) {   // --plan reports the split; the per-pair worker resolves every pair
    job.batched.clear();
    job.todo.clear();
    for (size_t i = 0; i < job.n; ++i) job.todo.push_back(i);
  }
  return strip_batch;
}

// `per_device` worker threads on every GPU, joined
void run_workers(JobState &job, int per_device, void (*worker)(JobState &, int)) {
  std::vector<std::thread> th;
  for (int f = 0; f < per_device; ++f)
    for (int d : job.devices) th.emplace_back(worker, std::ref(job), d);
  for (auto &t : th) t.join();
}

// point-match batching in pair order (optflow.cpp:160-175): the reference PUTs
// args["point_matches"] every batch_size pairs; here each batch is one JSON file.
// The batches are grouped in pair order (cheap), then serialised and written on the decode
// pool in parallel: 40,860 strip pairs' records took 1.6 s on one thread (profiles/r6/cli/)
void write_point_matches(JobState &job) {
  Value &args = job.args;
  const std::string mfile = args.get("matches_file", args["output_dir"].asString() + "/point_matches").asString();
  const int batch = args.get("batch_size", 100).asInt();
  const bool debug = job.debug;
  Value pending;
  bool any_since = false;
  size_t last_upload = 0;
  int nbatch = 0;
  std::vector<std::shared_future<void>> writes;
  auto upload = [&]() {
    const std::string owner = args.get("owner", "flyem").asString();
    const std::string mc = args.get("matchCollection", "forgetful_owner").asString();
    const std::string host = args.get("host", "10.40.3.162").asString();
    const std::string port = args.get("port", "8080").asString();
    const std::string url = "http://" + host + ":" + port + "/render-ws/v1/owner/" + owner +
                            "/matchCollection/" + mc + "/matches";
    const std::string path = mfile + "_" + std::to_string(nbatch++) + ".json";
    auto body = std::make_shared<Value>(std::move(pending));
    auto write = [body, path, url, debug] {
      const std::string payload = body->dump(3);
      if (debug) {
        std::lock_guard<std::mutex> lk(g_io_mutex);
        printf("%s\n%s", payload.c_str(), url.c_str());
      }
      FILE *f = fopen(path.c_str(), "w");
      if (!f) {
        std::lock_guard<std::mutex> lk(g_io_mutex);
        fprintf(stderr, "cannot write point matches to %s\n", path.c_str());
        return;
      }
      fprintf(f, "%s\n", payload.c_str());
      fclose(f);
    };
    if (debug) write();   // debug prints the payloads in batch order, as the reference does
    else writes.push_back(job.pool.submit(write));
  };
  for (size_t i = 0; i < job.n; ++i) {
    const Value &im = job.images[i];
    for (auto &pm : job.results[i].pms) pending.append(pm);
    if (output_type_of(im, args) == "random_points") {
      any_since = true;
      if (i > last_upload + (size_t)batch) {
        upload();
        pending = Value();
        last_upload = i;
        any_since = false;
      }
    }
  }
  if (any_since) upload();
  for (auto &w : writes) w.wait();
}

// build-only "timing_json": per-stage host timing (tools/cli_e2e.py)
void write_timing(const JobState &job, double records_s) {
  Value t;
  t["wall_s"] = secs_since(g_t0);
  t["pairs"] = (int64_t)job.n;
  t["decode"]["band_reads"] = (int64_t)g_band_reads.load();
  t["decode"]["band_read_s"] = 1e-9 * (double)g_band_read_ns.load();
  t["decode"]["threads"] = DecodePool::threads_asked(job.args);
  t["point_match_records_s"] = records_s;
  t["batch_workers"] = g_stage_workers.isNull() ? Value() : g_stage_workers;
  FILE *f = fopen(job.args["timing_json"].asString().c_str(), "w");
  if (f) {
    fprintf(f, "%s\n", t.dump(1).c_str());
    fclose(f);
  }
}

// build-only "stats_json": every pair's solves
void write_stats(const JobState &job) {
  Value st;
  for (size_t i = 0; i < job.n; ++i) {
    Value e = job.results[i].stats;
    e["index"] = (int64_t)i;
    e["ok"] = job.results[i].ok;
    e["host_pinned_bytes"] = (int64_t)PinnedPool::pinned_bytes();   // process total at exit
    st.append(e);
  }
  FILE *f = fopen(job.args["stats_json"].asString().c_str(), "w");
  if (f) {
    fprintf(f, "%s\n", st.dump(1).c_str());
    fclose(f);
  }
}

// ---------------------------------------------------------------- from_file ("style": 1)
int from_file(Value &args, bool plan_only) {
  {
    Value images = args["images"];
    if (const int rc = check_job(images, args)) return rc;
  }
  PinnedPool::install_if_asked(args.get("pinned_host", false).asBool(), plan_only);
  DecodePool pool(std::max(1, DecodePool::threads_asked(args)));
  JobState job(args, plan_only, pool);
  // build-only: shard pairs over several GPUs (contiguous chunks keep slice reuse)
  if (args.isMember("devices")) {
    for (size_t i = 0; i < args["devices"].size(); ++i) job.devices.push_back(args["devices"][i].asInt());
  } else {
    job.devices.push_back(args.get("device", 0).asInt());
  }
  const size_t ndev = job.devices.size();

  // build-only "inflight": pairs solved concurrently per GPU (one worker thread, ctx and
  // stream each) so one pair's residual read-backs overlap another pair's kernels.  Strip
  // jobs are launch- and sync-bound per solve, so they default to 8 in flight, full frames to 3
  // (DESIGN.md 5.1, 9).
  const bool strip_job = is_strip_job(args);
  const int strip_batch = split_pairs(job, strip_job);
  if (!job.batched.empty()) {
    // "inflight" batches per GPU (default 2: one batch's residual syncs overlap the other's
    // kernels), chunks small enough that every worker gets one
    const int binflight = std::max(1, args.get("inflight", 2).asInt());
    const size_t workers = ndev * (size_t)binflight;
    job.bchunk = std::max<size_t>(1, std::min<size_t>(strip_batch, (job.batched.size() + workers - 1) / workers));
    run_workers(job, binflight, run_strip_worker);
    for (size_t i = 0; i < job.n; ++i)
      if (job.deferred[i]) job.todo.push_back(i);
    std::sort(job.todo.begin(), job.todo.end());
  }
  const size_t m = job.todo.size();
  job.chunk = std::max<size_t>(1, std::min<size_t>(16, m / std::max<size_t>(1, ndev * 4)));
  const int inflight = std::max(1, args.get("inflight", strip_job ? 8 : 3).asInt());
  if (m == 0) {
  } else if (plan_only || (ndev == 1 && inflight == 1)) {
    run_pair_worker(job, job.devices[0]);
  } else {
    run_workers(job, inflight, run_pair_worker);
  }
  if (job.hard_error) return 1;

  if (plan_only) {
    Value out;
    for (auto &p : job.plans) out.append(p);
    printf("%s\n", out.dump(1).c_str());
    return 0;
  }
  const auto t_records = Clock::now();
  write_point_matches(job);
  const double records_s = secs_since(t_records);
  if (args.isMember("timing_json")) write_timing(job, records_s);
  if (args.isMember("stats_json")) write_stats(job);
  if (const char *e = getenv("OPTFLOW_PINNED_TRACE"); e && atoi(e))
    fprintf(stderr, "%s\n", PinnedPool::summary().c_str());
  return 0;  // like the reference: per-pair failures are reported, exit status 0
}

}  // namespace

static void usage() {
  printf("Usage: optflow [--plan] <config.json[.gz]>\n"
         "       optflow --decode <image> <out.tiff> [scale]\n"
         "  Dense TV-L1 optical flow for FIB-SEM slice pairs on AMD MI355X (gfx950).\n"
         "  --plan    resolve the config (pairs, ROIs, output files, TV-L1 parameters)\n"
         "            and print it as JSON without touching the GPU.\n"
         "  \"style\": 2 in the config aligns a slice list (\"slices\" or \"file_list\") to the\n"
         "            average of each slice's six neighbours and writes {output_dir}/{i}.tiff.\n"
         "  --decode  read an image as the pair loop does (IMREAD_GRAYSCALE + optional\n"
         "            cv::resize pre-scale) and write it as an 8-bit TIFF.\n");
}

int main(int argc, const char *argv[]) {
  bool plan = false;
  std::string filename;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-h" || a == "--help") {
      usage();
      return 0;
    }
    if (a == "--plan") {
      plan = true;
      continue;
    }
    if (a == "--decode-bands") {   // tests: the ROI-limited read of strip jobs
      // optflow --decode-bands <image> <out.tiff> <scale> <top> <bottom>: the top and bottom
      // row bands of the pre-scaled slice (get_rois' top / bottom), stacked, as an 8-bit TIFF;
      // stdout says whether only their rows were read
      if (i + 5 >= argc) {
        usage();
        return 2;
      }
      const float sc = (float)atof(argv[i + 3]);
      const int top = atoi(argv[i + 4]), bottom = atoi(argv[i + 5]);
      int W = 0, H = 0;
      bool partial = false;
      std::vector<ofio::Image8> bands;
      std::string err;
      if (!ofio::read_gray8_bands(argv[i + 1], sc,
                                  [&](int, int h) {
                                    return std::vector<std::pair<int, int>>{{0, top}, {h - bottom, h}};
                                  },
                                  W, H, bands, err, &partial)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      ofio::Image8 out;
      out.width = W;
      out.height = bands[0].height + bands[1].height;
      out.data.resize((size_t)W * out.height);
      memcpy(out.data.data(), bands[0].data.data(), bands[0].data.size());
      memcpy(out.data.data() + bands[0].data.size(), bands[1].data.data(), bands[1].data.size());
      if (!ofio::write_tiff_u8(argv[i + 2], out, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      printf("%dx%d %s\n", W, H, partial ? "partial" : "whole");
      return 0;
    }
    if (a == "--decode-flow") {   // tests: a flow file read as a chain's link is, and rewritten
      if (i + 2 >= argc) {
        usage();
        return 2;
      }
      int W = 0, H = 0;
      ofio::HostVec<float> data;
      std::string err;
      if (!ofio::read_tiff_f32(argv[i + 1], W, H, data, err) ||
          !ofio::write_tiff_f32(argv[i + 2], data.data(), W, H, (size_t)W * sizeof(float), err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      return 0;
    }
    if (a == "--decode") {
      if (i + 2 >= argc) {
        usage();
        return 2;
      }
      ofio::Image8 img, out;
      std::string err;
      if (!ofio::read_gray8(argv[i + 1], img, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      const double sc = i + 3 < argc ? atof(argv[i + 3]) : 1.0;
      if (sc != 1.0) ofio::resize_u8(img, (float)sc, (float)sc, out);
      else out = img;
      if (!ofio::write_tiff_u8(argv[i + 2], out, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      return 0;
    }
    filename = a;
  }
  if (filename.empty()) {
    usage();
    return 2;
  }
  std::string text, err;
  if (!ofio::read_file(filename, text, err, true)) {
    fprintf(stderr, "%s\n", err.c_str());
    return 2;
  }
  Value args;
  try {
    args = ofjson::parse(text);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s: %s\n", filename.c_str(), e.what());
    return 2;
  }
  int rc = 0;
  const int style = args.get("style", 1).asInt();
  if (style == 1 || style == 2) {
    try {
      rc = style == 1 ? from_file(args, plan) : from_list(args, plan);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      rc = 2;
    }
  } else {
    fprintf(stderr, "style %d is not implemented (only style 1, optflow.cpp:62-66)\n", style);
    rc = 2;
  }
  return rc;
}
