// from_list.cpp — "style": 2.
// Average-flow alignment of a slice list (the reference's disabled average_flow /
// remap_and_save, optflow.cpp:180-226, 263-300): for i = 3 .. n-4 the six
// neighbours of slice i are blended (tvl1_blend6_u8), TV-L1 is solved from the pre-scaled
// slice to the pre-scaled blend, and the slice is warped by the flow onto a canvas with
// `border` px around it (tvl1_remap_flow_u8) and written as {output_dir}/{i}.tiff.
//
// Every slice is decoded once (DecodePool, decode-ahead) and uploaded once at full size into
// a device ring of 7 + inflight - 1 slots, where its pre-scaled copy is made once.  `inflight`
// consecutive outputs form a group: the ring then holds exactly the slices the group reads, the
// group's outputs run concurrently, each on a worker's own ctx and stream, and the slots are
// refilled between groups (no work is in flight then).
#include <cstring>

#include "job.hpp"

namespace ofcli {
namespace {

struct ListSlot {
  DevBuf full, pre;
  long index = -1;
};

struct ListWorker {
  DeviceCtx dc;
  DevBuf blend, pre, canvas;
  DevBuf u, v;
  double gpu_s = 0, host_prescale_s = 0;
};

enum PrePath { kPreNone, kPreDevice, kPreHost };
const char *pre_name(PrePath p) { return p == kPreNone ? "none" : (p == kPreDevice ? "device" : "host"); }

PrePath pre_path(double scale, int W, int H) {
  if (scale == 1.0) return kPreNone;
  return scale == 0.5 && W % 2 == 0 && H % 2 == 0 ? kPreDevice : kPreHost;
}

}  // namespace

int from_list(Value &args, bool plan_only) {
  auto fail = [](const std::string &what) {
    fprintf(stderr, "Error: %s\n", what.c_str());
    return 2;
  };
  // ---- the job, checked before the GPU is touched
  const bool has_slices = args.isMember("slices"), has_list = args.isMember("file_list");
  if (has_slices == has_list)
    return fail("style 2 takes exactly one of \"slices\" (an array of paths) and \"file_list\" (a text file)");
  std::vector<std::string> names;
  if (has_slices) {
    if (!args["slices"].isArray()) return fail("\"slices\" must be an array of paths");
    for (size_t i = 0; i < args["slices"].size(); ++i) names.push_back(args["slices"][i].asString());
  } else {
    std::string text, err;
    if (!ofio::read_file(args["file_list"].asString(), text, err, false))
      return fail("cannot read file_list " + args["file_list"].asString() + ": " + err);
    size_t p = 0;
    while (p <= text.size()) {
      size_t e = text.find('\n', p);
      if (e == std::string::npos) e = text.size();
      std::string line = text.substr(p, e - p);
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty()) names.push_back(line);
      p = e + 1;
    }
  }
  const size_t n = names.size();
  if (n < 7) return fail("style 2 needs at least 7 slices (got " + std::to_string(n) + ")");
  if (!args.isMember("output_dir")) return fail("style 2 needs \"output_dir\"");
  const std::string outdir = args["output_dir"].asString();
  const int border = args.get("border", 0).asInt();
  if (border < 0) return fail("\"border\" must be >= 0 (got " + std::to_string(border) + ")");
  const double scale = args.get("scale", 0.5).asDouble();
  if (!(scale > 0.0)) return fail("\"scale\" must be > 0");
  int device = args.get("device", 0).asInt();
  if (args.isMember("devices") && args["devices"].size() > 0) {
    device = args["devices"][0].asInt();
    if (args["devices"].size() > 1)
      fprintf(stderr, "style 2 runs on one GPU: using device %d, the first of \"devices\"\n", device);
  }
  const int inflight = std::max(1, args.get("inflight", 3).asInt());
  const bool skip_existing = args.get("skip_existing", false).asBool();
  const bool save_flow = args.get("save_flow", false).asBool();
  auto out_path = [&](size_t i) { return outdir + "/" + std::to_string(i) + ".tiff"; };

  PinnedPool::install_if_asked(args.get("pinned_host", false).asBool(), plan_only);

  if (plan_only) {
    // the pre-scale path depends on the slices' size: that of the first readable one
    int W = 0, H = 0;
    for (size_t j = 0; j < n && W == 0; ++j) {
      ofio::Image8 img;
      std::string err;
      if (ofio::read_gray8(names[j], img, err) && img.width > 0 && img.height > 0) W = img.width, H = img.height;
    }
    if (W == 0) return fail("no slice of the list can be read");
    for (size_t i = 3; i + 3 < n; ++i) {
      Value pl;
      pl["index"] = (int64_t)i;
      pl["input"] = names[i];
      int k = 0;
      for (int d = -3; d <= 3; ++d)
        if (d) pl["neighbours"][k++] = names[i + d];
      pl["output"] = out_path(i);
      pl["prescale"] = pre_name(pre_path(scale, W, H));
      printf("%s\n", pl.dump().c_str());
    }
    return 0;
  }

  // ---- which slices are read: those of outputs that are not skipped
  std::vector<char> want(n, 0), need(n, 0);
  for (size_t i = 3; i + 3 < n; ++i) {
    want[i] = !(skip_existing && file_exists(out_path(i)));
    if (want[i])
      for (size_t j = i - 3; j <= i + 3; ++j) need[j] = 1;
  }
  const int nthreads = std::max(1, DecodePool::threads_asked(args));
  DecodePool pool(nthreads);
  const size_t R = 7 + (size_t)inflight - 1;
  const size_t ahead = 2 * R;   // slices queued for decode beyond the one waited for
  std::vector<LoadFuture> loads(n);
  size_t queued = 0;
  auto queue_to = [&](size_t upto) {
    for (; queued < std::min(n, upto); ++queued)
      if (need[queued]) loads[queued] = pool.load(names[queued], 1.0f);
  };

  std::vector<ListWorker> workers((size_t)inflight);
  std::vector<ListSlot> ring(R);
  hipStream_t up = nullptr;
  int rc = 0;
  auto cleanup = [&] {
    for (auto &w : workers) {
      if (w.dc.stream) (void)hipStreamSynchronize(w.dc.stream);
      for (DevBuf *b : {&w.blend, &w.pre, &w.canvas, &w.u, &w.v}) b->reset();
      w.dc.close();
    }
    for (auto &s : ring) s.full.reset(), s.pre.reset();
    if (up) (void)hipStreamDestroy(up);
  };
  auto hard = [&](const std::string &what) {
    std::lock_guard<std::mutex> lk(g_io_mutex);
    fprintf(stderr, "Error: %s\n", what.c_str());
    rc = 1;
  };
  for (auto &w : workers) {
    std::string err;
    if (!w.dc.open(device, err)) {
      hard("cannot use GPU " + std::to_string(device) + ": " + err);
      cleanup();
      return 1;
    }
    const tvl1_params prm = generate_TV_args(Value(), args);
    if (tvl1_set_params(w.dc.ctx, &prm) != TVL1_OK) {
      const std::string e = tvl1_last_error(w.dc.ctx);
      cleanup();
      return fail(e);
    }
  }
  const tvl1_params prm = generate_TV_args(Value(), args);
  if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) {
    hard("hipStreamCreate failed");
    cleanup();
    return 1;
  }

  int W = 0, H = 0, fw = 0, fh = 0;   // slice size (the first readable one's), solve size
  PrePath path = kPreNone;
  std::vector<char> bad(n, 0);
  std::vector<Value> stats(n);
  std::vector<std::pair<size_t, std::shared_future<void>>> writes;
  std::mutex writes_mutex;
  double decode_wait_s = 0, upload_s = 0;
  size_t written = 0;

  // slice j into its ring slot: wait for its decode, check its size, upload, pre-scale once
  auto enter = [&](size_t j) -> bool {
    ListSlot &s = ring[j % R];
    if (s.index == (long)j) return true;
    s.index = -1;
    queue_to(j + 1 + ahead);
    const auto t0 = Clock::now();
    const std::shared_ptr<Loaded> r = loads[j].get();
    loads[j] = LoadFuture();
    decode_wait_s += secs_since(t0);
    if (!r->ok) {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      fprintf(stderr, "Error: %s: %s\n", names[j].c_str(), r->err.empty() ? "cannot read" : r->err.c_str());
      return false;
    }
    if (W == 0) {
      W = r->img.width, H = r->img.height;
      path = pre_path(scale, W, H);
      fw = W, fh = H;
      if (path == kPreDevice) fw = W / 2, fh = H / 2;
      if (path == kPreHost) ofio::resized_size(W, H, (float)scale, (float)scale, fw, fh);
      if (W + 2 * (int64_t)border > 32767 || H + 2 * (int64_t)border > 32767 || fw < 1 || fh < 1) {
        hard("slice size " + std::to_string(W) + "x" + std::to_string(H) + " with border " +
             std::to_string(border) + " is not served (canvas above 32767, or an empty solve)");
        return false;
      }
    }
    if (r->img.width != W || r->img.height != H) {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      fprintf(stderr, "Error: %s: size %dx%d differs from the list's %dx%d\n", names[j].c_str(),
              r->img.width, r->img.height, W, H);
      return false;
    }
    const auto t1 = Clock::now();
    const size_t full = (size_t)W * H, pre = (size_t)fw * fh;
    if (!s.full.p && !s.full.alloc(full)) return hard("hipMalloc failed for a slice"), false;
    if (path != kPreNone && !s.pre.p && !s.pre.alloc(pre))
      return hard("hipMalloc failed for a pre-scaled slice"), false;
    bool ok = hipMemcpyAsync(s.full.p, r->img.data.data(), full, hipMemcpyHostToDevice, up) == hipSuccess;
    ofio::Image8 small;
    if (ok && path == kPreDevice)
      ok = tvl1_half_u8(workers[0].dc.ctx, s.full.u8(), (size_t)W, W, H, s.pre.u8(), (size_t)fw, up) == TVL1_OK;
    if (ok && path == kPreHost) {
      ofio::resize_u8(r->img, (float)scale, (float)scale, small);
      ok = hipMemcpyAsync(s.pre.p, small.data.data(), pre, hipMemcpyHostToDevice, up) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(up) == hipSuccess;   // the host buffers go away here
    upload_s += secs_since(t1);
    if (!ok) return hard("upload of " + names[j] + " failed"), false;
    s.index = (long)j;
    return true;
  };

  // output i on worker w: blend, pre-scale the blend, solve, remap, download, queue the writes
  auto align = [&](ListWorker &w, size_t i) {
    const auto t0 = Clock::now();
    DeviceCtx &dc = w.dc;
    const size_t full = (size_t)W * H, pre = (size_t)fw * fh;
    const int CW = W + 2 * border, CH = H + 2 * border;
    // the contexts were opened on the main thread; a fresh thread's current device is 0, and
    // the buffers below must live on the GPU that the ctx and its stream run on
    if (hipSetDevice(dc.device) != hipSuccess) return hard("cannot use GPU " + std::to_string(dc.device));
    auto alloc = [&](DevBuf &b, size_t bytes) { return b.p || b.alloc(bytes); };
    if (!alloc(w.blend, full) || !alloc(w.canvas, (size_t)CW * CH) || !alloc(w.u, pre * 4) || !alloc(w.v, pre * 4) ||
        (path != kPreNone && !alloc(w.pre, pre)))
      return hard("hipMalloc failed for the buffers of an output");
    const uint8_t *fr[6];
    size_t pt[6];
    int k = 0;
    for (int d = -3; d <= 3; ++d)
      if (d) fr[k] = ring[(i + d) % R].full.u8(), pt[k++] = (size_t)W;
    const ListSlot &me = ring[i % R];
    auto engine_err = [&](const char *what) { hard(std::string(what) + ": " + tvl1_last_error(dc.ctx)); };
    if (tvl1_blend6_u8(dc.ctx, fr, pt, W, H, w.blend.u8(), (size_t)W, dc.stream) != TVL1_OK) return engine_err("blend");
    const uint8_t *I0 = me.full.u8(), *I1 = w.blend.u8();
    if (path == kPreDevice) {
      if (tvl1_half_u8(dc.ctx, w.blend.u8(), (size_t)W, W, H, w.pre.u8(), (size_t)fw, dc.stream) != TVL1_OK)
        return engine_err("pre-scale");
      I0 = me.pre.u8(), I1 = w.pre.u8();
    } else if (path == kPreHost) {   // correct but slow: the blend goes through the host's cv::resize
      const auto th = Clock::now();
      ofio::Image8 b, small;
      b.width = W, b.height = H;
      b.data.resize(full);
      if (hipMemcpyAsync(b.data.data(), w.blend.p, full, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
          hipStreamSynchronize(dc.stream) != hipSuccess)
        return hard("download of a blend failed");
      ofio::resize_u8(b, (float)scale, (float)scale, small);
      if (hipMemcpyAsync(w.pre.p, small.data.data(), pre, hipMemcpyHostToDevice, dc.stream) != hipSuccess ||
          hipStreamSynchronize(dc.stream) != hipSuccess)
        return hard("upload of a pre-scaled blend failed");
      I0 = me.pre.u8(), I1 = w.pre.u8();
      w.host_prescale_s += secs_since(th);
    }
    tvl1_stats st;
    memset(&st, 0, sizeof st);
    std::vector<int32_t> warp_iters((size_t)TVL1_MAX_LEVELS * std::max(1, prm.warps), -1);
    st.warp_iterations = warp_iters.data();
    st.warp_iterations_capacity = (int32_t)warp_iters.size();
    const size_t fp = (size_t)fw * sizeof(float);
    if (tvl1_calc(dc.ctx, I0, (size_t)fw, I1, (size_t)fw, fw, fh, w.u.f32(), w.v.f32(), fp, &st, dc.stream) != TVL1_OK)
      return engine_err("solve");
    if (tvl1_remap_flow_u8(dc.ctx, me.full.u8(), (size_t)W, W, H, w.u.f32(), w.v.f32(), fp, fw, fh, 1.0 / scale,
                           border, w.canvas.u8(), (size_t)CW, dc.stream) != TVL1_OK)
      return engine_err("remap");
    auto img = std::make_shared<ofio::Image8>();
    img->width = CW, img->height = CH;
    img->data.resize((size_t)CW * CH);
    auto fx = std::make_shared<ofio::HostVec<float>>(), fy = std::make_shared<ofio::HostVec<float>>();
    bool ok = hipMemcpyAsync(img->data.data(), w.canvas.p, img->data.size(), hipMemcpyDeviceToHost, dc.stream) == hipSuccess;
    if (ok && save_flow) {
      fx->resize(pre), fy->resize(pre);
      ok = hipMemcpyAsync(fx->data(), w.u.p, pre * 4, hipMemcpyDeviceToHost, dc.stream) == hipSuccess &&
           hipMemcpyAsync(fy->data(), w.v.p, pre * 4, hipMemcpyDeviceToHost, dc.stream) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(dc.stream) != hipSuccess) return hard("download of an output failed");
    w.gpu_s += secs_since(t0);
    Value sv;
    sv["index"] = (int64_t)i;
    sv["input"] = names[i];
    sv["output"] = out_path(i);
    sv["prescale"] = pre_name(path);
    sv["levels"] = st.levels;
    sv["iterations"] = (int64_t)st.iterations_total;
    const size_t nw = std::min(warp_iters.size(), (size_t)std::max(0, st.levels) * std::max(1, prm.warps));
    for (size_t q = 0; q < nw; ++q) sv["warp_iterations"][(int)q] = warp_iters[q];
    stats[i] = sv;
    const std::string base = outdir + "/" + std::to_string(i), path_out = out_path(i);
    const int fw_ = fw, fh_ = fh;
    auto job = [img, fx, fy, base, path_out, save_flow, fw_, fh_, fp] {
      std::string e;
      if (!ofio::write_tiff_u8(path_out, *img, e)) throw std::runtime_error(path_out + ": " + e);
      if (save_flow && (!ofio::write_tiff_f32(base + "_x.tiff", fx->data(), fw_, fh_, fp, e) ||
                        !ofio::write_tiff_f32(base + "_y.tiff", fy->data(), fw_, fh_, fp, e)))
        throw std::runtime_error(base + "_x/_y.tiff: " + e);
    };
    std::lock_guard<std::mutex> lk(writes_mutex);
    writes.emplace_back(i, pool.submit(job));
  };

  const double setup_s = secs_since(g_t0);   // process start, config, contexts and streams
  const auto t_loop = Clock::now();
  for (size_t i0 = 3; i0 + 3 < n && rc == 0; i0 += (size_t)inflight) {
    const size_t i1 = std::min(n - 3, i0 + (size_t)inflight);   // outputs [i0, i1)
    // the group's slices enter the ring in list order; a slice that cannot is marked
    for (size_t j = i0 - 3; j < i1 + 3 && rc == 0; ++j)
      if (need[j] && !bad[j] && ring[j % R].index != (long)j && !enter(j)) bad[j] = 1;
    if (rc) break;
    std::vector<size_t> run;
    for (size_t i = i0; i < i1; ++i) {
      bool ok = want[i];
      for (size_t j = i - 3; j <= i + 3 && ok; ++j) ok = !bad[j];
      if (ok) run.push_back(i);
    }
    for (size_t i : run) printf("N: %zu %s\n", i, names[i].c_str());
    fflush(stdout);
    // Unlike style 1 there is no recovery after an engine or device error: hard() sets rc to 1
    // and the job ends after this group. rc is written by the workers under g_io_mutex and read
    // here without it, which is sound only because every read comes after the join below. An
    // exception (bad_alloc from a host buffer, say) must not leave a worker thread, where it
    // would end the process: it becomes a hard error too.
    auto guarded = [&](size_t k) {
      try {
        align(workers[k], run[k]);
      } catch (const std::exception &e) {
        hard("output " + std::to_string(run[k]) + ": " + e.what());
      }
    };
    if (run.size() == 1) {
      guarded(0);
    } else {
      std::vector<std::thread> th;
      for (size_t k = 0; k < run.size(); ++k) th.emplace_back(guarded, k);
      for (auto &t : th) t.join();
    }
  }
  const auto tw = Clock::now();
  for (auto &wr : writes) {
    try {
      wr.second.get();
      ++written;
    } catch (const std::exception &e) {
      fprintf(stderr, "Error: cannot write %s\n", e.what());
      stats[wr.first]["write_failed"] = true;
    }
  }
  const double write_wait_s = secs_since(tw);
  const double loop_s = secs_since(t_loop);   // first decode wait to last write

  if (args.isMember("timing_json")) {
    Value t;
    t["wall_s"] = secs_since(g_t0);
    t["slices"] = (int64_t)written;
    t["slices_per_s"] = written / std::max(1e-9, secs_since(g_t0));
    t["setup_s"] = setup_s;
    t["loop_s"] = loop_s;
    t["loop_slices_per_s"] = written / std::max(1e-9, loop_s);
    t["inflight"] = inflight;
    t["ring_slots"] = (int64_t)R;
    t["prescale"] = pre_name(path);
    t["decode"]["threads"] = nthreads;
    t["decode"]["wait_s"] = decode_wait_s;
    t["upload_prescale_s"] = upload_s;
    t["write_wait_s"] = write_wait_s;
    for (size_t k = 0; k < workers.size(); ++k) {
      t["workers"][(int)k]["gpu_s"] = workers[k].gpu_s;
      t["workers"][(int)k]["host_prescale_s"] = workers[k].host_prescale_s;
    }
    FILE *f = fopen(args["timing_json"].asString().c_str(), "w");
    if (f) {
      fprintf(f, "%s\n", t.dump(1).c_str());
      fclose(f);
    }
  }
  if (args.isMember("stats_json")) {
    Value st;
    for (size_t i = 3; i + 3 < n; ++i)
      if (!stats[i].isNull()) st.append(stats[i]);
    FILE *f = fopen(args["stats_json"].asString().c_str(), "w");
    if (f) {
      fprintf(f, "%s\n", st.isNull() ? "[]" : st.dump(1).c_str());
      fclose(f);
    }
  }
  cleanup();
  return rc;   // like style 1: a slice that cannot be used is reported, exit status 0
}

}  // namespace ofcli
