// strip_worker.cpp — batched strip jobs.  The production shape (SURVEY 3.2,
// gen_cross_file_list.py:75-99: global top / bottom ROIs at scale 0.5, per-image keys only
// p, q, the ids and output_name) is two ~100-row strips per pair: one tvl1_calc per strip
// is ~400 launches of a few microseconds, so the GPU idles on dispatch.  Here a worker
// takes a chunk of such pairs, reads only the strips' rows of each slice (read_gray8_bands),
// and solves each ROI key's strips of the whole chunk in one tvl1_calc_batch (every strip's
// flow and iteration counts identical to its own tvl1_calc), then writes each pair's
// outputs as solve_wrapper would (optflow.cpp:395-496).  Pairs that turn out not to fit
// (frames of different sizes, an ROI outside the slice, an unreadable file) are solved by
// the per-pair path afterwards, which reports them exactly as before.
//
// A chunk goes through StripWorker::run's steps: collect its items, retire decodes, then per
// attempt (solve_chunk) each ROI key's solve_key -- pack and upload, solve with the seed, score
// and reject, read back, write the pairs' outputs --, the debug point draws, and the commit
// of the results or one retry on a rebuilt context.
#include <cstring>

#include "job.hpp"
#include "points.hpp"

namespace ofcli {
namespace {

// a pair of the chunk whose two slices decoded to equal sizes, with their bands
struct Item {
  size_t i;
  Value im;
  std::shared_ptr<Loaded> p, q;
};

// what one attempt at a chunk gathers before it is committed
struct Attempt {
  std::string e;
  bool ok = true;
  std::vector<std::vector<Value>> solves;   // per pair, per ROI key: the stats_json records
  // debug random_points: the flows (and scores) of every key, drawn pair by pair afterwards so
  // the unseeded generator is consumed in the per-pair path's order (pair, then key)
  std::vector<std::vector<float>> dbg_fx, dbg_fy, dbg_fs;
  Attempt(size_t nb, size_t nkeys) : solves(nb), dbg_fx(nkeys), dbg_fy(nkeys), dbg_fs(nkeys) {}
};

// one ROI key's strips of the chunk: nb solves of one W x h geometry, packed
struct KeyBatch {
  size_t kk;   // index into roi_keys
  int nb, W, h, y0;
  size_t px;   // W * h
  std::vector<tvl1_stats> st;
  std::vector<int32_t> wi;   // the stats' warp_iterations
  // the chunk's seed, as solve_wrapper's per ROI: a constant, or each strip's drift within
  // auto_R on the packed strips (too small to search: unseeded)
  bool seeded = false;
  int auto_R = 0;
  std::vector<tvl1_shift> shifts;
  std::vector<uint64_t> rejected;
  // sampled random_points: each pair's candidates, drawn on the decode pool
  std::vector<Points> pts;
  std::vector<uint64_t> tot;
  std::vector<std::shared_future<void>> draws;
  Clock::time_point t0;
  double secs = 0;
  std::vector<float> fx, fy;   // whole flows (TIFF outputs, debug point matches), or the candidates'
  std::vector<float> fs;       // a check's scores, likewise
};

struct StripWorker {
  JobState &job;
  const int device;
  DeviceCtx dc;
  const PairConfig cfg;   // the job's global config: a pair with keys of its own is not batched
  const int mode;         // tvl1_postprocess' (no features on this path)
  // device buffers (grown): the chunk's packed frames and flows of one ROI key; with a check
  // also the scores and, forward-backward, the backward flows
  DevBuf dP, dQ, dU, dV, dUb, dVb, dS;
  PinnedPair host;   // page-locked packing buffers (reused)
  std::map<std::string, double> tm;   // stage -> seconds on this worker (timing_json)
  size_t t_chunks = 0, t_pairs = 0;
  hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr;   // the chunk's uploads on the stream
  std::map<std::string, LoadFuture> pending;       // path -> its bands (this chunk + the next)

  StripWorker(JobState &j, int d)
      : job(j), device(d), cfg(resolve_pair(Value(), j.args)), mode(cfg.otype == "map" ? 1 : 0) {}

  void release() {
    for (DevBuf *b : {&dP, &dQ, &dU, &dV, &dUb, &dVb, &dS}) b->reset();
    host.reset();
  }
  bool grow(size_t px) {
    if (px > dP.cap) {
      for (DevBuf *b : {&dP, &dQ, &dU, &dV, &dUb, &dVb, &dS}) b->reset();
      const bool ok = alloc_together({&dP, &dQ}, px) && alloc_together({&dU, &dV}, 4 * px) &&
                      (!cfg.check.on || cfg.check.zncc() || alloc_together({&dUb, &dVb}, 4 * px)) &&
                      (!cfg.check.on || dS.alloc(4 * px));
      if (!ok) {
        for (DevBuf *b : {&dP, &dQ, &dU, &dV, &dUb, &dVb, &dS}) b->reset();
        return false;
      }
    }
    return host.reserve(px);
  }
  void fail(Attempt &at, const std::string &what, tvl1_status st) {
    at.e = what + (dc.ctx ? std::string(": ") + tvl1_last_error(dc.ctx) : std::string());
    dc.faulted = device_fault(st);
    at.ok = false;
  }

  void queue_chunk(size_t start) {
    for (size_t k = start; k < std::min(job.batched.size(), start + job.bchunk); ++k)
      for (const char *side : {"p", "q"}) {
        const std::string path = job.images[job.batched[k]][side].asString();
        if (!pending.count(path))
          pending.emplace(path, job.pool.load_bands(path, cfg.scale, job.roi_keys, job.roi_top, job.roi_bottom));
      }
  }

  // step 1: the chunk's pairs that a batch can take
  std::vector<Item> collect(size_t start, size_t end) {
    std::vector<Item> items;
    for (size_t k = start; k < end; ++k) {
      const size_t i = job.batched[k];
      Item it{i, job.images[i], nullptr, nullptr};
      const std::string p = it.im["p"].asString(), q = it.im["q"].asString();
      fill_defaults(it.im, job.args, cfg.scale);
      {
        const auto tw = Clock::now();
        it.p = pending.at(p).get();
        it.q = pending.at(q).get();
        tm["wait_bands"] += secs_since(tw);
      }
      if (!it.p->ok || !it.q->ok || it.p->W != it.q->W || it.p->H != it.q->H) {
        job.deferred[i] = 1;   // the per-pair path reports or aligns it as the reference does
        continue;
      }
      {
        std::lock_guard<std::mutex> lk(g_io_mutex);
        printf("%s %s\n", p.c_str(), q.c_str());
        fflush(stdout);
      }
      if (job.skip_existing && !cfg.random_points() && outputs_exist(it.im["output"].asString(), job.roi_keys)) {
        job.results[i].done = job.results[i].ok = true;
        continue;
      }
      items.push_back(std::move(it));
    }
    return items;
  }

  // step 2: slices no pair of the next chunk names leave the map
  void retire_decodes(const ChunkWalk &w) {
    std::map<std::string, LoadFuture> keep;
    for (size_t k = w.next_start; k < w.next_end(); ++k)
      for (const char *side : {"p", "q"}) {
        const std::string path = job.images[job.batched[k]][side].asString();
        auto f = pending.find(path);
        if (f != pending.end()) keep.emplace(path, f->second);
      }
    pending.swap(keep);
  }

  // step 3a: the strips into the page-locked buffers and onto the device
  bool pack_and_upload(const std::vector<Item> &items, const KeyBatch &k, Attempt &at) {
    const auto ts = Clock::now();
    for (int b = 0; b < k.nb; ++b) {
      memcpy(host.a + k.px * b, items[b].p->bands[k.kk].data.data(), k.px);
      memcpy(host.b + k.px * b, items[b].q->bands[k.kk].data.data(), k.px);
    }
    tm["pack"] += secs_since(ts);
    (void)hipEventRecord(ev_up0, dc.stream);
    if (hipMemcpyAsync(dP.p, host.a, k.px * k.nb, hipMemcpyHostToDevice, dc.stream) != hipSuccess ||
        hipMemcpyAsync(dQ.p, host.b, k.px * k.nb, hipMemcpyHostToDevice, dc.stream) != hipSuccess) {
      fail(at, "upload failed", TVL1_EHIP);
      return false;
    }
    (void)hipEventRecord(ev_up1, dc.stream);
    return true;
  }

  // random_points without debug: which px each pair reports depends only on its bands' masks,
  // so the draws run on the decode pool while the batch solves (they were 16 % of a strip
  // worker's time on the worker thread, profiles/r6/cli/)
  void submit_draws(const std::vector<Item> &items, KeyBatch &k) {
    const int nb = k.nb, per = std::max(1, nb / 16);   // 16 jobs of the chunk's pairs
    const size_t kk = k.kk;
    const int nc = draw_count(cfg);   // a check: oversample times as many, the candidates
    for (int b0 = 0; b0 < nb; b0 += per)
      k.draws.push_back(job.pool.submit([&items, &k, b0, per, nb, kk, nc] {
        for (int b = b0; b < std::min(nb, b0 + per); ++b) {
          const ofio::Image8 &a = items[b].p->bands[kk], &c = items[b].q->bands[kk];
          k.pts[b] = sample_points([&](int y) { return a.row(y); }, [&](int y) { return c.row(y); }, a.width,
                                   a.height, nc, &k.tot[b]);
        }
      }));
  }

  // step 3b: the forward solve from the seed, the check's score of the raw flows, the
  // post-process, and the px that failed the check zeroed and counted
  tvl1_status solve_scored(KeyBatch &k) {
    const int nb = k.nb, W = k.W, h = k.h;
    const size_t px = k.px, fp = 4 * (size_t)W, fs = 4 * px;
    const InitFlow &seed = cfg.init;
    std::vector<float> seed_xy;
    k.seeded = seed.on;
    if (seed.automatic) {
      k.auto_R = auto_seed_range(seed.max_shift, W, h);
      k.seeded = k.auto_R >= 1;
      if (k.seeded) k.shifts.resize(nb);
    } else if (k.seeded) {
      for (int b = 0; b < nb; ++b) seed_xy.push_back(seed.dx), seed_xy.push_back(seed.dy);
    }
    tvl1_status sc;
    if (!k.seeded)
      sc = tvl1_calc_batch(dc.ctx, nb, dP.u8(), W, px, dQ.u8(), W, px, W, h, dU.f32(), dV.f32(), fp, fs, k.st.data(),
                           dc.stream);
    else if (seed.automatic)
      sc = tvl1_calc_batch_auto_init(dc.ctx, nb, dP.u8(), W, px, dQ.u8(), W, px, W, h, k.auto_R, k.shifts.data(),
                                     dU.f32(), dV.f32(), fp, fs, k.st.data(), dc.stream);
    else
      sc = tvl1_calc_batch_const_init(dc.ctx, nb, dP.u8(), W, px, dQ.u8(), W, px, W, h, seed_xy.data(), dU.f32(),
                                      dV.f32(), fp, fs, k.st.data(), dc.stream);
    FlowSet set;
    set.n = nb, set.W = W, set.H = h;
    set.I0 = dP.u8(), set.pitch0 = W, set.stride0 = px, set.I1 = dQ.u8(), set.pitch1 = W, set.stride1 = px;
    set.u = dU.f32(), set.v = dV.f32(), set.ub = dUb.f32(), set.vb = dVb.f32(), set.score = dS.f32();
    set.fpitch = fp, set.fstride = fs;
    if (sc == TVL1_OK && cfg.check.on) {
      // the same strips solved backward (the frames swapped; a seed negated, an "auto" pair's
      // taken from the record the forward call returned)
      auto backward = [&] {
        const auto tb = Clock::now();
        tvl1_status sb;
        if (!k.seeded) {
          sb = tvl1_calc_batch(dc.ctx, nb, dQ.u8(), W, px, dP.u8(), W, px, W, h, set.ub, set.vb, fp, fs, nullptr,
                               dc.stream);
        } else {
          std::vector<float> back(2 * (size_t)nb);
          for (int b = 0; b < nb; ++b) {
            back[2 * b] = -(seed.automatic ? (float)k.shifts[b].dx : seed.dx);
            back[2 * b + 1] = -(seed.automatic ? (float)k.shifts[b].dy : seed.dy);
          }
          sb = tvl1_calc_batch_const_init(dc.ctx, nb, dQ.u8(), W, px, dP.u8(), W, px, W, h, back.data(), set.ub,
                                          set.vb, fp, fs, nullptr, dc.stream);
        }
        tm["solve_backward"] += secs_since(tb);
        return sb;
      };
      const auto tz = Clock::now();
      sc = score_flows(dc, set, cfg.check, backward);
      if (cfg.check.zncc()) {   // a seed changes nothing here; timed to the score's end on the stream
        if (sc == TVL1_OK && hipStreamSynchronize(dc.stream) != hipSuccess) sc = TVL1_EHIP;
        tm["zncc_score"] += secs_since(tz);
      }
    }
    if (sc == TVL1_OK)
      sc = tvl1_postprocess_batch(dc.ctx, nb, set.u, set.v, fp, fs, dQ.u8(), W, px, W, h, mode, dc.stream);
    if (sc == TVL1_OK && cfg.check.on) sc = reject_flows(dc, set, cfg.check, k.rejected.data());
    return sc;
  }

  // step 3c: the candidates' flow (sampled random_points) or the whole planes onto the host
  bool read_back(KeyBatch &k, Attempt &at) {
    const size_t px = k.px, all = px * k.nb;
    auto ts = Clock::now();
    if (cfg.sampled()) {
      for (auto &f : k.draws) f.wait();
      std::vector<int64_t> off;
      for (int b = 0; b < k.nb; ++b)
        for (auto &pt : k.pts[b]) off.push_back((int64_t)(px * b + (size_t)pt.second * k.W + pt.first));
      tm["sample_points_wait"] += secs_since(ts);
      ts = Clock::now();
      k.fx.resize(off.size());
      k.fy.resize(off.size());
      tvl1_status sc = tvl1_gather_flow(dc.ctx, dU.f32(), dV.f32(), (int64_t)all, off.data(), (int32_t)off.size(),
                                        k.fx.data(), k.fy.data(), dc.stream);
      if (sc == TVL1_OK && cfg.check.on) {   // the score plane as both planes
        k.fs.resize(off.size());
        std::vector<float> fs2(off.size());
        sc = tvl1_gather_flow(dc.ctx, dS.f32(), dS.f32(), (int64_t)all, off.data(), (int32_t)off.size(), k.fs.data(),
                              fs2.data(), dc.stream);
      }
      if (sc != TVL1_OK) {
        fail(at, "flow read-back", sc);
        return false;
      }
    } else {
      k.fx.resize(all);
      k.fy.resize(all);
      if (hipMemcpyAsync(k.fx.data(), dU.p, 4 * all, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
          hipMemcpyAsync(k.fy.data(), dV.p, 4 * all, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
          hipStreamSynchronize(dc.stream) != hipSuccess) {
        fail(at, "flow download failed", TVL1_EHIP);
        return false;
      }
      if (cfg.check.on && (cfg.check.output || cfg.random_points())) {
        k.fs.resize(all);
        if (hipMemcpyAsync(k.fs.data(), dS.p, 4 * all, hipMemcpyDeviceToHost, dc.stream) != hipSuccess ||
            hipStreamSynchronize(dc.stream) != hipSuccess) {
          fail(at, "score download failed", TVL1_EHIP);
          return false;
        }
      }
    }
    k.secs = secs_since(k.t0);
    tm["read_back"] += secs_since(ts);
    return true;
  }

  // step 3d: every pair's stats_json record, sampled points and TIFF outputs of this key
  void write_pairs(std::vector<Item> &items, KeyBatch &k, Attempt &at) {
    const auto ts = Clock::now();
    const std::string suffix = roi_suffix(job.roi_keys[k.kk]);
    const Rect r{0, k.y0, k.W, k.h};
    const size_t px = k.px, fp = 4 * (size_t)k.W;
    const bool sampled = cfg.sampled();
    tvl1_shift none;
    memset(&none, 0, sizeof none);
    size_t o = 0;
    for (int b = 0; b < k.nb && at.ok; ++b) {
      Value &im = items[b].im;
      InitFlow used = cfg.init;   // the seed this strip was solved from
      used.on = k.seeded;
      if (k.seeded && used.automatic) used.dx = (float)k.shifts[b].dx, used.dy = (float)k.shifts[b].dy;
      PointCount count;
      if (sampled) {
        const size_t nc = k.pts[b].size();
        std::vector<float> vx(k.fx.begin() + o, k.fx.begin() + o + nc), vy(k.fy.begin() + o, k.fy.begin() + o + nc), vs;
        if (cfg.check.on) vs.assign(k.fs.begin() + o, k.fs.begin() + o + nc);
        o += nc;
        count = report_points(std::move(k.pts[b]), std::move(vx), std::move(vy), vs, cfg, k.tot[b] > 0, im, r, r,
                              1.f / cfg.scale, false);
      }
      Value sv = solve_record(r, k.secs, k.st[b], cfg.tv.warps, used, k.auto_R, k.shifts.empty() ? none : k.shifts[b],
                              cfg.check, k.rejected[b], sampled ? &count : nullptr);
      sv["batch"] = k.nb;
      sv["read_rows_only"] = items[b].p->partial && items[b].q->partial;
      at.solves[b].push_back(sv);
      if (sampled) continue;
      const std::string base = im["output"].asString() + suffix;
      std::string we;
      if (cfg.check.on && cfg.check.output &&
          !ofio::write_tiff_f32(base + check_suffix(cfg.check), k.fs.data() + px * b, k.W, k.h, fp, we)) {
        at.e = we, at.ok = false;   // an output error, not a device fault
        dc.faulted = false;
      }
      if (cfg.random_points()) continue;   // debug: drawn afterwards, pair by pair
      if (!ofio::write_tiff_f32(base + "_x.tiff", k.fx.data() + px * b, k.W, k.h, fp, we) ||
          !ofio::write_tiff_f32(base + "_y.tiff", k.fy.data() + px * b, k.W, k.h, fp, we)) {
        at.e = we, at.ok = false;
        dc.faulted = false;
      }
    }
    if (cfg.random_points() && !sampled) {
      at.dbg_fx[k.kk].swap(k.fx);
      at.dbg_fy[k.kk].swap(k.fy);
      at.dbg_fs[k.kk].swap(k.fs);
    }
    tm["write_outputs"] += secs_since(ts);
  }

  // step 3: one ROI key's strips of the whole chunk.  false: the attempt ends here (at.ok tells
  // a failure from a chunk handed to the per-pair path, which leaves `items` empty)
  bool solve_key(std::vector<Item> &items, size_t kk, Attempt &at) {
    KeyBatch k;
    k.kk = kk, k.nb = (int)items.size();
    const int nb = k.nb, H0 = items[0].p->H;
    k.W = items[0].p->W, k.h = items[0].p->bands[kk].height;
    k.y0 = job.roi_keys[kk] == "top" ? 0 : H0 - k.h;
    k.px = (size_t)k.W * k.h;
    bool same = true;   // one geometry per launch: every pair's slices of one size
    for (auto &it : items) same = same && it.p->W == k.W && it.p->bands[kk].height == k.h && it.p->H == H0;
    if (!same) {   // mixed slice sizes in one job: the per-pair path takes the chunk
      for (auto &it : items) job.deferred[it.i] = 1;
      items.clear();
      return false;
    }
    if (!grow(k.px * nb)) {
      fail(at, "hipMalloc failed for a strip batch", TVL1_ENOMEM);
      return false;
    }
    if (!pack_and_upload(items, k, at)) return false;
    const size_t nwi = (size_t)TVL1_MAX_LEVELS * std::max(1, cfg.tv.warps);
    k.st.resize(nb);
    k.wi.assign((size_t)nb * nwi, -1);
    for (int b = 0; b < nb; ++b) {
      memset(&k.st[b], 0, sizeof k.st[b]);
      k.st[b].warp_iterations = k.wi.data() + (size_t)b * nwi;
      k.st[b].warp_iterations_capacity = (int32_t)nwi;
    }
    k.pts.resize(nb);
    k.tot.assign(nb, 0);
    k.rejected.assign(nb, 0);
    if (cfg.sampled()) submit_draws(items, k);
    k.t0 = Clock::now();
    if (const tvl1_status sc = solve_scored(k); sc != TVL1_OK) {
      for (auto &f : k.draws) f.wait();   // they read this chunk's bands
      fail(at, "strip batch", sc);
      return false;
    }
    tm["solve"] += secs_since(k.t0);   // the batch's host time (it syncs at every check)
    {
      float up_ms = 0.0f;   // the uploads, on the GPU clock (done before the first check)
      if (hipEventElapsedTime(&up_ms, ev_up0, ev_up1) == hipSuccess) tm["upload_gpu"] += 1e-3 * up_ms;
    }
    if (!read_back(k, at)) return false;
    write_pairs(items, k, at);
    return at.ok;
  }

  // step 4: debug random_points, the exact shuffle, pair by pair and then key by key
  void draw_debug_points(std::vector<Item> &items, Attempt &at) {
    for (size_t b = 0; b < items.size(); ++b)
      for (size_t kk = 0; kk < job.roi_keys.size(); ++kk) {
        const ofio::Image8 &a = items[b].p->bands[kk], &c = items[b].q->bands[kk];
        const int W = a.width, h = a.height;
        const size_t px = (size_t)W * h;
        const Rect r{0, job.roi_keys[kk] == "top" ? 0 : items[b].p->H - h, W, h};
        std::vector<uint8_t> mask(px);
        for (size_t k = 0; k < px; ++k) mask[k] = (a.data[k] > 1) | (c.data[k] > 1);
        const PointCount count =
            random_points(at.dbg_fx[kk].data() + px * b, at.dbg_fy[kk].data() + px * b, at.dbg_fs[kk].data() + px * b,
                          W, h, items[b].im, cfg, r, r, mask, false);
        record_points(at.solves[b][kk], cfg.check, count);   // this key's record
      }
  }

  // step 5: the attempt's results become the pairs' results
  void commit(std::vector<Item> &items, Attempt &at) {
    ++t_chunks;
    t_pairs += items.size();
    for (size_t b = 0; b < items.size(); ++b) {
      PairResult &res = job.results[items[b].i];
      for (auto &sv : at.solves[b]) res.stats["solves"].append(sv);
      if (cfg.random_points()) res.pms.push_back(move_pm(items[b].im));
      res.ok = res.done = true;
    }
  }

  // after a device error: the items as decoded, on a rebuilt context
  bool fresh_context(std::vector<Item> &items, Attempt &at) {
    {
      std::lock_guard<std::mutex> lk(g_io_mutex);
      fprintf(stderr, "Warning: strip batch of %d pairs (%zu..): %s; retrying on a fresh device context\n",
              (int)items.size(), items[0].i, at.e.c_str());
    }
    for (auto &it : items) {   // the retry starts from the decoded bands again
      it.im = job.images[it.i];
      fill_defaults(it.im, job.args, cfg.scale);
    }
    release();
    return rebuild_device(dc, device, at.e);
  }

  // one attempt at the chunk, and after a device error one more on a rebuilt context
  void solve_chunk(std::vector<Item> &items) {
    bool inject = false;
    for (auto &it : items) inject = inject || inject_fault(it.i);
    for (int attempt = 0; attempt < 2; ++attempt) {
      Attempt at(items.size(), job.roi_keys.size());
      if (attempt == 0 && inject) fail(at, "injected device fault", TVL1_EHIP);
      if (at.ok && tvl1_set_params(dc.ctx, &cfg.tv) != TVL1_OK) fail(at, "tvl1_set_params", TVL1_EINVAL);
      for (size_t kk = 0; at.ok && kk < job.roi_keys.size(); ++kk)
        if (!solve_key(items, kk, at)) break;
      // host.a / host.b are reused page-locked buffers: after a failure the chunk's uploads from
      // them may still be queued, so the stream is drained before the retry or the next
      // chunk refills them (PinnedPool's rule, as solve_rois' SyncOnFailure)
      if (!at.ok && dc.stream) (void)hipStreamSynchronize(dc.stream);
      if (items.empty()) return;   // handed to the per-pair path
      if (at.ok && cfg.random_points() && cfg.debug) draw_debug_points(items, at);
      if (at.ok) return commit(items, at);
      if (attempt == 0 && dc.faulted && fresh_context(items, at)) continue;
      std::lock_guard<std::mutex> lk(g_io_mutex);
      for (auto &it : items) {
        job.results[it.i].done = true;
        job.results[it.i].ok = false;
        fprintf(stderr, "Error: pair %zu (%s %s): %s\n", it.i, it.im["p"].asString().c_str(),
                it.im["q"].asString().c_str(), at.e.c_str());
      }
      return;
    }
  }

  void report_timing(Clock::time_point t_worker) {
    Value w;
    w["device"] = device;
    w["chunks"] = (int64_t)t_chunks;
    w["pairs"] = (int64_t)t_pairs;
    w["worker_s"] = secs_since(t_worker);
    for (auto &kv : tm) w["stage_s"][kv.first] = kv.second;
    std::lock_guard<std::mutex> lk(g_stage_mutex);
    g_stage_workers.append(w);
  }

  void run() {
    if (!open_or_hard_error(dc, device, job)) return;
    const auto t_worker = Clock::now();
    (void)hipEventCreate(&ev_up0);
    (void)hipEventCreate(&ev_up1);
    auto queue = [this](size_t start) { queue_chunk(start); };
    ChunkWalk w(job.bnext, job.bchunk, job.batched.size(), queue);
    while (w.advance(queue)) {
      std::vector<Item> items = collect(w.start, w.end());
      retire_decodes(w);
      if (!items.empty()) solve_chunk(items);
    }
    if (dc.stream) (void)hipStreamSynchronize(dc.stream);
    (void)hipEventDestroy(ev_up0);
    (void)hipEventDestroy(ev_up1);
    release();
    dc.close();
    report_timing(t_worker);
  }
};

}  // namespace

void run_strip_worker(JobState &job, int device) { StripWorker(job, device).run(); }

}  // namespace ofcli
