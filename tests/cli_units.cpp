// cli_units: known answers of the CLI's HIP-free parts (cli/config.hpp, cli/points.hpp), built
// by tests/test_cli_units_cpu.py with g++ and the host sanitizers and run directly.  Prints one
// "ok <name>" line per check; the first failing check ends the program with status 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "config.hpp"
#include "json.hpp"
#include "points.hpp"

using namespace ofcli;

static void check(bool cond, const char *what) {
  if (!cond) {
    fprintf(stderr, "cli_units: FAILED %s\n", what);
    exit(1);
  }
  printf("ok %s\n", what);
}

// the engine's two default setters, never reached here (config.hpp names them in inline code)
extern "C" void tvl1_params_default(tvl1_params *) { abort(); }
extern "C" void tvl1_align_params_default(tvl1_align_params *) { abort(); }

static void test_rand(const int *first, int n) {
  GlibcRand fresh;
  bool same = true;
  for (int i = 0; i < n; ++i) same = same && fresh.next() == first[i];
  check(same, "GlibcRand: a fresh generator gives the process's own first rand() values");
  for (unsigned s : {1u, 42u, 1729u}) {
    GlibcRand r;
    r.seed(s);
    srand(s);
    same = true;
    for (int i = 0; i < 64; ++i) same = same && r.next() == rand();
    check(same, "GlibcRand: seed(s) gives srand(s); rand()");
  }
}

static void test_sample_points() {
  const int W = 7, H = 5;
  // frame0 masks 5 px, frame1 4 others (values 0 and 1 are not masked): 9 in all
  uint8_t a[H][W] = {}, b[H][W] = {};
  a[0][0] = 2, a[0][6] = 255, a[2][3] = 9, a[4][0] = 2, a[4][6] = 3;
  b[1][1] = 2, b[1][5] = 77, b[3][2] = 2, b[3][4] = 200;
  a[2][2] = 1, b[2][4] = 1, b[0][0] = 1;
  auto r0 = [&](int y) { return (const uint8_t *)a[y]; };
  auto r1 = [&](int y) { return (const uint8_t *)b[y]; };
  auto masked = [&](const std::pair<int, int> &p) { return a[p.second][p.first] > 1 || b[p.second][p.first] > 1; };
  uint64_t total = 0;
  Points p4 = sample_points(r0, r1, W, H, 4, &total);
  std::set<std::pair<int, int>> s4(p4.begin(), p4.end());
  bool in = true;
  for (auto &p : p4) in = in && masked(p);
  check(p4.size() == 4 && s4.size() == 4 && in && total == 9, "sample_points: 4 distinct masked px, total 9");
  for (int np : {9, 10, 1000}) {
    Points all = sample_points(r0, r1, W, H, np, &total);
    std::set<std::pair<int, int>> sa(all.begin(), all.end());
    in = true;
    for (auto &p : all) in = in && masked(p);
    check(all.size() == 9 && sa.size() == 9 && in && total == 9, "sample_points: npoints >= 9 gives every masked px once");
  }
  check(sample_points(r0, r1, W, H, 0, &total).empty() && total == 9, "sample_points: npoints 0 gives none");
  check(sample_points(r0, r1, W, H, -3, &total).empty() && total == 9, "sample_points: npoints < 0 gives none");
  uint8_t z[H][W] = {};
  auto rz = [&](int y) { return (const uint8_t *)z[y]; };
  total = 7;
  check(sample_points(rz, rz, W, H, 4, &total).empty() && total == 0, "sample_points: empty mask, no points, total 0");
}

static void test_keep() {
  const std::vector<float> sc = {0.1f, NAN, INFINITY, 0.5f, 0.6f, 0.2f};
  auto run = [&](int npoints, std::vector<int> want) {
    Points pts;
    std::vector<float> vx, vy;
    for (int i = 0; i < 6; ++i) pts.emplace_back(i, 10 + i), vx.push_back(100.f + i), vy.push_back(200.f + i);
    PairConfig cfg;
    cfg.check.on = true, cfg.check.beta = 0.5f, cfg.npoints = npoints, cfg.scale = 0.5f;
    Value im;
    const Rect r{0, 0, 6, 16};
    const PointCount n = report_points(pts, vx, vy, sc, cfg, true, im, r, r, 2.f, false);
    bool ok = n.candidates == 6 && n.kept == want.size();
    // the kept points, in drawing order: p = (x, y) / scale, q = p + flow / scale; none: the dummy point
    const Value &pm = im["point_matches"];
    if (want.empty()) {
      ok = ok && pm["w"].size() == 1 && pm["w"][0].asInt() == 0 && pm["p"][0][0].asInt() == -1;
    } else {
      ok = ok && pm["w"].size() == want.size();
      for (size_t k = 0; k < want.size() && ok; ++k) {
        const int i = want[k];
        ok = pm["p"][0][k].asDouble() == 2.0 * i && pm["p"][1][k].asDouble() == 2.0 * (10 + i) &&
             pm["q"][0][k].asDouble() == 2.0 * (i + 100.f + i) && pm["q"][1][k].asDouble() == 2.0 * (10 + i + 200.f + i) &&
             pm["w"][k].asInt() == 1;
      }
    }
    // keep_consistent itself, on the same candidates
    const size_t kept = keep_consistent(pts, vx, vy, sc, 0.5f, npoints);
    ok = ok && kept == want.size() && pts.size() == kept;
    for (size_t k = 0; k < want.size() && ok; ++k) ok = pts[k].first == want[k] && vx[k] == 100.f + want[k];
    return ok;
  };
  check(run(2, {0, 3}), "keep: npoints 2 keeps candidates 0 and 3");
  check(run(5, {0, 3, 5}), "keep: npoints 5 keeps candidates 0, 3 and 5");
  check(run(-1, {}), "keep: negative npoints keeps none");
  // unchecked: every candidate is reported, the counters say so
  PairConfig plain;
  Value im;
  const Rect r{0, 0, 2, 2};
  const PointCount n = report_points({{0, 0}, {1, 1}}, {0.f, 0.f}, {0.f, 0.f}, {}, plain, true, im, r, r, 2.f, false);
  check(n.candidates == 2 && n.kept == 2 && im["point_matches"]["w"].size() == 2, "keep: unchecked reports all");
}

static void test_rois() {
  Value a = ofjson::parse("{\"top\": 40, \"bottom\": 30}"), rois;
  get_rois(rois, a, 150, 200);
  auto is = [](const Value &v, int x, int y, int w, int h) {
    return v.size() == 4 && v[0].asInt() == x && v[1].asInt() == y && v[2].asInt() == w && v[3].asInt() == h;
  };
  check(is(rois["top"], 0, 0, 200, 40), "get_rois: top = [0, 0, cols, top]");
  check(is(rois["bottom"], 0, 120, 200, 30), "get_rois: bottom = [0, rows - b, cols, b]");
  const std::vector<std::string> names = rois.memberNames();
  check(names == std::vector<std::string>{"bottom", "top"}, "get_rois: keys in sorted order");
  check(roi_suffix("top") == "_top" && roi_suffix("bottom") == "_bottom" && roi_suffix("custom").empty(),
        "roi_suffix: _top / _bottom only");
  const Rect r = roi_from_array(rois["bottom"]);
  check(r.x == 0 && r.y == 120 && r.width == 200 && r.height == 30, "roi_from_array");
  check(scale_string(0.5f) == "0.50" && scale_string(1.f) == "1.00", "scale_string: %0.2f");
  check(auto_seed_range(32, 400, 40) == 10 && auto_seed_range(500, 4000, 4000) == 128 && auto_seed_range(32, 3, 100) == 0 &&
            auto_seed_range(-5, 100, 100) == 0,
        "auto_seed_range: min(max_shift, 128, min(W, H) / 4), never below 0");
}

static void test_check_parser() {
  const Value none;
  auto of = [&](const char *json, const char **err) { return check_of(none, ofjson::parse(json), err); };
  const char *err = nullptr;
  FlowCheck c = of("{\"consistency\": true}", &err);
  check(c.on && !c.zncc() && c.alpha == 0.01f && c.beta == 0.5f && c.oversample == 4 && !c.output && !err,
        "check: consistency true gives alpha 0.01, beta 0.5, oversample 4");
  check(std::string(check_key(c)) == "consistency" && std::string(check_suffix(c)) == "_fb.tiff" &&
            check_features_error(c) == kConsistencyFeatures,
        "check: consistency's key, suffix and error");
  c = of("{\"zncc\": true}", &err);
  check(c.on && c.zncc() && c.radius == 3 && c.beta == 0.25f && c.oversample == 4 && !c.output && !err,
        "check: zncc true gives radius 3, beta 0.25, oversample 4");
  check(std::string(check_key(c)) == "zncc" && std::string(check_suffix(c)) == "_zncc.tiff" &&
            check_features_error(c) == kZnccFeatures,
        "check: zncc's key, suffix and error");
  of("{\"zncc\": true, \"consistency\": true}", &err);
  check(err && std::string(err) == "zncc cannot be combined with consistency", "check: both keys on");
  for (const char *j : {"{\"zncc\": {\"radius\": 0}}", "{\"zncc\": {\"radius\": 5}}"}) {
    of(j, &err);
    check(err && std::string(err) == "zncc: radius must be 1..4", "check: radius 0 or 5");
  }
  c = of("{\"zncc\": {\"radius\": 4, \"beta\": 0.125}, \"znccOversample\": 0, \"znccOutput\": true}", &err);
  check(c.on && c.radius == 4 && c.beta == 0.125f && c.oversample == 1 && c.output && !err, "check: zncc object");
  for (const char *j : {"{\"zncc\": \"yes\"}", "{\"consistency\": \"yes\"}", "{\"zncc\": [1]}", "{}"}) {
    c = of(j, &err);
    check(!c.on && !err, "check: a non-numeric, non-object value stays inert");
  }
  // the image's key goes before the job's
  c = check_of(ofjson::parse("{\"consistency\": false}"), ofjson::parse("{\"consistency\": {\"alpha\": 0.5}}"), &err);
  check(!c.on && !err, "check: per-image value first");
}

static void test_solve_record() {
  tvl1_stats st;
  memset(&st, 0, sizeof st);
  int32_t wi[TVL1_MAX_LEVELS * 3];
  for (int i = 0; i < TVL1_MAX_LEVELS * 3; ++i) wi[i] = 10 + i;
  st.levels = 2, st.iterations_total = 77, st.checks_total = 9;
  st.warp_iterations = wi, st.warp_iterations_capacity = TVL1_MAX_LEVELS * 3;
  tvl1_shift sh;
  memset(&sh, 0, sizeof sh);
  sh.dx = 3, sh.dy = -2, sh.sad = 1000, sh.count = 50, sh.sad_zero = 2000, sh.count_zero = 60;
  InitFlow seed;
  seed.on = seed.automatic = true, seed.dx = 3.f, seed.dy = -2.f, seed.max_shift = 32;
  FlowCheck zn;
  zn.kind = FlowCheck::kZncc, zn.on = true, zn.radius = 3, zn.beta = 0.25f;
  const PointCount pc{100, 25};
  const Rect roi{0, 120, 200, 30};
  // the per-pair call site's record, and the batch call site's with its two keys of its own
  const Value pair = solve_record(roi, 1.5, st, 3, seed, 7, sh, zn, 12, &pc);
  Value batch = solve_record(roi, 1.5, st, 3, seed, 7, sh, zn, 12, &pc);
  batch["batch"] = 4;
  batch["read_rows_only"] = true;
  check(pair.dump(1) == "{\n \"checks\": 9,\n \"initial_flow\": [\n  3.0,\n  -2.0\n ],\n \"initial_flow_auto\": {\n  "
                        "\"count\": 50,\n  \"count_zero\": 60,\n  \"max_shift\": 7,\n  \"sad\": 1000,\n  \"sad_zero\": 2000\n },\n"
                        " \"iterations\": 77,\n \"levels\": 2,\n \"roi\": [\n  0,\n  120,\n  200,\n  30\n ],\n \"seconds\": 1.5,\n"
                        " \"warp_iterations\": [\n  10,\n  11,\n  12,\n  13,\n  14,\n  15\n ],\n \"zncc\": {\n  \"beta\": 0.25,\n  "
                        "\"candidates\": 100,\n  \"kept\": 25,\n  \"px\": 6000,\n  \"radius\": 3,\n  \"rejected_px\": 12\n }\n}" ||
            (fprintf(stderr, "%s\n", pair.dump(1).c_str()), false),
        "solve_record: the known record");
  Value stripped = batch;
  bool same = stripped.isMember("batch") && stripped.isMember("read_rows_only");
  Value rebuilt;
  for (auto &k : stripped.memberNames())
    if (k != "batch" && k != "read_rows_only") rebuilt[k] = stripped[k];
  check(same && rebuilt.dump(1) == pair.dump(1), "solve_record: batch = per-pair + batch, read_rows_only");
  // unseeded, unchecked: none of the optional blocks; an auto seed too small to search says so
  const Value plain = solve_record(roi, 0.0, st, 3, InitFlow(), 0, sh, FlowCheck(), 0, nullptr);
  check(!plain.isMember("initial_flow") && !plain.isMember("initial_flow_auto") && !plain.isMember("zncc") &&
            !plain.isMember("consistency"),
        "solve_record: no seed, no check");
  InitFlow tiny;
  tiny.automatic = true;
  const Value small = solve_record(roi, 0.0, st, 3, tiny, 0, sh, FlowCheck(), 0, nullptr);
  check(!small.isMember("initial_flow") && small["initial_flow_auto"]["max_shift"].asInt() == 0 &&
            !small["initial_flow_auto"].isMember("sad"),
        "solve_record: auto seed too small to search");
}

int main() {
  int first[8];
  for (int &v : first) v = rand();   // before anything else: the process's own first values
  test_rand(first, 8);
  test_sample_points();
  test_keep();
  test_rois();
  test_check_parser();
  test_solve_record();
  return 0;
}
