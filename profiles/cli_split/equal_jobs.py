"""The parent commit's optflow binary against this tree's on the same inputs.
usage: OPTFLOW_PARENT=/path/to/parent/bin/optflow python profiles/cli_split/equal_jobs.py OUTDIR [--plan]
Both binaries run every job from a directory of their own with relative paths, so stdout,
stderr and every file can be compared byte for byte."""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
from optflow_amd import synth  # noqa: E402

NEW = ROOT / "fibsem-optflow_amd" / "bin" / "optflow"
OLD = Path(os.environ["OPTFLOW_PARENT"]).resolve()
W, H, Z = 400, 300, 9
out = Path(sys.argv[1]).resolve()
plan = "--plan" in sys.argv
out.mkdir(parents=True, exist_ok=True)
stk = out / "stk"
stk.mkdir(exist_ok=True)
sl = synth.gen_stack(W, H, Z, seed=77)
sl[3][:, :9] = 0
for z in range(Z):
    Image.fromarray(sl[z]).save(stk / f"s{z}.tif")
    Image.fromarray(sl[z]).save(stk / f"s{z}.png")
Image.fromarray(sl[1][:, :380].copy()).save(stk / "narrow.tif")
(stk / "broken.tif").write_bytes(b"II*\x00garbage")


def base(otype, ext="tif", **kw):
    pairs = [(z, z + 1) for z in range(6)] + [(0, 4), (2, 6)]
    cfg = {"output_dir": "out", "scale": 0.5, "output_type": otype, "nscales": 5, "warps": 3,
           "rois": {"top": 40, "bottom": 30}, "stats_json": "out/stats.json", "inflight": 1,
           "images": [{"p": f"../../stk/s{a}.{ext}", "q": f"../../stk/s{b}.{ext}", "pId": f"t{a}", "qId": f"t{b}",
                       "pGroupId": f"{a}.0", "qGroupId": f"{b}.0", "output_name": f"z{a}_{b}"} for a, b in pairs]}
    cfg.update(kw)
    return cfg


jobs = {}   # name -> (cfg, env, exact)
CHECKS = {"none": {}, "fb": {"consistency": True, "consistencyOutput": True},
          "zncc": {"zncc": True, "znccOutput": True}}
for otype in ("flow", "map", "random_points"):
    for sb in (256, 0):
        for cn, ck in CHECKS.items():
            jobs[f"{otype}_sb{sb}_{cn}"] = (base(otype, debug=True, strip_batch=sb, **ck), {}, True)
for sn, seed in (("const", [3, -2]), ("auto", "auto")):
    for ssb in (True, False):
        jobs[f"seed_{sn}_ssb{int(ssb)}"] = (base("map", useInitialFlow=True, initialFlow=seed, seededStripBatch=ssb), {}, True)
    jobs[f"seed_{sn}_fb_points"] = (base("random_points", debug=True, useInitialFlow=True, initialFlow=seed,
                                         seededStripBatch=True, **CHECKS["fb"]), {}, True)
    jobs[f"seed_{sn}_zncc_sb0"] = (base("flow", useInitialFlow=True, initialFlow=seed, strip_batch=0, **CHECKS["zncc"]), {}, True)
jobs["auto_tiny"] = (base("map", useInitialFlow=True, initialFlow="auto", seededStripBatch=True, rois={"top": 3, "bottom": 30}), {}, True)
jobs["fault_sb256"] = (base("map"), {"OPTFLOW_INJECT_FAULT": "1,4"}, True)
jobs["fault_sb0"] = (base("map", strip_batch=0), {"OPTFLOW_INJECT_FAULT": "1,4"}, True)
jobs["fault_points"] = (base("random_points", debug=True, **CHECKS["zncc"]), {"OPTFLOW_INJECT_FAULT": "1,4"}, True)
mixed = base("map")
mixed["images"][2]["nscales"] = 4
mixed["images"][5]["rois"] = {"custom": [10, 20, 120, 60]}
mixed["images"][6]["output_type"] = "flow"
mixed["images"][7]["rois"] = {"custom": {"0": [0, 0, 100, 50], "1": [5, 5, 100, 50]}}
jobs["mixed"] = (mixed, {}, True)
mixedp = base("random_points", debug=True, **CHECKS["fb"])
mixedp["images"][3]["npoints"] = 7
mixedp["images"][4]["consistency"] = False
jobs["mixed_points"] = (mixedp, {}, True)
full = base("map", ext="png", debug=True)
del full["rois"]
full["images"] = full["images"][:2]
jobs["full_frame_align"] = (full, {}, True)
fullp = copy.deepcopy(full)
fullp["output_type"] = "random_points"
fullp["features"] = 1
jobs["full_frame_points"] = (fullp, {}, True)
sizes = base("map")
sizes["images"][1]["q"] = "../../stk/narrow.tif"
sizes["images"][4]["p"] = "../../stk/broken.tif"
sizes["images"][5]["q"] = "../../stk/missing.tif"
jobs["sizes_unreadable"] = (sizes, {}, True)
sizes0 = copy.deepcopy(sizes)
sizes0["strip_batch"] = 0
jobs["sizes_unreadable_sb0"] = (sizes0, {}, True)
outside = base("map")
outside["images"][2]["rois"] = {"custom": [0, 0, 500, 100]}
outside["rois"] = {"top": 40, "bottom": 30}
jobs["roi_outside"] = (outside, {}, True)
jobs["roi_outside_global"] = (base("map", rois={"top": 40, "bottom": 400}), {}, True)
jobs["skip_existing"] = (base("map", skip_existing=True), {}, True)
jobs["err_both_checks"] = (base("map", zncc=True, consistency=True), {}, True)
jobs["err_seed_features"] = (base("map", useInitialFlow=True, initialFlow=[1, 1], features=1), {}, True)
jobs["err_check_align"] = (dict(full, zncc=True), {}, True)
jobs["seed_align"] = (dict(full, useInitialFlow=True, initialFlow="auto"), {}, True)
jobs["style2"] = ({"style": 2, "slices": [f"../../stk/s{z}.png" for z in range(9)], "output_dir": "out", "scale": 0.5,
                   "nscales": 5, "warps": 3, "inflight": 1, "border": 4, "save_flow": True, "stats_json": "out/stats.json"}, {}, True)
# time-seeded points: stats without seconds and the records' shapes only
for sb in (256, 0):
    for cn, ck in CHECKS.items():
        jobs[f"sampled_sb{sb}_{cn}"] = (base("random_points", strip_batch=sb, **ck), {}, False)


def strip_seconds(v):
    if isinstance(v, dict):
        return {k: strip_seconds(x) for k, x in v.items() if k != "seconds"}
    if isinstance(v, list):
        return [strip_seconds(x) for x in v]
    return v


def shape(v):
    if isinstance(v, dict):
        return {k: shape(x) for k, x in v.items()}
    if isinstance(v, list):
        return [len(v)] + ([shape(v[0])] if v and isinstance(v[0], (dict, list)) else [])
    return type(v).__name__


def arm(name, binary, which, cfg, env):
    d = out / name / which
    (d / "out").mkdir(parents=True, exist_ok=True)
    (d / "cfg.json").write_text(json.dumps(cfg))
    cmd = [str(binary)] + (["--plan"] if plan else []) + ["cfg.json"]
    try:
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        print(f"HUNG {name} {which}: stopping", flush=True)
        sys.exit(3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        print(f"CRASHED {name} {which} rc {r.returncode}: stopping\n{r.stderr[-2000:]}", flush=True)
        sys.exit(3)
    files = {}
    for f in sorted((d / "out").rglob("*")):
        if f.is_file():
            files[str(f.relative_to(d))] = f.read_bytes()
    return r, files


bad = 0
for name, (cfg, env, exact) in jobs.items():
    ro, fo = arm(name, OLD, "old", cfg, env)
    rn, fn = arm(name, NEW, "new", cfg, env)
    diffs = []
    if ro.returncode != rn.returncode:
        diffs.append(f"rc {ro.returncode} != {rn.returncode}")
    if ro.stderr != rn.stderr:
        diffs.append("stderr")
    if exact and ro.stdout != rn.stdout:
        diffs.append("stdout")
    if not exact and sorted(ro.stdout.splitlines()) != sorted(rn.stdout.splitlines()):
        diffs.append("stdout lines")
    if sorted(fo) != sorted(fn):
        diffs.append(f"file lists {sorted(set(fo) ^ set(fn))}")
    for k in sorted(set(fo) & set(fn)):
        if k.endswith("stats.json"):
            if strip_seconds(json.loads(fo[k])) != strip_seconds(json.loads(fn[k])):
                diffs.append(k)
        elif not exact and k.endswith(".json"):
            if shape(json.loads(fo[k])) != shape(json.loads(fn[k])):
                diffs.append(k + " shape")
        elif fo[k] != fn[k]:
            diffs.append(k)
    nsolves = ""
    if "out/stats.json" in fn:
        st = json.loads(fn["out/stats.json"])
        if st and isinstance(st[0], dict) and "ok" in st[0]:
            nsolves = f" ok {sum(1 for e in st if e.get('ok'))}/{len(st)} solves {sum(len(e.get('solves', [])) for e in st)}"
    print(f"{'EQUAL' if not diffs else 'DIFFER'} {name}: rc {rn.returncode}, {len(fn)} files, "
          f"stdout {len(rn.stdout)} B, stderr {len(rn.stderr)} B{nsolves}" + (f" -- {diffs}" if diffs else ""), flush=True)
    bad += bool(diffs)
print(f"{len(jobs)} jobs, {bad} differ", flush=True)
sys.exit(1 if bad else 0)
