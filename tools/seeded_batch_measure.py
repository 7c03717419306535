#!/usr/bin/env python3
"""Measurements of the seeded strip batch (tvl1_calc_batch_auto_init, "seededStripBatch";
DESIGN 12) on one MI355X.

    python tools/seeded_batch_measure.py chain OUT_DIR   # OUT_DIR/chain.json
    python tools/seeded_batch_measure.py cli OUT_DIR [--slices 129] [--reps 2]   # OUT_DIR/cli.jsonl

chain: 256 strips of 3072x100 (10 scales, 5 warps), cold as tools/shift_measure.py measures:
every call works on another batch after a 1 GiB fill; tvl1_calc_batch_auto_init (max_shift 25)
against tvl1_calc_batch, the host clock around the call and the device's work, and with
tvl1_set_profiling the engine's class 2 of each, which in a batch is the seed chain alone
(kb_flow_down_const and the kb_flow_down steps, one mark; an unseeded batch reports none).
Beside it the bytes a level-0 seed plane per pair and component would have held.

cli: one gen_cross-style strip job (scale 0.5, top / bottom 100-row ROIs of 6144-px slices that
drift, uncompressed TIFF, random_points) with "useInitialFlow" and "initialFlow": "auto",
through the CLI with "seededStripBatch" on and off, alternating, and the same job unseeded
(the batched ceiling).  Rates are pairs per second of the whole process."""
import argparse
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
sys.path.insert(0, str(ROOT / "tools"))
OPTFLOW = ROOT / "fibsem-optflow_amd" / "bin" / "optflow"


def chain(out):
    import torch

    import shift_measure as sm
    from optflow_amd import capi
    sm.torch = torch
    dev = torch.device("cuda", 0)
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    W, H, R, n = 3072, 100, 25, 256
    fr = sm.Frames(W, H, dev, 0xBEEF)
    bshifts = [((7 * b) % 51 - 25, (11 * b) % 51 - 25) for b in range(n)]
    batches = []
    for k in range(3):
        A = torch.stack([fr.window(0, 0) for _ in range(n)])
        B = torch.stack([fr.window(*bshifts[(b + k) % n]) for b in range(n)])
        batches.append((A, B, k))
    eng = capi.Engine(capi.make_params(nscales=10, warps=5))
    u = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    v = torch.empty_like(u)

    def call(t, **kw):
        return eng.calc_batch_device(n, t[0].data_ptr(), W, W * H, t[1].data_ptr(), W, W * H, W, H,
                                     u.data_ptr(), v.data_ptr(), 4 * W, 4 * W * H, stream=eng.stream, **kw)

    res = {"w": W, "h": H, "pairs": n, "max_shift": R, "runs": []}
    call(batches[0])                     # arena, first launches
    call(batches[0], auto_shift=R)
    torch.cuda.synchronize()
    for prof in (False, True):
        eng.set_profiling(prof)
        for rep in range(2):
            for t in batches:
                for arm in ("unseeded", "auto"):
                    got = {}

                    def go():
                        got["r"] = call(t, auto_shift=R) if arm == "auto" else call(t)
                    ms = sm.wall(go, evict, rep)
                    row = {"arm": arm, "profiling": prof, "batch": t[2], "wall_ms": ms}
                    st = got["r"][0] if arm == "auto" else got["r"]
                    if arm == "auto":
                        row["shifts_recovered"] = all(
                            (got["r"][1][b]["dx"], got["r"][1][b]["dy"]) == bshifts[(b + t[2]) % n]
                            for b in range(n))
                    if prof:
                        row["class2_ms"] = st[0]["kernel_ms"][2]
                        row["class2_launches"] = st[0]["kernel_launches"][2]
                    res["runs"].append(row)
    eng.close()

    def med(arm, key, prof):
        x = sorted(r[key] for r in res["runs"] if r["arm"] == arm and r["profiling"] == prof)
        return x[len(x) // 2]
    res["wall_ms_median"] = {a: med(a, "wall_ms", False) for a in ("unseeded", "auto")}
    res["class2_ms_median"] = {a: med(a, "class2_ms", True) for a in ("unseeded", "auto")}
    res["seed_chain_ms"] = res["class2_ms_median"]["auto"] - res["class2_ms_median"]["unseeded"]
    # two f32 planes of the frame per pair, written once and read once by the first step
    res["level0_seed_plane_bytes_not_stored"] = 2 * n * W * H * 4
    (out / "chain.json").write_text(json.dumps(res, indent=1))
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}, indent=1))


def cli(out, Z, reps):
    import numpy as np
    import torch
    from PIL import Image

    from optflow_amd.synth_device import DeviceStack
    W, H, pad = 6144, 512, 64
    work = Path(tempfile.mkdtemp(prefix="seeded_batch_"))   # slices and job outputs: not kept
    d = work / "stack"
    d.mkdir()
    base = DeviceStack(W + 2 * pad, H + 2 * pad, torch.device("cuda", 0), seed=0x5EED).base[0, 0]
    g = torch.Generator(device=base.device)
    g.manual_seed(7)
    paths = []
    for z in range(Z):   # a stage that wanders: up to +-24 px at full size, 12 after pre-scale
        ox, oy = int(round(24 * np.sin(0.37 * z))), int(round(24 * np.cos(0.23 * z)))
        a = base[pad - oy:pad - oy + H, pad - ox:pad - ox + W]
        a = a + 2.0 * torch.randn((H, W), generator=g, device=base.device)
        paths.append(d / f"s{z:04d}.tif")
        Image.fromarray(torch.clamp(torch.round(a), 0, 255).to(torch.uint8).cpu().numpy()).save(paths[-1])
    del base
    torch.cuda.empty_cache()
    pairs = [{"p": str(paths[z]), "q": str(paths[z + 1]), "output_name": f"z{z}", "pId": f"{z}",
              "qId": f"{z + 1}", "pGroupId": f"{z}.0", "qGroupId": f"{z + 1}.0"} for z in range(Z - 1)]
    arms = {"seeded_batch_on": {"useInitialFlow": True, "initialFlow": "auto", "seededStripBatch": True},
            "seeded_batch_off": {"useInitialFlow": True, "initialFlow": "auto"},
            "unseeded_batched": {}}
    rows = []
    with open(out / "cli.jsonl", "w") as log:
        for rep in range(reps):
            for name, extra in arms.items():
                o = work / f"{name}_{rep}"
                o.mkdir(exist_ok=True)
                cfg = {"output_dir": str(o), "output_type": "random_points", "matches_file": str(o / "pm"),
                       "scale": 0.5, "rois": {"top": 100, "bottom": 100}, "stats_json": str(o / "stats.json"),
                       "images": pairs, **extra}
                (o / "cfg.json").write_text(json.dumps(cfg))
                t0 = time.perf_counter()
                r = subprocess.run([str(OPTFLOW), str(o / "cfg.json")], capture_output=True, text=True,
                                   timeout=900)
                dt = time.perf_counter() - t0
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                st = json.loads((o / "stats.json").read_text())
                sol = [s for e in st for s in e["solves"]]
                row = {"arm": name, "rep": rep, "pairs": len(pairs), "wall_s": round(dt, 3),
                       "pairs_per_s": round(len(pairs) / dt, 2), "all_ok": all(e["ok"] for e in st),
                       "batched_solves": sum("batch" in s for s in sol), "solves": len(sol),
                       "seeded_solves": sum("initial_flow" in s for s in sol),
                       "iterations": sum(s["iterations"] for s in sol)}
                rows.append(row)
                log.write(json.dumps(row) + "\n")
                log.flush()
                print(json.dumps(row), flush=True)

    def med(arm):
        x = sorted(r["pairs_per_s"] for r in rows if r["arm"] == arm)
        return x[len(x) // 2]
    s = {a: med(a) for a in arms}
    s["on_over_off"] = round(s["seeded_batch_on"] / s["seeded_batch_off"], 3)
    (out / "cli_summary.json").write_text(json.dumps(s, indent=1))
    print(json.dumps(s))
    shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("chain", "cli"))
    ap.add_argument("out")
    ap.add_argument("--slices", type=int, default=129)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    if a.what == "chain":
        chain(out)
    else:
        cli(out, a.slices, a.reps)


if __name__ == "__main__":
    main()
