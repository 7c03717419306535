#!/usr/bin/env python3
"""Measurement of the forward-backward consistency score (tvl1_fb_score, tvl1_zero_above;
DESIGN 13) on one MI355X.

    python tools/fbcheck_measure.py OUT_DIR             # OUT_DIR/measure.json
    python tools/fbcheck_measure.py OUT_DIR --no-cli    # the kernels only

Kernels, cold, as DESIGN 11 measured the slice-list kernels: two shapes, one 6144x4096 plane set
and 256 strips of 3072x100; every call works on another set of buffers after a 1 GiB fill has
pushed the planes out of the 256 MB last-level cache; the time is between two events on the
call's stream.  The flows are the engine's own, forward and backward, of a synthetic pair (C2's
parameters: 5 scales, 30 warps; the strips': 10 scales, 5 warps), so the gather sees what a job
gives it.  Compulsory bytes: 16 B/px read and 4 written for the score; 4 read for the zeroing
plus 8 read and 8 written per 4-px word that holds a rejected px (at most 12 and 8 per px).
Beside them the forward solve of the same shape alone.

Strip job: the CLI on a small stack of 3072-px-wide slices with top / bottom 100-row strips,
"consistency" on and off, three alternations, wall time around the process."""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
sys.path.insert(0, str(ROOT / "tools"))

ALPHA, BETA = 0.01, 0.5


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "calls": len(ms)}


def timed(fn, evict, tag):
    evict.fill_(tag)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn, evict, tag):
    evict.fill_(tag)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def shape(eng, I0, I1, n, W, H, evict, s):
    """I0, I1: (n, H, W) u8 on the device.  Solves both ways, then times the two kernels cold."""
    fl = torch.empty((4, n, H, W), dtype=torch.float32, device=I0.device)
    P, S = 4 * W, 4 * W * H

    def solve(a, b, u, v):
        if n == 1:
            eng.calc_device(a.data_ptr(), W, b.data_ptr(), W, W, H, u.data_ptr(), v.data_ptr(), P,
                            stream=eng.stream, stats=False)
        else:
            eng.calc_batch_device(n, a.data_ptr(), W, W * H, b.data_ptr(), W, W * H, W, H, u.data_ptr(),
                                  v.data_ptr(), P, S, stream=eng.stream)

    sol = [wall(lambda: solve(I0, I1, fl[0], fl[1]), evict, k) for k in range(3)]   # the first allocates
    back = wall(lambda: solve(I1, I0, fl[2], fl[3]), evict, 3)
    sets = [(fl.clone(), torch.empty((n, H, W), dtype=torch.float32, device=I0.device)) for _ in range(3)]
    torch.cuda.synchronize()
    score = lambda t: eng.fb_score_batch(n, t[0][0].data_ptr(), t[0][1].data_ptr(), P, S, t[0][2].data_ptr(),
                                         t[0][3].data_ptr(), P, S, W, H, ALPHA, t[1].data_ptr(), P, S, stream=s)
    zero = lambda t: eng.zero_above_batch(n, t[0][0].data_ptr(), t[0][1].data_ptr(), P, S, t[1].data_ptr(), P, S,
                                          W, H, BETA, stream=s, count=False)
    score(sets[0])
    torch.cuda.synchronize()
    ms_s = [timed(lambda: score(t), evict, i + r)[0] for r in range(3) for i, t in enumerate(sets)]
    sc = sets[0][1]
    rej = int((~(sc <= BETA)).sum().item())
    words = int((~(sc <= BETA)).reshape(n, H, W // 4, 4).any(-1).sum().item()) if W % 4 == 0 else None
    ms_z = []
    for r in range(3):
        for i, t in enumerate(sets):
            t[0][:2].copy_(fl[:2])   # zeroing again what is zero would write the same words, but keep it honest
            ms_z.append(timed(lambda: zero(t), evict, i + r)[0])
    counted = eng.zero_above_batch(n, sets[0][0][0].data_ptr(), sets[0][0][1].data_ptr(), P, S,
                                   sets[0][1].data_ptr(), P, S, W, H, BETA, stream=s)
    px = n * W * H
    out = {"w": W, "h": H, "pairs": n, "px": px, "rejected_px": rej, "rejected_counted": int(counted.sum()),
           "solve_forward_wall_ms": sol, "solve_backward_wall_ms": back}
    for name, ms, nbytes in (("fb_score", ms_s, 20 * px),
                             ("zero_above", ms_z, 4 * px + (64 * words if words is not None else 16 * rej))):
        st = stats(ms)
        st["compulsory_bytes"] = nbytes
        st["TB_per_s"] = nbytes / st["ms_median"] / 1e9
        st["fraction_of_8TBps"] = st["TB_per_s"] / 8.0
        st["share_of_forward_solve"] = st["ms_median"] / min(sol[1:])
        out[name] = st
    return out


def cli_job(out):
    """The strip job with the key on and off, alternating."""
    import numpy as np
    from PIL import Image
    from optflow_amd import capi, synth
    W, H, Z = 3072, 400, 17
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        pad = Z
        base = synth.base_texture(W + 2 * pad, H + 2 * pad, seed=0xFBC)
        g = np.random.default_rng(5)
        for z in range(Z):
            a = base[pad - z // 2:pad - z // 2 + H, pad + z // 3:pad + z // 3 + W]
            a = a + g.normal(0.0, 2.0, size=(H, W)).astype(np.float32)
            Image.fromarray(np.clip(np.rint(a), 2, 255).astype(np.uint8)).save(d / f"s{z}.tif")
        runs = []
        for rep in range(3):
            for on in (False, True):
                o = d / f"out_{rep}_{int(on)}"
                o.mkdir()
                cfg = {"output_dir": str(o), "scale": 1, "output_type": "random_points", "npoints": 25,
                       "rois": {"top": 100, "bottom": 100}, "timing_json": str(o / "timing.json"),
                       "consistency": on,
                       "images": [{"p": str(d / f"s{z}.tif"), "q": str(d / f"s{z + 1}.tif"), "pId": f"t{z}",
                                   "qId": f"t{z + 1}", "output_name": f"z{z}"} for z in range(Z - 1)]}
                (o / "cfg.json").write_text(json.dumps(cfg))
                t = time.perf_counter()
                r = subprocess.run([str(capi.PKG_ROOT / "bin" / "optflow"), str(o / "cfg.json")],
                                   capture_output=True, text=True, timeout=300)
                secs = time.perf_counter() - t
                assert r.returncode == 0, r.stderr
                tj = json.loads((o / "timing.json").read_text())
                stage = {}
                for w in tj.get("batch_workers") or []:
                    for k, v in (w.get("stage_s") or {}).items():   # a worker that got no chunk has none
                        stage[k] = stage.get(k, 0.0) + v
                runs.append({"consistency": on, "wall_s": secs, "stage_s": stage})
    off = sorted(r["wall_s"] for r in runs if not r["consistency"])
    on = sorted(r["wall_s"] for r in runs if r["consistency"])
    sol = lambda c: sorted(r["stage_s"].get("solve", 0.0) for r in runs if r["consistency"] == c)[1]
    return {"slices": Z, "w": W, "h": H, "strips": [100, 100], "runs": runs,
            "wall_ratio_on_off": on[1] / off[1], "solve_stage_ratio_on_off": sol(True) / sol(False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    global torch
    import torch
    from optflow_amd import capi
    import shift_measure
    shift_measure.torch = torch   # its Frames (windows of one device-made texture) use the module's
    Frames = shift_measure.Frames
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    res = {}

    W, H = 6144, 4096
    fr = Frames(W, H, dev, 0x5EED)
    eng = capi.Engine(capi.make_params(nscales=5, warps=30))
    res["planes_6144x4096"] = shape(eng, fr.window(0, 0)[None], fr.window(2, -1)[None], 1, W, H, evict, s)
    eng.close()
    del fr
    torch.cuda.empty_cache()

    W, H, n = 3072, 100, 256
    fr = Frames(W, H, dev, 0xBEEF)
    A = torch.stack([fr.window(0, 0) for _ in range(n)])
    B = torch.stack([fr.window(b % 5 - 2, b % 3 - 1) for b in range(n)])
    eng = capi.Engine(capi.make_params(nscales=10, warps=5))
    res["strips_256x3072x100"] = shape(eng, A, B, n, W, H, evict, s)
    eng.close()
    del evict, A, B, fr
    torch.cuda.empty_cache()

    (out / "measure.json").write_text(json.dumps(res, indent=1))
    if not a.no_cli:
        res["strip_job"] = cli_job(out)
    (out / "measure.json").write_text(json.dumps(res, indent=1))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
