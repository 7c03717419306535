#!/usr/bin/env python3
"""Measurement of the photometric (ZNCC) score of a flow (tvl1_zncc_score, tvl1_warp_by_flow_u8;
DESIGN 14) on one MI355X.

    python tools/zncc_measure.py OUT_DIR             # OUT_DIR/measure.json
    python tools/zncc_measure.py OUT_DIR --no-cli    # the kernels only

Kernels, cold, as DESIGN 11 measured the slice-list kernels: two shapes, one 6144x4096 plane set
and 256 strips of 3072x100; every call works on another set of buffers after a 1 GiB fill has
pushed the planes out of the 256 MB last-level cache; the time is between two events on the
call's stream, the median of 9 calls per radius.  The flow is the engine's own forward flow of
a synthetic pair (C2's parameters: 5 scales, 30 warps; the strips': 10 scales, 5 warps), so the
gather sees what a job gives it, and the forward solve is timed in the same call.  Compulsory
bytes: 14 B/px (I0 1, I1 1, u and v 8, score 4); halo columns and run-in rows are re-read from
cache.

Strip job: the CLI on a small stack of 3072-px-wide slices with top / bottom 100-row strips,
"zncc" on, both keys off, and "consistency" on, three alternations: the batch workers' stage
times and the wall time around the process."""
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

BETA = 0.25


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
    """I0, I1: (n, H, W) u8 on the device.  Solves forward, then times the score cold."""
    fl = torch.empty((2, n, H, W), dtype=torch.float32, device=I0.device)
    P, S = 4 * W, 4 * W * H

    def solve():
        if n == 1:
            eng.calc_device(I0.data_ptr(), W, I1.data_ptr(), W, W, H, fl[0].data_ptr(), fl[1].data_ptr(), P,
                            stream=eng.stream, stats=False)
        else:
            eng.calc_batch_device(n, I0.data_ptr(), W, W * H, I1.data_ptr(), W, W * H, W, H, fl[0].data_ptr(),
                                  fl[1].data_ptr(), P, S, stream=eng.stream)

    sol = [wall(solve, evict, k) for k in range(3)]   # the first allocates
    sets = [(I0.clone(), I1.clone(), fl.clone(), torch.empty((n, H, W), dtype=torch.float32, device=I0.device))
            for _ in range(3)]
    torch.cuda.synchronize()
    px = n * W * H
    out = {"w": W, "h": H, "pairs": n, "px": px, "solve_forward_wall_ms": sol}
    for r in (3, 1, 2, 4):
        score = lambda t: eng.zncc_score_batch(n, t[0].data_ptr(), W, W * H, t[1].data_ptr(), W, W * H,
                                               t[2][0].data_ptr(), t[2][1].data_ptr(), P, S, W, H, r,
                                               t[3].data_ptr(), P, S, stream=s)
        score(sets[0])
        torch.cuda.synchronize()
        ms = [timed(lambda: score(t), evict, i + k)[0] for k in range(3) for i, t in enumerate(sets)]
        st = stats(ms)
        st["compulsory_bytes"] = 14 * px
        st["TB_per_s"] = 14 * px / st["ms_median"] / 1e9
        st["fraction_of_8TBps"] = st["TB_per_s"] / 8.0
        st["share_of_forward_solve"] = st["ms_median"] / min(sol[1:])
        if r == 3:
            sc = sets[0][3]
            st["rejected_share_at_beta_0.25"] = float((~(sc <= BETA)).float().mean().item())
            st["inf_share"] = float(torch.isinf(sc).float().mean().item())
        out[f"zncc_score_r{r}"] = st
    if n == 1:
        J = [torch.empty((H, W), dtype=torch.uint8, device=I0.device) for _ in range(3)]
        warp = lambda i, t: eng.warp_by_flow_u8(t[1].data_ptr(), W, t[2][0].data_ptr(), t[2][1].data_ptr(), P,
                                                W, H, J[i].data_ptr(), W, stream=s)
        warp(0, sets[0])
        torch.cuda.synchronize()
        ms = [timed(lambda: warp(i, t), evict, i + k)[0] for k in range(3) for i, t in enumerate(sets)]
        st = stats(ms)
        st["compulsory_bytes"] = 10 * px
        st["TB_per_s"] = 10 * px / st["ms_median"] / 1e9
        out["warp_by_flow_u8"] = st
    return out


def cli_job(out):
    """The strip job with "zncc" on, both keys off and "consistency" on, alternating."""
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
            for mode in ("off", "zncc", "consistency"):
                o = d / f"out_{rep}_{mode}"
                o.mkdir()
                cfg = {"output_dir": str(o), "scale": 1, "output_type": "random_points", "npoints": 25,
                       "rois": {"top": 100, "bottom": 100}, "timing_json": str(o / "timing.json"),
                       "images": [{"p": str(d / f"s{z}.tif"), "q": str(d / f"s{z + 1}.tif"), "pId": f"t{z}",
                                   "qId": f"t{z + 1}", "output_name": f"z{z}"} for z in range(Z - 1)]}
                if mode != "off":
                    cfg[mode] = True
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
                runs.append({"mode": mode, "wall_s": secs, "stage_s": stage})
    med = lambda mode, f: sorted(f(r) for r in runs if r["mode"] == mode)[1]
    res = {"slices": Z, "w": W, "h": H, "strips": [100, 100], "runs": runs}
    for mode in ("off", "zncc", "consistency"):
        res[f"solve_stage_s_{mode}"] = med(mode, lambda r: r["stage_s"].get("solve", 0.0))
        res[f"wall_s_{mode}"] = med(mode, lambda r: r["wall_s"])
    res["zncc_score_stage_s"] = med("zncc", lambda r: r["stage_s"].get("zncc_score", 0.0))
    res["solve_stage_ratio_zncc_off"] = res["solve_stage_s_zncc"] / res["solve_stage_s_off"]
    res["solve_stage_ratio_consistency_off"] = res["solve_stage_s_consistency"] / res["solve_stage_s_off"]
    return res


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
    res["planes_6144x4096"] = shape(eng, fr.window(0, 0)[None].contiguous(), fr.window(2, -1)[None].contiguous(),
                                    1, W, H, evict, s)
    eng.close()
    del fr
    torch.cuda.empty_cache()
    (out / "measure.json").write_text(json.dumps(res, indent=1))

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
