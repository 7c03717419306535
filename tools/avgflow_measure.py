#!/usr/bin/env python3
"""Measurement of the average-flow alignment ("style": 2) on one MI355X.

    python tools/avgflow_measure.py gen STACK_DIR                 # no GPU: 16 slices 6144x4096, TIFF
    python tools/avgflow_measure.py cli STACK_DIR OUT_DIR         # the CLI job, timing_json + stats_json
    python tools/avgflow_measure.py kernels STACK_DIR OUT_DIR     # solve-only rate + kernel times

gen      synth.gen_stack's recipe (the slices made by a pool of processes) as uncompressed TIFF.
cli      optflow with style 2, scale 0.5, border 32, the reference's default TV-L1 keys; writes
         OUT_DIR/timing.json, stats.json and cli_stdout.txt (aligned slices go to STACK_DIR/out).
kernels  OUT_DIR/measure.json: the solve-only rate of the same 3072x2048 (slice, blend) pairs
         through capi.Engine with `--inflight` engines in flight; times of k_blend6_u8,
         k_half_u8 and k_remap_flow_u8 on full-size planes, cold (another slice per call after a
         cache-evicting fill, by the engine's profiling) and warm (20 calls on the same buffers),
         their compulsory bytes and the fraction of 8 TB/s; and their share of a slice's GPU
         time (cold) against one profiled solve alone.
Run the three steps as separate processes (gen forks workers and must not hold the GPU)."""
import argparse
import json
import subprocess
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

W, H, Z, SEED, BORDER = 6144, 4096, 16, 0x5EED, 32
_base = None


def _one(args):
    z, out = args
    from optflow_amd import synth
    Image.fromarray(synth.make_slice(_base, z, SEED)).save(Path(out) / f"z{z:02d}.tiff")
    return z


def gen(stack: Path):
    global _base
    from multiprocessing import Pool
    from optflow_amd import synth
    stack.mkdir(parents=True, exist_ok=True)
    t = time.time()
    _base = synth.base_texture(W, H, SEED)      # inherited by the forked workers
    with Pool(8) as p:
        p.map(_one, [(z, str(stack)) for z in range(Z)])
    print(f"generated {Z} slices {W}x{H} in {time.time() - t:.1f} s", flush=True)


def cli(stack: Path, out: Path, inflight: int):
    out.mkdir(parents=True, exist_ok=True)
    (stack / "out").mkdir(exist_ok=True)
    cfg = {"style": 2, "slices": [str(p) for p in sorted(stack.glob("z*.tiff"))],
           "output_dir": str(stack / "out"), "scale": 0.5, "border": BORDER, "inflight": inflight,
           "timing_json": str(out / "timing.json"), "stats_json": str(out / "stats.json")}
    (stack / "cfg.json").write_text(json.dumps(cfg))
    t = time.time()
    r = subprocess.run([str(ROOT / "fibsem-optflow_amd" / "bin" / "optflow"), str(stack / "cfg.json")],
                       capture_output=True, text=True, timeout=600)
    wall = time.time() - t
    (out / "cli_stdout.txt").write_text(r.stdout + r.stderr + f"\nrc {r.returncode}, {wall:.3f} s\n")
    print((out / "timing.json").read_text())
    return r.returncode


def kernels(stack: Path, out: Path, inflight: int):
    import torch
    from optflow_amd import capi
    out.mkdir(parents=True, exist_ok=True)
    fw, fh = W // 2, H // 2
    dev = torch.device("cuda", 0)
    sl = [torch.from_numpy(np.array(Image.open(p))).to(dev) for p in sorted(stack.glob("z*.tiff"))]
    n = len(sl)
    eng = capi.Engine(capi.make_params())
    res = {"W": W, "H": H, "border": BORDER, "slices": n, "inflight": inflight}

    def neighbours(i):
        return [sl[i + d].data_ptr() for d in (-3, -2, -1, 1, 2, 3)]

    pairs = []
    for i in range(3, n - 3):
        bl = torch.empty((H, W), dtype=torch.uint8, device=dev)
        eng.blend6_u8(neighbours(i), [W] * 6, W, H, bl.data_ptr(), W)
        i0 = torch.empty((fh, fw), dtype=torch.uint8, device=dev)
        i1 = torch.empty_like(i0)
        eng.half_u8(sl[i].data_ptr(), W, W, H, i0.data_ptr(), fw)
        eng.half_u8(bl.data_ptr(), W, W, H, i1.data_ptr(), fw)
        pairs.append((i0, i1))
    torch.cuda.synchronize()

    # ---- solve-only rate, `inflight` engines in flight, each on its own stream
    engs = [capi.Engine(capi.make_params()) for _ in range(inflight)]
    bufs = [(torch.empty((fh, fw), dtype=torch.float32, device=dev),
             torch.empty((fh, fw), dtype=torch.float32, device=dev)) for _ in engs]

    def solve(k, p):
        e, (u, v) = engs[k], bufs[k]
        st = e.calc_device(p[0].data_ptr(), fw, p[1].data_ptr(), fw, fw, fh, u.data_ptr(),
                           v.data_ptr(), 4 * fw, stream=e.stream)
        torch.cuda.ExternalStream(e.stream, device=dev).synchronize()   # this solve's stream only
        return st

    for k in range(inflight):
        solve(k, pairs[0])          # warm-up: the solver's scratch is allocated here
    for rep in range(2):
        nxt, lock, its = [0], threading.Lock(), []

        def work(k):
            while True:
                with lock:
                    j = nxt[0]
                    nxt[0] += 1
                if j >= len(pairs):
                    return
                its.append(solve(k, pairs[j])["iterations_total"])

        t = time.time()
        th = [threading.Thread(target=work, args=(k,)) for k in range(inflight)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        dt = time.time() - t
        res[f"solve_only_rep{rep}"] = {"pairs": len(pairs), "seconds": dt,
                                       "pairs_per_s": len(pairs) / dt, "iterations": sorted(its)}

    # ---- one solve alone, profiled: the GPU time of a slice's solve
    eng.set_profiling(True)
    u, v = bufs[0]
    one = []
    for j in (0, len(pairs) // 2):
        t = time.time()
        st = eng.calc_device(pairs[j][0].data_ptr(), fw, pairs[j][1].data_ptr(), fw, fw, fh,
                             u.data_ptr(), v.data_ptr(), 4 * fw, stream=eng.stream)
        torch.cuda.synchronize()
        one.append({"wall_ms": 1e3 * (time.time() - t), "kernel_ms": st["kernel_ms"],
                    "kernel_ms_sum": sum(st["kernel_ms"]), "iterations": st["iterations_total"]})
    eng.set_profiling(False)
    res["solve_alone"] = one

    # ---- the three kernels on full-size planes, two ways.
    # cold: what the pipeline sees, where a slice's planes are touched once per stage. Each call
    #   works on another slice, after a 1 GiB fill has pushed the planes out of the 256 MB
    #   last-level cache; the time is the engine's own profiling (class 2: the calls' marks are
    #   added to the ctx's next solve, so that solve's class 2 alone is subtracted), with torch
    #   events around the same calls beside it.
    # warm: 20 calls back to back on the same buffers, whose working sets (176, 31, 101 MB) fit
    #   the last-level cache: a cache rate, not an HBM rate.
    s = torch.cuda.current_stream().cuda_stream
    bl = torch.empty((H, W), dtype=torch.uint8, device=dev)
    hf = torch.empty((fh, fw), dtype=torch.uint8, device=dev)
    cw, ch = W + 2 * BORDER, H + 2 * BORDER
    cv = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    calls = {
        "k_blend6_u8": (lambda i: eng.blend6_u8(neighbours(i), [W] * 6, W, H, bl.data_ptr(), W, stream=s),
                        7.0 * W * H),
        "k_half_u8": (lambda i: eng.half_u8(sl[i].data_ptr(), W, W, H, hf.data_ptr(), fw, stream=s),
                      1.25 * W * H),
        "k_remap_flow_u8": (lambda i: eng.remap_flow_u8(sl[i].data_ptr(), W, W, H, u.data_ptr(),
                                                        v.data_ptr(), 4 * fw, fw, fh, 2.0, BORDER,
                                                        cv.data_ptr(), cw, stream=s),
                            1.0 * W * H + 1.0 * cw * ch + 8.0 * fw * fh),
    }
    mid = 3 + len(pairs) // 2
    order = list(range(3, n - 3))

    def profiled_solve():
        st = eng.calc_device(pairs[0][0].data_ptr(), fw, pairs[0][1].data_ptr(), fw, fw, fh,
                             u.data_ptr(), v.data_ptr(), 4 * fw, stream=eng.stream)
        torch.cuda.synchronize()
        return st["kernel_ms"][2], st["kernel_launches"][2]

    def rates(ms, nbytes):
        return {"TB_per_s": nbytes / ms / 1e9, "fraction_of_8TBps": nbytes / ms / 1e9 / 8.0}

    for fn, _ in calls.values():
        fn(mid)                                              # first launch of each kernel, untimed
    torch.cuda.synchronize()
    eng.set_profiling(True)
    base = sorted(profiled_solve() for _ in range(3))[1]     # the solve's own class 2
    kern = {}
    for name, (fn, nbytes) in calls.items():
        ev = []
        for i in order:
            evict.fill_(i)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        ms2, n2 = profiled_solve()
        if n2 - base[1] != len(order):
            raise SystemExit(f"{name}: {n2 - base[1]} class-2 marks for {len(order)} calls")
        cold = (ms2 - base[0]) / len(order)
        ev.sort()
        kern[name] = {"compulsory_bytes": nbytes, "calls": len(order),
                      "cold": {"ms_engine_profiling_mean": cold, **rates(cold, nbytes),
                               "solve_class2_ms": base[0], "with_calls_class2_ms": ms2,
                               "ms_torch_events_median": ev[len(ev) // 2], "ms_torch_events_min": ev[0],
                               "ms_torch_events_max": ev[-1]}}
    eng.set_profiling(False)
    for name, (fn, nbytes) in calls.items():
        for _ in range(3):
            fn(mid)
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(mid)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        med = ms[len(ms) // 2]
        kern[name]["warm"] = {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], **rates(med, nbytes)}
    res["kernels"] = kern

    def t(name):
        return kern[name]["cold"]["ms_engine_profiling_mean"]

    per_slice = t("k_blend6_u8") + 2 * t("k_half_u8") + t("k_remap_flow_u8")
    solve_ms = sum(o["kernel_ms_sum"] for o in one) / len(one)
    res["per_slice"] = {"new_kernels_ms": per_slice, "solve_kernel_ms": solve_ms,
                        "share_of_gpu_time": per_slice / (per_slice + solve_ms)}
    (out / "measure.json").write_text(json.dumps(res, indent=1))
    print(json.dumps({k: res[k] for k in ("solve_only_rep1", "kernels", "per_slice")}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=("gen", "cli", "kernels"))
    ap.add_argument("stack")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--inflight", type=int, default=3)
    a = ap.parse_args()
    if a.step == "gen":
        return gen(Path(a.stack))
    if not a.out:
        ap.error("OUT_DIR is needed")
    if a.step == "cli":
        return cli(Path(a.stack), Path(a.out), a.inflight)
    return kernels(Path(a.stack), Path(a.out), a.inflight)


if __name__ == "__main__":
    sys.exit(main())
