#!/usr/bin/env python3
"""Measurement of the integer drift estimate (tvl1_estimate_shift) on one MI355X.

    python tools/shift_measure.py OUT_DIR            # OUT_DIR/measure.json
    python tools/shift_measure.py OUT_DIR --trace    # the same calls, few, for a kernel trace
    python tools/shift_measure.py --per-launch run_kernel_trace.csv   # no GPU: the trace's launches

Two shapes: one 6144x4096 pair alone at max_shift 64, and a 256-pair batch of 3072x100 strips at
max_shift 25.  Cold, as DESIGN 11 measured the slice-list kernels: every call works on another
pair (another batch) after a 1 GiB fill has pushed the frames out of the 256 MB last-level
cache; the time is between two events on the call's stream (the call's own host wait for its
record lies inside).  Beside them the solve of the same shape alone (C2's parameters: 5 scales,
30 warps; the strips': 10 scales, 5 warps) and the compulsory bytes of the byte model over the
time, against 8 TB/s.  The frames are windows of one device-made texture with N(0, 2) noise per
frame, so every estimate has a known answer, which is checked."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))

PAD = 128


def levels_of(R):
    L = 0
    while (R + (1 << L) - 1) >> L > 4:
        L += 1
    return L


def byte_model(w, h, R, n=1):
    """Compulsory bytes: per level both frames read once by k_sad_shifts; per pyramid step both
    frames read once and the halved ones written once."""
    L = levels_of(R)
    per, ws, hs = [], w, h
    for l in range(L + 1):
        b = {"level": l, "w": ws, "h": hs, "sad_read": 2 * ws * hs * n}
        if l < L:
            b["half_read"] = 2 * (ws & ~1) * (hs & ~1) * n
            b["half_write"] = 2 * (ws // 2) * (hs // 2) * n
        per.append(b)
        ws, hs = ws // 2, hs // 2
    total = sum(v for b in per for k, v in b.items() if k not in ("level", "w", "h"))
    return {"levels": per, "total": total}


def per_launch(path):
    """The estimate's launches of a rocprofv3 kernel trace, in start order, with their times."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "tvl1k::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("tvl1k::", "")
        if not name.startswith(("k_sad_shifts", "k_shift_")):
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        print(f"{name:24s} grid {r['Grid_Size_X']:>6} x {r['Grid_Size_Y']:>4} x {r['Grid_Size_Z']:<4} {us:9.2f} us")


class Frames:
    def __init__(self, W, H, dev, seed):
        from optflow_amd import synth_device
        self.W, self.H, self.dev = W, H, dev
        self.base = synth_device.DeviceStack(W + 2 * PAD, H + 2 * PAD, dev, seed=seed).base[0, 0]
        self.g = torch.Generator(device=dev)
        self.g.manual_seed(seed + 1)

    def window(self, ox, oy):
        a = self.base[PAD - oy:PAD - oy + self.H, PAD - ox:PAD - ox + self.W]
        a = a + 2.0 * torch.randn((self.H, self.W), generator=self.g, device=self.dev)
        return torch.clamp(torch.round(a), 0, 255).to(torch.uint8).contiguous()


def timed(fn, evict, tag):
    evict.fill_(tag)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn, evict, tag):
    """Host clock around a call and the device's work (solves run on the engine's own stream)."""
    evict.fill_(tag)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--trace", action="store_true", help="two calls per shape, no solves")
    ap.add_argument("--per-launch", metavar="CSV", help="list the launches of a kernel trace (no GPU)")
    a = ap.parse_args()
    if a.per_launch:
        return per_launch(a.per_launch)
    if not a.out:
        ap.error("OUT_DIR is needed")
    global torch
    import torch
    from optflow_amd import capi
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    res = {}

    # ---- one 6144x4096 pair alone
    W, H, R = 6144, 4096, 64
    fr = Frames(W, H, dev, 0x5EED)
    shifts = [(37, -52), (-64, 64), (5, 3), (-21, -40), (64, -1), (0, 0)]
    pairs = [(fr.window(0, 0), fr.window(dx, dy)) for dx, dy in shifts]
    eng = capi.Engine(capi.make_params(nscales=5, warps=30))
    est = lambda p: eng.estimate_shift(p[0].data_ptr(), W, p[1].data_ptr(), W, W, H, R, stream=s)
    est(pairs[0])                       # first launches, workspace
    torch.cuda.synchronize()
    ms, got = [], []
    for rep in range(1 if a.trace else 3):
        for i, p in enumerate(pairs[:2] if a.trace else pairs):
            t, r = timed(lambda: est(p), evict, i + rep)
            ms.append(t)
            got.append((r["dx"], r["dy"]) == shifts[i])
    bm = byte_model(W, H, R)
    one = {"w": W, "h": H, "max_shift": R, "all_shifts_recovered": all(got), "cold": stats(ms),
           "byte_model": bm}
    med = one["cold"]["ms_median"]
    one["TB_per_s"] = bm["total"] / med / 1e9
    one["fraction_of_8TBps"] = one["TB_per_s"] / 8.0
    if not a.trace:
        u = torch.empty((H, W), dtype=torch.float32, device=dev)
        v = torch.empty_like(u)
        sol = []
        for i in range(3):
            sol.append(wall(lambda: eng.calc_device(pairs[i][0].data_ptr(), W, pairs[i][1].data_ptr(), W, W, H,
                                                    u.data_ptr(), v.data_ptr(), 4 * W, stream=eng.stream,
                                                    stats=False), evict, i))
        one["solve_alone_wall_ms"] = sol     # the first one allocates the solver's scratch
        one["estimate_wall_ms"] = [wall(lambda: est(p), evict, 9) for p in pairs[:3]]
        one["share_of_solve"] = med / min(sol[1:])
    res["pair_6144x4096"] = one
    del pairs, fr
    eng.close()

    # ---- a 256-pair batch of 3072x100 strips
    W, H, R, n = 3072, 100, 25, 256
    fr = Frames(W, H, dev, 0xBEEF)
    bshifts = [((7 * b) % 51 - 25, (11 * b) % 51 - 25) for b in range(n)]
    batches = []
    for k in range(1 if a.trace else 3):
        A = torch.stack([fr.window(0, 0) for _ in range(n)])
        B = torch.stack([fr.window(*bshifts[(b + k) % n]) for b in range(n)])
        batches.append((A, B, k))
    eng = capi.Engine(capi.make_params(nscales=10, warps=5))
    estb = lambda t: eng.estimate_shift_batch(n, t[0].data_ptr(), W, W * H, t[1].data_ptr(), W, W * H,
                                              W, H, R, stream=s)
    estb(batches[0])
    torch.cuda.synchronize()
    ms, got = [], []
    for rep in range(2 if a.trace else 3):
        for t in batches:
            tt, r = timed(lambda: estb(t), evict, rep)
            ms.append(tt)
            got.append(all((r[b]["dx"], r[b]["dy"]) == bshifts[(b + t[2]) % n] for b in range(n)))
    bm = byte_model(W, H, R, n)
    bat = {"w": W, "h": H, "pairs": n, "max_shift": R, "all_shifts_recovered": all(got),
           "cold": stats(ms), "byte_model": bm}
    med = bat["cold"]["ms_median"]
    bat["TB_per_s"] = bm["total"] / med / 1e9
    bat["fraction_of_8TBps"] = bat["TB_per_s"] / 8.0
    if not a.trace:
        u = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        v = torch.empty_like(u)
        sol = []
        for t in batches:
            sol.append(wall(lambda: eng.calc_batch_device(n, t[0].data_ptr(), W, W * H, t[1].data_ptr(), W,
                                                          W * H, W, H, u.data_ptr(), v.data_ptr(), 4 * W,
                                                          4 * W * H, stream=eng.stream), evict, t[2]))
        bat["solve_batch_wall_ms"] = sol
        bat["estimate_wall_ms"] = [wall(lambda: estb(t), evict, 9) for t in batches]
        bat["share_of_solve"] = med / min(sol[1:])
    res["batch_256x3072x100"] = bat
    eng.close()

    (out / ("measure_trace.json" if a.trace else "measure.json")).write_text(json.dumps(res, indent=1))
    brief = {k: {x: v[x] for x in v if x != "byte_model"} for k, v in res.items()}
    print(json.dumps(brief, indent=1))


if __name__ == "__main__":
    main()
