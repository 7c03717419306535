#!/usr/bin/env python3
"""Measurement of flow composition (tvl1_compose_flow) on one MI355X.

    python tools/compose_measure.py OUT_DIR             # OUT_DIR/measure.json

Cold, as tools/zncc_measure.py measured the ZNCC score: two shapes, one 6144x4096 plane set and
256 strips of 3072x100; every call works on another set of buffers after a 1 GiB fill has pushed
the planes out of the 256 MB last-level cache; the time is between two events on the call's
stream, the median of 9 calls.  Flow a and flow b are the engine's own forward flow of a
synthetic pair (C2's parameters: 5 scales, 30 warps; the strips': 10 scales, 5 warps), so the
gather sees what a chain gives it, and the forward solve is timed in the same call.  Compulsory
bytes: 24 B/px (a 8, b 8, c 8); the four taps of a px lie in cache lines its neighbours load.
Uncounted calls only: a counted call also waits for its counts on the host."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
sys.path.insert(0, str(ROOT / "tools"))


def shape(eng, zm, I0, I1, n, W, H, evict, s):
    """I0, I1: (n, H, W) u8 on the device.  Solves forward, then times the composition cold."""
    fl = torch.empty((2, n, H, W), dtype=torch.float32, device=I0.device)
    P, S = 4 * W, 4 * W * H

    def solve():
        if n == 1:
            eng.calc_device(I0.data_ptr(), W, I1.data_ptr(), W, W, H, fl[0].data_ptr(), fl[1].data_ptr(), P,
                            stream=eng.stream, stats=False)
        else:
            eng.calc_batch_device(n, I0.data_ptr(), W, W * H, I1.data_ptr(), W, W * H, W, H, fl[0].data_ptr(),
                                  fl[1].data_ptr(), P, S, stream=eng.stream)

    sol = [zm.wall(solve, evict, k) for k in range(3)]   # the first allocates
    sets = [(fl.clone(), fl.clone(), torch.empty_like(fl)) for _ in range(3)]   # a, b, c
    torch.cuda.synchronize()
    px = n * W * H
    out = {"w": W, "h": H, "pairs": n, "px": px, "solve_forward_wall_ms": sol,
           "flow_abs_max_px": float(fl.abs().max().item())}
    comp = lambda t, count: eng.compose_flow_batch(
        n, t[0][0].data_ptr(), t[0][1].data_ptr(), P, S, t[1][0].data_ptr(), t[1][1].data_ptr(), P, S, W, H,
        t[2][0].data_ptr(), t[2][1].data_ptr(), P, S, stream=s, count=count)
    cnt = comp(sets[0], True)
    torch.cuda.synchronize()
    out["outside_share"] = float(cnt.sum()) / px
    ms = [zm.timed(lambda: comp(t, False), evict, i + k)[0] for k in range(3) for i, t in enumerate(sets)]
    st = zm.stats(ms)
    st["compulsory_bytes"] = 24 * px
    st["TB_per_s"] = 24 * px / st["ms_median"] / 1e9
    st["fraction_of_8TBps"] = st["TB_per_s"] / 8.0
    st["share_of_forward_solve"] = st["ms_median"] / min(sol[1:])
    out["compose_flow"] = st
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    a = ap.parse_args()
    global torch
    import torch
    from optflow_amd import capi
    import shift_measure
    import zncc_measure as zm
    shift_measure.torch = zm.torch = torch   # their helpers use the module's
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
    res["planes_6144x4096"] = shape(eng, zm, fr.window(0, 0)[None].contiguous(),
                                    fr.window(2, -1)[None].contiguous(), 1, W, H, evict, s)
    eng.close()
    del fr
    torch.cuda.empty_cache()
    (out / "measure.json").write_text(json.dumps(res, indent=1))

    W, H, n = 3072, 100, 256
    fr = Frames(W, H, dev, 0xBEEF)
    A = torch.stack([fr.window(0, 0) for _ in range(n)])
    B = torch.stack([fr.window(b % 5 - 2, b % 3 - 1) for b in range(n)])
    eng = capi.Engine(capi.make_params(nscales=10, warps=5))
    res["strips_256x3072x100"] = shape(eng, zm, A, B, n, W, H, evict, s)
    eng.close()
    (out / "measure.json").write_text(json.dumps(res, indent=1))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
