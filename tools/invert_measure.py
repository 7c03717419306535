#!/usr/bin/env python3
"""Measurement of flow inversion (tvl1_invert_flow) on one MI355X.

    python tools/invert_measure.py OUT_DIR             # OUT_DIR/measure.json

Cold, as tools/compose_measure.py measured the composition: two shapes, one 6144x4096 plane set
and 256 strips of 3072x100; every call works on another set of buffers after a 1 GiB fill has
pushed the planes out of the 256 MB last-level cache; the time is between two events on the
call's stream, the median of 9 uncounted calls.  f is the engine's own forward flow of a synthetic
pair (C2's parameters: 5 scales, 30 warps; the strips': 10 scales, 5 warps) composed with itself
three times through tvl1_compose_flow, so it looks like a four-link chain, and the forward solve
is timed in the same call.  K = 1, 4 and 8 on both arms of the kernel (TVL1_INVERT_WINDOW = 0 / 1,
read when the ctx is created).  Compulsory bytes: 20 B/px (f 8 read once, g 8 and resid 4
written); the taps of a px lie in cache lines its neighbours load."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
sys.path.insert(0, str(ROOT / "tools"))

KS = (1, 4, 8)


def shape(capi, params, zm, I0, I1, n, W, H, evict, s):
    """I0, I1: (n, H, W) u8 on the device.  Solves forward, chains, then times the inversion cold."""
    fl = torch.empty((2, n, H, W), dtype=torch.float32, device=I0.device)
    P, S = 4 * W, 4 * W * H
    eng = capi.Engine(params)

    def solve():
        if n == 1:
            eng.calc_device(I0.data_ptr(), W, I1.data_ptr(), W, W, H, fl[0].data_ptr(), fl[1].data_ptr(), P,
                            stream=eng.stream, stats=False)
        else:
            eng.calc_batch_device(n, I0.data_ptr(), W, W * H, I1.data_ptr(), W, W * H, W, H, fl[0].data_ptr(),
                                  fl[1].data_ptr(), P, S, stream=eng.stream)

    sol = [zm.wall(solve, evict, k) for k in range(3)]   # the first allocates
    chain = fl.clone()
    torch.cuda.synchronize()
    for _ in range(3):   # in place on the accumulator
        eng.compose_flow_batch(n, chain[0].data_ptr(), chain[1].data_ptr(), P, S, fl[0].data_ptr(),
                               fl[1].data_ptr(), P, S, W, H, chain[0].data_ptr(), chain[1].data_ptr(), P, S,
                               stream=eng.stream, count=False)
    torch.cuda.synchronize()
    eng.close()
    px = n * W * H
    out = {"w": W, "h": H, "pairs": n, "px": px, "solve_forward_wall_ms": sol,
           "link_abs_max_px": float(fl.abs().max().item()), "chain_abs_max_px": float(chain.abs().max().item())}
    del fl
    sets = [(chain.clone(), torch.empty((3, n, H, W), dtype=torch.float32, device=I0.device)) for _ in range(3)]
    torch.cuda.synchronize()
    for arm in ("0", "1"):
        os.environ["TVL1_INVERT_WINDOW"] = arm
        eng = capi.Engine(params)
        del os.environ["TVL1_INVERT_WINDOW"]
        inv = lambda t, K, counts: eng.invert_flow_batch(
            n, t[0][0].data_ptr(), t[0][1].data_ptr(), P, S, K, 0.01, t[1][0].data_ptr(), t[1][1].data_ptr(),
            P, S, t[1][2].data_ptr(), P, S, W, H, stream=s, counts=counts)
        res = {}
        for K in KS:
            cnt = inv(sets[0], K, True)
            torch.cuda.synchronize()
            ms = [zm.timed(lambda: inv(t, K, False), evict, i + k)[0] for k in range(3) for i, t in enumerate(sets)]
            st = zm.stats(ms)
            st["ms_all"] = ms
            st["outside_share"] = float(cnt[:, 0].sum()) / px
            st["unconverged_share"] = float(cnt[:, 1].sum()) / px
            st["compulsory_bytes"] = 20 * px
            st["TB_per_s"] = 20 * px / st["ms_median"] / 1e9
            st["fraction_of_8TBps"] = st["TB_per_s"] / 8.0
            st["share_of_forward_solve"] = st["ms_median"] / min(sol[1:])
            res[f"K{K}"] = st
        out["window" if arm == "1" else "global"] = res
        eng.close()
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
    res["planes_6144x4096"] = shape(capi, capi.make_params(nscales=5, warps=30), zm,
                                    fr.window(0, 0)[None].contiguous(), fr.window(2, -1)[None].contiguous(),
                                    1, W, H, evict, s)
    del fr
    torch.cuda.empty_cache()
    (out / "measure.json").write_text(json.dumps(res, indent=1))

    W, H, n = 3072, 100, 256
    fr = Frames(W, H, dev, 0xBEEF)
    A = torch.stack([fr.window(0, 0) for _ in range(n)])
    B = torch.stack([fr.window(b % 5 - 2, b % 3 - 1) for b in range(n)])
    res["strips_256x3072x100"] = shape(capi, capi.make_params(nscales=10, warps=5), zm, A, B, n, W, H, evict, s)
    (out / "measure.json").write_text(json.dumps(res, indent=1))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
