"""The warp gathers' LDS-window switch, pinned in flow: tests/warp_window.py's table on the GPU,
bitwise against the oracle's seeded entry (tests/test_warp_window_cpu.py shows on the CPU that
every seed sits on the edge it was built for, that the reference cares which pixel a tap reads,
and that no stopping decision is close).

With nscales = 1 tvl1_calc_init hands the seed to the first warp unchanged, so every pixel's taps
are chosen: the first and last tap footprint inside each kernel's window and the first outside
on every side, at integer coordinates, 1 ulp off them and at sums that round up, and flows that
leave the frame.  One test per (kernel row, arithmetic): one engine under the knob set that
reaches the kernel, every parameter set and seed of the row through tvl1_calc_init
(tvl1_calc_batch_init for the batch rows, one pair per seed):
  k_warp_ring<6,2>        TVL1_ROLL_SEG=8, fixed work
  k_warp_img              TVL1_BUF_LIMIT=0, fixed work
  k_warp_iter<6,.,128,.>  TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8 with two consumer wavefronts and
                          (+ TVL1_WI_NC=1) one; the stopping rule (the fused pass needs epsilon > 0)
  kb_warp_iter            TVL1_BATCH_SMALL=0, seeds x / xy / beyond as three pairs
  kb_warp_ring            TVL1_BATCH_FUSE=0,TVL1_BATCH_SMALL=0, the same seeds
  kb_small_level          the default on-chip path, all five seeds as five pairs
fast_math 0 and 2: the flow's bits and the per-warp counts are checker.oracle_calc(init=...)'s;
single-pair fixed-work cases also count their iteration passes (kernel_launches[0]).
fast_math 1 is bitwise the oracle's fast branch on every row and parameter set in
tests/test_gpu_fast_bitwise.py; here its fixed-work cases are also held to
tests/test_gpu_fastmath.py's bar against the IEEE reference, mean EPE <= 1e-3 px and at most 1e-3 of the px over 1e-2 px
(on the CPU the IEEE and fma references of these cases are at most 1.3e-5 px apart in the mean,
no px over 1e-2: the bar is one the reference side meets).
"""
import numpy as np
import pytest

import edge_cases as ec
import warp_window as ww
from optflow_amd import capi
from test_gpu_edge_cases import KNOBS

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MATH_IDS = {0: "ieee", 1: "fast", 2: "fma"}


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


def dev(a):
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def run_single(eng, I0, I1, seed):
    """tvl1_calc_init on device buffers -> (u, v, stats with warp_iters)."""
    h, w = I0.shape
    d0, d1, s0, s1 = dev(I0), dev(I1), dev(seed[0]), dev(seed[1])
    du = torch.zeros((h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    torch.cuda.synchronize()
    st = eng.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, du.data_ptr(), dv.data_ptr(), 4 * w,
                         warp_iters=True, init=(s0.data_ptr(), s1.data_ptr(), 4 * w))
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


def run_batch(eng, I0s, I1s, U0, V0):
    """tvl1_calc_batch_init, one seed per pair -> (u, v, per-pair stats)."""
    n, h, w = I0s.shape
    d0, d1, s0, s1 = dev(I0s), dev(I1s), dev(U0), dev(V0)
    du = torch.zeros((n, h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    torch.cuda.synchronize()
    st = eng.calc_batch_device(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h, du.data_ptr(),
                               dv.data_ptr(), 4 * w, 4 * w * h, warp_iters=True,
                               init=(s0.data_ptr(), s1.data_ptr(), 4 * w, 4 * w * h))
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


def mismatch(name, u, v, st, ref):
    """None, or what differs from the oracle: levels, per-warp counts, or where the flow's bits
    differ (how many px, the box that holds them, and how far)."""
    ur, vr, sr, wr = ref
    if st["levels"] != sr["levels"] or st["sizes"] != sr["sizes"]:
        return f"{name}: levels {st['sizes']} != {sr['sizes']}"
    if not np.array_equal(st["warp_iters"], wr):
        return f"{name}: per-warp iterations {np.asarray(st['warp_iters']).tolist()} != {wr.tolist()}"
    bad = (u.view(np.uint32) != ur.view(np.uint32)) | (v.view(np.uint32) != vr.view(np.uint32))
    if bad.any():
        ys, xs = np.nonzero(bad)
        d = max(np.abs(u - ur)[bad].max(), np.abs(v - vr)[bad].max())
        return (f"{name}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} y {ys.min()}..{ys.max()}, "
                f"max |d| {d:.3g}")
    return None


def off_budget(name, u, v, st, ref):
    """fast_math 1 against the IEEE reference: the schedule, then test_gpu_fastmath.py's bar."""
    ur, vr, sr, wr = ref
    if not np.array_equal(st["warp_iters"], wr):
        return f"{name}: per-warp iterations {np.asarray(st['warp_iters']).tolist()} != {wr.tolist()}"
    e = capi.epe(u, v, ur, vr)
    mean, over = float(e.mean()), float((e > 1e-2).mean())
    print(f"{name}: fast vs IEEE mean {mean:.3g} px, {over:.3g} of the px over 1e-2 px, max {float(e.max()):.3g}")
    if not np.isfinite(e).all() or mean > 1e-3 or over > 1e-3:
        return f"{name}: mean EPE {mean:.3g}, {over:.3g} of the px over 1e-2 px"
    return None


def psets_of(row, math):
    """fast_math 1 runs the fixed-work sets only."""
    return {n: p for n, p in row.psets.items() if math != 1 or p.get("epsilon", 0.01) == 0}


ROWS = [(r.name, m) for r in ww.ROWS for m in (0, 2, 1) if psets_of(r, m)]


@pytest.mark.parametrize("name,math", ROWS, ids=[f"{n}-{MATH_IDS[m]}" for n, m in ROWS])
def test_window_edge_seeds(built, monkeypatch, name, math):
    row = ww.ROW_OF[name]
    set_knobs(monkeypatch, row.knobs)
    check = off_budget if math == 1 else mismatch
    ref_math = 0 if math == 1 else math
    eng, bad, ran = None, [], 0
    try:
        for pname, params in psets_of(row, math).items():
            p = capi.make_params(fast_math=math, **params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            fixed = params.get("epsilon", 0.01) == 0
            if row.batch:
                prs = [ww.frames(row, b) for _, b in ww.solves(row)]
                sds = [ww.make_seed(row.geom, kind, row.W, row.H) for kind, _ in ww.solves(row)]
                u, v, st = run_batch(eng, np.stack([a for a, _ in prs]), np.stack([b for _, b in prs]),
                                     np.stack([s[0] for s in sds]), np.stack([s[1] for s in sds]))
                for kind, b in ww.solves(row):
                    bad.append(check(f"{pname} {kind} (pair {b})", u[b], v[b], st[b],
                                     ww.reference(row, pname, kind, b, ref_math)))
                    ran += 1
                continue
            eng.set_profiling(fixed)
            I0, I1 = ww.frames(row)
            for kind, _ in ww.solves(row):
                u, v, st = run_single(eng, I0, I1, ww.make_seed(row.geom, kind, row.W, row.H))
                bad.append(check(f"{pname} {kind}", u, v, st, ww.reference(row, pname, kind, 0, ref_math)))
                ran += 1
                if fixed:   # nothing fused or speculated with epsilon = 0: warps x sched_after's passes
                    passes = ec.fixed_work_passes(params["iterations"], 4)
                    if st["kernel_launches"][0] != params["warps"] * len(passes):
                        bad.append(f"{pname} {kind}: {st['kernel_launches'][0]} iteration passes, schedule "
                                   f"{passes} per warp")
    finally:
        if eng is not None:
            eng.close()
    bad = [b for b in bad if b]
    assert ran == len(psets_of(row, math)) * len(row.seeds)
    assert not bad, f"[{row.knobs}] {len(bad)} of {ran} solves: " + "; ".join(bad)
