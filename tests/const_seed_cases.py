"""TEST INFRASTRUCTURE: the cases of the batched solves seeded by one constant per pair
(tvl1_calc_batch_const_init, tvl1_calc_batch_auto_init), shared by the CPU and GPU tests, and
their reference: tests/initflow_ref.py's composed solve (the oracle's own seeded entry in fma
mode) on two planes filled with the pair's constants.

A constant seed is not a constant coarsest level: the seed pyramid's bilinear weights are
rounded per px, so its levels hold several bit patterns (test_batch_const_seed_cpu.py counts
them for every non-integer constant here).  That is what lets the GPU tests tell the kernel
that evaluates the weights from one that fills the level with c * scaleStep^(L - 1)."""
from __future__ import annotations

import numpy as np

import initflow_ref as ref
import shift_ref

# Per pair (dx, dy): (0, 0) equals the unseeded solve; negative and non-integer values, dx != dy
# and every pair different (a swapped component or pair index shows); an integer pair; one
# that leaves the frame.  The one-step chain of nscales 2 rounds most constants one way on
# every px, so its cases take constants picked for the ones it does not.
CONSTS = [(0.0, 0.0), (-3.5, 4.25), (2.75, -0.7), (1.0, 3.0), (200.5, -150.25)]
CONSTS_2 = [(0.0, 0.0), (-3.45, 4.15), (2.7, -0.7), (1.0, 3.0), (150.7, -120.7)]

# Frames off the 64 x 4 launch tile; nscales 1 the fill (65 x 33 streams its only level, 130 x
# 12 is solved on chip), 2 the const step alone (into set 0), 3 and 4 both set parities.
CASES = {
    "65x33_s1": dict(w=65, h=33, kw=dict(nscales=1, warps=3), rng=501, consts=CONSTS),
    "130x12_s1": dict(w=130, h=12, kw=dict(nscales=1, warps=3), rng=607, consts=CONSTS),
    "65x33_s2": dict(w=65, h=33, kw=dict(nscales=2, warps=3), rng=511, consts=CONSTS_2),
    "100x37_s3": dict(w=100, h=37, kw=dict(nscales=3, warps=3), rng=521, consts=CONSTS),
    "130x70_s4": dict(w=130, h=70, kw=dict(nscales=4, warps=3), rng=531, consts=CONSTS),
}
# gamma != 0: the pairs are solved one by one from planes filled in scratch
GAMMA = dict(w=97, h=61, kw=dict(gamma=0.1, nscales=4, warps=3), rng=541,
             consts=[(0.0, 0.0), (-3.5, 4.25), (2.75, -0.7)])
# two chunks (256 + 1) of the smallest two-level frame, one frame pair for every pair of the
# batch (pair_stride 0), every pair its own constant
CHUNKS = dict(w=40, h=24, n=257, kw=dict(nscales=2, warps=2), rng=551)


def chunk_consts(n):
    b = np.arange(n, dtype=np.float64)
    return np.stack([(b % 23) * 0.35 - 3.85, 5.9 - (b % 19) * 0.1], 1).astype(np.float32)


def frames(case, b=0):
    """Frames of pair b of a case (every pair its own)."""
    return ref.frames_of(dict(w=case["w"], h=case["h"], rng=case["rng"] + b, z=1 + b % 3))


def filled(case, c):
    h, w = case["h"], case["w"]
    return np.full((h, w), c[0], np.float32), np.full((h, w), c[1], np.float32)


def reference(name, case, b, math=0):
    """(u, v, warp_iters, trace) of pair b from its filled planes, computed once and shared."""
    I0, I1 = frames(case, b)
    return ref.reference(("const", name, b), I0, I1, case["kw"], *filled(case, case["consts"][b]),
                         math=math)


def is_integer(c):
    return float(c) == float(int(c))


# ---- the auto route: tests/shift_ref.py's windows at small sizes, drift inside R.  One-level
# searches (R <= 4) and a pyramid (R = 8); a pair whose estimate is (0, 0); `shared`: one
# frame 0 for every pair (pair_stride0 = 0).
AUTO = {
    "64x48_R4": dict(w=64, h=48, R=4, kw=dict(nscales=3, warps=2),
                     shifts=[(3, -2), (0, 0), (-4, 4), (1, 0)]),
    "67x45_R8": dict(w=67, h=45, R=8, kw=dict(nscales=3, warps=2),
                     shifts=[(8, -8), (0, 0), (-5, 3), (2, 7), (-8, -1)]),
    "96x40_R8_shared": dict(w=96, h=40, R=8, kw=dict(nscales=3, warps=2), shared=True,
                            shifts=[(0, 0), (6, -3), (-7, 8)]),
}


def auto_batch(case, n=None):
    """(I0s, I1s) of an AUTO case, n pairs (default one per listed shift, repeating after)."""
    sh = case["shifts"]
    n = n or len(sh)
    w, h = case["w"], case["h"]
    if case.get("shared"):   # windows of one frame: I1_b(x + d_b) = I0(x) exactly
        m = 8
        base = shift_ref.window_pair(w + 2 * m, h + 2 * m, 0, 0, rng=310)[0]
        I0s = np.stack([base[m:m + h, m:m + w]])
        I1s = np.stack([base[m - dy:m - dy + h, m - dx:m - dx + w]
                        for dx, dy in (sh[b % len(sh)] for b in range(n))])
        return I0s, I1s
    prs = [shift_ref.window_pair(w, h, *sh[b % len(sh)], rng=300 + b % len(sh)) for b in range(n)]
    return np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])
