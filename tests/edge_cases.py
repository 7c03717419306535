"""TEST INFRASTRUCTURE: the one table of frame sizes that sit on the solve kernels' geometry
edges -- the last band one pixel wide, a band ending on the frame edge, a last segment of one
row, frames narrower than a halo -- with the parameters and dispatch knobs that send each size
through the kernel it was built for.

The iteration and warp kernels cut a level into fixed pieces (csrc/tvl1_plan.hpp):
  k_warp_ring<6,2> / kb_warp_ring          64-px bands, segments of seg_rows rows
  k_warp_iter<6,.,128,.,2> / kb_warp_iter  124-px bands (128 - 2 * 2 px of halo), segments
  k_iterate_roll<G,1|2,2>                  124-px bands; <G,3|4,2> and _mid: 120; <G,1|2,4>: 248
  kb_iterate_roll<K,1>                     64 - 2K px: 62, 60, 58, 56; <K,2>: 124 / 120
  k_iterate_tb4 (64 x 48 regions)          56-px tiles, 48 - 2K output rows: 44, 42, 40 (K = 2, 3, 4)
  k_iterate_tb<.,32,1,2> (64 x 32)         56-px tiles, 32 - 2K output rows: 30, 28, 26, 24
  k_warp_img                               64 x 16 tiles (kWarpTW x kWarpTH, tvl1_kernels.hpp)
  k_iterate<G,true>                        248-px wave segments (kSegPx), 32-row strips
Every width and height below is derived from those periods, and tests/test_edge_cases_cpu.py
asks the planner itself (tests/plan_dump.cpp) whether each one still straddles an edge, so a
changed band width fails there instead of leaving this table quietly stale.  The same CPU test
holds every stopping-rule case to the project's residual margin; tests/test_gpu_edge_cases.py
runs the table on the GPU, bitwise against the oracle.

All groups but `pyramid` use nscales = 1: the level is the frame and the geometry is exact.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from optflow_amd import synth

Case = namedtuple("Case", "name W H seed params group")

# ---------------------------------------------------------------- parameter sets
# Stopping rule: epsilon > 0 gives a 2-iteration first pass and lets warps end by a check; the
# cap of 40 keeps the tiny frames cheap (at 300 they run 300 iterations in the first warp).
# Fixed work (epsilon = 0): passes follow sched_after -- 10 iterations = 4, 4, 2; 7 = 4, 3;
# 1 = 1 -- so between them every K of every kernel runs at every edge.
STOP = dict(warps=3, iterations=40)
FIX10 = dict(warps=2, epsilon=0.0, iterations=10)
FIX7 = dict(warps=2, epsilon=0.0, iterations=7)
FIX1 = dict(warps=2, epsilon=0.0, iterations=1)
PLAIN = {"stop": STOP, "fix10": FIX10, "fix7": FIX7, "fix1": FIX1}
# gamma != 0: k_iterate_tb<true, ..>, k_iterate_roll<true, ..>
GAMMA = {k + "-gamma": dict(v, gamma=0.2) for k, v in PLAIN.items()}
# tau / theta < 0: k_iterate<false|true, true>, one iteration per launch whatever the schedule
TAU = {"stop-tau": dict(STOP, tau=-0.05), "fix7-tau": dict(FIX7, tau=-0.05),
       "stop-tau-gamma": dict(STOP, tau=-0.05, gamma=0.2), "fix7-tau-gamma": dict(FIX7, tau=-0.05, gamma=0.2)}

# ---------------------------------------------------------------- planner probes
# What the CPU test asks plan_dump about a group's sizes:
#   ("site", NAME, k, px)   bands / segments of a streaming launch site (plan_dump's `site`)
#   ("tb", k), ("tb4", k)   tiles_x / block rows of a blocked pass of k iterations (`blocked`)
#   ("iterate",)            wave segments / strips of k_iterate (`blocked`'s iterate_blocks)
#   ("warp_img",)           kWarpTW x kWarpTH tiles, read from tvl1_kernels.hpp
SEG = 8   # TVL1_ROLL_SEG of the streaming y edges (kRollMinSeg: the shortest segment)

# x edges: group -> (period B, parameter sets, probes, knob sets).  W in {B-1, B, B+1, 2B, 2B+1}
# at H = 9: with TVL1_ROLL_SEG=8 two segments, the second one row.
X_H = 9
X_GROUPS = {
    "x64": (64, PLAIN, [("site", "warp_ring", 6, 0), ("warp_img",)],
            ["TVL1_ROLL_SEG=8", "", "TVL1_BUF_LIMIT=0"]),
    "x124": (124, {**PLAIN, **GAMMA},
             [("site", "warp_iter", 8, 0), ("site", "roll", 1, 2), ("site", "roll", 2, 2)],
             ["TVL1_ROLL_SEG=8", "TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8",
              "TVL1_FUSE_MIN=0,TVL1_WI_NC=1,TVL1_ROLL_SEG=8"]),
    "x120": (120, {**PLAIN, **GAMMA}, [("site", "roll", 3, 2), ("site", "roll", 4, 2)],
             ["TVL1_ROLL_LONG_MIN=0,TVL1_ROLL_SEG=8",
              "TVL1_ROLL_LONG_MIN=0,TVL1_SPEC=0,TVL1_MID=1,TVL1_MID_MIN=1,TVL1_ROLL_SEG=8"]),
    "x248": (248, {**PLAIN, **GAMMA}, [("site", "roll", 1, 4), ("site", "roll", 2, 4)],
             ["TVL1_ROLL_PX4_MIN=0,TVL1_ROLL_SEG=8"]),
    "x56": (56, {**PLAIN, **GAMMA}, [("tb", k) for k in (1, 2, 3, 4)] + [("tb4", k) for k in (1, 2, 3, 4)],
            ["", "TVL1_TB4=0", "TVL1_BUF_LIMIT=0", "TVL1_TB4=0,TVL1_BUF_LIMIT=0"]),
    "x248-iterate": (248, TAU, [("iterate",)], [""]),
}

# y edges at W = 65: a one-px second band for the 64-px ring, a 9-px second tile for the
# blocked kernels.  group -> (heights, parameter sets, probes with their period, knob sets)
Y_W = 65
_TB4_OUT = {k: 48 - 2 * k for k in (2, 3, 4)}   # k = 2 only with TVL1_BUF_LIMIT=0 (k = 1: 46 + 1 rows, over the
                                                # 45-row cap on these frames)
_TB_OUT = {k: 32 - 2 * k for k in (1, 2, 3, 4)}


def _around(periods):
    return sorted({o + d for o in periods for d in (-1, 0, 1)})


Y_GROUPS = {
    # the streaming kernels, always with TVL1_ROLL_SEG=8; TVL1_BUF_LIMIT=0: k_warp_img's 16 rows
    "y-stream": ([7, 8, 9, 15, 16, 17], {**PLAIN, **GAMMA},
                 [(("site", "warp_ring", 6, 0), SEG), (("site", "warp_iter", 8, 0), SEG)] +
                 [(("site", "roll", k, 2), SEG) for k in (1, 2, 3, 4)] +
                 [(("site", "roll", k, 4), SEG) for k in (1, 2)] + [(("warp_img",), 16)],
                 ["TVL1_ROLL_SEG=8", "TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8",
                  "TVL1_FUSE_MIN=0,TVL1_WI_NC=1,TVL1_ROLL_SEG=8",
                  "TVL1_ROLL_LONG_MIN=0,TVL1_ROLL_SEG=8",
                  "TVL1_ROLL_LONG_MIN=0,TVL1_SPEC=0,TVL1_MID=1,TVL1_MID_MIN=1,TVL1_ROLL_SEG=8",
                  "TVL1_ROLL_PX4_MIN=0,TVL1_ROLL_SEG=8", "TVL1_BUF_LIMIT=0"]),
    "y-tb4": (_around(_TB4_OUT.values()), PLAIN, [(("tb4", k), o) for k, o in _TB4_OUT.items()],
              ["", "TVL1_BUF_LIMIT=0"]),
    "y-tb": (_around(_TB_OUT.values()), {**PLAIN, **GAMMA}, [(("tb", k), o) for k, o in _TB_OUT.items()],
             ["TVL1_TB4=0", "TVL1_TB4=0,TVL1_BUF_LIMIT=0"]),
    "y-iterate": ([31, 32, 33], TAU, [(("iterate",), 32)], [""]),
}

# both edges at once: 124 + 1 x 40 + 1 (tb4, k = 4), 248 + 1 x 44 + 1 (tb4, k = 2 under
# TVL1_BUF_LIMIT=0), 56 + 1 x 24 + 1 (tb, k = 4), 120 + 1 x 8 + 1 (streaming, TVL1_ROLL_SEG=8)
CORNERS = [(125, 41), (249, 45), (57, 25), (121, 9)]
CORNER_KNOBS = ["", "TVL1_TB4=0", "TVL1_BUF_LIMIT=0", "TVL1_ROLL_LONG_MIN=0,TVL1_ROLL_SEG=8",
                "TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8", "TVL1_ROLL_PX4_MIN=0,TVL1_ROLL_SEG=8"]

# frames narrower or shorter than every halo
DEGENERATE = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (3, 3), (4, 5), (5, 4), (1, 64), (64, 1),
              (1, 130), (130, 1), (2, 65)]
# the kernels the tiny frames and the pyramids run under
WIDE_KNOBS = ["", "TVL1_FUSE_MIN=0", "TVL1_ROLL_LONG_MIN=0", "TVL1_BUF_LIMIT=0", "TVL1_TB4=0"]

# pyramids whose coarse levels sit on an edge, so the upsample kernel sees one:
# (W, H, nscales, the level sizes it must give)
PYRAMIDS = [(20, 20, 2, [(20, 20), (16, 16)]),      # 16 x 16: the smallest level the pyramid allows
            (155, 25, 2, [(155, 25), (124, 20)]),
            (81, 21, 2, [(81, 21), (65, 17)]),
            (100, 25, 3, [(100, 25), (80, 20), (64, 16)])]   # one ring band / k_warp_img tile exactly

# group -> the knob sets (TVL1_* settings, comma separated) its kernels are reached with
KNOBS_OF = {**{g: v[3] for g, v in X_GROUPS.items()}, **{g: v[3] for g, v in Y_GROUPS.items()},
            "corner": CORNER_KNOBS, "degenerate": WIDE_KNOBS, "pyramid": WIDE_KNOBS}

# Seeds.  A case's frames are synth.gen_pair(W, H, seed); the default seed is 131 W + H.  Where
# a stopping-rule case of that seed has a check closer than MIN_MARGIN to a threshold of the
# schedule (tests/test_edge_cases_cpu.py, IEEE or fma arithmetic), the size takes another seed
# here: the margin is a condition on the inputs, and no case is dropped to meet it.
SEED_OF_SIZE = {(249, 45): 40583}   # at 131 W + H = 32664 a check sits 2.1e-5 from a threshold


def seed_of(W, H):
    return SEED_OF_SIZE.get((W, H), 131 * W + H)


def x_widths(B):
    return [B - 1, B, B + 1, 2 * B, 2 * B + 1]


def _cases():
    out = []

    def add(group, W, H, psets, nscales=1):
        for pname, p in psets.items():
            out.append(Case(f"{group}-{W}x{H}-{pname}", W, H, seed_of(W, H), dict(p, nscales=nscales), group))

    for g, (B, psets, _, _) in X_GROUPS.items():
        for W in x_widths(B):
            add(g, W, X_H, psets)
    for g, (hs, psets, _, _) in Y_GROUPS.items():
        for H in hs:
            add(g, Y_W, H, psets)
    for W, H in CORNERS:
        add("corner", W, H, {**PLAIN, **GAMMA})
    for W, H in DEGENERATE:
        add("degenerate", W, H, PLAIN)
    for W, H, ns, _ in PYRAMIDS:
        add("pyramid", W, H, PLAIN, nscales=ns)
    return out


CASES = _cases()
GROUPS = list(KNOBS_OF)


def cases_of(group):
    return [c for c in CASES if c.group == group]


def frames(case):
    return synth.gen_pair(case.W, case.H, seed=case.seed)


# ---------------------------------------------------------------- batches
# tvl1_calc_batch, n = 3 pairs of different seeds per size (seed, seed + 1, seed + 2), all with
# TVL1_BATCH_SMALL=0 so that the streaming kernels and not kb_small_level solve the level.
BATCH_N = 3
# x edges: period -> probes.  kb_iterate_roll<K,1> has 64 - 2K px (default: every level of
# these sizes is under the TVL1_BATCH_PX1_W cut-off), <K,2> (TVL1_BATCH_PX1_W=0) 124 / 120,
# kb_warp_iter 124 (default), kb_warp_ring 64 (TVL1_BATCH_FUSE=0; fixed work gathers with it
# under every knob set)
BATCH_X = {56: [("site", "kb_roll", 4, 1)], 58: [("site", "kb_roll", 3, 1)], 60: [("site", "kb_roll", 2, 1)],
           62: [("site", "kb_roll", 1, 1)], 64: [("site", "kb_warp_ring", 6, 0)],
           120: [("site", "kb_roll", 3, 2), ("site", "kb_roll", 4, 2)],
           124: [("site", "kb_roll", 1, 2), ("site", "kb_roll", 2, 2), ("site", "kb_warp_iter", 8, 0)]}
# y edges around TVL1_BATCH_SEG_MIN=8 at W = 65 (two bands of every 1-px-per-lane pass)
BATCH_Y = [7, 8, 9, 15, 16, 17]
BATCH_Y_PROBES = [("site", "kb_roll", k, px) for px in (1, 2) for k in (1, 2, 3, 4)] + \
                 [("site", "kb_warp_iter", 8, 0), ("site", "kb_warp_ring", 6, 0)]
BATCH_KNOBS = ["TVL1_BATCH_SMALL=0", "TVL1_BATCH_SMALL=0,TVL1_BATCH_PX1_W=0",
               "TVL1_BATCH_SMALL=0,TVL1_BATCH_FUSE=0", "TVL1_BATCH_SMALL=0,TVL1_BATCH_SEG_MIN=8"]
# one batch of an identical pair, a textured pair and a constant pair, at edge sizes: the pairs
# of one launch stop at different passes
BATCH_MIXED = [(125, 9), (65, 17)]


def _batch_cases():
    out = []

    def add(group, W, H, psets):
        for pname, p in psets.items():
            out.append(Case(f"{group}-{W}x{H}-{pname}", W, H, seed_of(W, H), dict(p, nscales=1), group))

    for W in sorted({w for B in BATCH_X for w in x_widths(B)}):
        add("batch-x", W, X_H, PLAIN)
    for H in BATCH_Y:
        add("batch-y", Y_W, H, PLAIN)
    for W, H in DEGENERATE:
        add("batch-degenerate", W, H, PLAIN)
    for W, H in BATCH_MIXED:
        add("batch-mixed", W, H, {"stop": STOP})
    return out


BATCH_CASES = _batch_cases()
BATCH_GROUPS = ["batch-x", "batch-y", "batch-degenerate", "batch-mixed"]


def batch_cases_of(group):
    return [c for c in BATCH_CASES if c.group == group]


def batch_frames(case):
    """(I0s, I1s) of a batch case, (3, H, W) u8 each."""
    if case.group == "batch-mixed":
        t0, t1 = synth.gen_pair(case.W, case.H, seed=case.seed)
        i0, _ = synth.gen_pair(case.W, case.H, seed=case.seed + 1)
        c0 = np.full((case.H, case.W), 100, np.uint8)
        c1 = np.full((case.H, case.W), 140, np.uint8)
        return np.stack([i0, t0, c0]), np.stack([i0.copy(), t1, c1])
    prs = [synth.gen_pair(case.W, case.H, seed=case.seed + b) for b in range(BATCH_N)]
    return np.stack([a for a, _ in prs]), np.stack([b for _, b in prs])


# ---------------------------------------------------------------- the schedule
def sched_after(prev, thr, n, iters, kmax, eps_pos):
    """tvl1_plan.hpp's sched_after, restated: (k, calc_end, prev_end) of the pass that follows
    iteration count n.  test_edge_cases_cpu.py holds it to the C++ one."""
    k, ce = 0, False
    while k < kmax and n + k < iters:
        calc = bool(eps_pos) and bool((n + k) & 1) and prev < thr
        k += 1
        if calc:
            ce = True
            break
        prev -= thr
    return k, ce, prev


def fixed_work_passes(iterations, kmax):
    """Pass lengths of one warp with epsilon = 0 (no check ever ends a pass)."""
    out, n = [], 0
    while n < iterations:
        k, _, _ = sched_after(0.0, 0.0, n, iterations, kmax, 0)
        out.append(k)
        n += k
    return out


def kmax_of(params):
    """Iterations per pass the single-pair solve allows: 1 on the exact-division path (tau /
    theta < 0), else kRollMax = kTbMax = 4."""
    return 1 if params.get("tau", 0.25) / params.get("theta", 0.3) < 0 else 4
