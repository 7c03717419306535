"""TEST INFRASTRUCTURE: the one table of profile-1 solves (tvl1_params.profile = 1, OpenCV's CPU
DualTVL1OpticalFlow schedule) that sit on the geometry edges of the kernels only that profile
runs, in the manner of tests/edge_cases.py.

  k_iterate<G, EXACT, CPUP = true>   248-px wave segments, 32-row strips; four instantiations
                                     (gamma, tau / theta < 0), one residual read per iteration
  k_resize_hp                        copy, bilinear (x clamped, last column a single tap) and the
                                     exact-2x area branch, whose destination rounds up over an odd
                                     source (35 -> 18: the last column has one source column)
  k_gradient, k_remap_cubic          64 x 4 launch blocks; the remap's interior, partial and
                                     fully-outside branches (W - 3, H - 3 clamped at 0)
  k_median                           3 x 3 and 5 x 5 windows clamped to the frame

tests/test_dualtvl1_edges_cpu.py asks the planner (tests/plan_dump.cpp) whether every size still
sits on the edge it names, holds every stopping-rule case to the project's residual margin, counts
the remap's branches and shows that the oracle's flow is sensitive to a one-px slip of frame1;
tests/test_gpu_dualtvl1_edges.py runs the table on the GPU, bitwise against the oracle.

Every case is cheap: each iteration is a launch plus a host read, so warps <= 3,
inner_iterations <= 5 and outer_iterations <= 2 throughout.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from optflow_amd import capi, synth

# shift: None (frames are synth.gen_pair(W, H, seed)), or the (dx, dy) px by which frame1 is
# frame0's texture translated (remap group)
Case = namedtuple("Case", "name W H seed params group shift", defaults=(None,))

# ---------------------------------------------------------------- parameter sets
# Stopping rule: error > scaledEps, read after every iteration; fixed work: epsilon = 0, every
# warp runs outer x inner iterations.
STOP = dict(warps=2, inner_iterations=5, outer_iterations=2)
FIX = dict(warps=2, inner_iterations=3, outer_iterations=2, epsilon=0.0)
# the four instantiations of k_iterate<G, EXACT, true>
INST = {"plain": {}, "gamma": dict(gamma=0.2), "tau": dict(tau=-0.05), "tau-gamma": dict(tau=-0.05, gamma=0.2)}
# With epsilon = 0.01 no textured pair of these sizes gets under scaledEps within the ten
# iterations of a warp (the ratio is still above 40 then), so the residual the kernels sum would
# decide nothing: `stop10` (epsilon = 0.1, scaledEps 100 times larger) ends the warps after 4 to 7
# iterations, on the value of that sum.
STOP10 = dict(STOP, epsilon=0.1)
ITERATE = {f"{k}-{m}": dict(b, **v) for k, v in INST.items()
           for m, b in (("stop", STOP), ("stop10", STOP10), ("fix", FIX))}

# ---------------------------------------------------------------- iterate-x / iterate-y
X_B, X_H = 248, 9       # k_iterate's wave segment (kSegPx); W in {B-1, B, B+1, 2B, 2B+1} at H = 9
Y_B, Y_W = 32, 65       # its strip; H in {B-1, B, B+1} at W = 65 (a one-px second launch block)
BLOCK = (64, 4)         # kBlk2, the launch block of k_gradient / k_remap_cubic / k_median / k_resize_hp
X_WIDTHS = [X_B - 1, X_B, X_B + 1, 2 * X_B, 2 * X_B + 1]
Y_HEIGHTS = [Y_B - 1, Y_B, Y_B + 1]

# ---------------------------------------------------------------- degenerate
# W - 3 <= 0 or H - 3 <= 0: imax(W - 3, 0) = 0 sends every px of the remap through the partial
# branch; the median's clamps cover the whole window.  (4, 5), (5, 4): (W - 3)(H - 3) = 2 tap
# origins are interior, every other one partial, within one wavefront.
DEGENERATE = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 3), (3, 1), (4, 5), (5, 4), (1, 64), (64, 1), (2, 65)]
MEDIANS = (1, 3, 5)
DEGENERATE_P = dict(warps=3, inner_iterations=5, outer_iterations=2)

# ---------------------------------------------------------------- pyramid
# (W, H, scale_step, nscales, extra parameters, the level sizes the planner must give, note).
# 0.5: `up` lists per step which sides round up ("w", "h"), i.e. where the 2x path's last column
# or row has a single source column or row; the others are the in-range neighbours.
PYRAMIDS = [
    (35, 36, 0.5, 3, {}, [(35, 36), (18, 18)], dict(up=[{"w"}])),
    (36, 35, 0.5, 3, {}, [(36, 35), (18, 18)], dict(up=[{"h"}])),
    (35, 35, 0.5, 3, {}, [(35, 35), (18, 18)], dict(up=[{"w", "h"}])),
    (39, 67, 0.5, 3, {}, [(39, 67), (20, 34)], dict(up=[{"w", "h"}])),
    (70, 70, 0.5, 4, {}, [(70, 70), (35, 35), (18, 18)], dict(up=[set(), {"w", "h"}])),   # odd at the second step
    (33, 37, 0.5, 3, {}, [(33, 37), (16, 18)], dict(up=[set()])),          # both sides round down
    (128, 96, 0.5, 4, {}, [(128, 96), (64, 48), (32, 24)], dict(up=[set(), set()])),   # the all-even control
    # 0.98: equal sizes -> k_resize_hp's copy branch; width alone changing -> one axis at ratio 1
    (20, 20, 0.98, 3, {}, [(20, 20)] * 3, dict(equal=True)),
    (50, 20, 0.98, 3, {}, [(50, 20), (49, 20), (48, 20)], dict(equal_h=True)),
    (20, 50, 0.98, 3, {}, [(20, 50), (20, 49), (20, 48)], dict(equal_w=True)),   # and the other axis
    # 0.75, 0.9: the upsample's last column is a single tap; widths straddle the 64-px block.
    # (81, 17) is a single level at both steps (17 px scale to under the 16-px floor): it pins
    # that, and (81, 21) beside it has the levels.
    (65, 21, 0.75, 3, {}, [(65, 21), (49, 16)], dict(single_tap=True, straddle=True)),
    (81, 17, 0.75, 3, {}, [(81, 17)], {}),
    (81, 21, 0.75, 3, {}, [(81, 21), (61, 16)], dict(single_tap=True, straddle=True)),
    (65, 21, 0.9, 3, {}, [(65, 21), (58, 19), (52, 17)], dict(single_tap=True, straddle=True)),
    (81, 17, 0.9, 3, {}, [(81, 17)], {}),
    (81, 21, 0.9, 3, {}, [(81, 21), (73, 19), (66, 17)], dict(single_tap=True)),
    # 0.8, the default
    (155, 25, 0.8, 3, {}, [(155, 25), (124, 20), (99, 16)], {}),
    (100, 25, 0.8, 3, dict(gamma=0.2), [(100, 25), (80, 20), (64, 16)], {}),    # u3 resized unscaled
    (100, 25, 0.8, 3, dict(median_filtering=5), [(100, 25), (80, 20), (64, 16)], {}),
]
ODD_HALF = [(w, h) for w, h, step, _, _, _, note in PYRAMIDS if step == 0.5 and any(note["up"])]

# ---------------------------------------------------------------- remap
# Profile 1 takes no seed, so the frames make the flows: frame1 is frame0's texture translated
# by `shift` px (an integer crop of one larger synth.base_texture), far enough that after a warp
# the flow points out of the frame along an edge.  scale_step 0.5 and a large lambda let ten
# iterations per warp follow a 6-px shift (1.5 px at the coarsest level).
REMAP_SHIFTS = [(6, 0), (-6, 0), (0, 6), (0, -6), (7, -5)]
REMAP_SIZE = (64, 48)
REMAP_P = dict(warps=3, inner_iterations=5, outer_iterations=2, nscales=3, scale_step=0.5, lambda_=1.0)
REMAP_TINY = (12, 10, (6, 0), dict(warps=3, inner_iterations=5, outer_iterations=2, nscales=1, lambda_=1.0))
REMAP_MARGIN = 8   # px of texture around the crop


# Seeds.  The default is 131 W + H; where a stopping-rule case of that seed has a check within
# MIN_MARGIN of the threshold (tests/test_dualtvl1_edges_cpu.py) the size takes another here:
# the margin is a condition on the inputs, and no case is dropped to meet it.
SEED_OF_SIZE = {}


def seed_of(W, H):
    return SEED_OF_SIZE.get((W, H), 131 * W + H)


PYRAMID_OF = {}   # case name -> its PYRAMIDS row


def _cases():
    out = []
    for W in X_WIDTHS:
        for pname, p in ITERATE.items():
            out.append(Case(f"iterate-x-{W}x{X_H}-{pname}", W, X_H, seed_of(W, X_H), dict(p, nscales=1), "iterate-x"))
    for H in Y_HEIGHTS:
        for pname, p in ITERATE.items():
            out.append(Case(f"iterate-y-{Y_W}x{H}-{pname}", Y_W, H, seed_of(Y_W, H), dict(p, nscales=1), "iterate-y"))
    for W, H in DEGENERATE:
        for m in MEDIANS:
            out.append(Case(f"degenerate-{W}x{H}-median{m}", W, H, seed_of(W, H),
                            dict(DEGENERATE_P, nscales=1, median_filtering=m), "degenerate"))
    for row in PYRAMIDS:
        W, H, step, ns, extra = row[:5]
        tag = "".join(f"-{k}" for k in extra)
        sets = (("stop", STOP), ("fix", FIX)) if (W, H) in ODD_HALF else (("stop", STOP),)
        for m, b in sets:
            out.append(Case(f"pyramid-{W}x{H}-step{step}{tag}-{m}", W, H, seed_of(W, H),
                            dict(b, nscales=ns, scale_step=step, **extra), "pyramid"))
            PYRAMID_OF[out[-1].name] = row
    W, H = REMAP_SIZE
    for dx, dy in REMAP_SHIFTS:
        out.append(Case(f"remap-{W}x{H}-shift{dx},{dy}", W, H, seed_of(W, H), dict(REMAP_P), "remap", (dx, dy)))
    W, H, sh, p = REMAP_TINY
    out.append(Case(f"remap-{W}x{H}-shift{sh[0]},{sh[1]}", W, H, seed_of(W, H), dict(p), "remap", sh))
    return out


CASES = _cases()
GROUPS = ["iterate-x", "iterate-y", "degenerate", "pyramid", "remap"]


def cases_of(group):
    return [c for c in CASES if c.group == group]


def case(name):
    return next(c for c in CASES if c.name == name)


def pyramid_row(c):
    """The PYRAMIDS row a pyramid case was made from."""
    return PYRAMID_OF[c.name]


def is_odd_half(c):
    return c.group == "pyramid" and c.params["scale_step"] == 0.5 and (c.W, c.H) in ODD_HALF


def stops(c):
    return c.params.get("epsilon", 0.01) > 0


def params_of(c):
    return capi.make_params(profile=1, **c.params)


def frames(c):
    if c.shift is None:
        return synth.gen_pair(c.W, c.H, seed=c.seed)
    dx, dy = c.shift
    m = REMAP_MARGIN
    assert abs(dx) <= m and abs(dy) <= m
    tex = np.clip(np.rint(synth.base_texture(c.W + 2 * m, c.H + 2 * m, seed=c.seed)), 0, 255).astype(np.uint8)
    I0 = tex[m:m + c.H, m:m + c.W]
    I1 = tex[m - dy:m - dy + c.H, m - dx:m - dx + c.W]   # I1(x + d) = I0(x): the flow is (dx, dy)
    return np.ascontiguousarray(I0), np.ascontiguousarray(I1)
