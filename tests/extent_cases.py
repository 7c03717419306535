"""TEST INFRASTRUCTURE: the one table of frame sizes at the far end of what include/tvl1.h
accepts -- frames taller than the utility kernels' row-group cap, so that their row walk takes
a second step; frames taller than 4 x 65535 rows in every other 2-D launch, which puts rows / 4
straight into the grid; and sizes exactly on the stated arithmetic bounds (2^19 px for the
1/32-px map, a 32767-px canvas, 65535 pairs).

Every size is derived from a constant that is parsed from the source here, and
tests/test_extent_cases_cpu.py holds the table to them and shows on the CPU that each case's
reference alone has content where it matters: in the rows y >= ROWS_CAP (the second row step)
and just below them.  tests/test_gpu_extents.py runs the table on the GPU, bitwise against the
project's references.

Thin frames keep all of it cheap: a 5 x 262149 float plane is 5 MB.
"""
from __future__ import annotations

import re
from collections import namedtuple
from pathlib import Path

import numpy as np

import invert_ref

F = np.float32
_CSRC = Path(__file__).resolve().parent.parent / "fibsem-optflow_amd" / "csrc"


def _const(header, name):
    m = re.search(rf"constexpr int {name} = (\d+);", (_CSRC / header).read_text())
    assert m, f"{name} not found in {header}"
    return int(m.group(1))


def _limit_bits(name):
    m = re.search(rf"constexpr SizeLimit {name} = \{{(\d+),", (_CSRC / "tvl1_planes.hpp").read_text())
    assert m, f"{name} not found in tvl1_planes.hpp"
    return int(m.group(1))


def _engine(pattern):
    m = re.search(pattern, (_CSRC / "tvl1_engine.hip").read_text())
    assert m, f"{pattern} not found in tvl1_engine.hip"
    return int(m.group(1))


# ---------------------------------------------------------------- constants of the source
FB_MAX_ROW_GROUPS = _const("tvl1_fbcheck.hpp", "kFbMaxRowGroups")   # k_fb_score, k_zero_above, k_compose_flow,
ZN_MAX_ROW_GROUPS = _const("tvl1_score.hpp", "kZnMaxRowGroups")     # k_invert_flow; k_warp_flow_u8
LANE_PX = _const("tvl1_fbcheck.hpp", "kFbPx")                       # px of a row per lane
GROUP_ROWS = _const("tvl1_invert.hpp", "kInvTileH")                 # rows of a row group: one per wavefront
INV_DRIFT = _const("tvl1_invert.hpp", "kInvDrift")
INV_WIN_FLOATS = _const("tvl1_invert.hpp", "kInvWinFloats")
MAP32_BITS = _limit_bits("kMap32Limit")                             # tvl1_zncc_score, tvl1_warp_by_flow_u8
FLOATX_BITS = _limit_bits("kFloatXLimit")                           # the other flow utilities
CANVAS_MAX = _engine(r"2 \* \(int64_t\)border > (\d+) \|\|")        # tvl1_remap_flow_u8
POST_BATCH_MAX = _engine(r"if \(n > (\d+)\) return set_err\(c, TVL1_EINVAL, \"at most \d+ pairs per call\"\)")
SHIFT_AREA_BITS = _engine(r"\(int64_t\)w \* h > \(\(int64_t\)1 << (\d+)\)")   # tvl1_estimate_shift

# ---------------------------------------------------------------- sizes
ROWS_CAP = GROUP_ROWS * min(FB_MAX_ROW_GROUPS, ZN_MAX_ROW_GROUPS)   # 262140: rows of the first row step
# A second step of 9 rows: row groups 0 and 1 full, group 2 one row (three of its wavefronts have
# nothing to do while the block still meets at the barriers); above 4 x 65536 too, so over the
# limit whichever of 65535 / 65536 blocks a runtime would apply.
H_TALL = ROWS_CAP + 9
# At scale_step 0.8 level 1 of 20 x H_PYR is 16 x 262148: over the cap as well; 16 px is the
# narrowest level the pyramid allows.
H_PYR = 327685
PYR_LEVELS = [(20, H_PYR), (16, 262148)]
W_THIN = LANE_PX + 1         # one full float4 lane and a 1-px tail
W_PYR = 20
W_BLEND = 8                  # tvl1_blend6_u8
HALF_SRC = (8, 2 * (ROWS_CAP + 8))     # tvl1_half_u8: a 4 x 262148 destination
SHIFT_SIZE = (20, 2 * (ROWS_CAP + 8))  # tvl1_estimate_shift, max_shift 5: one level of 262148 rows in k_shift_half
SHIFT_R, SHIFT_TRUE = 5, (2, -3)
# A view: a pitch that is no multiple of 16 bytes and a first element 4 bytes past a 16-byte
# boundary, so every row of a float plane takes the float-by-float arm of fb_load4 / fb_store4 /
# zn_store4.  (allocation W, allocation H, first element)
VIEW = (W_THIN + 2, H_TALL + 2, (W_THIN + 2) + 2)

SPECIAL_ROWS = dict(nan=ROWS_CAP + GROUP_ROWS + 1,      # row group 1 of the second step
                    pinf=ROWS_CAP + 2 * GROUP_ROWS,     # row group 2: its only row
                    ninf=ROWS_CAP + 2)                  # row group 0
HOP = 20                      # px the probe px of the inversion lands away (invert_cases.HOP)
PROBE = (1, ROWS_CAP + 1)     # the probe px (x, y): row group 0 of the second step


def second_step(plane):
    """The rows of a (.., H, W) plane that only the second trip through a row walk writes."""
    return plane[..., ROWS_CAP:, :]


# ---------------------------------------------------------------- A. row-walk inputs
def _smooth(rng, W, H, amp, kmax=0.15):
    """Three plane waves of random direction and phase (fbcheck_cases._smooth's recipe)."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(3):
        kx, ky = rng.uniform(-kmax, kmax, 2)
        f += np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
    return (f * (amp / 3.0)).astype(F)


def tall_flow(seed, W=W_THIN, H=H_TALL, specials=True):
    """A forward flow (u, v) of W x H with its content around ROWS_CAP and at the far edges:
    rows just below the cap land above it and rows above it land below (so both steps read the
    other's rows), px that land exactly on the last row and column (inside, the far tap clamped)
    and px that land beyond them (outside, clamped), a NaN, a +inf and a -inf in the second
    step, and the inversion's probe px (a landing HOP rows up whose next landing leaves the
    window by more than its drift)."""
    rng = np.random.default_rng(seed)
    u, v = _smooth(rng, W, H, 0.8), _smooth(rng, W, H, 2.0)
    C = ROWS_CAP
    v[C - 8:C, :] = F(6.5)            # cross the cap upwards: land in the second step
    v[C:C + 4, :] = F(-6.5)           # and downwards: the second step reads the first's rows
    v[C - 14:C - 10, 0::2] = F(-3.75)
    ys = np.arange(H, dtype=F)
    # the last row and column: exactly on them, and beyond
    v[H - 3, :] = F(H - 1) - ys[H - 3]
    v[H - 1, 0::2] = F(5)             # Y > H - 1: outside, clamped to the last row
    u[C + 5, :] = F(W - 1) - np.arange(W, dtype=F)
    u[C + 6, :] = F(3)                # X > W - 1 for x >= 2
    u[C - 2, :] = F(-2.5)             # X < 0 for x < 3, below the cap
    if specials:
        u[SPECIAL_ROWS["pinf"], 0] = F(np.inf)
        u[SPECIAL_ROWS["ninf"], W - 1] = F(-np.inf)
        v[SPECIAL_ROWS["nan"], 2] = F(np.nan)
    # the inversion's probe: g0 = -f lands exactly HOP rows up, on a px whose flow takes the next
    # landing INV_DRIFT + 2 rows further up: out of the window's box
    px, py = PROBE
    qy, ry = py - HOP, py - HOP - (INV_DRIFT + 2)
    u[py, px], v[py, px] = F(0), F(py - qy)
    u[qy, px], v[qy, px] = F(0), F(py - ry)
    return u, v


def tall_backward(seed, uf, vf):
    """A backward flow for tvl1_fb_score and the second operand of tvl1_compose_flow: about the
    forward flow's opposite, perturbed by up to 0.6 px, and by 2 px in every other row group of
    the second step so that scores fall on both sides of beta there."""
    rng = np.random.default_rng(seed + 1)
    H, W = uf.shape
    with np.errstate(invalid="ignore"):
        ub = np.where(np.isfinite(uf), -uf, F(0.5)).astype(F) + _smooth(rng, W, H, 0.6)
        vb = np.where(np.isfinite(vf), -vf, F(0.25)).astype(F) + _smooth(rng, W, H, 0.6)
    C = ROWS_CAP
    # the rows the crossing px land on carry the opposite of those px's flow, so that they are
    # consistent: rows C .. C + 3 (v = -6.5) land on rows C - 7 .. C - 3
    vb[C - 8:C - 2, :] = F(6.5) + vb[C - 8:C - 2, :] - np.where(np.isfinite(vf[C - 8:C - 2, :]), -vf[C - 8:C - 2, :], 0)
    vb[C:C + 7, :] = F(-6.5) + _smooth(rng, W, 7, 0.3)
    ub[C + GROUP_ROWS:C + 2 * GROUP_ROWS, :] += F(2)
    ub[C - 3, :] += F(2)
    vb[C + 3, 1] = F(np.inf)
    ub[C + 7, 3] = F(np.nan)
    return ub.astype(F), vb.astype(F)


ALPHA, BETA = 0.01, 0.5          # tvl1_fb_score / tvl1_zero_above
INV_K, INV_TOL = 4, 0.01         # tvl1_invert_flow
WalkCase = namedtuple("WalkCase", "name n roi")
WALK_CASES = [WalkCase("dense-n1", 1, None), WalkCase("dense-n2", 2, None),
              WalkCase("view-n1", 1, VIEW), WalkCase("view-n2", 2, VIEW)]
WALK_SEEDS = [262149, 262150]    # pair b of every row-walk case

_cache: dict = {}


def _once(key, make):
    if key not in _cache:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def walk_planes(b):
    """uf, vf, ub, vb of pair b (0 or 1), (H_TALL, W_THIN) float32 each; computed once."""
    def make():
        uf, vf = tall_flow(WALK_SEEDS[b])
        return (uf, vf) + tall_backward(WALK_SEEDS[b], uf, vf)
    return _once(("walk", b), make)


def walk_frame(b):
    """The u8 frame tvl1_warp_by_flow_u8 warps by pair b's forward flow: texture that changes
    from row to row and px to px, so a tap of the wrong row shows."""
    def make():
        rng = np.random.default_rng(WALK_SEEDS[b] + 7)
        return rng.integers(0, 256, (H_TALL, W_THIN), dtype=np.uint8)
    return _once(("frame", b), make)


def invert_window_census(b, group, K=None):
    """The window arm's box rule (invert_cases.window_model, restated for one row group of the
    second step of pair b's one-tile-wide plane): {"on", "floats", "in_box": (K + 1, rows, W)
    bool, whether all taps of that px's sample k lie in the box}."""
    K = INV_K if K is None else K
    uf, vf = walk_planes(b)[:2]
    H, W = uf.shape
    ysl = slice(ROWS_CAP + group * GROUP_ROWS, min(ROWS_CAP + (group + 1) * GROUP_ROWS, H))
    g = _once(("iterates", b, K), lambda: tuple(invert_ref.iterates(uf, vf, K)[0]))
    taps = []
    for gu, gv in g:
        with np.errstate(all="ignore"):
            X = np.arange(W, dtype=F)[None, :] + gu[ysl]
            Y = np.arange(H, dtype=F)[ysl, None] + gv[ysl]
            Xc = np.where(X >= 0, np.where(X <= W - 1, X, W - 1), 0)
            Yc = np.where(Y >= 0, np.where(Y <= H - 1, Y, H - 1), 0)
        x0, y0 = np.floor(Xc).astype(np.int64), np.floor(Yc).astype(np.int64)
        taps.append((x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1)))
    x0, _, y0, _ = taps[0]
    bx0, bx1 = max(int(x0.min()) - INV_DRIFT, 0), min(int(x0.max()) + INV_DRIFT + 1, W - 1)
    by0, by1 = max(int(y0.min()) - INV_DRIFT, 0), min(int(y0.max()) + INV_DRIFT + 1, H - 1)
    floats = (bx1 - bx0 + 1) * (by1 - by0 + 1)
    in_box = np.stack([(a >= bx0) & (b <= bx1) & (c >= by0) & (d <= by1) for a, b, c, d in taps])
    return dict(on=floats <= INV_WIN_FLOATS, floats=floats, in_box=in_box)


# ---------------------------------------------------------------- B. at the arithmetic bounds
MAP32_MAX = 1 << MAP32_BITS      # 2^19: the largest w and h of the 1/32-px map
ZnCase = namedtuple("ZnCase", "name W H")
ZNCC_CASES = [ZnCase("wide", MAP32_MAX, 3), ZnCase("tall", 3, MAP32_MAX)]
ZNCC_RADII = [1, 4]
MAP32_TOP = (1 << (MAP32_BITS + 5)) - 32   # rint(32 mx) of a px that lands on the last column: 2^24 - 32


def zncc_planes(case):
    """I0, I1 (u8), u, v (f32) of a bound case: sub-pixel flows everywhere; over the last 64 px
    of the long axis px that land exactly on the far edge (32 mx = MAP32_TOP), 1/32 px before
    it, and beyond it (outside)."""
    def make():
        W, H = case.W, case.H
        rng = np.random.default_rng(W * 7 + H)
        I1 = rng.integers(0, 256, (H, W), dtype=np.uint8)
        I0 = np.clip(I1.astype(np.int32) + rng.integers(-9, 10, (H, W)), 0, 255).astype(np.uint8)
        u = (rng.integers(-40, 41, (H, W)) / 32.0).astype(F)
        v = (rng.integers(-40, 41, (H, W)) / 32.0).astype(F)
        far = np.arange(64)
        if W > H:
            xs = W - 64 + far
            u[1, xs[0::3]] = (F(W - 1) - xs[0::3].astype(F)).astype(F)
            u[1, xs[1::3]] = (F(W - 1) - xs[1::3].astype(F) - F(1 / 32)).astype(F)
            u[2, xs[0::2]] = (F(W) - xs[0::2].astype(F)).astype(F)          # one px beyond
            v[1, xs] = F(0.5)
        else:
            ys = H - 64 + far
            v[ys[0::3], 1] = (F(H - 1) - ys[0::3].astype(F)).astype(F)
            v[ys[1::3], 1] = (F(H - 1) - ys[1::3].astype(F) - F(1 / 32)).astype(F)
            v[ys[0::2], 2] = (F(H) - ys[0::2].astype(F)).astype(F)
            u[ys, 1] = F(0.5)
        return I0, I1, u, v
    return _once(("zncc", case.name), make)


REMAP_BORDER = 5
RemapCase = namedtuple("RemapCase", "name W H")   # the frame; the canvas is W + 2 border x H + 2 border
REMAP_CASES = [RemapCase("wide", CANVAS_MAX - 2 * REMAP_BORDER, 13 - 2 * REMAP_BORDER),
               RemapCase("tall", 13 - 2 * REMAP_BORDER, CANVAS_MAX - 2 * REMAP_BORDER)]


def remap_planes(case):
    """frame (u8), u, v (f32, the frame's size): small sub-pixel flows, and at both ends of the
    long axis flows that push the map past the frame and past the range of a short."""
    def make():
        W, H = case.W, case.H
        rng = np.random.default_rng(W * 3 + H)
        frame = rng.integers(1, 256, (H, W), dtype=np.uint8)
        u = (rng.integers(-48, 49, (H, W)) / 32.0).astype(F)
        v = (rng.integers(-48, 49, (H, W)) / 32.0).astype(F)
        long_ = u if W > H else v          # map = X - U: negative flows push it past the far end
        ax = 1 if W > H else 0
        n = long_.shape[ax]
        near, far = [slice(None)] * 2, [slice(None)] * 2
        near[ax], far[ax] = slice(0, 8), slice(n - 8, n)
        long_[tuple(near)] = np.array([3, 40000, 70000, 0.5, 1e9, 33000, 6, 2 ** 31], F).reshape(
            (1, 8) if ax else (8, 1))
        long_[tuple(far)] = np.array([-3, -40000, -70000, -0.5, -1e9, -6, -9.75, -2 ** 31], F).reshape(
            (1, 8) if ax else (8, 1))
        return frame, u, v
    return _once(("remap", case.name), make)


def post_batch_planes():
    """u, v (n, 1, 1) f32 and I1 (n, 1, 1) u8 of n = POST_BATCH_MAX pairs of 1 x 1; about one
    pair in four is masked (I1 <= 1)."""
    def make():
        n = POST_BATCH_MAX
        rng = np.random.default_rng(n)
        u = rng.uniform(-4, 4, (n, 1, 1)).astype(F)
        v = rng.uniform(-4, 4, (n, 1, 1)).astype(F)
        I1 = rng.integers(0, 8, (n, 1, 1), dtype=np.uint8)
        return u, v, I1
    return _once("post_batch", make)


def postprocess_numpy(u, v, I1, mode):
    """tvl1_postprocess on (.., H, W) planes, one float32 rounding per operation: mode 1 adds the
    px grid, mode 2 adds and subtracts it again, then the flow is zeroed where I1 <= 1."""
    u, v = np.array(u, F), np.array(v, F)
    H, W = u.shape[-2:]
    xs = np.arange(W, dtype=F)
    ys = np.arange(H, dtype=F)[:, None]
    if mode >= 1:
        u, v = (u + xs).astype(F), (v + ys).astype(F)
    if mode == 2:
        u, v = (u - xs).astype(F), (v - ys).astype(F)
    mask = np.asarray(I1) <= 1
    u[mask], v[mask] = 0, 0
    return u, v


# ---------------------------------------------------------------- C. rows over the cap in every 2-D launch
# Solve cases: name -> (W, H, seed, parameters).  Frames are solve_frames(case).  `stop` and
# `stop-t` are the stopping-rule cases (their seeds keep MIN_MARGIN at every check, IEEE and fma,
# and `stop` has a warp that ends by a check before its cap: tests/test_extent_cases_cpu.py).
SolveCase = namedtuple("SolveCase", "name W H seed params")
FIX = dict(nscales=2, warps=2, epsilon=0.0, iterations=7)
# epsilon 0.06: at 0.01 every warp of a synthetic pair of this size runs to its cap; here the four
# warps end after 6, 2, 18 and 8 iterations, each by a check
STOP = dict(nscales=2, warps=2, iterations=20, epsilon=0.06)
SOLVE_CASES = {c.name: c for c in [
    SolveCase("fix", W_PYR, H_PYR, 11, FIX),
    SolveCase("stop", W_PYR, H_PYR, 12, STOP),
    SolveCase("median", W_PYR, H_PYR, 13, dict(FIX, median_filtering=5, gamma=0.2)),
    SolveCase("f32", W_PYR, H_TALL, 14, dict(FIX, nscales=1)),
    SolveCase("init", W_PYR, H_PYR, 15, FIX),
    SolveCase("batch", W_PYR, H_PYR, 16, FIX),
    SolveCase("const", W_PYR, H_PYR, 17, FIX),
    SolveCase("profile1", W_PYR, H_PYR, 18, dict(nscales=2, warps=1, outer_iterations=2, inner_iterations=3,
                                                 median_filtering=5, profile=1, epsilon=0.0)),
    SolveCase("wide", H_PYR, W_PYR, 19, FIX),
]}
STOPPING = ["stop"]
BATCH_N = 2
CONST_SEEDS = np.array([[1.0, -2.0], [-0.5, 1.5]], F)   # (dx, dy) per pair of the `const` case


def solve_frames(case, b=0):
    """The case's pair b: a smooth drift of under a px on a texture, so the stopping rule has
    warps that converge early; deterministic from the case's seed."""
    from optflow_amd import synth
    return _once(("solve", case.name, b), lambda: tuple(synth.gen_pair(case.W, case.H, seed=case.seed + 100 * b)))


def solve_seed(case, b=0):
    """A non-constant initial flow for the `init` case: smooth, up to 1.5 px."""
    def make():
        rng = np.random.default_rng(case.seed + 1000 + b)
        return _smooth(rng, case.W, case.H, 1.5, 0.05), _smooth(rng, case.W, case.H, 1.5, 0.05)
    return _once(("seed", case.name, b), make)


# Stand-alone calls
# One non-identity affine: a 2 % squeeze and a shear in x, a shift of 1.5 rows, and a y scale one
# float above 1 that drifts the source row by a quarter px over the frame's height
AFFINE = np.array([[0.98, 0.0, 0.3], [0.01, 1.000001, -1.5]], F)


def post_planes(b=0):
    """u, v (f32), I1 (u8) of tvl1_postprocess at W_THIN x H_TALL; about one px in four masked."""
    def make():
        rng = np.random.default_rng(4242 + b)
        u = rng.uniform(-3, 3, (H_TALL, W_THIN)).astype(F)
        v = rng.uniform(-3, 3, (H_TALL, W_THIN)).astype(F)
        return u, v, rng.integers(0, 8, (H_TALL, W_THIN), dtype=np.uint8)
    return _once(("post", b), make)


def blend_frames():
    """Six u8 frames of W_BLEND x H_TALL."""
    return _once("blend", lambda: np.random.default_rng(6).integers(0, 256, (6, H_TALL, W_BLEND), dtype=np.uint8))


def half_frame():
    return _once("half", lambda: np.random.default_rng(8).integers(0, 256, HALF_SRC[::-1], dtype=np.uint8))


def shift_pair(b=0):
    import shift_ref
    return _once(("shift", b), lambda: shift_ref.window_pair(SHIFT_SIZE[0], SHIFT_SIZE[1], SHIFT_TRUE[0],
                                                             SHIFT_TRUE[1], rng=40 + b))
