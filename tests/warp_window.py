"""TEST INFRASTRUCTURE: the one table of seeded flows that sit on the edges of the warp
gathers' LDS windows -- tests/edge_cases.py pins the kernels' geometry in frame size, this
table pins it in flow.

Every warpBackward kernel decides per pixel, from the flow at that pixel, whether its 4 x 4
cubic taps (columns fx-1 .. fx+2, rows fy-1 .. fy+2; fx = floor(x + u1), fy = floor(y + u2))
come from an LDS window or through the global-memory fallback ("same taps, same order").  A
predicate one column or row too generous reads a stale ring slot or a neighbouring plane; a
window row that enters the ring one step late, or a wrong slot in the ring's wrap, shows only
where fy sits on the last resident row.  With nscales = 1 tvl1_calc_init hands the seed to the
first warp unchanged, so a test chooses the flow of every pixel.

GEOMETRY mirrors each kernel's window once (tests/test_warp_window_cpu.py reads the margins
back out of csrc/tvl1_kernels.hpp and the band starts out of the planner, so a changed margin
fails there until this table follows):
  ring   k_warp_ring<6,2> / kb_warp_ring (warp_ring_step): 64-px bands, 64 + 2 * 5 columns
         from band start - 5, rows y - 6 .. y + 6 of the pixel's own row y
  iter   k_warp_iter<6,.,128,.> / kb_warp_iter (wi_prod_step): 124-px bands, 128 + 2 * 5
         columns from band start - 2 - 5, rows y - 6 .. y + 6
  img    k_warp_img: 64 x 16 tiles, 76 x 28 window from tile - 6: the rows are the tile's
  small  kb_small_level: the whole level in LDS, every tap clamped; no window

SEEDS (float32, deterministic, built so that float(x) + u1 / float(y) + u2 land where intended;
every census is taken from the float32 sums themselves):
  x      fx cycles by row over the first and the last admissible column of the pixel's window,
         one and two columns inside and one and two outside; the fraction cycles over an exact
         integer, 1 ulp above it, one half and 1 ulp below the next integer (every other one of
         those 1 ulp of the FLOW below, so that the sum rounds up to the integer); u2 = 0.25
  y      the same for fy against the row window, cycling by column; u1 = 0.25
  xy     both at once (where both coordinates would be integers, or clamp, one takes the half:
         _both_axes says why)
  ulp    coordinates at and just below 64, 128, the band starts and the tile / segment rows, in
         (-1, 0) and just above W - 1 / H - 1, each in the four fraction classes (the two 1-ulp
         classes twice per cycle); even rows take the nearest such column (short flows, inside
         the windows), odd rows one by turns, and the row coordinate likewise by column
  beyond flows that leave the frame by up to W + 8 / H + 8 px to the left, right, top and
         bottom (with the other axis staying, leaving low or leaving high by turns): every tap
         of the leaving axis clamps
No NaN, no infinity, nothing beyond +-2^20.

ROWS: per kernel the frame (synth.gen_pair, textured), the knob set that reaches it, the
parameter sets and the seeds; tests/test_gpu_warp_window.py runs them bitwise against
checker.oracle_calc(init=...) in IEEE and fma.  All with nscales = 1.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from optflow_amd import capi, synth
from oracle import checker

# ---------------------------------------------------------------- geometry
# period: band / tile width; x_first: first window column relative to the band start; width:
# window columns; rows: "pixel" (row_first .. row_last relative to the pixel's row) or "tile"
# (relative to the tile's first row, tiles of tile_h rows)
Geom = namedtuple("Geom", "period x_first width rows row_first row_last tile_h")
GEOMETRY = {
    "ring": Geom(64, -5, 74, "pixel", -6, 6, 0),
    "iter": Geom(124, -7, 138, "pixel", -6, 6, 0),
    "img": Geom(64, -6, 76, "tile", -6, 21, 16),
}
SEG = 8   # TVL1_ROLL_SEG of the streaming rows: segments of 8 rows


def band_start(g, x):
    return x // g.period * g.period


def row_origin(g, y):
    return y if g.rows == "pixel" else y // g.tile_h * g.tile_h


def fx_range(g, x):
    """(first, last) tap floor fx whose four columns fx-1 .. fx+2 are inside the window."""
    lo = band_start(g, x) + g.x_first
    return lo + 1, lo + g.width - 1 - 2


def fy_range(g, y):
    lo = row_origin(g, y)
    return lo + g.row_first + 1, lo + g.row_last - 2


def in_window(g, x, y, fx, fy):
    """The kernel's predicate, mirrored: do the taps of (fx, fy) come from the LDS window?"""
    x0, x1 = fx_range(g, x)
    y0, y1 = fy_range(g, y)
    return (fx >= x0) & (fx <= x1) & (fy >= y0) & (fy <= y1)


# ---------------------------------------------------------------- seeds
KINDS = ("x", "y", "xy", "ulp", "beyond")
F32 = np.float32
_INF = F32(np.inf)


def coords(u, v):
    """The float32 sums the kernels form: (wx, wy, fx, fy) of every pixel."""
    h, w = u.shape
    ys, xs = np.mgrid[0:h, 0:w]
    wx = xs.astype(F32) + u
    wy = ys.astype(F32) + v
    assert wx.dtype == F32 and wy.dtype == F32
    return wx, wy, np.floor(wx).astype(np.int64), np.floor(wy).astype(np.int64)


def frac_class(w):
    """0: an integer, 1: 1 ulp above one, 2: one half, 3: 1 ulp below the next, -1: other."""
    fl = np.floor(w)
    out = np.full(w.shape, -1, np.int64)
    out[w == np.nextafter(fl + F32(1), -_INF)] = 3
    out[w - fl == F32(0.5)] = 2
    out[w == np.nextafter(fl, _INF)] = 1
    out[w == fl] = 0
    return out


def _flow_to(T, cls, by_flow, pos):
    """The float32 flow that takes integer position pos to tap floor T in fraction class cls.
    by_flow (class 3 only): 1 ulp of the flow below T + 1 - pos instead of 1 ulp of the
    coordinate below T + 1 -- where the flow's ulp is the finer one the sum rounds up to T + 1."""
    T = T.astype(np.float64)
    Tf = T.astype(F32)
    target = np.select([cls == 0, cls == 1, cls == 2],
                       [T, np.nextafter(Tf, _INF).astype(np.float64), T + 0.5],
                       np.nextafter(Tf + F32(1), -_INF).astype(np.float64))
    u = (target - pos).astype(F32)
    alt = np.nextafter((T + 1.0 - pos).astype(F32), -_INF)
    return np.where((cls == 3) & by_flow, alt, u).astype(F32)


def _edge_targets(first, last, k):
    """k in 0..9 -> the tap floor: first + (-2 .. 2), then last + (-2 .. 2)."""
    return np.where(k < 5, first + (k - 2), last + (k - 7))


def _plan_x(g, xs, ys):
    """(tap floor, fraction class, by_flow) of the x case at every pixel."""
    first, last = fx_range(g, xs)
    return _edge_targets(first, last, ys % 10), (xs + ys // 10) % 4, (xs // 4 + ys) % 2 == 1


def _plan_y(g, xs, ys):
    first, last = fy_range(g, ys)
    return _edge_targets(first, last, xs % 10), (ys + xs // 10) % 4, (ys // 4 + xs) % 2 == 1


def _clamped(T, n):
    """All four taps T-1 .. T+2 of an axis of n px clamp onto one border pixel."""
    return (T + 2 <= 0) | (T - 1 >= n - 1)


def _both_axes(px, py, xs, ys, w, h):
    """The flows of a seed that pins both axes.  Along an axis whose coordinate is an integer
    (or 1 ulp from one), or whose taps all clamp, the gather returns one pixel's value: where
    that holds for both axes the sample is the u8 image's own centred gradient at one pixel,
    which equals its neighbour's at 0.2 % of the pixels of these frames -- more than the 0.1 %
    the sensitivity condition allows, and many pixels of a band share such a point.  Each axis
    is covered at those coordinates by its own case (x, y) with the other axis at 0.25; where
    both meet here, one axis (by turns; never one whose taps clamp) takes the class one half."""
    (Tx, cx, bx), (Ty, cy, by) = px, py
    clx, cly = _clamped(Tx, w), _clamped(Ty, h)
    both = (clx | (cx != 2)) & (cly | (cy != 2))
    y_yields = both & ~cly & (clx | ((xs // 2 + ys // 2) % 2 == 0))
    cx = np.where(both & ~y_yields & ~clx, 2, cx)
    cy = np.where(y_yields, 2, cy)
    return _flow_to(Tx, cx, bx, xs), _flow_to(Ty, cy, by, ys)


def ulp_targets(g, n, rows):
    """Integers T whose [T, T + 1) holds the ulp case's coordinates along an axis of n px:
    at and just below 64, 128 and the band starts (columns) or the tile and segment rows,
    (-1, 0), and just above n - 1."""
    if rows:
        starts = set(range(0, n, SEG)) | (set(range(0, n, g.tile_h)) if g.tile_h else set())
    else:
        starts = set(range(0, n, g.period)) | {64, 128}
    ts = {-1, n - 1}
    for s in starts:
        if 0 < s < n:
            ts |= {s - 1, s}
    return np.array(sorted(ts), np.int64)


_ULP_CYCLE = np.array([0, 1, 2, 3, 1, 3])


def _plan_ulp(ts, pos, other, shift):
    near = ts[np.abs(ts[None, None, :] - pos[..., None]).argmin(-1)]
    turn = ts[(other // 2 + pos) % len(ts)]
    T = np.where(other % 2 == 0, near, turn)
    # the two 1-ulp classes twice per cycle: they are what this case is for, and many of
    # their sums round onto the integer
    return T, _ULP_CYCLE[(pos + other // shift) % 6], (pos // 4 + other) % 2 == 1


def _axis_beyond(n, pos, mode, salt):
    """mode 0: stay (0.25 px); 1: leave low, coordinate in [-(4 + m), -(3 + m)]; 2: leave high,
    in [n + 1 + m, n + 2 + m]; m in 0 .. n + 4 and the fraction one of the four classes, so
    the frame is left by 3 .. n + 8 px and the four tap columns (rows) all clamp."""
    m = (7 * pos + 13 * salt) % (n + 5)
    cls = (pos + salt) % 4
    low = _flow_to(-(4 + m), cls, np.zeros(pos.shape, bool), pos)
    high = _flow_to(n + 1 + m, cls, np.zeros(pos.shape, bool), pos)
    return np.select([mode == 1, mode == 2], [low, high], F32(0.25)).astype(F32)


_seed_cache = {}


def make_seed(geom, kind, w, h):
    """(u1, u2) float32 of one seed kind against one kernel's window geometry."""
    key = (geom, kind, w, h)
    if key in _seed_cache:
        return _seed_cache[key]
    g = GEOMETRY[geom]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    q = np.full((h, w), 0.25, F32)
    if kind == "x":
        u, v = _flow_to(*_plan_x(g, xs, ys), xs), q
    elif kind == "y":
        u, v = q, _flow_to(*_plan_y(g, xs, ys), ys)
    elif kind == "xy":
        u, v = _both_axes(_plan_x(g, xs, ys), _plan_y(g, xs, ys), xs, ys, w, h)
    elif kind == "ulp":
        u, v = _both_axes(_plan_ulp(ulp_targets(g, w, False), xs, ys, 1),
                          _plan_ulp(ulp_targets(g, h, True), ys, xs, 4), xs, ys, w, h)
    elif kind == "beyond":
        d = (xs // 2 + ys) % 4                  # the leaving axis and its direction
        o = (ys // 3 + xs) % 3                  # what the other axis does
        u = _axis_beyond(w, xs, np.select([d == 0, d == 1], [1, 2], o), ys)
        v = _axis_beyond(h, ys, np.select([d == 2, d == 3], [1, 2], o), xs)
    else:
        raise KeyError(kind)
    for a in (u, v):
        assert a.dtype == F32 and a.shape == (h, w)
        assert np.isfinite(a).all() and np.abs(a).max() < 2.0 ** 20
        a.setflags(write=False)
    _seed_cache[key] = (u, v)
    return u, v


# ---------------------------------------------------------------- parameters
# Fixed work (epsilon = 0): one warp of one iteration (the output is the gather's, one TH step
# on) and two warps of seven (passes of 4 and 3; the second warp gathers at the first's flow),
# each at lambda 0.05 (about 5 % of the px take TH's middle branch: the output carries I1wx and
# I1wy) and at 5 (about 90 %: rho's value reaches it too).  The fused kernels need epsilon > 0:
# the stopping rule with two warps of two iterations (each warp is one fused pass).
def _lambdas(name, p):
    return {f"{name}-l0.05": dict(p, lambda_=0.05), f"{name}-l5": dict(p, lambda_=5.0)}


FIXED = {**_lambdas("fix1", dict(nscales=1, warps=1, epsilon=0.0, iterations=1)),
         **_lambdas("fix7", dict(nscales=1, warps=2, epsilon=0.0, iterations=7))}
STOP = _lambdas("stop", dict(nscales=1, warps=2, iterations=2))

# ---------------------------------------------------------------- the rows
# name: the kernel; geom: whose window the seeds are built against; knobs: the TVL1_* settings
# that reach it; seeds: the kinds, one solve each -- or, batch, one pair each of a single
# tvl1_calc_batch_init (pair b's frames are gen_pair(W, H, seed + b))
Row = namedtuple("Row", "name geom W H knobs psets seeds batch")
BATCH_SEEDS = ("x", "xy", "beyond")
ROWS = [
    Row("k_warp_ring", "ring", 193, 41, "TVL1_ROLL_SEG=8", FIXED, KINDS, False),
    Row("k_warp_img", "img", 193, 41, "TVL1_BUF_LIMIT=0", FIXED, KINDS, False),
    Row("k_warp_iter", "iter", 249, 17, "TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8", STOP, KINDS, False),
    Row("k_warp_iter-nc1", "iter", 249, 17, "TVL1_FUSE_MIN=0,TVL1_ROLL_SEG=8,TVL1_WI_NC=1", STOP, KINDS, False),
    Row("kb_warp_iter", "iter", 249, 17, "TVL1_BATCH_SMALL=0", STOP, BATCH_SEEDS, True),
    Row("kb_warp_ring", "ring", 193, 41, "TVL1_BATCH_FUSE=0,TVL1_BATCH_SMALL=0", {**STOP, **FIXED}, BATCH_SEEDS,
        True),
    # no window: the seeds are the ring's (what matters is that every tap clamps correctly)
    Row("kb_small_level", "ring", 130, 12, "", {**STOP, **FIXED}, KINDS, True),
]
ROW_OF = {r.name: r for r in ROWS}

# Frames: synth.gen_pair(W, H, seed); the default seed is 131 W + H.  A stopping-rule case with
# a check closer than MIN_MARGIN to a threshold (tests/test_warp_window_cpu.py, IEEE or fma)
# gives its size another seed here, never another margin.
SEED_OF_SIZE = {}


def frame_seed(W, H):
    return SEED_OF_SIZE.get((W, H), 131 * W + H)


def frames(row, b=0):
    return synth.gen_pair(row.W, row.H, seed=frame_seed(row.W, row.H) + b)


def solves(row):
    """(seed kind, pair index) of every solve of a row; a batch row's pair b has frames of
    its own, the single-pair rows all solve pair 0's."""
    return [(kind, b if row.batch else 0) for b, kind in enumerate(row.seeds)]


_ref_cache = {}


def reference(row, pname, kind, b, math, roll=None):
    """checker.oracle_calc(init=seed) of one solve, computed once and shared (read-only): rows
    of one geometry and size share it.  roll = (dy, dx): I1 rolled, the sensitivity probe."""
    key = (row.geom, row.W, row.H, pname, kind, b, math, roll)
    if key not in _ref_cache:
        I0, I1 = frames(row, b)
        if roll:
            I1 = np.roll(I1, roll, axis=(0, 1))
        u, v, st, wi = checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **row.psets[pname]),
                                           init=make_seed(row.geom, kind, row.W, row.H))
        for a in (u, v, wi):
            a.setflags(write=False)
        _ref_cache[key] = (u, v, st, wi)
    return _ref_cache[key]
