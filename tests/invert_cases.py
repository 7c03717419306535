"""One table of flow-inversion cases, shared by the CPU census (test_invert_cpu.py) and the GPU
comparison (test_gpu_invert.py).

A case is a size, a layout, a kind of flow and an iteration count K; planes(case) builds its
(n, H, W) float32 planes uf, vf, deterministic from the case alone.  Sizes are W x H, those of
compose_cases.py: a single px, a single row and column, three rows of exactly one 256-px tile row
and of one lane more, sizes that are no multiple of the lane's 4 px or the tile, more than one
block both ways; a pitched ROI view that starts 1 float off a 16-byte boundary (every row takes
the float-by-float path), at all four K; 257 pairs, so a second chunk of pairs runs.

The window-edge cases are derived from the constants that csrc/tvl1_invert.hpp exports (parsed
here, as warp_window.py parses the warp gathers'), and window_model() restates the kernel's box
rule so that the census can show on which side of each edge a case lies.
"""
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import invert_ref as ref

F = np.float32

_HPP = Path(__file__).resolve().parent.parent / "fibsem-optflow_amd" / "csrc" / "tvl1_invert.hpp"
CONST = {m.group(1): int(m.group(2))
         for m in re.finditer(r"constexpr int (kInv\w+) = (\d+);", _HPP.read_text())}
TILE_W, TILE_H = CONST["kInvTileW"], CONST["kInvTileH"]
DRIFT, WIN_FLOATS, MAX_ITER = CONST["kInvDrift"], CONST["kInvWinFloats"], CONST["kInvMaxIter"]

SIZES = [(1, 1), (7, 1), (1, 5), (256, 3), (259, 3), (67, 45), (257, 131)]
KINDS = ["zero", "integer", "smooth", "chain", "edges", "edges_out", "special", "fold"]
KS = [1, 2, 8, 32]
ROI = (130, 70, 160, 80, 5 * 160 + 5)   # W, H, allocation W, H, first float: 4 * 805 = 4 mod 16
BATCH = (130, 20, 257)                  # W, H, pairs
TOL = 0.01

SPECIALS = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0]


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    kind: str
    K: int
    n: int = 1
    roi: tuple = None   # (allocation W, allocation H, first float) or None: dense planes
    tol: float = TOL


# ---- the window-edge cases: geometry from the header's constants ----
def _fit_size():
    """W, box rows: the widest W <= one tile that divides the window's floats into 12..200 rows,
    so that a box of W columns and that many rows holds exactly kInvWinFloats floats."""
    for W in range(TILE_W, 15, -1):
        if WIN_FLOATS % W == 0 and 12 <= WIN_FLOATS // W <= 200:
            return W, WIN_FLOATS // W
    raise AssertionError("no size fits kInvWinFloats exactly")


FIT_W, FIT_ROWS = _fit_size()
HOP = 20                 # px the probe px of the drift cases lands away, along y
HOP_X = TILE_W + 44      # ... along x: into another tile column
DRIFT_Y = (64, 64)       # W, H of the drift cases along y
DRIFT_X = (TILE_W + 344, 8)
PROBE = (10, 1)          # the probe px (x, y) of the far-side cases
PROBE_NEAR = (10, 41)    # ... of the near-side case along y

WINDOW_KINDS = ["box_fit", "box_over", "drift_y_at", "drift_y_over", "drift_yneg_at", "drift_yneg_over",
                "drift_x_at", "drift_x_over"]


def _cases():
    out = []
    i = 0
    for W, H in SIZES:
        for kind in KINDS:
            out.append(Case(f"{W}x{H}-{kind}-k{KS[i % 4]}", W, H, kind, KS[i % 4]))
            i += 1   # 8 kinds a size and one more step a size: every kind meets every K
        i += 1
    W, H, AW, AH, first = ROI
    for K in KS:
        for kind in ("smooth", "chain"):
            out.append(Case(f"roi{W}x{H}-{kind}-k{K}", W, H, kind, K, roi=(AW, AH, first)))
    for kind, K in (("special", 2), ("edges", 1), ("edges_out", 8), ("fold", 32)):
        out.append(Case(f"roi{W}x{H}-{kind}-k{K}", W, H, kind, K, roi=(AW, AH, first)))
    W, H, n = BATCH
    out.append(Case(f"batch{n}x{W}x{H}-smooth-k2", W, H, "smooth", 2, n=n))
    out.append(Case(f"{FIT_W}x{FIT_ROWS + 8}-box_fit-k2", FIT_W, FIT_ROWS + 8, "box_fit", 2))
    out.append(Case(f"{FIT_W}x{FIT_ROWS + 8}-box_over-k2", FIT_W, FIT_ROWS + 8, "box_over", 2))
    for kind in WINDOW_KINDS[2:]:
        W, H = DRIFT_X if "_x_" in kind else DRIFT_Y
        out.append(Case(f"{W}x{H}-{kind}-k2", W, H, kind, 2))
    return out


def _smooth(rng, W, H, amp, kmax=0.15):
    """A smooth field of the given amplitude: three plane waves of random direction and phase
    (compose_cases._smooth's recipe, restated; kmax is its 0.15 rad/px)."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(3):
        kx, ky = rng.uniform(-kmax, kmax, 2)
        f += np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
    return (f * (amp / 3.0)).astype(F)


def integer_flow(case):
    """(dx, dy) of the `integer` kind."""
    return (2, -1) if (case.W + case.H) % 2 else (-3, 2)


def drift_probe(kind):
    """The probe px (x, y), where it first lands and where the next iteration takes it."""
    over = kind.endswith("_over")
    s = DRIFT + (1 if over else 0)
    if kind.startswith("drift_yneg"):
        (x, y) = PROBE_NEAR
        return (x, y), (x, y - HOP), (x, y - HOP - s)
    (x, y) = PROBE
    if kind.startswith("drift_y"):
        return (x, y), (x, y + HOP), (x, y + HOP + s)
    return (x, y), (x + HOP_X, y), (x + HOP_X + s, y)


def _planes_one(case, rng):
    W, H, kind = case.W, case.H, case.kind
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    k = ys * W + xs
    full = lambda c: np.full((H, W), c, F)
    if kind == "zero":
        return full(0), full(0)
    if kind == "integer":
        dx, dy = integer_flow(case)
        return full(dx), full(dy)
    if kind == "smooth":
        return _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
    if kind == "chain":
        # the chain-seed regime: 25 px one way, a smooth 2 px on top
        return (F(25) + _smooth(rng, W, H, 2.0)).astype(F), (F(-18) + _smooth(rng, W, H, 2.0)).astype(F)
    if kind == "fold":
        # 8 px at twice the smooth kind's wavenumbers: gradients above 1, so px of A overtake each
        # other and g = -f(y + g) has no attracting fixed point there
        return _smooth(rng, W, H, 8.0, 0.3), _smooth(rng, W, H, 8.0, 0.3)
    if kind in ("edges", "edges_out"):
        # px by px, the first landing x + g0 = x - uf: on X = 0, X = W - 1, Y = 0, Y = H - 1 (inside,
        # the last tap clamped); or one ulp beyond (clamped to the same point).  The planes between
        # are what the later iterations read.
        out = kind == "edges_out"
        gu, gv = _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
        tx0, tx1, ty0, ty1 = -xf, F(W - 1) - xf, -yf, F(H - 1) - yf
        if out:
            tx0, ty0 = np.nextafter(tx0, F(-np.inf)), np.nextafter(ty0, F(-np.inf))
            tx1 = np.nextafter(F(W - 1), F(np.inf)) - xf
            ty1 = np.nextafter(F(H - 1), F(np.inf)) - yf
        m = k % 8
        gu[m < 4], gv[m < 4] = 0, 0
        gu[m == 0], gu[m == 1] = tx0[m == 0], tx1[m == 1]
        gv[m == 2], gv[m == 3] = ty0[m == 2], ty1[m == 3]
        frac = F(0.25)
        gv[(m < 2) & (ys + 1 < H)] = frac
        gu[(m >= 2) & (m < 4) & (xs + 1 < W)] = frac
        return -gu, -gv
    if kind == "special":
        pl = [_smooth(rng, W, H, 1.5) for _ in range(2)]
        i = 0
        for p in range(2):
            for sv in SPECIALS:
                pl[p].flat[(7 * i + 3) % (W * H)] = F(sv)
                i += 1
        return tuple(pl)
    if kind in ("box_fit", "box_over"):
        # the first tile's rows land on rows 0 and L: its box is W x (L + DRIFT + 2) floats
        L = FIT_ROWS - DRIFT - 2 + (1 if kind == "box_over" else 0)
        u, v = _smooth(rng, W, H, 0.45), full(0)
        v[TILE_H - 1, :] = F(-(L - (TILE_H - 1)))
        return u, v
    if kind.startswith("drift_"):
        # a background below half a px, and a probe px that lands exactly on a px whose flow takes
        # the probe's next landing DRIFT (or DRIFT + 1) px further: integer landings, so the samples
        # at them are the px's own values
        u, v = _smooth(rng, W, H, 0.45), _smooth(rng, W, H, 0.45)
        (px, py), (qx, qy), (rx, ry) = drift_probe(kind)
        u[py, px], v[py, px] = F(px - qx), F(py - qy)
        u[qy, qx], v[qy, qx] = F(px - rx), F(py - ry)
        return u, v
    raise ValueError(kind)


def planes(case):
    """uf, vf as (n, H, W) float32 arrays."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(case.name))
    rng = np.random.default_rng(seed)
    per = [_planes_one(case, rng) for _ in range(case.n)]
    return tuple(np.stack([p[j] for p in per]).astype(F) for j in range(2))


def window_model(uf, vf, K, tx=0, ty=0):
    """The window arm's box rule restated for the block of tile column tx and row step ty of a
    dense plane: {"floats": the box's floats, "on": whether it is staged, "box": (bx0, bx1, by0,
    by1), "in_box": (K + 1, rows, cols) bool, whether all taps of that px's sample k lie in it}."""
    H, W = uf.shape
    xs = slice(tx * TILE_W, min((tx + 1) * TILE_W, W))
    ysl = slice(ty * TILE_H, min((ty + 1) * TILE_H, H))
    g, _ = ref.iterates(uf, vf, K)
    taps = []
    for gu, gv in g:
        _, _, _, X, Y = ref.step(uf, vf, gu, gv)
        with np.errstate(invalid="ignore"):
            Xc = np.where(X >= 0, np.where(X <= W - 1, X, W - 1), 0)
            Yc = np.where(Y >= 0, np.where(Y <= H - 1, Y, H - 1), 0)
        x0, y0 = np.floor(Xc).astype(np.int64)[ysl, xs], np.floor(Yc).astype(np.int64)[ysl, xs]
        taps.append((x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1)))
    x0, _, y0, _ = taps[0]
    bx0, bx1 = max(int(x0.min()) - DRIFT, 0), min(int(x0.max()) + DRIFT + 1, W - 1)
    by0, by1 = max(int(y0.min()) - DRIFT, 0), min(int(y0.max()) + DRIFT + 1, H - 1)
    floats = (bx1 - bx0 + 1) * (by1 - by0 + 1)
    in_box = np.stack([(a >= bx0) & (b <= bx1) & (c >= by0) & (d <= by1) for a, b, c, d in taps])
    return dict(floats=floats, on=floats <= WIN_FLOATS, box=(bx0, bx1, by0, by1), in_box=in_box,
                taps=taps, origin=(xs.start, ysl.start))


CASES = _cases()
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)

# ---- the zoom stack of "why negation is not enough"  ----
# Five 192 x 160 frames: frame k is a base texture zoomed about the centre by 1 + 0.02 k and
# shifted by k (5, -3) px (bilinear resampling of the base), plus N(0, 2) noise; solved with
# nscales 3, warps 3.  A point b of the base lies in frame k at c + (1 + 0.02 k)(b - c) + k s.
ZOOM_W, ZOOM_H, ZOOM_FRAMES = 192, 160, 5
ZOOM_RATE = 0.02
ZOOM_STEP = (5.0, -3.0)
ZOOM_PARAMS = dict(nscales=3, warps=3)
ZOOM_MARGIN = 24     # EPE is averaged over px at least this far from the frame edge
# The noise's seed.  Of seeds 1..12 it is the one whose five solves (four links, the backward pair
# from the inverse) keep their stopping decisions furthest from the thresholds: a smallest
# check_margins of 5.4e-4 (seed 5 gave 2.5e-5 on a link, below MIN_MARGIN).
ZOOM_RNG = 3


def _bilinear(img, X, Y):
    H, W = img.shape
    X, Y = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
    x0, y0 = np.minimum(np.floor(X).astype(int), W - 2), np.minimum(np.floor(Y).astype(int), H - 2)
    ax, ay = X - x0, Y - y0
    t = img[y0, x0] * (1 - ax) + img[y0, x0 + 1] * ax
    b = img[y0 + 1, x0] * (1 - ax) + img[y0 + 1, x0 + 1] * ax
    return t * (1 - ay) + b * ay


def zoom_frames(rng_seed=ZOOM_RNG):
    from optflow_amd import synth
    P = 64   # the base is larger than a frame, so that every frame px has texture under it
    base = synth.gen_pair(ZOOM_W + 2 * P, ZOOM_H + 2 * P, seed=31)[0].astype(np.float64)
    rng = np.random.default_rng(rng_seed)
    ys, xs = np.mgrid[0:ZOOM_H, 0:ZOOM_W].astype(np.float64)
    cx, cy = (ZOOM_W - 1) / 2.0, (ZOOM_H - 1) / 2.0
    out = []
    for k in range(ZOOM_FRAMES):
        z = 1.0 + ZOOM_RATE * k
        bx = cx + (xs - cx - k * ZOOM_STEP[0]) / z
        by = cy + (ys - cy - k * ZOOM_STEP[1]) / z
        f = _bilinear(base, bx + P, by + P) + rng.normal(0.0, 2.0, bx.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out


def zoom_true_flow(k, j):
    """The true flow (u, v) of the pair (frame k -> frame j), float64, on frame k's grid."""
    ys, xs = np.mgrid[0:ZOOM_H, 0:ZOOM_W].astype(np.float64)
    cx, cy = (ZOOM_W - 1) / 2.0, (ZOOM_H - 1) / 2.0
    zk, zj = 1.0 + ZOOM_RATE * k, 1.0 + ZOOM_RATE * j
    bx = cx + (xs - cx - k * ZOOM_STEP[0]) / zk
    by = cy + (ys - cy - k * ZOOM_STEP[1]) / zk
    return (cx + zj * (bx - cx) + j * ZOOM_STEP[0] - xs, cy + zj * (by - cy) + j * ZOOM_STEP[1] - ys)


def zoom_epe(u, v, k, j):
    """Mean EPE against the true flow of (k -> j), away from the frame edge."""
    tu, tv = zoom_true_flow(k, j)
    m = ZOOM_MARGIN
    du, dv = u.astype(np.float64) - tu, v.astype(np.float64) - tv
    return float(np.sqrt(du * du + dv * dv)[m:-m, m:-m].mean())
