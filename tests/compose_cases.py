"""One table of flow-composition cases, shared by the CPU census (test_compose_cpu.py) and the
GPU comparison (test_gpu_compose.py).

A case is a size, a layout and a kind of flow; planes(case) builds its (n, H, W) float32 planes
ua, va, ub, vb, deterministic from the case alone.  Sizes are W x H: a single px, a single row
and column, three rows of exactly one 256-px tile row and of one lane more, sizes that are no
multiple of the lane's 4 px or the tile, more than one block both ways; a pitched ROI view that
starts 1 float off a 16-byte boundary (every row takes the float-by-float path); 257 pairs, so
a second chunk of pairs runs; and one case composed in place on a.
"""
from dataclasses import dataclass

import numpy as np

F = np.float32

SIZES = [(1, 1), (7, 1), (1, 5), (256, 3), (259, 3), (67, 45), (257, 131)]
KINDS = ["integer", "edges", "edges_out", "special", "smooth", "far"]
ROI = (130, 70, 160, 80, 5 * 160 + 5)   # W, H, allocation W, H, first float: 4 * 805 = 4 mod 16
BATCH = (130, 20, 257)                  # W, H, pairs
INPLACE = (67, 45)

SPECIALS = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0]


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    kind: str
    n: int = 1
    roi: tuple = None   # (allocation W, allocation H, first float) or None: dense planes
    inplace: bool = False


def _cases():
    out = [Case(f"{W}x{H}-{kind}", W, H, kind) for W, H in SIZES for kind in KINDS]
    W, H, AW, AH, first = ROI
    for kind in ("smooth", "special", "edges", "edges_out"):
        out.append(Case(f"roi{W}x{H}-{kind}", W, H, kind, roi=(AW, AH, first)))
    W, H, n = BATCH
    out.append(Case(f"batch{n}x{W}x{H}-smooth", W, H, "smooth", n=n))
    W, H = INPLACE
    out.append(Case(f"inplace{W}x{H}-smooth", W, H, "smooth", inplace=True))
    return out


def _smooth(rng, W, H, amp):
    """A smooth field of the given amplitude: three plane waves of random direction and phase."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(3):
        kx, ky = rng.uniform(-0.15, 0.15, 2)
        f += np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
    return (f * (amp / 3.0)).astype(F)


def integer_flows(case):
    """(a, b) of the `integer` kind: two constant integer flows."""
    return ((2, -1), (-3, 2)) if (case.W + case.H) % 2 else ((-1, 1), (2, -3))


def _planes_one(case, rng):
    W, H, kind = case.W, case.H, case.kind
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    k = ys * W + xs
    if kind == "integer":
        # c = a + b exactly wherever the px lands inside (and everywhere: b is constant)
        (ax, ay), (bx, by) = integer_flows(case)
        full = lambda c: np.full((H, W), c, F)
        return full(ax), full(ay), full(bx), full(by)
    if kind in ("edges", "edges_out"):
        # px by px: land on X = 0, X = W - 1, Y = 0, Y = H - 1 (inside, the last tap clamped); or
        # aim one ulp beyond (clamped to the same point, and counted)
        out = kind == "edges_out"
        ua, va = np.zeros((H, W), F), np.zeros((H, W), F)
        tx0, tx1, ty0, ty1 = -xf, F(W - 1) - xf, -yf, F(H - 1) - yf
        if out:
            # the near side: X = -ulp(x), the smallest step below 0 that x + ua can take; the far
            # side: X = the float above W - 1 (the difference and the sum are both exact)
            tx0, ty0 = np.nextafter(tx0, F(-np.inf)), np.nextafter(ty0, F(-np.inf))
            tx1 = np.nextafter(F(W - 1), F(np.inf)) - xf
            ty1 = np.nextafter(F(H - 1), F(np.inf)) - yf
        m = k % 4
        ua[m == 0], ua[m == 1] = tx0[m == 0], tx1[m == 1]
        va[m == 2], va[m == 3] = ty0[m == 2], ty1[m == 3]
        # the other component: a fractional flow that stays inside where it can
        frac = F(0.25)
        ua[(m >= 2) & (xs + 1 < W)] = frac
        va[(m < 2) & (ys + 1 < H)] = frac
        return ua, va, _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
    if kind == "special":
        pl = [_smooth(rng, W, H, 1.5) for _ in range(4)]
        i = 0
        for p in range(4):
            for sv in SPECIALS:
                pos = (7 * i + 3) % (W * H)
                pl[p].flat[pos] = F(sv)
                i += 1
        return tuple(pl)
    if kind == "smooth":
        return tuple(_smooth(rng, W, H, 3.0) for _ in range(4))
    if kind == "far":
        # a leaves the frame everywhere, by x or by y, on either side, and by fractions
        ua, va = _smooth(rng, W, H, 0.4), _smooth(rng, W, H, 0.4)
        m = k % 4
        ua = np.where(m == 0, F(W) + F(1.5) + ua, np.where(m == 1, -(xf + F(1.25)) + ua, ua))
        va = np.where(m == 2, F(H) + F(2.5) + va, np.where(m == 3, -(yf + F(1.75)) + va, va))
        return ua.astype(F), va.astype(F), _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
    raise ValueError(kind)


def planes(case):
    """ua, va, ub, vb as (n, H, W) float32 arrays."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(case.name))
    rng = np.random.default_rng(seed)
    per = [_planes_one(case, rng) for _ in range(case.n)]
    return tuple(np.stack([p[j] for p in per]).astype(F) for j in range(4))


CASES = _cases()
IDS = [c.name for c in CASES]

# The chain experiment: five 192 x 160 frames, frame k the base rolled by k (-3, 5) (rows,
# columns) plus N(0, 2) noise, so a stride-1 pair moves by (5, -3) px and the pair (0, 4) by
# (20, -12); solved with nscales 3, warps 3.
CHAIN_W, CHAIN_H, CHAIN_FRAMES = 192, 160, 5
CHAIN_STEP = (5.0, -3.0)       # true flow (dx, dy) of a stride-1 pair
CHAIN_PARAMS = dict(nscales=3, warps=3)
CHAIN_MARGIN = 24              # EPE is averaged over px at least this far from the frame edge
CHAIN_RNG = 5                  # the noise's seed


def chain_frames(rng_seed=CHAIN_RNG, w=CHAIN_W, h=CHAIN_H):
    from optflow_amd import synth
    base = synth.gen_pair(w, h, seed=31)[0].astype(np.float64)
    rng = np.random.default_rng(rng_seed)
    out = []
    for k in range(CHAIN_FRAMES):
        f = np.roll(base, (k * -3, k * 5), axis=(0, 1)) + rng.normal(0.0, 2.0, base.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out


def chain_epe(u, v, links=CHAIN_FRAMES - 1):
    """Mean EPE against the true flow of a pair `links` frames apart, away from the frame edge."""
    m = CHAIN_MARGIN
    du = u.astype(np.float64) - links * CHAIN_STEP[0]
    dv = v.astype(np.float64) - links * CHAIN_STEP[1]
    return float(np.sqrt(du * du + dv * dv)[m:-m, m:-m].mean())
