"""One table of forward-backward score cases, shared by the CPU census (test_fbcheck_cpu.py)
and the GPU comparison (test_gpu_fbcheck.py).

A case is a size, a layout and a kind of flow; planes(case) builds its (n, H, W) float32 planes
uf, vf, ub, vb, deterministic from the case alone.  Sizes are W x H: a single px, a single row
and column, three rows wider than one 256-px tile row, sizes that are no multiple of the
lane's 4 px or the tile, more than one block both ways; a pitched ROI view that starts 1 float
off a 16-byte boundary (every row takes the float-by-float path); and 257 pairs, so a second
chunk of pairs runs.
"""
from dataclasses import dataclass

import numpy as np

F = np.float32

SIZES = [(1, 1), (1, 7), (5, 1), (3, 256), (67, 45), (257, 131)]
KINDS = ["integer", "edges", "edges_out", "special", "smooth", "tie"]
ROI = (130, 70, 160, 80, 5 * 160 + 5)   # W, H, allocation W, H, first float: 4 * 805 = 4 mod 16
BATCH = (130, 20, 257)                  # W, H, pairs

SPECIALS = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0]
TIE_BETA = F(0.25)
TIE_OVER = F(1.1 * 2.0 ** -13)   # 0.25 + TIE_OVER^2 rounds to the float above 0.25


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    kind: str
    alpha: float
    beta: float
    n: int = 1
    roi: tuple = None   # (allocation W, allocation H, first float) or None: dense planes


def _ab(kind):
    if kind in ("integer", "edges", "edges_out"):
        return 0.0, 0.5
    if kind == "tie":
        return 0.0, float(TIE_BETA)
    return 0.01, 0.5


def _cases():
    out = []
    for W, H in SIZES:
        for kind in KINDS:
            a, b = _ab(kind)
            out.append(Case(f"{W}x{H}-{kind}", W, H, kind, a, b))
    W, H, AW, AH, first = ROI
    for kind in ("smooth", "special", "edges", "tie"):
        a, b = _ab(kind)
        out.append(Case(f"roi{W}x{H}-{kind}", W, H, kind, a, b, roi=(AW, AH, first)))
    W, H, n = BATCH
    out.append(Case(f"batch{n}x{W}x{H}-smooth", W, H, "smooth", 0.01, 0.5, n=n))
    return out


def _smooth(rng, W, H, amp):
    """A smooth field of the given amplitude: three plane waves of random direction and phase."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(3):
        kx, ky = rng.uniform(-0.15, 0.15, 2)
        f += np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
    return (f * (amp / 3.0)).astype(F)


def _planes_one(case, rng):
    W, H, kind = case.W, case.H, case.kind
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    k = ys * W + xs
    if kind == "integer":
        # b = -f exactly, so the score is exactly 0 at alpha = 0 wherever the px lands inside
        dx, dy = (2, -1) if (W + H) % 2 else (-1, 1)
        uf, vf = np.full((H, W), dx, F), np.full((H, W), dy, F)
        return uf, vf, -uf, -vf
    if kind in ("edges", "edges_out"):
        # px by px: land on X = 0, X = W - 1, Y = 0, Y = H - 1 (inside, the last tap clamped); or
        # aim one ulp beyond
        out = kind == "edges_out"
        uf, vf = np.zeros((H, W), F), np.zeros((H, W), F)
        tx0, tx1, ty0, ty1 = -xf, F(W - 1) - xf, -yf, F(H - 1) - yf
        if out:
            tx0, ty0 = np.nextafter(tx0, F(-np.inf)), np.nextafter(ty0, F(-np.inf))
            tx1, ty1 = np.nextafter(tx1, F(np.inf)), np.nextafter(ty1, F(np.inf))
        m = k % 4
        uf[m == 0], uf[m == 1] = tx0[m == 0], tx1[m == 1]
        vf[m == 2], vf[m == 3] = ty0[m == 2], ty1[m == 3]
        # the other component: a fractional flow that stays inside where it can
        frac = F(0.25)
        uf[(m >= 2) & (xs + 1 < W)] = frac
        vf[(m < 2) & (ys + 1 < H)] = frac
        return uf, vf, _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
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
        uf, vf = _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
        # an independently perturbed backward flow: about the forward flow's opposite
        ub = -uf + _smooth(rng, W, H, 0.6)
        vb = -vf + _smooth(rng, W, H, 0.6)
        return uf, vf, ub.astype(F), vb.astype(F)
    if kind == "tie":
        # zero flow: a px lands on itself; alpha = 0, ex = 0.5: err = 0.25 = beta exactly on even
        # px, and the float above 0.25 on odd px
        z = np.zeros((H, W), F)
        ub = np.full((H, W), 0.5, F)
        vb = np.where(k % 2 == 0, F(0), TIE_OVER).astype(F)
        return z, z.copy(), ub, vb
    raise ValueError(kind)


def planes(case):
    """uf, vf, ub, vb as (n, H, W) float32 arrays."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(case.name))
    rng = np.random.default_rng(seed)
    per = [_planes_one(case, rng) for _ in range(case.n)]
    return tuple(np.stack([p[j] for p in per]).astype(F) for j in range(4))


CASES = _cases()
IDS = [c.name for c in CASES]

# The discrimination pair: a 192 x 160 synthetic pair whose frame1 has a 48 x 48 patch of
# unrelated texture (a region that exists in one slice only); solved with nscales 3, warps 3.
PATCH_W, PATCH_H = 192, 160
PATCH_BOX = (72, 56, 120, 104)   # x0, y0, x1, y1 (exclusive)
PATCH_PARAMS = dict(nscales=3, warps=3)


def patch_pair():
    from optflow_amd import synth
    I0, I1 = synth.gen_pair(PATCH_W, PATCH_H, seed=23)
    x0, y0, x1, y1 = PATCH_BOX
    tex = synth.base_texture(x1 - x0, y1 - y0, seed=99)
    I1 = I1.copy()
    I1[y0:y1, x0:x1] = np.clip(np.rint(tex), 0, 255).astype(np.uint8)
    return I0, I1


def patch_masks(margin=16):
    """(px inside the patch, px at least `margin` px away from the patch and the frame edge)."""
    ys, xs = np.mgrid[0:PATCH_H, 0:PATCH_W]
    x0, y0, x1, y1 = PATCH_BOX
    inp = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    near = (xs >= x0 - margin) & (xs < x1 + margin) & (ys >= y0 - margin) & (ys < y1 + margin)
    frame = (xs >= margin) & (xs < PATCH_W - margin) & (ys >= margin) & (ys < PATCH_H - margin)
    return inp, frame & ~near
