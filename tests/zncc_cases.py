"""One table of ZNCC score cases, shared by the CPU census (test_zncc_cpu.py) and the GPU
comparison (test_gpu_zncc.py).

A case is a size, a layout, a radius and a kind of frames and flow; planes(case) builds its u8
frames I0, I1 and float32 flow u, v as (n, H, W) arrays (I0 as (1, H, W) where the pairs share
frame0), deterministic from the case alone.  Sizes are W x H: a single px, a single column and
row, a frame lower than every window, sizes that are no multiple of a band, a width that crosses
a 256-px band and its halo, a height above one 64-row segment; a pitched ROI view whose u8 planes
start at an odd byte and whose f32 planes start 1 float off a 16-byte boundary; and 257 pairs, so
a second chunk of pairs runs.
"""
from dataclasses import dataclass

import numpy as np

F = np.float32

SIZES = [(1, 1), (1, 7), (5, 1), (3, 256), (67, 45), (257, 131)]
KINDS = ["identical", "shift", "ties", "edges", "edges_out", "special", "const0", "const1", "half",
         "negative", "smooth"]
ROI = (130, 70, 160, 80, 5 * 160 + 5)   # W, H, allocation W, H, first element: odd; 4 * 805 = 4 mod 16
BATCH = (130, 20, 257)                  # W, H, pairs

SPECIALS = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0]


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    kind: str
    r: int
    n: int = 1
    roi: tuple = None      # (allocation W, allocation H, first element) or None: dense planes
    shared0: bool = False  # one frame0 for every pair (pair stride 0)


def _cases():
    out = []
    for si, (W, H) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            r = 1 + (si + ki) % 4
            out.append(Case(f"{W}x{H}-{kind}-r{r}", W, H, kind, r))
    for W, H in ((67, 45), (257, 131)):     # every radius on one kind
        for r in (1, 2, 3, 4):
            name = f"{W}x{H}-smooth-r{r}"
            if all(c.name != name for c in out):
                out.append(Case(name, W, H, "smooth", r))
    W, H, AW, AH, first = ROI
    for r, kind in enumerate(("smooth", "special", "edges_out", "ties"), 1):
        out.append(Case(f"roi{W}x{H}-{kind}-r{r}", W, H, kind, r, roi=(AW, AH, first)))
    W, H, n = BATCH
    out.append(Case(f"batch{n}x{W}x{H}-smooth-r3", W, H, "smooth", 3, n=n))
    out.append(Case(f"batch{n}x{W}x{H}-shared0-r2", W, H, "smooth", 2, n=n, shared0=True))
    return out


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _texture(rng, W, H):
    """synth.base_texture plus noise: no flat window."""
    from optflow_amd import synth
    base = synth.base_texture(W, H, seed=int(rng.integers(1, 1 << 30)))
    return base.astype(np.float64)


def _smooth(rng, W, H, amp):
    """A smooth field of the given amplitude: three plane waves of random direction and phase."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(3):
        kx, ky = rng.uniform(-0.15, 0.15, 2)
        f += np.sin(kx * xs + ky * ys + rng.uniform(0, 2 * np.pi))
    return (f * (amp / 3.0)).astype(F)


def _tie_component(pos, last, k, q):
    """A flow component that puts pos + flow exactly on a rint tie of the 1/32 px grid (an odd
    multiple of 1/64), k % 3 == 0, one ulp below it (1) or one ulp above it (2); 0 where the frame
    has no room for it."""
    c = ((2 * (q % 16) + 1) / 64.0).astype(F)               # in (0, 0.5): exact
    target = np.where(pos + 1 <= last, pos.astype(F) + c, pos.astype(F) - c).astype(F)
    ok = (target >= 0) & (target <= F(last))
    target = np.where(k % 3 == 1, np.nextafter(target, F(-np.inf)), target)
    target = np.where(k % 3 == 2, np.nextafter(target, F(np.inf)), target).astype(F)
    flow = (target - pos.astype(F)).astype(F)
    assert np.all((pos.astype(F) + flow)[ok] == target[ok])   # the engine's mx is that target
    return np.where(ok, flow, F(0)).astype(F)


def _one(case, rng):
    W, H, kind = case.W, case.H, case.kind
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    k = ys * W + xs
    z = np.zeros((H, W), F)
    noise = lambda: rng.normal(0.0, 2.0, (H, W))
    tex = _texture(rng, W, H)
    if kind == "identical":
        I = _u8(tex + noise())
        return I, I.copy(), z, z.copy()
    if kind == "negative":
        I = _u8(tex + noise())
        return I, (255 - I).astype(np.uint8), z, z.copy()
    if kind == "shift":
        # I1(x + dx, y + dy) = I0(x, y) where that lies inside; unrelated values elsewhere
        dx, dy = (2, -1) if (W + H) % 2 else (-1, 1)
        I0 = _u8(tex + noise())
        I1 = rng.integers(0, 256, (H, W)).astype(np.uint8)
        ins = (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H)
        I1[(ys + dy)[ins], (xs + dx)[ins]] = I0[ins]
        return I0, I1, np.full((H, W), dx, F), np.full((H, W), dy, F)
    if kind == "ties":
        I0, I1 = _u8(tex + noise()), _u8(tex + noise())
        u = _tie_component(xs, W - 1, k, k)
        v = _tie_component(ys, H - 1, k // 3, k // 5 + 3)
        return I0, I1, u, v
    if kind in ("edges", "edges_out"):
        # px by px: land on mx = 0, mx = W - 1, my = 0, my = H - 1; or aim one ulp beyond
        out = kind == "edges_out"
        u, v = z.copy(), z.copy()
        tx0, tx1, ty0, ty1 = -xf, F(W - 1) - xf, -yf, F(H - 1) - yf
        if out:
            tx0, ty0 = np.nextafter(tx0, F(-np.inf)), np.nextafter(ty0, F(-np.inf))
            tx1, ty1 = np.nextafter(tx1, F(np.inf)), np.nextafter(ty1, F(np.inf))
        m = k % 4
        u[m == 0], u[m == 1] = tx0[m == 0], tx1[m == 1]
        v[m == 2], v[m == 3] = ty0[m == 2], ty1[m == 3]
        frac = F(0.28125)   # 9/32: an exact 1/32 px fraction
        u[(m >= 2) & (xs + 1 < W)] = frac
        v[(m < 2) & (ys + 1 < H)] = frac
        return _u8(tex + noise()), _u8(tex + noise()), u, v
    if kind == "special":
        u, v = _smooth(rng, W, H, 1.5), _smooth(rng, W, H, 1.5)
        i = 0
        for p in (u, v):
            for sv in SPECIALS:
                p.flat[(7 * i + 3) % (W * H)] = F(sv)
                i += 1
        return _u8(tex + noise()), _u8(tex + noise()), u, v
    if kind == "const0":    # B == 0 everywhere, C > 0
        return np.full((H, W), 77, np.uint8), _u8(tex + noise()), _smooth(rng, W, H, 1.0), _smooth(rng, W, H, 1.0)
    if kind == "const1":    # C == 0 everywhere, B > 0
        return _u8(tex + noise()), np.full((H, W), 140, np.uint8), _smooth(rng, W, H, 1.0), _smooth(rng, W, H, 1.0)
    if kind == "half":      # frame0 flat on the left, frame1 flat on top: B == 0 and C == 0 apart
        I0, I1 = _u8(tex + noise()), _u8(tex + noise())
        I0[:, :(W + 1) // 2] = 90
        I1[:(H + 1) // 2, :] = 201
        return I0, I1, z, z.copy()
    if kind == "smooth":
        return _u8(tex + noise()), _u8(tex + noise()), _smooth(rng, W, H, 3.0), _smooth(rng, W, H, 3.0)
    raise ValueError(kind)


_CACHE = {}


def planes(case):
    """I0, I1 (uint8), u, v (float32) as (n, H, W) arrays; I0 is (1, H, W) where shared.  Built
    once per case and read-only."""
    if case.name not in _CACHE:
        seed = sum(ord(c) * (i + 1) for i, c in enumerate(case.name))
        rng = np.random.default_rng(seed)
        per = [_one(case, rng) for _ in range(case.n)]
        out = [np.stack([p[j] for p in per]) for j in range(4)]
        if case.shared0:
            out[0] = out[0][:1].copy()
        out = (out[0].astype(np.uint8), out[1].astype(np.uint8), out[2].astype(F), out[3].astype(F))
        for a in out:
            a.setflags(write=False)
        _CACHE[case.name] = out
    return _CACHE[case.name]


CASES = _cases()
IDS = [c.name for c in CASES]
