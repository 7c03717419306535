"""TEST INFRASTRUCTURE: numpy restatements of the pre-alignment stages that share no code with
oracle/tvl1_oracle_align.c -- a brute-force Hamming matcher, cv::cuda::warpAffine on u8 and the
map post-process in float32, and level 0 of the keypoint detector (FAST-9 as sixteen explicit
rotations of a 9-run, the Harris sum in float32 in tap order, 3x3 non-maximum suppression with
the top-left tie rule, the best quota by (score, raster position)).

tests/test_align_edges_cpu.py holds the oracle to them; tests/test_gpu_align_edges.py holds the
GPU to the matcher and the warps directly, so a slip the oracle and the kernels share (they
were written side by side) still fails."""
from __future__ import annotations

import numpy as np

F = np.float32
NO_DIST = 1 << 30   # the distance reported where the train set has no such neighbour

FAST_DX = (0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1)
FAST_DY = (-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3)


# ---------------------------------------------------------------- matching
def match_knn2(query: np.ndarray, train: np.ndarray):
    """(idx (nq, 2), dist (nq, 2)): the two nearest train descriptors by Hamming distance, the
    lower index first among equals (a stable sort of the distance rows)."""
    q = np.asarray(query, np.uint8).reshape(-1, 32)
    t = np.asarray(train, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), NO_DIST, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    for i in range(nq):
        d = np.unpackbits(q[i][None, :] ^ t, axis=1).sum(axis=1, dtype=np.int64)
        order = np.argsort(d, kind="stable")[:2]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[order]
    return idx, dist


# ---------------------------------------------------------------- warpAffine
def affine_inverse(M) -> np.ndarray:
    """cv::invertAffineTransform: the inverse in double (all zero for a singular matrix),
    stored as float32."""
    a, b, c, d, e, f = (float(x) for x in np.asarray(M, np.float32).ravel())
    D = a * e - b * d
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = e * D, a * D, -b * D, -d * D
    return np.array([A11, A12, -A11 * c - A12 * f, A21, A22, -A21 * c - A22 * f], np.float64).astype(F)


def _source_coords(m, dw, dh):
    x = np.arange(dw, dtype=F)[None, :]
    y = np.arange(dh, dtype=F)[:, None]
    xs = (m[0] * x + m[1] * y) + m[2]
    ys = (m[3] * x + m[4] * y) + m[5]
    assert xs.dtype == F and ys.dtype == F
    return xs, ys


def _bilinear(src: np.ndarray, xs: np.ndarray, ys: np.ndarray) -> np.ndarray:
    """cuda LinearFilter over BORDER_CONSTANT 0 in float32: the taps (x1, y1), (x2, y1),
    (x1, y2), (x2, y2) added in that order, each weight the product of two differences."""
    sh, sw = src.shape
    s = src.astype(F)
    x1f, y1f = np.floor(xs), np.floor(ys)
    x1, y1 = x1f.astype(np.int64), y1f.astype(np.int64)
    x2, y2 = x1 + 1, y1 + 1

    def at(yy, xx):
        ok = (xx >= 0) & (yy >= 0) & (xx < sw) & (yy < sh)
        return np.where(ok, s[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], F(0))

    x1f, y1f, x2f, y2f = x1.astype(F), y1.astype(F), x2.astype(F), y2.astype(F)
    out = np.zeros(xs.shape, F)
    out = out + at(y1, x1) * ((x2f - xs) * (y2f - ys))
    out = out + at(y1, x2) * ((xs - x1f) * (y2f - ys))
    out = out + at(y2, x1) * ((x2f - xs) * (ys - y1f))
    out = out + at(y2, x2) * ((xs - x1f) * (ys - y1f))
    assert out.dtype == F
    return out


def warp_affine_u8(src: np.ndarray, dw: int, dh: int, M) -> np.ndarray:
    """dst(x, y) = src(M^-1 (x, y)), INTER_LINEAR, BORDER_CONSTANT 0, saturate_cast<uchar>
    (round half to even, clamp)."""
    xs, ys = _source_coords(affine_inverse(M), dw, dh)
    out = _bilinear(np.asarray(src, np.uint8), xs, ys)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def postprocess_affine(u, v, I1, flow_output: int, M):
    """map = flow + grid, warpAffine of both map planes, minus the grid for flow output, zero
    where I1 <= 1."""
    u = np.asarray(u, F)
    v = np.asarray(v, F)
    H, W = u.shape
    gx = np.arange(W, dtype=F)[None, :]
    gy = np.arange(H, dtype=F)[:, None]
    m1, m2 = u + gx, v + gy
    xs, ys = _source_coords(affine_inverse(M), W, H)
    a, b = _bilinear(m1, xs, ys), _bilinear(m2, xs, ys)
    if flow_output:
        a, b = a - gx, b - gy
    mask = np.asarray(I1) <= 1
    return np.where(mask, F(0), a).astype(F), np.where(mask, F(0), b).astype(F)


# ---------------------------------------------------------------- keypoints of level 0
def harris_scores(img: np.ndarray, border: int, fast_threshold: int = 20) -> np.ndarray:
    """The score plane of level 0: the Harris response (7x7 Sobel window, k = 0.04, floored at
    1e-30) at FAST-9 corners at least `border` px inside, 0 elsewhere."""
    I = np.asarray(img, np.uint8).astype(F)
    H, W = I.shape
    score = np.zeros((H, W), F)
    x0, x1, y0, y1 = border, W - border, border, H - border
    if x1 <= x0 or y1 <= y0:
        return score
    c = I[y0:y1, x0:x1]
    t = F(fast_threshold)
    ring = [I[y0 + dy:y1 + dy, x0 + dx:x1 + dx] for dx, dy in zip(FAST_DX, FAST_DY)]
    bright = [r > c + t for r in ring]
    dark = [r < c - t for r in ring]
    corner = np.zeros(c.shape, bool)
    for masks in (bright, dark):
        for start in range(16):
            run = np.ones(c.shape, bool)
            for k in range(9):
                run &= masks[(start + k) % 16]
            corner |= run
    # Sobel gradients wherever a corner's 7x7 window can reach (3 px around the candidates)
    P = np.pad(I, 1, mode="edge")   # never read at a candidate: border >= 16 > 4
    r0, r1, r2 = P[:-2], P[1:-1], P[2:]
    gx = (r0[:, 2:] - r0[:, :-2]) + F(2) * (r1[:, 2:] - r1[:, :-2]) + (r2[:, 2:] - r2[:, :-2])
    gy = (r2[:, :-2] - r0[:, :-2]) + F(2) * (r2[:, 1:-1] - r0[:, 1:-1]) + (r2[:, 2:] - r0[:, 2:])
    a = np.zeros(c.shape, F)
    b = np.zeros(c.shape, F)
    cc = np.zeros(c.shape, F)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            wx = gx[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            wy = gy[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            a = a + wx * wx
            b = b + wy * wy
            cc = cc + wx * wy
    s = F(1.0) / (F(4.0) * F(255.0) * F(49.0))
    a, b, cc = a * (s * s), b * (s * s), cc * (s * s)
    resp = np.maximum(a * b - cc * cc - F(0.04) * (a + b) * (a + b), F(1e-30))
    assert resp.dtype == F
    score[y0:y1, x0:x1] = np.where(corner, resp, F(0))
    return score


def nms3(score: np.ndarray, position_rule: bool = True) -> np.ndarray:
    """Survivors of the 3x3 suppression: positive, no larger neighbour, and no equal neighbour
    above or to the left on the same row (of two equal neighbours exactly one survives)."""
    H, W = score.shape
    keep = np.zeros((H, W), bool)
    if H < 3 or W < 3:
        return keep
    s = score[1:-1, 1:-1]
    k = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            o = score[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
            k &= ~(o > s)
            if position_rule and (dy < 0 or (dy == 0 and dx < 0)):
                k &= ~(o == s)
    keep[1:-1, 1:-1] = k
    return keep


def level0_keypoints(img: np.ndarray, nfeatures: int, border: int, fast_threshold: int = 20):
    """(x, y, response) of the level-0 keypoints at nlevels = 1 (the whole budget on level 0):
    the best nfeatures survivors by score, raster order among equal scores, best first.
    Also returns every survivor the same way, for the census of ties."""
    score = harris_scores(img, border, fast_threshold)
    ys, xs = np.nonzero(nms3(score))
    r = score[ys, xs]
    order = np.lexsort((ys * img.shape[1] + xs, -r.astype(np.float64)))
    allk = np.stack([xs[order].astype(F), ys[order].astype(F), r[order]], axis=1)
    return allk[:nfeatures], allk
