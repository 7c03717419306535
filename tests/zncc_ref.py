"""The photometric (ZNCC) score of a flow restated in numpy (include/tvl1.h, tvl1_zncc_score;
DESIGN 14).  Shares no code with the engine, which must match it bit for bit.

    J, m  = warp(I1, u, v)                    step 1: uint8 warped frame (0 where !m), bool validity
    score = zncc_score(I0, I1, u, v, r)       (H, W) float32, lower is better, +inf = no evidence
    n, Sa, Sb, Saa, Sbb, Sab = window_sums(I0, J, m, r)      step 2, int64 planes
    ... = window_sums_bruteforce(I0, J, m, r)                the same by a loop per px
    accepted(score, beta), zero_above(u, v, score, beta)     tvl1_zero_above's rule
"""
import numpy as np

F = np.float32


def warp(I1, u, v):
    """Step 1.  float32 throughout, one rounding per operation; the sample in integers."""
    I1 = np.asarray(I1, np.uint8)
    u, v = np.asarray(u, F), np.asarray(v, F)
    H, W = I1.shape
    assert u.shape == v.shape == (H, W)
    xs = np.arange(W, dtype=F)[None, :]
    ys = np.arange(H, dtype=F)[:, None]
    J = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        mx = xs + u
        my = ys + v
        assert mx.dtype == F and my.dtype == F
        m = (mx >= F(0)) & (mx <= F(W - 1)) & (my >= F(0)) & (my <= F(H - 1))   # False for NaN
    idx = np.nonzero(m)                      # nothing is converted where !m
    mx32 = mx[idx] * F(32)
    my32 = my[idx] * F(32)
    assert mx32.dtype == F
    ix = np.rint(mx32).astype(np.int64)      # half to even
    iy = np.rint(my32).astype(np.int64)
    sx, fx = ix >> 5, ix & 31
    sy, fy = iy >> 5, iy & 31
    x1 = np.minimum(sx + 1, W - 1)
    y1 = np.minimum(sy + 1, H - 1)
    T = I1.astype(np.int64)
    s00, s01, s10, s11 = T[sy, sx], T[sy, x1], T[y1, sx], T[y1, x1]
    val = (s00 * (32 - fx) * (32 - fy) + s01 * fx * (32 - fy) + s10 * (32 - fx) * fy + s11 * fx * fy + 512) >> 10
    assert val.size == 0 or (val.min() >= 0 and val.max() <= 255)
    J[idx] = val.astype(np.uint8)
    return J, m


def _box(P, r):
    """Sum of P over the (2r+1)^2 window cut to the frame: P is int64 (H, W)."""
    H, W = P.shape
    Z = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    Z[r + 1:r + 1 + H, r + 1:r + 1 + W] = P
    S = Z.cumsum(0).cumsum(1)
    k = 2 * r + 1
    return S[k:k + H, k:k + W] - S[:H, k:k + W] - S[k:k + H, :W] + S[:H, :W]


def window_sums(I0, J, m, r):
    """Step 2: n, Sa, Sb, Saa, Sbb, Sab over the window cut to the frame and to px with m."""
    a = np.where(m, np.asarray(I0, np.uint8).astype(np.int64), 0)
    b = np.where(m, np.asarray(J, np.uint8).astype(np.int64), 0)
    return (_box(m.astype(np.int64), r), _box(a, r), _box(b, r), _box(a * a, r), _box(b * b, r),
            _box(a * b, r))


def window_sums_bruteforce(I0, J, m, r):
    I0 = np.asarray(I0, np.uint8)
    H, W = I0.shape
    out = np.zeros((6, H, W), np.int64)
    for y in range(H):
        for x in range(W):
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    yy, xx = y + j, x + i
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx]:
                        a, b = int(I0[yy, xx]), int(J[yy, xx])
                        out[:, y, x] += (1, a, b, a * a, b * b, a * b)
    return tuple(out)


def abc(sums):
    n, Sa, Sb, Saa, Sbb, Sab = sums
    A = n * Sab - Sa * Sb
    B = n * Saa - Sa * Sa
    C = n * Sbb - Sb * Sb
    assert max(np.abs(A).max(), B.max(), C.max()) < 1 << 29 and B.min() >= 0 and C.min() >= 0
    return A, B, C


def score_from(J, m, I0, r):
    """Steps 2 and 3 on a given warped frame."""
    A, B, C = abc(window_sums(I0, J, m, r))
    score = np.full(m.shape, np.inf, F)
    ok = m & (B != 0) & (C != 0)
    Ad, Bd, Cd = (q[ok].astype(np.float64) for q in (A, B, C))
    bc = Bd * Cd                      # four f64 operations, each rounded once
    rt = np.sqrt(bc)
    q = Ad / rt
    s = np.float64(1.0) - q
    assert s.dtype == np.float64
    score[ok] = s.astype(F)
    return score


def zncc_score(I0, I1, u, v, r):
    assert 1 <= r <= 4
    J, m = warp(I1, u, v)
    return score_from(J, m, I0, r)


def accepted(score, beta):
    with np.errstate(invalid="ignore"):
        return np.asarray(score, F) <= F(beta)


def zero_above(u, v, score, beta):
    """(u, v) with 0 where !(score <= beta), and how many such px (tvl1_zero_above)."""
    rej = ~accepted(score, beta)
    u2 = np.array(u, F, copy=True)
    v2 = np.array(v, F, copy=True)
    u2[rej] = 0
    v2[rej] = 0
    return u2, v2, int(rej.sum())
