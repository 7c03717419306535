"""Flow composition restated in numpy (include/tvl1.h, tvl1_compose_flow).
float32 throughout, one rounding per operation, in the header's order; shares no code with the
engine, which must match it bit for bit.

    uc, vc, outside = compose(ua, va, ub, vb)        (H, W) float32 planes, an int
    u, v, counts    = compose_chain(links)           links: [(u, v), ...], left to right
"""
import numpy as np

F = np.float32


def landing(ua, va):
    """X, Y and inside of the first two steps (also for the tests' census of the case table)."""
    ua, va = np.asarray(ua, F), np.asarray(va, F)
    H, W = ua.shape
    with np.errstate(all="ignore"):
        X = np.arange(W, dtype=F)[None, :] + ua
        Y = np.arange(H, dtype=F)[:, None] + va
        inside = (X >= F(0)) & (X <= F(W - 1)) & (Y >= F(0)) & (Y <= F(H - 1))
    return X, Y, inside


def _clamp(X, hi):
    """X >= 0 ? (X <= hi ? X : hi) : 0 -- NaN and -inf give 0, +inf gives hi."""
    with np.errstate(invalid="ignore"):
        return np.where(X >= F(0), np.where(X <= hi, X, hi), F(0)).astype(F)


def compose(ua, va, ub, vb):
    ua, va, ub, vb = (np.asarray(a, F) for a in (ua, va, ub, vb))
    H, W = ua.shape
    assert va.shape == ub.shape == vb.shape == (H, W)
    X, Y, inside = landing(ua, va)
    Xc, Yc = _clamp(X, F(W - 1)), _clamp(Y, F(H - 1))
    x0 = np.floor(Xc).astype(np.int64)
    y0 = np.floor(Yc).astype(np.int64)
    assert x0.min() >= 0 and x0.max() <= W - 1 and y0.min() >= 0 and y0.max() <= H - 1
    with np.errstate(all="ignore"):
        ax = Xc - x0.astype(F)
        ay = Yc - y0.astype(F)
        x1 = np.minimum(x0 + 1, W - 1)
        y1 = np.minimum(y0 + 1, H - 1)

        def sample(P):
            p00, p01, p10, p11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
            t = p00 + ax * (p01 - p00)
            b = p10 + ax * (p11 - p10)
            return t + ay * (b - t)

        ubs, vbs = sample(ub), sample(vb)
        uc = ua + ubs
        vc = va + vbs
    for a in (X, Xc, ax, ay, ubs, vbs, uc, vc):
        assert a.dtype == F
    return uc, vc, int((~inside).sum())


def compose_chain(links):
    """Left to right: ((l0 . l1) . l2) ..., as Engine.compose_chain_host accumulates."""
    u, v = (np.array(a, F, copy=True) for a in links[0])
    counts = []
    for ub, vb in links[1:]:
        u, v, n = compose(u, v, ub, vb)
        counts.append(n)
    return u, v, counts
