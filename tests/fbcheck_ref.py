"""The forward-backward consistency score restated in numpy (include/tvl1.h,
tvl1_fb_score).  float32 throughout, one rounding per operation, in the header's
order; shares no code with the engine, which must match it bit for bit.

    score = fb_score(uf, vf, ub, vb, alpha)          (H, W) float32 planes
    ok    = consistent(score, beta)                  score <= beta: False for NaN and +inf
    u, v, rejected = zero_above(u, v, score, beta)   tvl1_zero_above
"""
import numpy as np

F = np.float32


def fb_score(uf, vf, ub, vb, alpha):
    uf, vf, ub, vb = (np.asarray(a, F) for a in (uf, vf, ub, vb))
    H, W = uf.shape
    assert vf.shape == ub.shape == vb.shape == (H, W)
    alpha = F(alpha)
    xs = np.arange(W, dtype=F)[None, :]
    ys = np.arange(H, dtype=F)[:, None]
    score = np.full((H, W), np.inf, F)
    with np.errstate(all="ignore"):
        X = xs + uf                                                   # step 1
        Y = ys + vf
        inside = (X >= F(0)) & (X <= F(W - 1)) & (Y >= F(0)) & (Y <= F(H - 1))   # step 2
        idx = np.nonzero(inside)            # steps 3-7 only where inside
        Xi, Yi, u, v = X[idx], Y[idx], uf[idx], vf[idx]
        x0 = np.floor(Xi).astype(np.int64)                            # step 3
        y0 = np.floor(Yi).astype(np.int64)
        ax = Xi - x0.astype(F)
        ay = Yi - y0.astype(F)
        x1 = np.minimum(x0 + 1, W - 1)
        y1 = np.minimum(y0 + 1, H - 1)

        def sample(P):                                                # step 4
            p00, p01, p10, p11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
            t = p00 + ax * (p01 - p00)
            b = p10 + ax * (p11 - p10)
            return t + ay * (b - t)

        ubs, vbs = sample(ub), sample(vb)
        ex = u + ubs                                                  # step 5
        ey = v + vbs
        err = ex * ex + ey * ey
        mag = (u * u + v * v) + (ubs * ubs + vbs * vbs)               # step 6
        am = alpha * mag                                              # step 7
        s = err - am
    for a in (X, ax, ubs, err, mag, am, s):
        assert a.dtype == F
    score[idx] = s
    return score


def consistent(score, beta):
    with np.errstate(invalid="ignore"):
        return np.asarray(score, F) <= F(beta)


def zero_above(u, v, score, beta):
    """(u, v) with 0 where the px is not consistent at beta, and how many such px."""
    rej = ~consistent(score, beta)
    u2 = np.array(u, F, copy=True)
    v2 = np.array(v, F, copy=True)
    u2[rej] = 0
    v2[rej] = 0
    return u2, v2, int(rej.sum())


def landing(uf, vf):
    """X, Y, inside of step 1 and 2 (for the tests' census of the case table)."""
    uf, vf = np.asarray(uf, F), np.asarray(vf, F)
    H, W = uf.shape
    with np.errstate(all="ignore"):
        X = np.arange(W, dtype=F)[None, :] + uf
        Y = np.arange(H, dtype=F)[:, None] + vf
        inside = (X >= F(0)) & (X <= F(W - 1)) & (Y >= F(0)) & (Y <= F(H - 1))
    return X, Y, inside
