"""Flow inversion restated in numpy (include/tvl1.h, tvl1_invert_flow).
float32 throughout, one rounding per operation, in the header's order; shares no code with the
engine, which must match it bit for bit.

    ug, vg, resid, outside, unconverged = invert(uf, vf, K, tol)     (H, W) float32 planes, ints
    ug, vg, resid, inside, fixed_at     = invert_px(uf, vf, K)       a per-px loop, for the tests

g is the flow B -> A on B's grid of the flow f of A -> B: the fixed point of g = -f(y + g), started
at g0 = -f(y) and iterated K times; resid = |g + f(y + g)|^2 at the last iterate.
"""
import numpy as np

F = np.float32


def _clamp(X, hi):
    """X >= 0 ? (X <= hi ? X : hi) : 0 -- NaN and -inf give 0, +inf gives hi."""
    with np.errstate(invalid="ignore"):
        return np.where(X >= F(0), np.where(X <= hi, X, hi), F(0)).astype(F)


def step(uf, vf, ug, vg):
    """One sample of f at y + g: (us, vs, inside, X, Y), every plane (H, W)."""
    H, W = uf.shape
    with np.errstate(all="ignore"):
        X = np.arange(W, dtype=F)[None, :] + ug
        Y = np.arange(H, dtype=F)[:, None] + vg
        inside = (X >= F(0)) & (X <= F(W - 1)) & (Y >= F(0)) & (Y <= F(H - 1))
        Xc, Yc = _clamp(X, F(W - 1)), _clamp(Y, F(H - 1))
        x0 = np.floor(Xc).astype(np.int64)
        y0 = np.floor(Yc).astype(np.int64)
        assert x0.min() >= 0 and x0.max() <= W - 1 and y0.min() >= 0 and y0.max() <= H - 1
        ax = Xc - x0.astype(F)
        ay = Yc - y0.astype(F)
        x1 = np.minimum(x0 + 1, W - 1)
        y1 = np.minimum(y0 + 1, H - 1)

        def sample(P):
            p00, p01, p10, p11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
            t = p00 + ax * (p01 - p00)
            b = p10 + ax * (p11 - p10)
            return t + ay * (b - t)

        us, vs = sample(uf), sample(vf)
    for a in (X, Y, Xc, Yc, ax, ay, us, vs):
        assert a.dtype == F
    return us, vs, inside, X, Y


def iterates(uf, vf, K):
    """[g_0, ..., g_K] and the last sample (us, vs, inside) taken at g_K."""
    uf, vf = np.asarray(uf, F), np.asarray(vf, F)
    assert uf.shape == vf.shape and 1 <= K <= 32
    g = [(-uf, -vf)]
    for _ in range(K):
        us, vs, _, _, _ = step(uf, vf, *g[-1])
        g.append((-us, -vs))
    return g, step(uf, vf, *g[-1])[:3]


def invert(uf, vf, K, tol=0.01):
    g, (us, vs, inside) = iterates(uf, vf, K)
    ug, vg = g[-1]
    with np.errstate(all="ignore"):
        ex = ug + us
        ey = vg + vs
        resid = ex * ex + ey * ey
        conv = resid <= F(tol)   # false for NaN
    for a in (ug, vg, ex, ey, resid):
        assert a.dtype == F
    return ug, vg, resid, int((~inside).sum()), int((~conv).sum())


def fixed_at(uf, vf, K):
    """Per px, the first k < K with g_{k+1} == g_k bit for bit, or K where there is none."""
    g, _ = iterates(uf, vf, K)
    out = np.full(g[0][0].shape, K, np.int64)
    for k in range(K - 1, -1, -1):
        same = ((g[k + 1][0].view(np.uint32) == g[k][0].view(np.uint32)) &
                (g[k + 1][1].view(np.uint32) == g[k][1].view(np.uint32)))
        out[same] = k
    return out


def invert_px(uf, vf, K):
    """The same, px by px with scalar float32 arithmetic: (ug, vg, resid, inside)."""
    uf, vf = np.asarray(uf, F), np.asarray(vf, F)
    H, W = uf.shape
    ug, vg, rs = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    ins = np.zeros((H, W), bool)
    xm, ym = F(W - 1), F(H - 1)

    def sample_at(x, y, gu, gv):
        X, Y = F(x) + gu, F(y) + gv
        inside = bool(X >= 0 and X <= xm and Y >= 0 and Y <= ym)
        Xc = (X if X <= xm else xm) if X >= 0 else F(0)
        Yc = (Y if Y <= ym else ym) if Y >= 0 else F(0)
        x0, y0 = int(np.floor(Xc)), int(np.floor(Yc))
        ax, ay = F(Xc - F(x0)), F(Yc - F(y0))
        x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
        s = []
        for P in (uf, vf):
            t = F(P[y0, x0] + F(ax * F(P[y0, x1] - P[y0, x0])))
            b = F(P[y1, x0] + F(ax * F(P[y1, x1] - P[y1, x0])))
            s.append(F(t + F(ay * F(b - t))))
        return s[0], s[1], inside

    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                gu, gv = F(-uf[y, x]), F(-vf[y, x])
                for _ in range(K):
                    us, vs, _ = sample_at(x, y, gu, gv)
                    gu, gv = F(-us), F(-vs)
                us, vs, inside = sample_at(x, y, gu, gv)
                ex, ey = F(gu + us), F(gv + vs)
                ug[y, x], vg[y, x], ins[y, x] = gu, gv, inside
                rs[y, x] = F(F(ex * ex) + F(ey * ey))
    return ug, vg, rs, ins
