"""tests/warp_window.py held to the kernels' source, to the planner and to the oracle, with no GPU.

tests/test_gpu_warp_window.py runs that table bitwise against the oracle's seeded entry.  It
would be vacuous if a seed no longer sat on a window's edge, if the reference did not care
which pixel a tap reads, or if a stopping decision sat within the residual's accumulation
error of a threshold.  So here

  * the mirrored window geometry is rebuilt from csrc/tvl1_kernels.hpp (ring_mx, the margins
    the engine instantiates, kWarpTW / kWarpTH / kWarpHalo, the predicates' own text) and from
    tests/plan_dump.cpp (band starts, segment rows): a changed margin fails here;
  * census, from the float32 sums x + u1, y + u2 themselves: each of the eight classes (four
    window sides x last footprint in / first out) holds >= 100 px in the case that targets it,
    the ulp case >= 100 px in each fraction class on each axis;
  * sensitivity: the reference of every solve rerun with I1 rolled by one column and by one row
    (a gather that reads one pixel off) keeps both flow words of at most 0.1 % of the pixels;
  * every reference result is finite, every stopping-rule case clears MIN_MARGIN in IEEE and
    in fma.
Each condition is a bar on the inputs: a size that misses one gets a larger frame or another
cycle in warp_window.py, never a lower bar.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import warp_window as ww
from optflow_amd import capi
from oracle import checker
from test_plan_cpu import dump  # noqa: F401  (the module-scoped plan_dump fixture)
from test_residual_margin_cpu import MIN_MARGIN

CSRC = Path(__file__).resolve().parent.parent / "fibsem-optflow_amd" / "csrc"
MIN_CLASS = 100          # px per census class
MAX_KEEP = 1e-3          # share of px whose flow survives a rolled I1


def _int(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what} not found"
    return int(m.group(1))


# ---------------------------------------------------------------- geometry
def test_geometry_mirrors_the_kernels(dump):
    k = (CSRC / "tvl1_kernels.hpp").read_text()
    e = (CSRC / "tvl1_engine.hip").read_text()
    b = (CSRC / "tvl1_batch.hpp").read_text()
    # the margins the engine instantiates: M = 6 rows, ring_mx<6>() = 5 columns
    assert "(k_warp_ring<6, 2, FM>)" in e and "(kb_warp_ring<6, 2, FM>)" in e
    assert "(kb_warp_iter<6, FM, 2>)" in e and "(kb_warp_iter<6, FM, 1>)" in e
    assert "warp_iter_body<M, FM, 128, 0, NC>" in b
    M = _int(r"#define TVL1_WI_M (\d+)", e, "TVL1_WI_M")
    assert "constexpr int M = kWiMargin, BW = 128;" in e and M == 6
    m = re.search(r"constexpr int ring_mx\(\) \{ return M == 6 \? (\d+) : M; \}", k)
    assert m, "ring_mx"
    MX = int(m.group(1))
    BW, HALO = 128, 2   # roll_halo<2, 2>(): K = 2 iterations, PX = BW / 64 = 2
    assert "constexpr int K = 2, PX = BW / 64, HALO = roll_halo<2, PX>(), WW = wi_ww<M, BW>();" in k
    assert "constexpr int roll_halo() { return (K + PX - 1) / PX * PX; }" in k
    assert "constexpr int wi_ww() { return BW + 2 * ring_mx<M>(); }" in k
    # where each window starts, and the predicates themselves
    assert "const int x0 = band * 64;" in k
    assert "const int X0 = band * (BW - 2 * HALO) - HALO;" in k and "P.xw0 = X0 - ring_mx<M>();" in k
    assert ("const bool inwin = fx - 1 >= x0 - MX && fx + 2 < x0 + 64 + MX && fy - 1 >= y - M && "
            "fy + 2 <= y + M;") in k
    assert ("const bool inwin = fx - 1 >= P.xw0 && fx + 2 < P.xw0 + WW && fy - 1 >= gy - M && "
            "fy + 2 <= gy + M;") in k
    assert ("const bool inwin = fx - 1 >= ox && fx + 2 < ox + kWarpWW && fy - 1 >= oy && "
            "fy + 2 < oy + kWarpWH;") in k
    assert "const int ox = x0 - kWarpHalo, oy = y0 - kWarpHalo;" in k
    m = re.search(r"constexpr int kWarpTW = (\d+), kWarpTH = (\d+), kWarpHalo = (\d+);", k)
    assert m, "kWarpTW / kWarpTH / kWarpHalo"
    TW, TH, HL = (int(x) for x in m.groups())
    assert "kWarpWW = kWarpTW + 2 * kWarpHalo, kWarpWH = kWarpTH + 2 * kWarpHalo;" in k
    assert ww.GEOMETRY == {
        "ring": ww.Geom(64, -MX, 64 + 2 * MX, "pixel", -M, M, 0),
        "iter": ww.Geom(BW - 2 * HALO, -HALO - MX, BW + 2 * MX, "pixel", -M, M, 0),
        "img": ww.Geom(TW, -HL, TW + 2 * HL, "tile", -HL, TH + HL - 1, TH),
    }
    # band starts and segment rows: the planner cuts bands of exactly the mirrored period
    for site, geom, pairs in (("warp_ring", "ring", 1), ("warp_iter", "iter", 1),
                              ("kb_warp_ring", "ring", 3), ("kb_warp_iter", "iter", 3)):
        B = ww.GEOMETRY[geom].period
        seg = 0 if pairs > 1 else ww.SEG   # the batched gathers take no TVL1_ROLL_SEG
        ws = [B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B, 3 * B + 1]
        out = dump([f"site {site} {w} 41 {6 if geom == 'ring' else 8} 0 4096 100 {seg} {pairs} 0" for w in ws])
        assert [int(o.split()[0]) for o in out] == [1, 1, 2, 2, 3, 3, 4], site
        if pairs == 1:
            assert {int(o.split()[1]) for o in out} == {ww.SEG}, site


def test_frames_have_every_edge(dump):
    """193 x 41: three 64-px bands and a 1-px band, five 8-row segments and a one-row segment,
    three 16-row tiles less 7 rows; 249 x 17: two 124-px bands and a 1-px band, a one-row
    segment."""
    (ring,) = dump([f"site warp_ring 193 41 6 0 4096 100 {ww.SEG} 1 0"])
    (it,) = dump([f"site warp_iter 249 17 8 0 4096 100 {ww.SEG} 1 0"])
    assert [int(x) for x in ring.split()] == [4, 8, 4 * 6]
    assert [int(x) for x in it.split()] == [3, 8, 3 * 3]
    assert 193 == 3 * 64 + 1 and 41 == 5 * 8 + 1 == 3 * 16 - 7 and 249 == 2 * 124 + 1 and 17 == 2 * 8 + 1
    sizes = {r.name: (r.W, r.H) for r in ww.ROWS}
    assert sizes == {"k_warp_ring": (193, 41), "k_warp_img": (193, 41), "kb_warp_ring": (193, 41),
                     "k_warp_iter": (249, 17), "k_warp_iter-nc1": (249, 17), "kb_warp_iter": (249, 17),
                     "kb_small_level": (130, 12)}
    for r in ww.ROWS:
        assert r.W <= 249 and r.H <= 41
        for p in r.psets.values():
            assert p["nscales"] == 1 and p["warps"] * p["iterations"] <= 14
    assert ww.ROW_OF["kb_small_level"].W <= 64 * 9 and ww.ROW_OF["kb_small_level"].H <= 17   # kSmallWaves, kSmallR


# ---------------------------------------------------------------- census
WINDOWED = [("ring", 193, 41), ("img", 193, 41), ("iter", 249, 17)]
ALL_FRAMES = WINDOWED + [("ring", 130, 12)]


def _census(geom, kind, W, H):
    g = ww.GEOMETRY[geom]
    u, v = ww.make_seed(geom, kind, W, H)
    assert u.dtype == np.float32 and v.dtype == np.float32
    assert np.isfinite(u).all() and np.isfinite(v).all() and max(np.abs(u).max(), np.abs(v).max()) < 2.0 ** 20
    ys, xs = np.mgrid[0:H, 0:W]
    wx, wy, fx, fy = ww.coords(u, v)
    (x0, x1), (y0, y1) = ww.fx_range(g, xs), ww.fy_range(g, ys)
    okx, oky = (fx >= x0) & (fx <= x1), (fy >= y0) & (fy <= y1)
    # a class counts a px only where the other axis is inside: that side alone decides
    cls = {"left-in": (fx == x0) & oky, "left-out": (fx == x0 - 1) & oky,
           "right-in": (fx == x1) & oky, "right-out": (fx == x1 + 1) & oky,
           "top-in": (fy == y0) & okx, "top-out": (fy == y0 - 1) & okx,
           "bottom-in": (fy == y1) & okx, "bottom-out": (fy == y1 + 1) & okx}
    inw = ww.in_window(g, xs, ys, fx, fy)
    for name, m in cls.items():
        assert not m.any() or inw[m].all() == name.endswith("-in"), name
    return {n: int(m.sum()) for n, m in cls.items()}, wx, wy, inw


@pytest.mark.parametrize("geom,W,H", WINDOWED, ids=[f"{g}-{w}x{h}" for g, w, h in WINDOWED])
def test_census_of_the_window_edges(geom, W, H):
    cx, _, wy, _ = _census(geom, "x", W, H)
    assert np.all(wy - np.floor(wy) == 0.25)
    cy, wx, _, _ = _census(geom, "y", W, H)
    assert np.all(wx - np.floor(wx) == 0.25)
    cxy, _, _, inw = _census(geom, "xy", W, H)
    print(geom, W, H, "x", cx, "y", cy, "xy", cxy, "xy in window", float(inw.mean()))
    for side in ("left", "right"):
        for io in ("in", "out"):
            assert cx[f"{side}-{io}"] >= MIN_CLASS and cxy[f"{side}-{io}"] >= MIN_CLASS, (side, io, cx, cxy)
    for side in ("top", "bottom"):
        for io in ("in", "out"):
            assert cy[f"{side}-{io}"] >= MIN_CLASS and cxy[f"{side}-{io}"] >= MIN_CLASS, (side, io, cy, cxy)
    assert 0.2 < inw.mean() < 0.8   # both paths of the kernel, within one wavefront


@pytest.mark.parametrize("geom,W,H", ALL_FRAMES, ids=[f"{g}-{w}x{h}" for g, w, h in ALL_FRAMES])
def test_census_of_the_ulp_and_beyond_seeds(geom, W, H):
    g = ww.GEOMETRY[geom]
    _, wx, wy, _ = _census(geom, "ulp", W, H)
    for axis, w, n, rows in (("x", wx, W, False), ("y", wy, H, True)):
        fc = ww.frac_class(w)
        counts = [int((fc == c).sum()) for c in range(4)]
        print(geom, W, H, "ulp", axis, counts)
        assert min(counts) >= MIN_CLASS, (axis, counts)
        # the spots: every target's [T, T + 1] is visited (the sums may round onto T + 1)
        hit = set(np.floor(w).astype(int).ravel().tolist())
        ts = ww.ulp_targets(g, n, rows)
        assert {-1, n - 1} <= set(ts.tolist()) and set(ts.tolist()) <= hit, (axis, ts)
        if not rows:
            assert {63, 64, 127, 128} & set(range(n)) <= set(ts.tolist())
    # sums that round up onto the next integer: the flow is 1 ulp below an integer, the sum is one
    u, v = ww.make_seed(geom, "ulp", W, H)
    ys, xs = (a.astype(np.float32) for a in np.mgrid[0:H, 0:W])
    up = sum(int(((np.nextafter(f, np.float32(np.inf)) == np.round(f)) & (f != np.round(f)) &
                  (pos + f == np.round(pos + f))).sum()) for f, pos in ((u, xs), (v, ys)))
    assert up >= MIN_CLASS, up
    _, wx, wy, _ = _census(geom, "beyond", W, H)
    fx, fy = np.floor(wx), np.floor(wy)
    left, right, top, bottom = fx + 2 <= 0, fx - 1 >= W - 1, fy + 2 <= 0, fy - 1 >= H - 1
    assert (left | right | top | bottom).all()
    for m in (left, right, top, bottom):
        assert m.sum() >= MIN_CLASS
    assert wx.min() >= -(W + 8) and wx.max() <= W - 1 + W + 8 and wx.min() < -W and wx.max() > 2 * W
    assert wy.min() >= -(H + 8) and wy.max() <= H - 1 + H + 8 and wy.min() < -H and wy.max() > 2 * H


# ---------------------------------------------------------------- the references
def _solve_ids():
    out, seen = [], set()
    for row in ww.ROWS:
        for pname in row.psets:
            for kind, b in ww.solves(row):
                key = (row.geom, row.W, row.H, pname, kind, b)
                if key not in seen:
                    seen.add(key)
                    out.append(pytest.param(row, pname, kind, b, id=f"{row.geom}-{row.W}x{row.H}-{pname}-{kind}-{b}"))
    return out


@pytest.mark.parametrize("row,pname,kind,b", _solve_ids())
def test_reference_is_finite_sensitive_and_clear_of_the_thresholds(built, row, pname, kind, b):
    p = row.psets[pname]
    u, v, st, wi = ww.reference(row, pname, kind, b, 0)
    uf, vf, stf, wif = ww.reference(row, pname, kind, b, 2)
    for a in (u, v, uf, vf):
        assert np.isfinite(a).all()
    assert st["sizes"] == [(row.W, row.H)] and wi.shape == (1, p["warps"])
    np.testing.assert_array_equal(wi, wif)
    # a gather one pixel off: I1 rolled by a column, by a row
    for roll in ((0, 1), (1, 0)):
        ur, vr, _, _ = ww.reference(row, pname, kind, b, 0, roll)
        same = (u.view(np.uint32) == ur.view(np.uint32)) & (v.view(np.uint32) == vr.view(np.uint32))
        assert same.mean() <= MAX_KEEP, (roll, int(same.sum()), same.size)
    if p.get("epsilon", 0.01) == 0:
        assert np.all(wi == p["iterations"])
        return
    I0, I1 = ww.frames(row, b)
    for math in (0, 2):
        tr = checker.oracle_check_trace(I0, I1, capi.make_params(fast_math=math, **p),
                                        init=ww.make_seed(row.geom, kind, row.W, row.H))[4]
        assert len(tr) >= p["warps"]
        m = checker.check_margins(tr, p["iterations"])
        assert m.min() >= MIN_MARGIN, (math, float(m.min()), tr[np.argmin(m)])


def test_middle_branch_shares(built):
    """lambda 0.05: a few percent of the px take TH's middle branch (the output carries I1wx and
    I1wy); lambda 5: most do (rho's value reaches it too) -- measured on the oracle's stages at
    the first warp of the ring's 193 x 41 seeds."""
    import initflow_ref as ref
    lib = ref._lib()
    row = ww.ROW_OF["k_warp_ring"]
    I0, I1 = ww.frames(row)
    h, w = I0.shape
    f0, f1 = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    lib.orc_convert_u8(capi._u8_ptr(np.ascontiguousarray(I0)), w, w, h, ref._p(f0))
    lib.orc_convert_u8(capi._u8_ptr(np.ascontiguousarray(I1)), w, w, h, ref._p(f1))
    gx, gy = np.empty_like(f0), np.empty_like(f0)
    lib.orc_centered_gradient(ref._p(f1), w, h, ref._p(gx), ref._p(gy))
    for kind in ww.KINDS:
        u, v = (np.ascontiguousarray(a) for a in ww.make_seed(row.geom, kind, w, h))
        wxo, wyo, grad, rho = (np.empty_like(f0) for _ in range(4))
        lib.orc_warp_backward(ref._p(f0), ref._p(f1), ref._p(gx), ref._p(gy), ref._p(u), ref._p(v), w, h,
                              ref._p(wxo), ref._p(wyo), ref._p(grad), ref._p(rho))
        r = rho + (wxo * u + wyo * v)
        share = {lam: float((np.abs(r) <= np.float32(lam * 0.3) * grad).mean()) for lam in (0.05, 5.0)}
        print(kind, share)
        assert share[0.05] < 0.25 and share[5.0] > 0.6, (kind, share)
