"""tests/dualtvl1_cases.py held to the planner and to the oracle, with no GPU.

tests/test_gpu_dualtvl1_edges.py runs that table bitwise against the oracle.  It would be vacuous
if a size no longer sat on the edge it names, flaky if a stopping decision sat within the
residual's accumulation error of its threshold, and blind if the frames never sent the remap
through a branch or if a slipped tap left the flow unchanged.  So here

  * the planner (tests/plan_dump.cpp, csrc/tvl1_plan.hpp) is asked for k_iterate's wave segments
    and strips at every iterate size and for the pyramid of every pyramid case, and the launch
    block is read from the engine's source: each case must still sit on its edge -- which side
    of a 0.5 level rounds up, which 0.98 levels are equal;
  * profile 1 compares (float) error > scaledEps after every iteration; the engine sums
    per-block double partials, the oracle per-row doubles.  Every check of every stopping-rule
    case must keep |error / scaledEps - 1| >= MIN_MARGIN (test_residual_margin_cpu), no case
    left out;
  * the oracle's remap census (orc_set_remap_census) must show >= 100 px in each of its six
    classes over the remap group, a fully-outside px in the tiny case alone, and no interior px
    in the degenerate group (but at 4 x 5 and 5 x 4, which have two interior tap origins); the
    counts go to profiles/dualtvl1_edges/census.json;
  * the oracle's flow of every remap and pyramid case must change at >= 99 % of px when frame1
    is rolled by one px, so a kernel that read a neighbouring tap or level could not pass;
  * the oracle's result of a 0.5 odd case must not depend on what an earlier solve left behind.
"""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

import dualtvl1_cases as dc
from optflow_amd import capi
from oracle import checker
from test_edge_cases_cpu import counts, q
from test_plan_cpu import dump  # noqa: F401  (the module-scoped plan_dump fixture)
from test_residual_margin_cpu import MIN_MARGIN

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fibsem-optflow_amd" / "csrc"
CENSUS_JSON = ROOT / "profiles" / "dualtvl1_edges" / "census.json"
MIN_CLASS = 100     # px per census class over the remap group
MAX_KEEP = 0.01     # share of px whose flow may survive a rolled frame1


# ---------------------------------------------------------------- the table itself
def test_table_is_small_unique_and_complete():
    names = [c.name for c in dc.CASES]
    assert len(names) == len(set(names))
    assert {c.group for c in dc.CASES} == set(dc.GROUPS)
    for c in dc.CASES:
        p = c.params
        assert p["warps"] <= 3 and p["inner_iterations"] <= 5 and p["outer_iterations"] <= 2, c.name
        assert c.W <= 497 and c.W * c.H <= 128 * 96, c.name
        assert dc.params_of(c).profile == 1
    for g, sizes, n in (("iterate-x", {(w, dc.X_H) for w in dc.X_WIDTHS}, 5), ("iterate-y", {(dc.Y_W, h) for h in dc.Y_HEIGHTS}, 3)):
        cs = dc.cases_of(g)
        assert {(c.W, c.H) for c in cs} == sizes and len(sizes) == n
        assert all(c.params["nscales"] == 1 for c in cs)
        for W, H in sizes:   # the four instantiations, each with the stopping rule and with fixed work
            got = {(c.params.get("gamma", 0.0) != 0, c.params.get("tau", 0.25) < 0, c.params.get("epsilon", 0.01))
                   for c in cs if (c.W, c.H) == (W, H)}
            assert got >= {(g_, t, e) for g_ in (False, True) for t in (False, True) for e in (0.01, 0.0)}, (W, H)
    assert dc.X_WIDTHS == [247, 248, 249, 496, 497] and dc.Y_HEIGHTS == [31, 32, 33]
    deg = dc.cases_of("degenerate")
    assert {(c.W, c.H) for c in deg} == set(dc.DEGENERATE) and len(deg) == 3 * len(dc.DEGENERATE)
    assert {c.params["median_filtering"] for c in deg} == {1, 3, 5}
    assert all(min(c.W, c.H) <= 3 or (c.W, c.H) in ((4, 5), (5, 4)) for c in deg)
    pyr = dc.cases_of("pyramid")
    assert all(c.params["nscales"] in (3, 4) for c in pyr)
    assert {(c.W, c.H) for c in pyr if c.params["scale_step"] == 0.5} == \
        {(35, 36), (36, 35), (35, 35), (39, 67), (70, 70), (33, 37), (128, 96)}
    assert set(dc.ODD_HALF) == {(35, 36), (36, 35), (35, 35), (39, 67), (70, 70)}
    assert {(c.W, c.H, c.params["scale_step"]) for c in pyr if c.params["scale_step"] != 0.5} >= \
        {(20, 20, 0.98), (50, 20, 0.98), (65, 21, 0.75), (81, 17, 0.75), (65, 21, 0.9), (81, 17, 0.9),
         (155, 25, 0.8), (100, 25, 0.8)}
    assert any(c.params.get("gamma") == 0.2 and (c.W, c.H) == (100, 25) for c in pyr)
    assert any(c.params.get("median_filtering") == 5 and c.params["scale_step"] == 0.8 for c in pyr)
    rm = dc.cases_of("remap")
    assert {c.shift for c in rm if (c.W, c.H) == dc.REMAP_SIZE} == {(6, 0), (-6, 0), (0, 6), (0, -6), (7, -5)}
    assert [(c.W, c.H, c.params["nscales"], c.params["warps"]) for c in rm if (c.W, c.H) != dc.REMAP_SIZE] == [(12, 10, 1, 3)]
    assert all(c.params["nscales"] == 3 for c in rm if (c.W, c.H) == dc.REMAP_SIZE)
    # a translated pair really is one: frame1(x + d) = frame0(x) where both exist
    c = dc.case("remap-64x48-shift7,-5")
    I0, I1 = dc.frames(c)
    assert np.array_equal(I1[0:c.H - 5, 7:], I0[5:, :c.W - 7])


# ---------------------------------------------------------------- geometry
def launch_block():
    """kBlk2 and grid2 of the engine: the block of k_gradient, k_remap_cubic, k_median, k_resize_hp."""
    eng = (CSRC / "tvl1_engine.hip").read_text()
    m = re.search(r"static const dim3 kBlk2\((\d+), (\d+), 1\);", eng)
    assert m, "kBlk2 not found in tvl1_engine.hip"
    bx, by = int(m.group(1)), int(m.group(2))
    assert f"return dim3((unsigned)((w + {bx - 1}) / {bx}), (unsigned)((h + {by - 1}) / {by}), (unsigned)z);" in eng
    for k in ("k_gradient, grid2(lw, lh), kBlk2", "k_remap_cubic, grid2(lw, lh), kBlk2",
              "k_median, grid2(lw, lh, 2), kBlk2", "k_resize_hp, grid2(g.ws[s], g.hs[s], 2), kBlk2",
              "k_resize_hp, grid2(dw, dh, gam ? 3 : 2), kBlk2"):
        assert k in eng, k
    return bx, by


def test_iterate_sizes_straddle_the_wave_segment_and_the_strip(dump):
    got = counts(dump, [q(("iterate",), w, dc.X_H) for w in dc.X_WIDTHS])
    assert [c[0] for c in got] == [1, 1, 2, 2, 3]
    got = counts(dump, [q(("iterate",), dc.Y_W, h) for h in dc.Y_HEIGHTS])
    assert [c[1] for c in got] == [1, 1, 2]
    assert dc.X_WIDTHS == [dc.X_B - 1, dc.X_B, dc.X_B + 1, 2 * dc.X_B, 2 * dc.X_B + 1]
    assert dc.Y_HEIGHTS == [dc.Y_B - 1, dc.Y_B, dc.Y_B + 1]
    bx, by = launch_block()
    assert (bx, by) == dc.BLOCK
    assert dc.Y_W == bx + 1 and dc.X_H == 2 * by + 1       # a one-px second block, a one-row third
    assert {h % by for h in dc.Y_HEIGHTS} == {3, 0, 1}


def _up_sides(sizes):
    """Per pyramid step, the sides whose destination is more than half the source: the 2x path's
    last column / row there has one source column / row."""
    return [{s for s, a, b in (("w", w0, w1), ("h", h0, h1)) if 2 * b > a}
            for (w0, h0), (w1, h1) in zip(sizes, sizes[1:])]


def upsample_ends(lw, dw):
    """(first column clamped, last column a single tap) of k_resize_hp's bilinear branch."""
    scale = 1.0 / (dw / lw)
    f0 = np.float32(0.5 * scale - 0.5)
    fl = np.float32((dw - 1 + 0.5) * scale - 0.5)
    return bool(np.floor(f0) < 0), bool(int(np.floor(fl)) + 1 >= lw)


def test_pyramid_cases_have_the_levels_they_were_chosen_for(dump):
    rows = dc.PYRAMIDS
    out = dump([f"pyr {w} {h} {ns} {step}" for w, h, step, ns, _, _, _ in rows])
    bx, _ = launch_block()
    for (w, h, step, ns, _, sizes, note), o in zip(rows, out):
        v = [int(x) for x in o.split()]
        L = v[0]
        assert list(zip(v[1:1 + L], v[1 + L:])) == sizes, (w, h, step)
        if step == 0.5:
            assert _up_sides(sizes) == note["up"], (w, h)
            for (w0, h0), (w1, h1) in zip(sizes, sizes[1:]):   # a side rounds up iff it is 3 mod 4
                assert (2 * w1 > w0) == (w0 % 4 == 3) and (2 * h1 > h0) == (h0 % 4 == 3)
        if note.get("equal"):
            assert len(set(sizes)) == 1 and L == ns >= 3
        if note.get("equal_h"):
            assert len({s[1] for s in sizes}) == 1 and len({s[0] for s in sizes}) == L >= 3
        if note.get("equal_w"):
            assert len({s[0] for s in sizes}) == 1 and len({s[1] for s in sizes}) == L >= 3
        if note.get("single_tap"):
            assert L >= 2
            for (w0, _), (w1, _) in zip(sizes, sizes[1:]):
                assert upsample_ends(w1, w0) == (True, True), (w, h, step)
        if note.get("straddle"):
            ws = [s[0] for s in sizes]
            assert max(ws) > bx >= min(ws), (w, h, step)   # level widths on both sides of the block
    # the 0.5 neighbours: a size that rounds down, and the all-even control
    assert any(step == 0.5 and not any(n["up"]) and w % 2 for w, h, step, _, _, _, n in rows)
    assert any(step == 0.5 and not any(n["up"]) and w % 2 == 0 and h % 2 == 0 for w, h, step, _, _, _, n in rows)
    assert any(step == 0.5 and n["up"][0] == set() and any(n["up"][1:]) for w, h, step, _, _, _, n in rows)
    assert {tuple(sorted(u)) for *_, n in rows if "up" in n for u in n["up"]} >= {("w",), ("h",), ("h", "w"), ()}


# ---------------------------------------------------------------- the oracle and the margins
def profile1_margins(trace):
    """|error / scaledEps - 1| per check.  A non-finite ratio (tau < 0 overflowing) is infinitely
    far: a sum of squares that holds an inf or a NaN is inf or NaN in every accumulation order."""
    r = trace[:, 3]
    return np.where(np.isfinite(r), np.abs(r - 1.0), np.inf)


def expected_levels(c):
    return dc.pyramid_row(c)[5] if c.group == "pyramid" else None


@pytest.mark.parametrize("group", dc.GROUPS)
def test_oracle_defines_every_case_and_margins_hold(built, group):
    cases = dc.cases_of(group)
    checked, low = 0, np.inf
    for c in cases:
        p = dc.params_of(c)
        u, v, st, wi, tr = checker.oracle_check_trace(*dc.frames(c), p)
        if c.params.get("tau", 0.25) >= 0:
            assert np.isfinite(u).all() and np.isfinite(v).all(), c.name
        if c.group == "pyramid":
            assert st["sizes"] == expected_levels(c), c.name
        elif c.params["nscales"] == 1:
            assert st["sizes"] == [(c.W, c.H)], c.name
        cap = p.inner_iterations * p.outer_iterations
        assert wi.shape == (st["levels"], p.warps) and wi.min() >= 1 and wi.max() <= cap, (c.name, wi)
        assert len(tr) == st["checks_total"] == st["iterations_total"] == int(wi.sum()), c.name
        if not dc.stops(c):
            assert np.all(wi == cap), c.name
            continue
        m = profile1_margins(tr)
        assert m.min() >= MIN_MARGIN, (c.name, float(m.min()), tr[np.argmin(m)])
        # the trace is the schedule: a warp ends at its first ratio <= 1 (or not > 1: NaN), or at the cap
        for lv in range(st["levels"]):
            for wp in range(p.warps):
                r = tr[(tr[:, 0] == lv) & (tr[:, 1] == wp), 3]
                assert len(r) == wi[lv, wp] and np.all(r[:-1] > 1) and (len(r) == cap or not r[-1] > 1), c.name
        low = min(low, float(m.min()))
        checked += 1
    print(f"{group}: minimum stopping margin {low:.3g} over {checked} stopping-rule cases")
    assert checked == sum(dc.stops(c) for c in cases) > 0   # the share of cases left out is zero


def test_some_warp_of_every_iterate_size_stops_on_the_residual(built):
    """Otherwise the residual the kernels sum at these sizes would decide nothing."""
    for g in ("iterate-x", "iterate-y"):
        for W, H in sorted({(c.W, c.H) for c in dc.cases_of(g)}):
            early = 0
            for c in dc.cases_of(g):
                if (c.W, c.H) == (W, H) and dc.stops(c):
                    p = dc.params_of(c)
                    wi = checker.oracle_calc(*dc.frames(c), p)[3]
                    early += int((wi < p.inner_iterations * p.outer_iterations).sum())
            assert early > 0, (W, H)


# ---------------------------------------------------------------- the remap census
def census_of(c):
    cen = checker.oracle_remap_census(*dc.frames(c), dc.params_of(c))[4]
    return dict(zip(checker.CENSUS_CLASSES, (int(x) for x in cen.sum(axis=0)))), len(cen)


def test_remap_census(built):
    out = {"classes": list(checker.CENSUS_CLASSES), "remap": {}, "degenerate": {}}
    total = dict.fromkeys(checker.CENSUS_CLASSES, 0)
    for c in dc.cases_of("remap"):
        cen, calls = census_of(c)
        p = dc.params_of(c)
        assert calls == p.warps * (1 if p.nscales == 1 else 2), c.name   # one remap per warp and level
        out["remap"][c.name] = cen
        for k, v in cen.items():
            total[k] += v
        if (c.W, c.H) != dc.REMAP_SIZE:
            assert cen["outside"] >= 1, (c.name, cen)
    out["remap_total"] = total
    assert all(v >= MIN_CLASS for v in total.values()), total
    for c in dc.cases_of("degenerate"):
        cen, calls = census_of(c)
        out["degenerate"][c.name] = cen
        assert calls == 3, c.name
        if min(c.W, c.H) <= 3:   # imax(W - 3, 0) = 0 or imax(H - 3, 0) = 0: no interior px can be
            assert cen["interior"] == 0, (c.name, cen)
        else:                    # 4 x 5, 5 x 4: (W - 3)(H - 3) = 2 interior tap origins beside the rest
            assert 0 < cen["interior"] < 3 * c.W * c.H, (c.name, cen)
        # every px of every call is outside or partial, and a partial px misses a side
        assert cen["outside"] + cen["left"] + cen["right"] + cen["top"] + cen["bottom"] >= 3 * c.W * c.H, (c.name, cen)
    text = json.dumps(out, indent=1) + "\n"
    print(json.dumps(total))
    try:   # the record beside the README (unchanged on a clean checkout: the counts are deterministic)
        if not CENSUS_JSON.exists() or CENSUS_JSON.read_text() != text:
            CENSUS_JSON.parent.mkdir(parents=True, exist_ok=True)
            CENSUS_JSON.write_text(text)
    except OSError:
        pass


# ---------------------------------------------------------------- sensitivity
SENSITIVE = dc.cases_of("remap") + dc.cases_of("pyramid")


@pytest.mark.parametrize("c", SENSITIVE, ids=[c.name for c in SENSITIVE])
def test_flow_is_sensitive_to_a_one_px_slip(built, c):
    p = dc.params_of(c)
    I0, I1 = dc.frames(c)
    u, v, _, _ = checker.oracle_calc(I0, I1, p)
    for axis in (1, 0):
        ur, vr, _, _ = checker.oracle_calc(I0, np.roll(I1, 1, axis=axis), p)
        same = (u.view(np.uint32) == ur.view(np.uint32)) & (v.view(np.uint32) == vr.view(np.uint32))
        assert same.mean() <= MAX_KEEP, (axis, int(same.sum()), same.size)


# ---------------------------------------------------------------- history independence
def test_oracle_odd_half_cases_do_not_depend_on_history(built):
    """A 2x step over an odd level once read past the source plane (a heap overflow in the
    oracle): the result then hung on what the allocator held.  Solve each such case, fill the
    heap differently (a constant-200 pair of a larger size, then a noise pair), and solve again."""
    cases = [c for c in dc.CASES if dc.is_odd_half(c)]
    assert {(c.W, c.H) for c in cases} == set(dc.ODD_HALF)
    big = np.full((192, 256), 200, np.uint8)
    noise = np.random.default_rng(7).integers(0, 256, (192, 256), dtype=np.uint8)
    pbig = capi.make_params(profile=1, nscales=3, warps=1, inner_iterations=2, outer_iterations=1, scale_step=0.5)
    for c in cases:
        p = dc.params_of(c)
        I0, I1 = dc.frames(c)
        u0, v0, _, w0 = checker.oracle_calc(I0, I1, p)
        checker.oracle_calc(big, big, pbig)
        u1, v1, _, w1 = checker.oracle_calc(I0, I1, p)
        checker.oracle_calc(noise, noise[::-1].copy(), pbig)
        u2, v2, _, w2 = checker.oracle_calc(I0, I1, p)
        for ua, va, wa in ((u1, v1, w1), (u2, v2, w2)):
            assert np.array_equal(wa, w0), c.name
            assert np.array_equal(ua.view(np.uint32), u0.view(np.uint32)), c.name
            assert np.array_equal(va.view(np.uint32), v0.view(np.uint32)), c.name
