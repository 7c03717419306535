"""tests/edge_cases.py held to the planner and to the oracle, with no GPU.

tests/test_gpu_edge_cases.py runs that table bitwise against the oracle.  It would be vacuous
if a size no longer sat on a kernel's edge, and flaky if a stopping decision of one of its
cases sat within the residual's accumulation error of a threshold.  So here

  * tests/plan_dump.cpp (built as tests/test_plan_cpu.py builds it) is asked for the launch
    plan of every edge size: bands / tiles / segments / block rows must step exactly between a
    period B and B + 1 and not between B - 1 and B, for every kernel a group names -- the
    periods of edge_cases.py are confirmed by csrc/tvl1_plan.hpp itself;
  * the oracle must give finite flow and per-warp counts in [1, iterations] for every case,
    single and batched, IEEE and fma, and the level sizes the pyramid cases were chosen for;
  * every stopping-rule case must clear test_residual_margin_cpu.MIN_MARGIN, none left out;
  * edge_cases.sched_after must be tvl1_plan.hpp's.
"""
from __future__ import annotations

import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import edge_cases as ec
from optflow_amd import capi
from oracle import checker
from test_plan_cpu import dump  # noqa: F401  (the module-scoped plan_dump fixture)
from test_residual_margin_cpu import MIN_MARGIN

CSRC = Path(__file__).resolve().parent.parent / "fibsem-optflow_amd" / "csrc"
SLOTS = (1024, 16384)   # resident wavefronts of a launch on the device, low and high


def warp_img_tile():
    """k_warp_img's tile, read from the kernel's constants and the launch that uses them."""
    m = re.search(r"constexpr int kWarpTW = (\d+), kWarpTH = (\d+),", (CSRC / "tvl1_kernels.hpp").read_text())
    assert m, "kWarpTW / kWarpTH not found in tvl1_kernels.hpp"
    eng = (CSRC / "tvl1_engine.hip").read_text()
    assert "tx = (lw + kWarpTW - 1) / kWarpTW, ty = (lh + kWarpTH - 1) / kWarpTH" in eng
    assert "x0 = bx * kWarpTW, y0 = by * kWarpTH" in (CSRC / "tvl1_kernels.hpp").read_text()
    return int(m.group(1)), int(m.group(2))


def counts(dump, queries):
    """(pieces in x, pieces in y) the planner cuts a level into, per query (probe, w, h, roll_seg,
    pairs, seg_min, slots): bands and segments of a streaming site, tiles_x and block rows of a
    blocked pass, wave segments and strips of k_iterate, tiles of k_warp_img."""
    lines, take = [], []
    for probe, w, h, roll_seg, pairs, seg_min, slots in queries:
        if probe[0] == "site":
            _, name, k, px = probe
            lines.append(f"site {name} {w} {h} {k} {px} {slots} 100 {roll_seg} {pairs} {seg_min}")
            take.append(("site", len(lines) - 1))
        elif probe[0] in ("tb", "tb4"):
            lines.append(f"blocked {w} {h} {probe[1]}")
            take.append((probe[0], len(lines) - 1))
        elif probe[0] == "iterate":
            # iterate_blocks = ceil(segments * strips / 4): 4 strips (128 rows) make the blocks
            # count the segments of w, 4 segments (992 px) make them count the strips of h
            lines += [f"blocked {w} 128 1", f"blocked 992 {h} 1"]
            take.append(("iterate", len(lines) - 2))
        else:
            assert probe[0] == "warp_img"
            take.append(("warp_img", (w, h)))
    out = [[int(x) for x in o.split()] for o in dump(lines)] if lines else []
    res = []
    for kind, i in take:
        if kind == "site":
            bands, _, waves = out[i]
            assert waves % bands == 0
            res.append((bands, waves // bands))
        elif kind in ("tb", "tb4"):
            tiles_x, out_h, blocks = out[i][1:4] if kind == "tb" else out[i][4:7]
            assert blocks % tiles_x == 0
            res.append((tiles_x, blocks // tiles_x))
        elif kind == "iterate":
            res.append((out[i][0], out[i + 1][0]))
        else:
            tw, th = warp_img_tile()
            res.append((-(-i[0] // tw), -(-i[1] // th)))
    return res


def q(probe, w, h, roll_seg=ec.SEG, pairs=1, seg_min=0, slots=4096):
    return (probe, w, h, roll_seg, pairs, seg_min, slots)


# ---------------------------------------------------------------- the table itself
def test_table_is_small_unique_and_complete():
    names = [c.name for c in ec.CASES + ec.BATCH_CASES]
    assert len(names) == len(set(names))
    for c in ec.CASES + ec.BATCH_CASES:
        assert c.W <= 497 and c.H <= 45 or c.group.endswith("degenerate"), c.name
        assert c.W * c.H <= 497 * 45 and c.params["iterations"] <= 40, c.name
    assert {c.group for c in ec.CASES} == set(ec.GROUPS) == set(ec.KNOBS_OF)
    assert {c.group for c in ec.BATCH_CASES} == set(ec.BATCH_GROUPS)
    for g, (B, psets, _, _) in ec.X_GROUPS.items():
        assert {(c.W, c.H) for c in ec.cases_of(g)} == {(w, ec.X_H) for w in (B - 1, B, B + 1, 2 * B, 2 * B + 1)}
        assert len(ec.cases_of(g)) == 5 * len(psets)
    for g, (hs, psets, probes, _) in ec.Y_GROUPS.items():
        assert {(c.W, c.H) for c in ec.cases_of(g)} == {(ec.Y_W, h) for h in hs}
        for _, o in probes:   # every period has its three heights in the group
            assert {o - 1, o, o + 1} <= set(hs), (g, o)
    assert {(c.W, c.H) for c in ec.cases_of("degenerate")} == set(ec.DEGENERATE)
    assert {(c.W, c.H) for c in ec.batch_cases_of("batch-degenerate")} == set(ec.DEGENERATE)
    assert {(c.W, c.H) for c in ec.cases_of("corner")} == set(ec.CORNERS)
    # every pass length 1..4 among the fixed-work schedules, and a stopping-rule set per size
    ks = set()
    for p in (ec.FIX10, ec.FIX7, ec.FIX1):
        ks |= set(ec.fixed_work_passes(p["iterations"], 4))
    assert ks == {1, 2, 3, 4}
    assert ec.fixed_work_passes(10, 4) == [4, 4, 2] and ec.fixed_work_passes(7, 4) == [4, 3]
    assert ec.fixed_work_passes(1, 4) == [1] and ec.fixed_work_passes(7, 1) == [1] * 7
    assert ec.kmax_of(ec.TAU["stop-tau"]) == 1 and ec.kmax_of(ec.STOP) == 4 and ec.kmax_of(ec.GAMMA["stop-gamma"]) == 4
    # the streaming y edges always run with TVL1_ROLL_SEG=8 (TVL1_BUF_LIMIT=0 takes no streaming kernel)
    for kn in ec.KNOBS_OF["y-stream"]:
        assert "TVL1_ROLL_SEG=8" in kn.split(",") or kn == "TVL1_BUF_LIMIT=0"


# ---------------------------------------------------------------- x edges
def test_x_sizes_straddle_the_planner_bands(dump):
    """W in {B-1, B, B+1, 2B, 2B+1}: 1, 1, 2, 2, 3 bands (tiles, wave segments) of every kernel of
    the group, at the cases' own height and TVL1_ROLL_SEG."""
    qs, who = [], []
    for g, (B, _, probes, _) in ec.X_GROUPS.items():
        for probe in probes:
            for w in ec.x_widths(B):
                qs.append(q(probe, w, ec.X_H))
                who.append((g, probe))
    for B, probes in ec.BATCH_X.items():
        for probe, sl, seg_min in itertools.product(probes, SLOTS, (8, 128)):
            for w in ec.x_widths(B):
                qs.append(q(probe, w, ec.X_H, roll_seg=0, pairs=ec.BATCH_N, seg_min=seg_min, slots=sl))
                who.append(("batch-x", probe))
    got = counts(dump, qs)
    for i in range(0, len(qs), 5):
        assert [c[0] for c in got[i:i + 5]] == [1, 1, 2, 2, 3], (who[i], [x[1] for x in qs[i:i + 5]])
    # H = 9 with TVL1_ROLL_SEG=8: two segments, the second one row
    for (g, probe), query, c in zip(who, qs, got):
        if g != "batch-x" and probe[0] == "site":
            assert c[1] == 2, (g, probe, query)
    widths = {c.W for c in ec.batch_cases_of("batch-x")}
    assert all(set(ec.x_widths(B)) <= widths for B in ec.BATCH_X)


# ---------------------------------------------------------------- y edges
def test_y_sizes_straddle_the_planner_segments(dump):
    """H in {o-1, o, o+1}: 1, 1, 2 segments (block rows, strips, tiles) of each kernel with
    period o; 2o-1, 2o, 2o+1: 2, 2, 3 where the group has them.  W = 65 is a one-px second band
    of the ring and a 9-px second tile of the blocked kernels."""
    qs, who = [], []
    for g, (hs, _, probes, _) in ec.Y_GROUPS.items():
        for probe, o in probes:
            for h in (o - 1, o, o + 1, 2 * o - 1, 2 * o, 2 * o + 1):
                qs.append(q(probe, ec.Y_W, h))
                who.append((g, probe, o, h in hs))
    got = counts(dump, qs)
    for i in range(0, len(qs), 6):
        g, probe, o, _ = who[i]
        assert [c[1] for c in got[i:i + 3]] == [1, 1, 2], (g, probe, o)
        if all(w[3] for w in who[i + 3:i + 6]):
            assert [c[1] for c in got[i + 3:i + 6]] == [2, 2, 3], (g, probe, o)
        if probe[0] in ("tb", "tb4", "warp_img") or probe[:2] == ("site", "warp_ring"):
            first = 56 if probe[0] in ("tb", "tb4") else 64   # the first piece ends there
            (a, _), (b, _) = counts(dump, [q(probe, first, o), q(probe, first + 1, o)])
            assert (a, b, got[i][0]) == (1, 2, 2), (g, probe)
    assert any(all(w[3] for w in who[i + 3:i + 6]) for i in range(0, len(qs), 6))


def test_batch_y_sizes_straddle_the_segment_floor(dump):
    """The batched launches at W = 65, three pairs: with TVL1_BATCH_SEG_MIN=8 a pass is cut into
    8-row segments (7, 8: one; 9, 15, 16: two; 17: three) and at the default 128 into none; the
    fused pass and the gather (no floor) are cut the same way."""
    for probe, sl in itertools.product(ec.BATCH_Y_PROBES, SLOTS):
        roll = probe[1] == "kb_roll"
        got = counts(dump, [q(probe, ec.Y_W, h, roll_seg=0, pairs=ec.BATCH_N, seg_min=8, slots=sl)
                            for h in ec.BATCH_Y])
        assert [c[1] for c in got] == [1, 1, 2, 2, 2, 3], (probe, sl)
        if roll:
            got = counts(dump, [q(probe, ec.Y_W, h, roll_seg=0, pairs=ec.BATCH_N, seg_min=128, slots=sl)
                                for h in ec.BATCH_Y])
            assert [c[1] for c in got] == [1] * 6, (probe, sl)
            assert got[0][0] == (2 if probe[3] == 1 else 1)   # 65 px: two 1-px-per-lane bands
    assert {c.H for c in ec.batch_cases_of("batch-y")} == set(ec.BATCH_Y)
    assert {c.W for c in ec.batch_cases_of("batch-y")} == {ec.Y_W}


# ---------------------------------------------------------------- corners
CORNER_PROBES = {   # size -> (probe of its x edge, probe of its y edge)
    (125, 41): (("site", "warp_iter", 8, 0), ("tb4", 4)),
    (249, 45): (("site", "roll", 2, 4), ("tb4", 2)),
    (57, 25): (("tb", 4), ("tb", 4)),
    (121, 9): (("site", "roll", 4, 2), ("site", "roll", 4, 2)),
}


def test_corners_sit_one_past_both_edges(dump):
    assert set(CORNER_PROBES) == set(ec.CORNERS)
    for (w, h), (px, py) in CORNER_PROBES.items():
        (a, _), (b, _), (_, c), (_, d) = counts(dump, [q(px, w - 1, h), q(px, w, h), q(py, w, h - 1), q(py, w, h)])
        assert (a, b, c, d) == (1, 2, 1, 2), (w, h)


# ---------------------------------------------------------------- pyramids, schedule
def test_pyramid_cases_have_the_levels_they_were_chosen_for(dump):
    out = dump([f"pyr {w} {h} {ns} 0.8" for w, h, ns, _ in ec.PYRAMIDS])
    for (w, h, ns, sizes), o in zip(ec.PYRAMIDS, out):
        v = [int(x) for x in o.split()]
        L = v[0]
        assert L == ns == len(sizes) and list(zip(v[1:1 + L], v[1 + L:])) == sizes, (w, h)
    assert any(ns >= 3 for _, _, ns, _ in ec.PYRAMIDS)
    assert {(c.W, c.H, c.params["nscales"]) for c in ec.cases_of("pyramid")} == {p[:3] for p in ec.PYRAMIDS}
    assert all(c.params["nscales"] == 1 for c in ec.CASES + ec.BATCH_CASES if c.group != "pyramid")


def test_sched_after_restatement_is_the_planners(dump):
    thr = 0.01 * 0.01 * 65 * 17
    prevs = [0.0, 0.3 * thr, thr, 1.7 * thr, 3.1 * thr, 50.3 * thr, -thr]
    cases = [(p, n, it, kmax, eps) for p in prevs for n in (0, 1, 2, 5, 38) for it in (1, 7, 10, 40)
             for kmax in (1, 4) for eps in (0, 1) if n < it]
    out = dump([f"sched {p.hex()} {thr.hex()} {n} {it} {kmax} {eps}" for p, n, it, kmax, eps in cases])
    for (p, n, it, kmax, eps), o in zip(cases, out):
        k, ce, pe = o.split()
        assert ec.sched_after(p, thr, n, it, kmax, eps) == (int(k), bool(int(ce)), float.fromhex(pe)), (p, n, it)


# ---------------------------------------------------------------- the oracle and the margins
def _check_oracle(name, I0, I1, params, math, levels):
    """Finite flow, counts in [1, iterations], the expected levels; the residual margin of a
    stopping-rule case.  Returns 1 if the margin was checked."""
    p = capi.make_params(fast_math=math, **params)
    u, v, st, wi, tr = checker.oracle_check_trace(I0, I1, p)
    assert np.isfinite(u).all() and np.isfinite(v).all(), name
    assert st["sizes"] == levels, name
    assert wi.shape == (len(levels), p.warps) and wi.min() >= 1 and wi.max() <= p.iterations, (name, wi)
    if p.epsilon == 0:
        assert len(tr) == 0 and np.all(wi == p.iterations), name
        return 0
    assert len(tr) == st["checks_total"] >= len(levels) * p.warps, name
    m = checker.check_margins(tr, p.iterations)
    assert m.min() >= MIN_MARGIN, (name, float(m.min()), tr[np.argmin(m)])
    return 1


def mid_check_candidates(cases, math):
    """Checks after which the engine, told to take every such continuation as a mid-check pass
    (TVL1_MID_MIN=1), launches k_iterate_roll_mid: not a warp's first check, 1 < r < 2 (the next
    pass is 2 iterations ending in a check) and 4 iterations left."""
    n_mid = 0
    for c in cases:
        if c.params.get("epsilon", 0.01) == 0 or c.params.get("gamma", 0.0) != 0:
            continue
        p = capi.make_params(fast_math=math, **c.params)
        tr = checker.oracle_check_trace(*ec.frames(c), p)[4]
        n_mid += sum(1 for _, _, n, r in tr if n > 2 and 1 < r < 2 and n + 4 <= p.iterations)
    return n_mid


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
def test_mid_check_knob_sets_reach_the_mid_check_pass(built, math):
    groups = [g for g in ec.GROUPS if any("TVL1_MID=1" in kn.split(",") for kn in ec.KNOBS_OF[g])]
    assert set(groups) == {"x120", "y-stream"}
    for g in groups:
        assert mid_check_candidates(ec.cases_of(g), math) > 0, g


def _levels(c):
    for w, h, ns, sizes in ec.PYRAMIDS:
        if (w, h, ns) == (c.W, c.H, c.params["nscales"]):
            return sizes
    return [(c.W, c.H)]


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("group", ec.GROUPS)
def test_oracle_defines_every_case_and_margins_hold(built, group, math):
    cases = ec.cases_of(group)
    checked = sum(_check_oracle(c.name, *ec.frames(c), c.params, math, _levels(c)) for c in cases)
    stopping = [c for c in cases if c.params.get("epsilon", 0.01) > 0]
    assert checked == len(stopping) > 0   # the share of cases left out for margin is zero


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("group", ec.BATCH_GROUPS)
def test_oracle_defines_every_batch_pair_and_margins_hold(built, group, math):
    cases = ec.batch_cases_of(group)
    checked = 0
    for c in cases:
        I0s, I1s = ec.batch_frames(c)
        assert I0s.shape == I1s.shape == (ec.BATCH_N, c.H, c.W)
        for b in range(ec.BATCH_N):
            checked += _check_oracle(f"{c.name} pair {b}", I0s[b], I1s[b], c.params, math, [(c.W, c.H)])
    stopping = [c for c in cases if c.params.get("epsilon", 0.01) > 0]
    assert checked == ec.BATCH_N * len(stopping) > 0


def test_mixed_batch_pairs_stop_at_different_passes(built):
    """The identical and the constant pair stop at every warp's first check, the textured pair
    runs on: one launch holds pairs at different points of their schedules."""
    for c in ec.batch_cases_of("batch-mixed"):
        I0s, I1s = ec.batch_frames(c)
        wi = [checker.oracle_calc(I0s[b], I1s[b], capi.make_params(**c.params))[3] for b in range(3)]
        assert np.all(wi[0] == 2) and np.all(wi[2] == 2) and wi[1].max() > 2, (c.name, wi)
