"""tests/extent_cases.py held to the source and to its own conditions, on the CPU: the sizes follow
from the constants the headers export, and every case's reference alone has content in the rows
that only a second row step writes (y >= ROWS_CAP) -- non-zero counts there, landings that cross
the cap both ways and clamp at the last row and column, a NaN and both infinities, scores on both
sides of beta, px of the inversion inside and outside its window.  So a row walk cut to its first
step cannot pass tests/test_gpu_extents.py, which compares these references with the GPU."""
import numpy as np
import pytest

import avgflow_ref
import compose_ref
import extent_cases as X
import fbcheck_ref
import invert_ref
import shift_ref
import zncc_ref
from optflow_amd import capi
from oracle import checker
from test_residual_margin_cpu import MIN_MARGIN

C = X.ROWS_CAP


def test_sizes_follow_from_the_sources_constants():
    assert X.FB_MAX_ROW_GROUPS == X.ZN_MAX_ROW_GROUPS == 65535
    assert (X.LANE_PX, X.GROUP_ROWS) == (4, 4)
    assert X.ROWS_CAP == 4 * 65535 == 262140
    assert X.H_TALL == 262149 and X.H_TALL > 4 * 65536
    # the second step: two full row groups and one of a single row
    assert divmod(X.H_TALL - X.ROWS_CAP, X.GROUP_ROWS) == (2, 1)
    assert X.W_THIN == 5 and X.W_THIN % X.LANE_PX == 1
    assert (X.MAP32_BITS, X.FLOATX_BITS, X.CANVAS_MAX, X.POST_BATCH_MAX, X.SHIFT_AREA_BITS) == (19, 24, 32767, 65535, 26)
    assert X.H_TALL <= 1 << X.FLOATX_BITS and X.H_TALL <= 1 << X.MAP32_BITS   # the headers accept it
    assert X.MAP32_TOP == 2 ** 24 - 32
    for c in X.REMAP_CASES:
        assert {c.W + 2 * X.REMAP_BORDER, c.H + 2 * X.REMAP_BORDER} == {X.CANVAS_MAX, 13}
    w, h = X.SHIFT_SIZE
    assert w * h <= 1 << X.SHIFT_AREA_BITS and h // 2 == X.ROWS_CAP + 8 and 4 * X.SHIFT_R <= w
    assert shift_ref.levels_of(X.SHIFT_R) == 1          # one k_shift_half level, of h / 2 rows
    assert X.HALF_SRC[1] // 2 > X.ROWS_CAP and X.HALF_SRC[0] // 2 == 4
    # the view: no row of a float plane is 16-byte aligned at its first px by pitch, and the first
    # px sits 4 bytes past a boundary
    aw, ah, first = X.VIEW
    assert (4 * aw) % 16 != 0 and (4 * first) % 16 == 4
    assert first % aw + X.W_THIN <= aw and first // aw + X.H_TALL <= ah


def test_pyramid_levels_are_over_the_cap(built):
    import initflow_ref
    for name in ("fix", "stop", "median", "init", "batch", "const", "profile1"):
        c = X.SOLVE_CASES[name]
        ws, hs = initflow_ref.pyramid_sizes(c.W, c.H, capi.make_params(**c.params))
        assert list(zip(ws, hs)) == X.PYR_LEVELS
        assert min(hs) > X.ROWS_CAP + X.GROUP_ROWS
    c = X.SOLVE_CASES["wide"]
    ws, hs = initflow_ref.pyramid_sizes(c.W, c.H, capi.make_params(**c.params))
    assert list(zip(hs, ws)) == X.PYR_LEVELS
    assert X.SOLVE_CASES["f32"].H == X.H_TALL


@pytest.mark.parametrize("b", [0, 1])
def test_row_walk_references_have_content_in_the_second_step(b):
    uf, vf, ub, vb = X.walk_planes(b)
    assert uf.shape == (X.H_TALL, X.W_THIN)
    tail = slice(C, None)
    # the specials sit in the second step, one in each row group
    assert np.isnan(vf[X.SPECIAL_ROWS["nan"]]).sum() == 1 and np.isposinf(uf[X.SPECIAL_ROWS["pinf"]]).sum() == 1
    assert np.isneginf(uf[X.SPECIAL_ROWS["ninf"]]).sum() == 1
    assert sorted((r - C) // X.GROUP_ROWS for r in X.SPECIAL_ROWS.values()) == [0, 1, 2]
    assert np.isfinite(uf[:C]).all() and np.isfinite(vf[:C]).all()

    # landings: across the cap both ways, on the last row and column, and beyond them
    Xl, Yl, inside = fbcheck_ref.landing(uf, vf)
    with np.errstate(invalid="ignore"):
        assert (Yl[:C] >= C).sum() > 0 and (Yl[tail] < C - 1).sum() > 0
        assert (inside[tail] & (Yl[tail] == X.H_TALL - 1)).sum() > 0
        assert (inside[tail] & (Xl[tail] == X.W_THIN - 1)).sum() > 0
        assert (Yl[tail] > X.H_TALL - 1).sum() > 0 and (Xl[tail] > X.W_THIN - 1).sum() > 0
        # a fractional landing row just under the cap blends a first-step row with a second-step one
        assert ((Yl > C - 1) & (Yl < C)).sum() > 0

    # tvl1_fb_score / tvl1_zero_above
    sc = fbcheck_ref.fb_score(uf, vf, ub, vb, X.ALPHA)
    with np.errstate(invalid="ignore"):
        acc = sc[tail] <= np.float32(X.BETA)
    assert acc.sum() > 0 and (~acc & np.isfinite(sc[tail])).sum() > 0
    assert np.isnan(sc[tail]).sum() > 0 and np.isposinf(sc[tail]).sum() > 0
    rejected_tail = fbcheck_ref.zero_above(uf[tail], vf[tail], sc[tail], X.BETA)[2]
    rejected = fbcheck_ref.zero_above(uf, vf, sc, X.BETA)[2]
    assert 0 < rejected_tail < rejected

    # tvl1_compose_flow
    uc, vc, outside = compose_ref.compose(uf, vf, ub, vb)
    outside_tail = int((~compose_ref.landing(uf, vf)[2][tail]).sum())
    assert 0 < outside_tail < outside
    assert np.isnan(uc[tail]).sum() + np.isnan(vc[tail]).sum() > 0

    # tvl1_invert_flow, K = 4
    ug, vg, rs, out, unc = invert_ref.invert(uf, vf, X.INV_K, X.INV_TOL)
    _, (_, _, ins) = invert_ref.iterates(uf, vf, X.INV_K)
    with np.errstate(invalid="ignore"):
        unc_tail = int((~(rs[tail] <= np.float32(X.INV_TOL))).sum())
    assert 0 < int((~ins[tail]).sum()) < out and 0 < unc_tail < unc
    with np.errstate(invalid="ignore"):
        assert (rs[tail] <= np.float32(X.INV_TOL)).sum() > 0
    # the window arm in the three row groups of the second step: staged with px that stay in the
    # box and the probe px that leaves it; not staged (a NaN lands at row 0: the box is the
    # plane); staged for a group of one row
    g0, g1, g2 = (X.invert_window_census(b, g) for g in range(3))
    assert g0["on"] and g0["in_box"].any() and (~g0["in_box"]).any()
    px, py = X.PROBE
    assert g0["in_box"][0, py - C, px] and not g0["in_box"][1, py - C, px]
    assert not g1["on"] and g1["floats"] > X.INV_WIN_FLOATS
    assert g2["on"] and g2["in_box"].shape[1] == 1

    # tvl1_warp_by_flow_u8
    J, m = zncc_ref.warp(X.walk_frame(b), uf, vf)
    assert m[tail].sum() > 0 and (~m[tail]).sum() > 0 and (J[tail] != 0).sum() > 0
    assert len(np.unique(J[tail][m[tail]])) > 8


@pytest.mark.parametrize("case", X.ZNCC_CASES, ids=[c.name for c in X.ZNCC_CASES])
def test_zncc_bound_cases_reach_the_top_of_the_map(case):
    I0, I1, u, v = X.zncc_planes(case)
    assert max(case.W, case.H) == X.MAP32_MAX == 1 << 19
    J, m = zncc_ref.warp(I1, u, v)
    with np.errstate(all="ignore"):
        if case.W > case.H:
            mx = np.arange(case.W, dtype=np.float32)[None, :] + u
        else:
            mx = np.arange(case.H, dtype=np.float32)[:, None] + v
        m32 = np.rint(mx * np.float32(32))
    # a px that lands on the far edge: 32 mx = 2^24 - 32, the largest value an inside px can have
    # (beyond it the px is outside and nothing is converted); one 1/32 px short of it; px beyond
    assert m32[m].max() == X.MAP32_TOP and (m32[m] == X.MAP32_TOP - 1).sum() > 0
    assert (m32 > X.MAP32_TOP).sum() > 0 and not m[m32 > X.MAP32_TOP].any()
    assert (m32[m] % 32 != 0).sum() > m.sum() // 2          # sub-pixel flows
    for r in X.ZNCC_RADII:
        sc = zncc_ref.score_from(J, m, I0, r)
        far = sc[:, -64:] if case.W > case.H else sc[-64:, :]
        assert np.isfinite(far).sum() > 0 and np.isposinf(far).sum() > 0
    if case.H > case.W:
        assert case.H > X.ROWS_CAP and m[C:].sum() > 0      # k_warp_flow_u8 walks rows here too


@pytest.mark.parametrize("case", X.REMAP_CASES, ids=[c.name for c in X.REMAP_CASES])
def test_remap_bound_cases_push_the_map_past_both_ends(case):
    frame, u, v = X.remap_planes(case)
    out = avgflow_ref.remap(frame, u, v, 1.0, X.REMAP_BORDER)
    assert sorted(out.shape) == [13, X.CANVAS_MAX]
    long_ = u if case.W > case.H else v
    n = max(case.W, case.H)
    with np.errstate(all="ignore"):
        m = np.arange(n, dtype=np.float32).reshape((1, n) if case.W > case.H else (n, 1)) - long_
    assert m.min() < -32768 and m.max() > 32767 + n          # the map saturates to short both ways
    assert (out != 0).sum() > out.size // 4 and (out == 0).sum() > 0


def test_postprocess_restatement_equals_the_oracles(built):
    import initflow_ref
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-3, 3, (2, 9, 7)).astype(np.float32)
    I1 = rng.integers(0, 4, (9, 7), dtype=np.uint8)
    for mode in (0, 1, 2):
        a, b = X.postprocess_numpy(u, v, I1, mode)
        ra, rb = initflow_ref.postprocess(u, v, I1, mode)
        assert np.array_equal(a.view(np.uint32), ra.view(np.uint32)) and np.array_equal(b.view(np.uint32), rb.view(np.uint32))
    u, v, I1 = X.post_batch_planes()
    assert u.shape == (X.POST_BATCH_MAX, 1, 1) and 0 < (I1 <= 1).sum() < I1.size


def test_the_shift_pair_has_its_planted_shift():
    I0, I1 = X.shift_pair()
    assert I0.shape == X.SHIFT_SIZE[::-1]
    r = shift_ref.estimate(I0, I1, X.SHIFT_R)
    assert (r["dx"], r["dy"]) == X.SHIFT_TRUE and r["levels"] == 2


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("name", X.STOPPING)
def test_stopping_rule_cases_keep_the_margin_and_end_by_a_check(built, name, math):
    c = X.SOLVE_CASES[name]
    p = capi.make_params(fast_math=math, **c.params)
    assert p.epsilon > 0
    _, _, st, wi, tr = checker.oracle_check_trace(*X.solve_frames(c), p)
    assert st["sizes"] == X.PYR_LEVELS
    m = checker.check_margins(tr, p.iterations)
    assert m.min() >= MIN_MARGIN, tr[np.argmin(m)]
    assert (wi < p.iterations).any() and (wi > 2).any(), wi   # a warp ends by a check, not the first


def test_every_other_solve_case_is_fixed_work():
    for name, c in X.SOLVE_CASES.items():
        if name not in X.STOPPING:
            assert c.params["epsilon"] == 0.0, name
