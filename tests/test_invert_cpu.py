"""Flow inversion without a GPU: the boundary (header, library, Engine), the numpy restatement
(tests/invert_ref.py) on the case table (tests/invert_cases.py), and the experiment of DESIGN 16
on the oracle alone.

  * the vectorised restatement equals a per-px loop, bit for bit;
  * a census shows that each kind of case has px in every class it is named for, and that the
    window-edge cases lie on the side of the edge they name (window_model restates the box rule
    from the constants of csrc/tvl1_invert.hpp);
  * constant integer flows invert to their negation with a zero residual, and the outside count
    has its closed form;
  * f composed with its inverse vanishes on the interior of a smooth flow;
  * on the zoom stack the negated chain is a poor seed for the backward pair and the inverse a
    good one, and the backward solve needs one of them.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import compose_ref as cref
import invert_cases as T
import invert_ref as ref
from optflow_amd import capi
from oracle import checker

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
MIN_MARGIN = 1e-4   # tests/test_residual_margin_cpu.py


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def case_named(prefix):
    return next(c for c in T.CASES if c.name.startswith(prefix))


def test_the_boundary_is_there(built):
    hdr = (ROOT / "include" / "tvl1.h").read_text()
    for sym in ("tvl1_invert_flow_batch", "tvl1_invert_flow"):
        assert re.search(r"tvl1_status\s+%s\(" % sym, hdr), sym
    assert re.search(r"uint64_t outside, unconverged;\s*}\s*tvl1_invert_counts;", hdr)
    lib = capi.load_engine()
    assert lib.tvl1_invert_flow_batch and lib.tvl1_invert_flow
    for m in ("invert_flow", "invert_flow_batch", "invert_flow_host"):
        assert callable(getattr(capi.Engine, m))
    import inspect
    assert "inverse" in inspect.signature(capi.Engine.calc_chained_host).parameters
    assert {"kInvTileW", "kInvTileH", "kInvDrift", "kInvWinFloats", "kInvMaxIter"} <= set(T.CONST)
    assert T.MAX_ITER == 32 and (T.TILE_W, T.TILE_H) == (256, 4)


@pytest.mark.parametrize("name", ["67x45-smooth", "67x45-special", "67x45-edges_out"])
def test_the_vectorised_restatement_is_the_per_px_loop(name):
    case = case_named(name)
    u, v = (p[0] for p in T.planes(case))
    ug, vg, rs, outside, unconv = ref.invert(u, v, case.K, case.tol)
    lu, lv, lr, lin = ref.invert_px(u, v, case.K)
    assert same_bits(ug, lu) and same_bits(vg, lv) and same_bits(rs, lr)
    assert outside == int((~lin).sum())
    with np.errstate(invalid="ignore"):
        assert unconv == int((~(lr <= F(case.tol))).sum())


def test_each_kind_has_px_in_every_class_it_is_named_for():
    seen, ks = set(), {}
    tot = {}
    for case in T.CASES:
        uf, vf = (p[0] for p in T.planes(case))
        W, H, K = case.W, case.H, case.K
        ug, vg, rs, outside, unconv = ref.invert(uf, vf, K, case.tol)
        fixed = int((ref.fixed_at(uf, vf, K) < K).sum())
        big = W > 8 and H > 8
        t = tot.setdefault(case.kind, dict(inside=0, outside=0, conv=0, unconv=0, fixed=0, unfixed=0))
        t["inside"] += W * H - outside
        t["outside"] += outside
        t["conv"] += W * H - unconv
        t["unconv"] += unconv
        t["fixed"] += fixed
        t["unfixed"] += W * H - fixed
        ks.setdefault(case.kind, set()).add(K)
        _, _, in0, X0, Y0 = ref.step(uf, vf, -uf, -vf)   # the first landing
        if case.kind == "zero":
            assert outside == 0 and unconv == 0 and fixed == W * H
            assert not ug.any() and not vg.any() and not rs.any()
        elif case.kind == "integer":
            assert fixed == W * H and unconv == 0
        elif case.kind == "edges":
            k = (np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 8
            assert np.all(X0[k == 0] == 0) and np.all(X0[k == 1] == W - 1)
            assert np.all(Y0[k == 2] == 0) and np.all(Y0[k == 3] == H - 1)
            assert in0[k < 4].all()
        elif case.kind == "edges_out":
            k = (np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 8
            assert np.all(X0[k == 0] < 0) and np.all(X0[k == 0] > -1e-4)
            assert np.all(Y0[k == 2] < 0) and np.all(Y0[k == 2] > -1e-4)
            assert np.all(X0[k == 1] == np.nextafter(F(W - 1), F(np.inf)))
            assert np.all(Y0[k == 3] == np.nextafter(F(H - 1), F(np.inf)))
            assert not in0[k < 4].any()
        elif case.kind == "special":
            if W * H >= 7 * 12:   # every special value fits without landing on another
                for p in (uf, vf):
                    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
                    assert (np.abs(p) == F(1e30)).sum() == 2
                    assert ((p == 0) & np.signbit(p)).any()
                assert unconv > 0
                t["nan"] = t.get("nan", 0) + int(np.isnan(ug).sum()) * int(np.isnan(rs).sum())
        elif case.kind == "smooth" and big and K >= 8:
            assert unconv == 0 and 0 < outside < W * H // 2 and fixed > 0
        elif case.kind == "chain" and big:
            # the first landings are 25 and 18 px away: a window centred on the tile misses them
            assert np.all(np.abs(X0 - np.arange(W, dtype=F)[None, :]) > 20)
            assert 0 < outside < W * H
        elif case.kind == "fold" and big and K <= 2:
            assert unconv > W * H // 4
        seen.add(case.kind)
    assert seen == set(T.KINDS) | set(T.WINDOW_KINDS)
    for kind in T.KINDS:
        assert ks[kind] == set(T.KS), kind
    for kind in ("integer", "smooth", "chain", "edges", "special", "fold"):
        assert tot[kind]["inside"] and tot[kind]["outside"], kind
    for kind in ("smooth", "chain", "fold", "edges", "special"):
        assert tot[kind]["conv"] and tot[kind]["unconv"], kind
        assert tot[kind]["fixed"] and tot[kind]["unfixed"], kind
    assert tot["special"]["nan"]   # a special value of f is sampled, and reaches g and resid
    assert {c.K for c in T.CASES if c.roi and c.kind == "smooth"} == set(T.KS)
    assert any(c.roi and (4 * c.roi[2]) % 16 == 4 for c in T.CASES)
    assert any(c.n > 256 for c in T.CASES)


def test_a_folding_flow_stays_unconverged_at_any_k():
    case = case_named("257x131-fold")
    u, v = (p[0] for p in T.planes(case))
    seen = {}
    for K in (8, 32):
        rs, unconv = ref.invert(u, v, K, T.TOL)[2::2]
        print(f"K = {K}: {unconv} px unconverged, max residual {float(np.sqrt(rs.max())):.2f} px")
        seen[K] = unconv
        assert unconv > 0 and rs.max() > 1.0   # px off by more than 1 px at any K


def test_the_window_cases_lie_on_both_sides_of_each_edge():
    def model(kind):
        case = next(c for c in T.CASES if c.kind == kind)
        u, v = (p[0] for p in T.planes(case))
        ty = T.PROBE_NEAR[1] // T.TILE_H if "yneg" in kind else 0
        return case, T.window_model(u, v, case.K, 0, ty)

    # a box of exactly the budget is staged; one more row of it is not
    _, fit = model("box_fit")
    _, over = model("box_over")
    assert fit["floats"] == T.WIN_FLOATS and fit["on"]
    bw = over["box"][1] - over["box"][0] + 1
    assert over["floats"] == T.WIN_FLOATS + bw and not over["on"]
    # every other tile of those two cases, and every tile of the table's 25-px chains, fits
    case = case_named("257x131-chain")
    u, v = (p[0] for p in T.planes(case))
    for tx in range(2):
        for ty in range(0, 33, 8):
            assert T.window_model(u, v, 1, tx, ty)["on"]
    # the probe px: its sample 1 moves by exactly the drift margin (its far tap on the box's last
    # row or column, its near tap on the first) or by one more (outside: the global gather)
    for stem, axis in (("drift_y", 2), ("drift_yneg", 2), ("drift_x", 0)):
        for side in ("at", "over"):
            case, m = model(f"{stem}_{side}")
            assert m["on"]
            (px, py), q, r = T.drift_probe(case.kind)
            ox, oy = m["origin"]
            x0, x1, y0, y1 = (a[py - oy, px - ox] for a in m["taps"][1])
            assert (x0, y0) == r
            t0 = m["taps"][0]
            assert (t0[0][py - oy, px - ox], t0[2][py - oy, px - ox]) == q
            moved = (r[0] - q[0]) + (r[1] - q[1])
            assert abs(moved) == T.DRIFT + (side == "over")
            bx0, bx1, by0, by1 = m["box"]
            inb = m["in_box"][:, py - oy, px - ox]
            assert inb[0]
            if side == "at":
                assert inb[1]
                if stem == "drift_y":
                    assert y1 == by1
                elif stem == "drift_yneg":
                    assert y0 == by0
                else:
                    assert x1 == bx1
            else:
                assert not inb[1]
                if stem == "drift_y":
                    assert y1 == by1 + 1
                elif stem == "drift_yneg":
                    assert y0 == by0 - 1
                else:
                    assert x1 == bx1 + 1
            # and the rest of the block stays inside the box in every sample
            assert int((~m["in_box"]).sum()) == (side == "over")


@pytest.mark.parametrize("W,H,dx,dy", [(40, 30, 5, -3), (40, 30, -7, 0), (9, 6, 0, 2), (9, 6, 12, 1)])
def test_constant_integer_flows_invert_to_their_negation(W, H, dx, dy):
    u, v = np.full((H, W), dx, F), np.full((H, W), dy, F)
    for K in (1, 8):
        ug, vg, rs, outside, unconv = ref.invert(u, v, K, T.TOL)
        assert np.all(ug == -dx) and np.all(vg == -dy)
        assert outside == W * H - max(W - abs(dx), 0) * max(H - abs(dy), 0)
        _, _, inside, _, _ = ref.step(u, v, ug, vg)
        assert not rs[inside].any() and not rs.any() and unconv == 0
    for case in (c for c in T.CASES if c.kind == "integer"):
        dx, dy = T.integer_flow(case)
        uf, vf = (p[0] for p in T.planes(case))
        ug, vg, rs, outside, unconv = ref.invert(uf, vf, case.K, case.tol)
        assert np.all(ug == -dx) and np.all(vg == -dy) and not rs.any()
        assert outside == case.W * case.H - max(case.W - abs(dx), 0) * max(case.H - abs(dy), 0)


def test_a_flow_composed_with_its_inverse_vanishes():
    """compose(g, f) = g + f(y + g) on the 257x131 smooth 3-px case at K = 8, away from the frame
    edge by 8 px: the restatement gave max |.| = 3.50e-5 px when the case was chosen (0.136 at K = 1,
    0.0488 at K = 2, 4.1e-3 at K = 4, 4.3e-6 at K = 10); the bound is twice that."""
    case = case_named("257x131-smooth")
    u, v = (p[0] for p in T.planes(case))
    ug, vg, rs, _, _ = ref.invert(u, v, 8, T.TOL)
    cu, cv, _ = cref.compose(ug, vg, u, v)
    m = 8
    worst = max(float(np.abs(cu[m:-m, m:-m]).max()), float(np.abs(cv[m:-m, m:-m]).max()))
    print(f"max |compose(invert(f), f)| on the interior: {worst:.3e} px")
    assert worst < 2 * 3.50e-5
    # which is what the residual plane reports: resid = |g + f(y + g)|^2
    assert same_bits(rs, cu * cu + cv * cv)


@pytest.fixture(scope="module")
def zoom(built):
    """The zoom stack, the oracle's four link flows with their check traces, the restatement's
    chain and its inverse; computed once and never changed."""
    frames = T.zoom_frames()
    p = capi.make_params(**T.ZOOM_PARAMS)
    links, traces = [], []
    for k in range(T.ZOOM_FRAMES - 1):
        u, v, _, _, trace = checker.oracle_check_trace(frames[k], frames[k + 1], p)
        links.append((u, v))
        traces.append(trace)
    cu, cv, _ = cref.compose_chain(links)
    ug, vg, _, outside, unconv = ref.invert(cu, cv, 8, T.TOL)
    for a in (cu, cv, ug, vg):
        a.setflags(write=False)
    return frames, p, traces, (cu, cv), (ug, vg), (outside, unconv)


def test_the_inverse_seeds_the_backward_pair_where_the_negation_is_off(zoom):
    """Measured when the case was chosen (mean EPE against the true flow of the pair (4 -> 0), up
    to 30.7 px long): the negated chain 1.723 px, the inverse at K = 8 0.0326 px; the backward
    solve 21.2 px unseeded and 0.0778 px from the inverse (0.0776 from the negation: at this
    gradient the solver absorbs it)."""
    frames, p, _, (cu, cv), (ug, vg), (outside, unconv) = zoom
    e_neg = T.zoom_epe(-cu, -cv, 4, 0)
    e_inv = T.zoom_epe(ug, vg, 4, 0)
    unseeded = checker.oracle_calc(frames[4], frames[0], p)
    e_unseeded = T.zoom_epe(unseeded[0], unseeded[1], 4, 0)
    seeded = checker.oracle_calc(frames[4], frames[0], p, init=(ug, vg))
    e_seeded = T.zoom_epe(seeded[0], seeded[1], 4, 0)
    print(f"mean EPE: negated seed {e_neg:.4f}, inverse {e_inv:.4f}; backward solve unseeded "
          f"{e_unseeded:.3f}, from the inverse {e_seeded:.4f}; outside {outside}, unconverged {unconv}")
    assert e_neg > 0.5 * 1.723
    assert e_inv < 2 * 0.0326
    assert e_seeded < 0.5
    assert e_unseeded > 10.0
    assert 0 < outside < T.ZOOM_W * T.ZOOM_H // 4 and unconv < 100


def test_the_zoom_solves_clear_the_residual_margin(zoom):
    frames, p, traces, _, (ug, vg), _ = zoom
    trace = checker.oracle_check_trace(frames[4], frames[0], p, init=(ug, vg))[4]
    for k, t in enumerate(traces + [trace]):
        m = checker.check_margins(t, p.iterations)
        assert m.min() >= MIN_MARGIN, (k, t[np.argmin(m)])
