"""Flow composition without a GPU: the numpy restatement (tests/compose_ref.py) on the case
table (tests/compose_cases.py), the chain experiment on the oracle alone, and the HIP-free
planner stack.chain_links.

  * b = 0 gives c = a and a = 0 gives c = b, bit for bit;
  * a census shows that each kind of case reaches the edge it is named for;
  * on the five-frame stack the pair (0, 4) fails unseeded (mean EPE above 10 px) and solves
    from the numpy-composed chain of the oracle's four link flows (below 0.1 px); the oracle
    gave 22.97 and 0.017 px when the case was chosen;
  * the four link solves and the chained solve keep their stopping decisions at least the
    project's MIN_MARGIN from the thresholds, so the GPU comparison of test_gpu_compose.py can
    ask for equal iteration counts.
"""
import numpy as np
import pytest

import compose_cases as T
import compose_ref as ref
from optflow_amd import capi, stack
from oracle import checker

F = np.float32
MIN_MARGIN = 1e-4   # tests/test_residual_margin_cpu.py


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


@pytest.mark.parametrize("case", [c for c in T.CASES if c.n == 1], ids=lambda c: c.name)
def test_a_zero_flow_on_either_side_is_the_identity(case):
    ua, va, ub, vb = (p[0] for p in T.planes(case))
    z = np.zeros_like(ua)
    # b = 0: c = a + 0.  -0.0 + 0.0 is +0.0, the one value that is equal and not the same bits
    uc, vc, _ = ref.compose(ua, va, z, z)
    neg0 = lambda a: (a == 0) & np.signbit(a)
    for c, a in ((uc, ua), (vc, va)):
        assert same_bits(c[~neg0(a)], a[~neg0(a)])
        assert np.all(c[neg0(a)] == 0) and not np.signbit(c[neg0(a)]).any()
    # a = 0: every px lands on itself, ax = ay = 0, and s = p00 + 0 * (...) is p00 where the
    # neighbouring taps are finite; c = 0 + b
    if case.kind != "special":
        uc, vc, outside = ref.compose(z, z, ub, vb)
        assert outside == 0
        assert same_bits(uc, ub) and same_bits(vc, vb)


def test_the_restatement_clamps_and_propagates_specials():
    W, H = 9, 6
    b = np.arange(W * H, dtype=F).reshape(H, W)
    for bad, (tx, ty) in ((np.nan, (0, 2)), (-np.inf, (0, 2)), (np.inf, (W - 1, 2)),
                          (1e30, (W - 1, 2)), (-1e30, (0, 2))):
        ua, va = np.zeros((H, W), F), np.zeros((H, W), F)
        ua[2, 4] = bad
        uc, vc, outside = ref.compose(ua, va, b, b)
        assert outside == 1
        # vc = 0 + b at the clamped point; uc carries the special value itself
        assert vc[2, 4] == b[ty, tx]
        with np.errstate(invalid="ignore"):
            want = F(bad) + b[ty, tx]
        assert same_bits(uc[2, 4], want)
    # a special value in b reaches c only through the px that sample it
    ub = b.copy()
    ub[3, 3] = np.nan
    z = np.zeros((H, W), F)
    uc, vc, outside = ref.compose(z, z, ub, b)
    assert outside == 0 and np.isnan(uc[3, 3])
    # 0 * NaN: the px whose x1 or y1 tap is (3, 3) see it too, nobody else
    assert set(map(tuple, np.argwhere(np.isnan(uc)))) == {(3, 3), (3, 2), (2, 3), (2, 2)}
    assert same_bits(vc, b)


def test_each_kind_reaches_the_edge_it_is_named_for():
    seen = set()
    for case in T.CASES:
        pl = T.planes(case)
        for b in range(min(case.n, 2)):
            ua, va, ub, vb = (p[b] for p in pl)
            X, Y, inside = ref.landing(ua, va)
            W, H = case.W, case.H
            if case.kind == "integer":
                (ax, ay), (bx, by) = T.integer_flows(case)
                uc, vc, outside = ref.compose(ua, va, ub, vb)
                assert np.all(uc == ax + bx) and np.all(vc == ay + by)
                assert outside == int((~inside).sum())
                if W > 3 and H > 3:
                    assert inside.any() and (~inside).any()
            elif case.kind == "edges":
                assert inside.all()
                k = (np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 4
                assert np.all(X[k == 0] == 0) and np.all(X[k == 1] == W - 1)
                assert np.all(Y[k == 2] == 0) and np.all(Y[k == 3] == H - 1)
                assert ref.compose(ua, va, ub, vb)[2] == 0
            elif case.kind == "edges_out":
                k = (np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 4
                assert np.all(X[k == 0] < 0) and np.all(X[k == 0] > -1e-4)
                assert np.all(Y[k == 2] < 0) and np.all(Y[k == 2] > -1e-4)
                assert np.all(X[k == 1] == np.nextafter(F(W - 1), F(np.inf)))
                assert np.all(Y[k == 3] == np.nextafter(F(H - 1), F(np.inf)))
                assert not inside.any()
                assert ref.compose(ua, va, ub, vb)[2] == W * H
            elif case.kind == "special":
                for p in (ua, va, ub, vb):
                    if W * H >= 7 * 24:   # every special value fits without landing on another
                        assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
                        assert (np.abs(p) == F(1e30)).sum() == 2
                        assert ((p == 0) & np.signbit(p)).any()
                uc, vc, outside = ref.compose(ua, va, ub, vb)
                if W * H >= 7 * 24:
                    assert outside >= 4 and np.isnan(uc).any() and np.isinf(uc).any()
            elif case.kind == "smooth":
                uc, vc, outside = ref.compose(ua, va, ub, vb)
                if W > 8 and H > 8:
                    assert 0 < outside < W * H // 2
                    fr = X[inside] - np.floor(X[inside])
                    assert (fr > 0).any()
            elif case.kind == "far":
                assert not inside.any()
                assert ref.compose(ua, va, ub, vb)[2] == W * H
            seen.add(case.kind)
    assert seen == set(T.KINDS)
    assert any(c.roi and (4 * c.roi[2]) % 16 == 4 for c in T.CASES)
    assert any(c.n > 256 for c in T.CASES) and any(c.inplace for c in T.CASES)


def test_composing_constant_integer_flows_adds_them():
    W, H = 40, 30
    full = lambda c: np.full((H, W), c, F)
    u, v, counts = ref.compose_chain([(full(5), full(-3))] * 4)
    assert np.all(u == 20) and np.all(v == -12)
    # px that x + 5 k or y - 3 k takes out of the frame, k = 1, 2, 3
    assert counts == [W * H - (W - 5 * k) * (H - 3 * k) for k in (1, 2, 3)]


@pytest.fixture(scope="module")
def chain(built):
    """The five frames, the oracle's four link flows with their check traces, and the
    restatement's composition of them; computed once and never changed."""
    frames = T.chain_frames()
    p = capi.make_params(**T.CHAIN_PARAMS)
    links, traces = [], []
    for k in range(T.CHAIN_FRAMES - 1):
        u, v, _, _, trace = checker.oracle_check_trace(frames[k], frames[k + 1], p)
        links.append((u, v))
        traces.append(trace)
    su, sv, counts = ref.compose_chain(links)
    for a in (su, sv):
        a.setflags(write=False)
    return frames, p, links, traces, (su, sv), counts


def test_the_chain_seeds_a_pair_that_fails_unseeded(chain):
    frames, p, links, _, (su, sv), counts = chain
    for k, (u, v) in enumerate(links):
        assert T.chain_epe(u, v, links=1) < 0.1, k
    unseeded = checker.oracle_calc(frames[0], frames[-1], p)
    e_unseeded = T.chain_epe(unseeded[0], unseeded[1])
    e_seed = T.chain_epe(su, sv)
    chained = checker.oracle_calc(frames[0], frames[-1], p, init=(su, sv))
    e_chained = T.chain_epe(chained[0], chained[1])
    print(f"mean EPE: unseeded {e_unseeded:.3f}, seed {e_seed:.4f}, chained {e_chained:.4f}; "
          f"outside {counts}")
    assert e_unseeded > 10.0
    assert e_chained < 0.1
    assert all(0 < c < T.CHAIN_W * T.CHAIN_H for c in counts) and counts == sorted(counts)


def test_the_chain_solves_clear_the_residual_margin(chain):
    frames, p, _, traces, (su, sv), _ = chain
    trace = checker.oracle_check_trace(frames[0], frames[-1], p, init=(su, sv))[4]
    for k, t in enumerate(traces + [trace]):
        m = checker.check_margins(t, p.iterations)
        assert m.min() >= MIN_MARGIN, (k, t[np.argmin(m)])


def test_chain_links_plans_the_walk():
    cl = stack.chain_links
    assert cl((3, 7), (1, 4, 16)) == [(3, 4), (4, 5), (5, 6), (6, 7)]
    assert cl((2, 18), (1, 4, 16)) == [(2, 6), (6, 10), (10, 14), (14, 18)]
    assert cl((5, 6), (1, 4, 16)) is None                      # a stride-1 pair has no chain
    assert cl((0, 6), (1, 4, 6)) == [(0, 4), (4, 5), (5, 6)]   # the largest that fits, then smaller
    assert cl((9, 13), (6, 4, 1)) == [(9, 10), (10, 11), (11, 12), (12, 13)]   # any order of strides
    assert cl((0, 7), (2, 4, 7)) is None                       # 4, 2, then 1 px short: cannot close
    assert cl((0, 6), (2, 4, 6)) == [(0, 4), (4, 6)]
    assert cl((0, 4), (4, 16)) is None and cl((0, 16), (16,)) is None
    # every chained pair of a job is made of pairs of the same job
    strides = (1, 4, 16)
    pairs = set(stack.stack_pairs(40, strides))
    for pr in pairs:
        links = cl(pr, strides)
        if pr[1] - pr[0] == 1:
            assert links is None
        else:
            assert len(links) == 4 and set(links) <= pairs
            assert links[0][0] == pr[0] and links[-1][1] == pr[1]
            assert all(a[1] == b[0] for a, b in zip(links, links[1:]))
    with pytest.raises(ValueError):
        cl((4, 4), (1,))
    with pytest.raises(ValueError):
        cl((0, 4), (0, 1))
