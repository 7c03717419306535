"""tvl1_invert_flow*, Engine.invert_flow_host and Engine.calc_chained_host(inverse=True), bit for
bit against tests/invert_ref.py (numpy float32) on every case of tests/invert_cases.py: the
inversion is one IEEE rounding per operation in a fixed order, so every finite value and every
infinity must be equal and a NaN must be a NaN; the outside and unconverged counts must be equal;
no float outside a ROI view may change and f stays what it was.  Holds on a ctx with fast_math = 1
and on one with profile = 1 alike, and on both arms of the kernel (TVL1_INVERT_WINDOW = 0 / 1,
read when the ctx is created)."""
from types import SimpleNamespace

import numpy as np
import pytest

import compose_ref as cref
import flowop_badargs as B
import invert_cases as T
import invert_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(777.25)
CTXS = {"ieee": dict(), "fast": dict(fast_math=1), "cpu_profile": dict(profile=1)}
ARMS = {"global": "0", "window": "1"}


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def assert_equal_bits(got, want, what):
    bad = ~(np.isnan(got) & np.isnan(want)) & (got.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


class Planes:
    """(n, H, W) float32 planes on the device: dense (pitch 4 W, pair stride 4 W H), or each a
    ROI view at float `first` of an allocation of AW x AH floats filled with a sentinel."""

    def __init__(self, a, roi=None):
        a = np.asarray(a, np.float32)
        self.n, self.H, self.W = a.shape
        if roi is None:
            self.AW, self.first, per = self.W, 0, self.W * self.H
        else:
            self.AW, AH, self.first = roi
            per = self.AW * AH
            assert self.first % self.AW + self.W <= self.AW and self.first // self.AW + self.H <= AH
        host = np.full((self.n, per), SENTINEL, np.float32)
        self._view(host)[...] = a
        self.t = torch.from_numpy(host).to(torch.device("cuda", 0))
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.first
        self.pitch, self.stride = 4 * self.AW, 4 * per

    def _view(self, host):
        v = host[:, self.first:self.first + (self.H - 1) * self.AW + self.W]
        return np.lib.stride_tricks.as_strided(
            v, (self.n, self.H, self.W), (host.strides[0], 4 * self.AW, 4), writeable=True)

    def get(self):
        """(the planes, True iff every float outside them still holds the sentinel)"""
        host = self.t.cpu().numpy()
        out = self._view(host).copy()
        self._view(host)[...] = SENTINEL
        return out, bool(np.all(host.view(np.uint32) == SENTINEL.view(np.uint32)))


def make_engine(params, arm, profiling=False):
    """The knob is read by tvl1_create: set around it only."""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("TVL1_INVERT_WINDOW", ARMS[arm])
        e = capi.Engine(params)
    finally:
        mp.undo()
    e.set_profiling(profiling)
    return e


@pytest.fixture(scope="module", params=[(c, a) for c in CTXS for a in ARMS], ids=lambda p: f"{p[0]}-{p[1]}")
def eng(request, built):
    ctx, arm = request.param
    e = make_engine(capi.make_params(**CTXS[ctx]), arm, ctx == "cpu_profile")
    yield e
    e.close()


@pytest.fixture(scope="module", params=list(ARMS))
def eng0(request, built):
    e = make_engine(capi.make_params(), request.param)
    yield e
    e.close()


_REF = {}


def reference(case):
    """The case's planes and the restatement's (ug, vg, resid, counts) per pair, computed once and
    never changed."""
    if case.name not in _REF:
        pl = T.planes(case)
        out = [ref.invert(pl[0][b], pl[1][b], case.K, case.tol) for b in range(case.n)]
        ug, vg, rs = (np.stack([o[j] for o in out]) for j in range(3))
        cnt = np.array([o[3:5] for o in out], np.uint64)
        for a in pl + (ug, vg, rs, cnt):
            a.setflags(write=False)
        _REF[case.name] = (pl, ug, vg, rs, cnt)
    return _REF[case.name]


def invert_on_device(eng, case, pl, batch=True, resid=True, counts=True):
    """-> (ug planes, vg planes, resid planes or None, counts, the two input planes)"""
    d = [Planes(a, case.roi) for a in pl]
    blank = np.full(pl[0].shape, SENTINEL, np.float32)
    gu, gv = Planes(blank, case.roi), Planes(blank, case.roi)
    rs = Planes(blank, case.roi) if resid else None
    torch.cuda.synchronize()
    n = pl[0].shape[0]
    rp = (rs.ptr, rs.pitch, rs.stride) if resid else (0, 0, 0)
    if batch:
        cnt = eng.invert_flow_batch(n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, case.K, case.tol,
                                    gu.ptr, gv.ptr, gu.pitch, gu.stride, rp[0], rp[1], rp[2], case.W,
                                    case.H, stream=eng.stream, counts=counts)
    else:
        assert n == 1
        cnt = eng.invert_flow(d[0].ptr, d[1].ptr, d[0].pitch, case.K, case.tol, gu.ptr, gv.ptr, gu.pitch,
                              rp[0], rp[1], case.W, case.H, stream=eng.stream, counts=counts)
        if counts:
            cnt = np.array([[cnt["outside"], cnt["unconverged"]]], np.uint64)
    torch.cuda.synchronize()
    return gu, gv, rs, cnt, d


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_inversion_matches_the_restatement(eng, case):
    pl, wu, wv, wr, wcnt = reference(case)
    gu, gv, rs, cnt, d = invert_on_device(eng, case, pl)
    (hu, clean_u), (hv, clean_v), (hr, clean_r) = gu.get(), gv.get(), rs.get()
    assert clean_u and clean_v and clean_r, "a float outside the output rows was written"
    assert_equal_bits(hu, wu, "ug")
    assert_equal_bits(hv, wv, "vg")
    assert_equal_bits(hr, wr, "resid")
    assert np.array_equal(cnt, wcnt), (cnt[:4], wcnt[:4])
    for k in (0, 1):   # f is what it was
        got, clean = d[k].get()
        assert clean and same_bits(got, pl[k]), k
    if case.n == 1:
        # the n = 1 wrapper, a call without a residual plane and an uncounted call give the same
        for kw in (dict(batch=False), dict(resid=False), dict(batch=False, resid=False),
                   dict(counts=False), dict(batch=False, counts=False, resid=False)):
            g1u, g1v, r1, c1, _ = invert_on_device(eng, case, pl, **kw)
            (au, cl_u), (av, cl_v) = g1u.get(), g1v.get()
            assert cl_u and cl_v and same_bits(au, wu) and same_bits(av, wv), kw
            if r1 is not None:
                ar, cl_r = r1.get()
                assert cl_r and same_bits(ar, wr), kw
            assert c1 is None if kw.get("counts") is False else np.array_equal(c1, wcnt), kw
    else:
        # a pair of the second chunk equals a call of its own
        b = case.n - 1
        g1u, g1v, r1, c1, _ = invert_on_device(eng, case, tuple(a[b:b + 1] for a in pl))
        assert same_bits(g1u.get()[0][0], hu[b]) and same_bits(g1v.get()[0][0], hv[b])
        assert same_bits(r1.get()[0][0], hr[b]) and np.array_equal(c1[0], cnt[b])


@pytest.mark.parametrize("name", ["257x131-fold", "roi130x70-smooth-k1", "67x45-special"])
def test_zero_above_on_the_residual_gives_the_restatements_set(eng0, name):
    case = next(c for c in T.CASES if c.name.startswith(name))
    pl, wu, wv, wr, wcnt = reference(case)
    gu, gv, rs, cnt, _ = invert_on_device(eng0, case, pl)
    rej = eng0.zero_above(gu.ptr, gv.ptr, gu.pitch, rs.ptr, rs.pitch, case.W, case.H, case.tol,
                          stream=eng0.stream)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        bad = ~(wr <= np.float32(case.tol))
    assert rej == int(bad.sum()) == int(wcnt[0, 1]) and rej > 0
    (hu, clean_u), (hv, clean_v) = gu.get(), gv.get()
    assert clean_u and clean_v
    assert same_bits(hu, np.where(bad, np.float32(0), wu)) and same_bits(hv, np.where(bad, np.float32(0), wv))


def test_profiled_calls_count_into_class_2_of_the_next_solve(built):
    from optflow_amd import synth
    case = next(c for c in T.CASES if c.name.startswith("67x45-smooth"))
    pl = reference(case)[0]
    I0, I1 = synth.gen_pair(64, 48, seed=3)
    for arm in ARMS:
        e = make_engine(capi.make_params(nscales=2, warps=1, iterations=4), arm)
        try:
            e.set_profiling(True)
            base = e.calc_host(I0, I1)[2]["kernel_launches"][2]
            invert_on_device(e, case, pl)
            invert_on_device(e, case, pl, counts=False, resid=False)
            assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base + 2
            assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base
        finally:
            e.close()


def test_bad_arguments_return_before_a_launch(eng0):
    """The rows of tests/flowop_badargs.py: each raises its status, with the message recorded
    before the checks moved into csrc/tvl1_planes.hpp, and nothing runs."""
    e = eng0
    W, H = B.W, B.H
    case = T.Case("err", W, H, "smooth", 2, n=2)
    pl = T.planes(case)
    d = [Planes(a) for a in pl]
    blank = np.full(pl[0].shape, SENTINEL, np.float32)
    gu, gv, rs = Planes(blank), Planes(blank), Planes(blank)
    big = Planes(np.full((1, 2 * H + 1, W), SENTINEL, np.float32))   # for overlapping views
    torch.cuda.synchronize()
    P = B.P
    assert (d[0].pitch, d[0].stride) == (B.P, B.S)
    A = SimpleNamespace(d0=d[0].ptr, d1=d[1].ptr, gu=gu.ptr, gv=gv.ptr, rs=rs.ptr, big=big.ptr)
    good = B.defaults("invert", A)["inv"]

    def inv(**kw):
        a = {**good, **kw}
        return e.invert_flow_batch(*(a[k] for k in ("n", "uf", "vf", "fp", "fs", "K", "tol", "ug", "vg", "gp",
                                                    "gs", "r", "rp", "rs_", "w", "h")), stream=e.stream)

    messages = []
    for _, kw, status in B.rows("invert", A):
        with pytest.raises(capi.TVL1Error, match=status) as err:
            inv(**kw)
        messages.append(str(err.value))
    B.assert_recorded("invert", messages)
    torch.cuda.synchronize()
    # nothing ran: every plane is what it was
    for p in (gu, gv, rs, big):
        assert np.all(p.get()[0] == SENTINEL)
    for k in range(2):
        assert same_bits(d[k].get()[0], pl[k])
    # one float short of overlapping is fine, and so are the limits of K and an infinite tol
    want = [ref.invert(pl[0][b], pl[1][b], 2, 0.01) for b in range(2)]
    cnt = inv()
    torch.cuda.synchronize()
    for j, p in enumerate((gu, gv, rs)):
        assert same_bits(p.get()[0], np.stack([o[j] for o in want]))
    assert [tuple(int(x) for x in c) for c in cnt] == [o[3:5] for o in want]
    cnt = inv(n=1, uf=big.ptr, ug=big.ptr + P * H, K=32, tol=float("inf"))
    assert int(cnt[0, 1]) == int(np.isnan(ref.invert(blank[0], pl[1][0], 32, np.inf)[2]).sum())
    inv(K=1, tol=-1.0)


@pytest.fixture(scope="module")
def zoom(built):
    """The zoom stack, the oracle's four link flows, the restatement's chain of them and its
    inverse: computed once and never changed."""
    from oracle import checker
    frames = T.zoom_frames()
    p = capi.make_params(**T.ZOOM_PARAMS)
    links = [checker.oracle_calc(frames[k], frames[k + 1], p)[:2] for k in range(T.ZOOM_FRAMES - 1)]
    cu, cv, ccounts = cref.compose_chain(links)
    ug, vg, rs, outside, unconv = ref.invert(cu, cv, 8, T.TOL)
    for a in (cu, cv, ug, vg, rs):
        a.setflags(write=False)
    return frames, p, links, (cu, cv), ccounts, (ug, vg, rs), dict(outside=outside, unconverged=unconv)


def test_invert_flow_host_of_the_composed_chain_is_the_restatements(zoom, eng):
    _, _, links, (cu, cv), ccounts, (ug, vg, rs), counts = zoom
    u, v, got = eng.compose_chain_host(links)
    assert same_bits(u, cu) and same_bits(v, cv) and got == ccounts
    gu, gv, gr, c = eng.invert_flow_host(u, v, iterations=8, tol=T.TOL, resid=True)
    assert same_bits(gu, ug) and same_bits(gv, vg) and same_bits(gr, rs) and c == counts
    gu, gv, c = eng.invert_flow_host(u, v)   # the defaults are K = 8 and tol = 0.01
    assert same_bits(gu, ug) and same_bits(gv, vg) and c == counts


@pytest.mark.parametrize("arm", list(ARMS))
def test_calc_chained_host_inverse_equals_the_oracle_seeded_from_the_restatement(zoom, arm):
    """The engine's four link flows equal the oracle's (the parity tests), so the reverse pair's
    solve is the oracle's solve from the restatement's inverse of the restatement's chain of the
    oracle's links: the flow and the per-warp iteration counts, bit for bit."""
    from oracle import checker
    frames, p, _, _, ccounts, (ug, vg, _), counts = zoom
    e = make_engine(p, arm)
    try:
        links = [e.calc_host(frames[k], frames[k + 1])[:2] for k in range(T.ZOOM_FRAMES - 1)]
        u, v, st, wi, got, inv = e.calc_chained_host(frames[4], frames[0], links, inverse=True)
    finally:
        e.close()
    ur, vr, sr, wr = checker.oracle_calc(frames[4], frames[0], p, init=(ug, vg))
    assert got == ccounts and inv == counts
    assert np.array_equal(wi, wr), (wi, wr)
    assert same_bits(u, ur) and same_bits(v, vr)
    assert T.zoom_epe(u, v, 4, 0) < 0.5
