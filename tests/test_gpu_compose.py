"""tvl1_compose_flow*, Engine.compose_chain_host and Engine.calc_chained_host, bit for bit
against tests/compose_ref.py (numpy float32) on every case of tests/compose_cases.py: the
composition is one IEEE rounding per operation in a fixed order, so every finite value and every
infinity must be equal and a NaN must be a NaN; the outside counts must be equal; no float outside
a ROI view may change; in place must equal out of place.  Holds on a ctx with fast_math = 1 and
on one with profile = 1 alike."""
from types import SimpleNamespace

import numpy as np
import pytest

import compose_cases as T
import flowop_badargs as B
import compose_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(777.25)
CTXS = {"ieee": dict(), "fast": dict(fast_math=1), "cpu_profile": dict(profile=1)}


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


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
        self.per = per
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


@pytest.fixture(scope="module", params=list(CTXS))
def eng(request, built):
    e = capi.Engine(capi.make_params(**CTXS[request.param]))
    e.set_profiling(request.param == "cpu_profile")   # one ctx also counts the calls' marks
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng0(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


_REF = {}


def reference(case):
    """The case's planes and the restatement's (uc, vc, outside) per pair, computed once and
    never changed."""
    if case.name not in _REF:
        pl = T.planes(case)
        out = [ref.compose(pl[0][b], pl[1][b], pl[2][b], pl[3][b]) for b in range(case.n)]
        uc, vc = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        cnt = np.array([o[2] for o in out], np.uint64)
        for a in pl + (uc, vc, cnt):
            a.setflags(write=False)
        _REF[case.name] = (pl, uc, vc, cnt)
    return _REF[case.name]


def compose_on_device(eng, case, pl, batch=True, inplace=False, count=True):
    """-> (uc planes, vc planes, counts, the four input planes)"""
    d = [Planes(a, case.roi) for a in pl]
    if inplace:
        cu, cv = d[0], d[1]
    else:
        cu = Planes(np.full(pl[0].shape, SENTINEL, np.float32), case.roi)
        cv = Planes(np.full(pl[0].shape, SENTINEL, np.float32), case.roi)
    torch.cuda.synchronize()
    n = pl[0].shape[0]
    if batch:
        cnt = eng.compose_flow_batch(n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, d[2].ptr, d[3].ptr,
                                     d[2].pitch, d[2].stride, case.W, case.H, cu.ptr, cv.ptr, cu.pitch,
                                     cu.stride, stream=eng.stream, count=count)
    else:
        assert n == 1
        cnt = eng.compose_flow(d[0].ptr, d[1].ptr, d[0].pitch, d[2].ptr, d[3].ptr, d[2].pitch, case.W,
                               case.H, cu.ptr, cv.ptr, cu.pitch, stream=eng.stream, count=count)
    torch.cuda.synchronize()
    return cu, cv, cnt, d


def assert_equal_bits(got, want, what):
    bad = ~(np.isnan(got) & np.isnan(want)) & (got.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_composition_matches_the_restatement(eng, case):
    pl, wu, wv, wcnt = reference(case)
    cu, cv, cnt, d = compose_on_device(eng, case, pl, batch=True, inplace=case.inplace)
    (gu, clean_u), (gv, clean_v) = cu.get(), cv.get()
    assert clean_u and clean_v, "a float outside the composed flow's rows was written"
    assert_equal_bits(gu, wu, "uc")
    assert_equal_bits(gv, wv, "vc")
    assert np.array_equal(cnt, wcnt), (cnt[:4], wcnt[:4])
    if case.kind == "far":
        assert np.all(cnt == case.W * case.H)
    for k in ((2, 3) if case.inplace else (0, 1, 2, 3)):   # the inputs are what they were
        got, clean = d[k].get()
        assert clean and same_bits(got, pl[k]), k
    if case.n == 1:
        # the n = 1 wrapper, and an uncounted call, give the same planes
        for kw in (dict(batch=False), dict(batch=True, count=False), dict(batch=False, count=False)):
            c1u, c1v, c1, _ = compose_on_device(eng, case, pl, inplace=case.inplace, **kw)
            assert same_bits(c1u.get()[0], wu) and same_bits(c1v.get()[0], wv)
            assert c1 is None if kw.get("count") is False else c1 == int(wcnt[0])
        # in place equals out of place (the flagged case ran in place above: run the other way)
        ou, ov, oc, _ = compose_on_device(eng, case, pl, inplace=not case.inplace)
        (hu, cl_u), (hv, cl_v) = ou.get(), ov.get()
        assert cl_u and cl_v
        assert same_bits(hu, gu) and same_bits(hv, gv) and np.array_equal(oc, cnt)
    else:
        # a pair of the second chunk equals a call of its own; in place on the whole batch too
        b = case.n - 1
        c1u, c1v, c1, _ = compose_on_device(eng, case, tuple(a[b:b + 1] for a in pl))
        assert same_bits(c1u.get()[0][0], gu[b]) and same_bits(c1v.get()[0][0], gv[b])
        assert int(c1[0]) == int(cnt[b])
        iu, iv, ic, _ = compose_on_device(eng, case, pl, inplace=True)
        assert same_bits(iu.get()[0], gu) and same_bits(iv.get()[0], gv) and np.array_equal(ic, cnt)


def test_profiled_calls_count_into_class_2_of_the_next_solve(built):
    from optflow_amd import synth
    case = next(c for c in T.CASES if c.name == "67x45-smooth")
    pl = reference(case)[0]
    I0, I1 = synth.gen_pair(64, 48, seed=3)
    e = capi.Engine(capi.make_params(nscales=2, warps=1, iterations=4))
    try:
        e.set_profiling(True)
        base = e.calc_host(I0, I1)[2]["kernel_launches"][2]
        compose_on_device(e, case, pl)
        compose_on_device(e, case, pl, count=False)
        assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base + 2
        assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base
    finally:
        e.close()


def test_bad_arguments_return_before_a_launch(eng0):
    """The rows of tests/flowop_badargs.py: each raises its status, with the message recorded
    before the checks moved into csrc/tvl1_planes.hpp, and nothing runs."""
    e = eng0
    W, H = B.W, B.H
    case = T.Case("err", W, H, "smooth", n=2)
    pl = T.planes(case)
    d = [Planes(a) for a in pl]
    cu = Planes(np.full(pl[0].shape, SENTINEL, np.float32))
    cv = Planes(np.full(pl[0].shape, SENTINEL, np.float32))
    big = Planes(np.full((1, 2 * H + 1, W), SENTINEL, np.float32))   # for overlapping views
    torch.cuda.synchronize()
    assert (d[0].pitch, d[0].stride) == (B.P, B.S)
    A = SimpleNamespace(d0=d[0].ptr, d1=d[1].ptr, d2=d[2].ptr, d3=d[3].ptr, cu=cu.ptr, cv=cv.ptr, big=big.ptr)
    good = B.defaults("compose", A)["comp"]

    def comp(**kw):
        a = {**good, **kw}
        return e.compose_flow_batch(*(a[k] for k in ("n", "ua", "va", "ap", "as_", "ub", "vb", "bp", "bs", "w",
                                                     "h", "uc", "vc", "cp", "cs")), stream=e.stream)

    messages = []
    for _, kw, status in B.rows("compose", A):
        with pytest.raises(capi.TVL1Error, match=status) as err:
            comp(**kw)
        messages.append(str(err.value))
    B.assert_recorded("compose", messages)
    torch.cuda.synchronize()
    # nothing ran: every plane is what it was
    assert np.all(cu.get()[0] == SENTINEL) and np.all(cv.get()[0] == SENTINEL)
    assert np.all(big.get()[0] == SENTINEL)
    for k in range(4):
        assert same_bits(d[k].get()[0], pl[k])
    # and the same call with good arguments works, out of place and in place
    want = [ref.compose(pl[0][b], pl[1][b], pl[2][b], pl[3][b]) for b in range(2)]
    for kw in (dict(), dict(uc=d[0].ptr, vc=d[1].ptr)):
        cnt = comp(**kw)
        torch.cuda.synchronize()
        gu, gv = (d[0], d[1]) if kw else (cu, cv)
        assert same_bits(gu.get()[0], np.stack([o[0] for o in want]))
        assert same_bits(gv.get()[0], np.stack([o[1] for o in want]))
        assert [int(c) for c in cnt] == [o[2] for o in want]


@pytest.fixture(scope="module")
def chain(built):
    """The five-frame stack, the oracle's four link flows and the restatement's composition of
    them: computed once and never changed."""
    from oracle import checker
    frames = T.chain_frames()
    p = capi.make_params(**T.CHAIN_PARAMS)
    links = [checker.oracle_calc(frames[k], frames[k + 1], p)[:2] for k in range(T.CHAIN_FRAMES - 1)]
    su, sv, counts = ref.compose_chain(links)
    for a in (su, sv):
        a.setflags(write=False)
    return frames, p, links, (su, sv), counts


def test_compose_chain_host_is_the_restatements_chain(chain, eng):
    _, _, links, (su, sv), counts = chain
    u, v, got = eng.compose_chain_host(links)
    assert same_bits(u, su) and same_bits(v, sv)
    assert got == counts
    u1, v1, got1 = eng.compose_chain_host(links[:1])   # a chain of one link is the link
    assert same_bits(u1, links[0][0]) and same_bits(v1, links[0][1]) and got1 == []


def test_calc_chained_host_equals_the_oracle_seeded_from_the_restatement(chain):
    """The engine's four link flows equal the oracle's (the parity tests), so the chained solve
    is the oracle's solve from the restatement's composition of the oracle's links: the flow and
    the per-warp iteration counts, bit for bit."""
    from oracle import checker
    frames, p, _, (su, sv), counts = chain
    e = capi.Engine(p)
    try:
        links = [e.calc_host(frames[k], frames[k + 1])[:2] for k in range(T.CHAIN_FRAMES - 1)]
        u, v, st, wi, got = e.calc_chained_host(frames[0], frames[-1], links)
    finally:
        e.close()
    ur, vr, sr, wr = checker.oracle_calc(frames[0], frames[-1], p, init=(su, sv))
    assert got == counts
    assert np.array_equal(wi, wr), (wi, wr)
    assert same_bits(u, ur) and same_bits(v, vr)
    assert T.chain_epe(u, v) < 0.1
