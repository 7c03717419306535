"""tvl1_fb_score*, tvl1_zero_above* and Engine.calc_consistent, bit for bit against
tests/fbcheck_ref.py (numpy float32) on every case of tests/fbcheck_cases.py: the score is one
IEEE rounding per operation in a fixed order, so every finite value and every infinity must be
equal and a NaN must be a NaN; tvl1_zero_above must zero exactly the restatement's px and count
them.  Holds on a ctx with fast_math = 1 and on one with profile = 1 alike."""
from types import SimpleNamespace

import numpy as np
import pytest

import fbcheck_cases as T
import flowop_badargs as B
import fbcheck_ref as ref
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
    """The case's planes and the restatement's score per pair, computed once and never changed."""
    if case.name not in _REF:
        pl = T.planes(case)
        sc = np.stack([ref.fb_score(pl[0][b], pl[1][b], pl[2][b], pl[3][b], case.alpha)
                       for b in range(case.n)])
        for a in pl + (sc,):
            a.setflags(write=False)
        _REF[case.name] = (pl, sc)
    return _REF[case.name]


def score_on_device(eng, case, pl, batch=True):
    d = [Planes(a, case.roi) for a in pl]
    s = Planes(np.full(pl[0].shape, SENTINEL, np.float32), case.roi)
    torch.cuda.synchronize()
    n = pl[0].shape[0]
    if batch:
        eng.fb_score_batch(n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, d[2].ptr, d[3].ptr,
                           d[2].pitch, d[2].stride, case.W, case.H, case.alpha, s.ptr, s.pitch,
                           s.stride, stream=eng.stream)
    else:
        assert n == 1
        eng.fb_score(d[0].ptr, d[1].ptr, d[0].pitch, d[2].ptr, d[3].ptr, d[2].pitch, case.W, case.H,
                     case.alpha, s.ptr, s.pitch, stream=eng.stream)
    torch.cuda.synchronize()
    return s, d


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_score_and_zeroing_match_the_restatement(eng, case):
    pl, want = reference(case)
    s, d = score_on_device(eng, case, pl, batch=True)
    got, clean = s.get()
    assert clean, "a float outside the score's rows was written"
    bad = ~(np.isnan(got) & np.isnan(want)) & (got.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    if case.n == 1:   # the n = 1 wrapper gives the same plane
        s1, _ = score_on_device(eng, case, pl, batch=False)
        assert same_bits(s1.get()[0], want)
    else:             # a pair of the second chunk equals a call of its own
        b = case.n - 1
        s1, _ = score_on_device(eng, case, tuple(a[b:b + 1] for a in pl), batch=True)
        assert same_bits(s1.get()[0][0], got[b]) and same_bits(got[b], want[b])
    # tvl1_zero_above on the forward flow, with the score the device just made
    rej = eng.zero_above_batch(case.n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, s.ptr, s.pitch,
                               s.stride, case.W, case.H, case.beta, stream=eng.stream)
    torch.cuda.synchronize()
    (u, cu), (v, cv) = d[0].get(), d[1].get()
    assert cu and cv, "a float outside the flow's rows was written"
    for b in range(case.n):
        wu, wv, wr = ref.zero_above(pl[0][b], pl[1][b], want[b], case.beta)
        assert int(rej[b]) == wr, (b, int(rej[b]), wr)
        assert same_bits(u[b], wu) and same_bits(v[b], wv), b
    if case.n == 1:   # the wrapper, uncounted and counted, on fresh copies
        for count in (False, True):
            d2 = [Planes(a, case.roi) for a in pl[:2]]
            torch.cuda.synchronize()
            if count:
                r = eng.zero_above(d2[0].ptr, d2[1].ptr, d2[0].pitch, s.ptr, s.pitch, case.W, case.H,
                                   case.beta, stream=eng.stream)
                assert r == ref.zero_above(pl[0][0], pl[1][0], want[0], case.beta)[2]
            else:
                eng.zero_above_batch(1, d2[0].ptr, d2[1].ptr, d2[0].pitch, d2[0].stride, s.ptr,
                                     s.pitch, s.stride, case.W, case.H, case.beta,
                                     stream=eng.stream, count=False)
            torch.cuda.synchronize()
            assert same_bits(d2[0].get()[0], u) and same_bits(d2[1].get()[0], v)


def test_profiled_calls_count_into_class_2_of_the_next_solve(eng0):
    from optflow_amd import synth
    case = next(c for c in T.CASES if c.name == "67x45-smooth")
    pl, _ = reference(case)
    I0, I1 = synth.gen_pair(64, 48, seed=3)
    p = capi.make_params(nscales=2, warps=1, iterations=4)
    e = capi.Engine(p)
    try:
        e.set_profiling(True)
        base = e.calc_host(I0, I1)[2]["kernel_launches"][2]
        s, d = score_on_device(e, case, pl)
        e.zero_above_batch(1, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, s.ptr, s.pitch, s.stride,
                           case.W, case.H, case.beta, stream=e.stream)
        assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base + 2
        assert e.calc_host(I0, I1)[2]["kernel_launches"][2] == base
    finally:
        e.close()


def test_bad_arguments_return_before_a_launch(eng0):
    """The rows of tests/flowop_badargs.py: each raises its status, with the message recorded
    before the checks moved into csrc/tvl1_planes.hpp, and nothing runs."""
    e = eng0
    W, H = B.W, B.H
    case = T.Case("err", W, H, "smooth", 0.01, 0.5, n=2)
    pl = T.planes(case)
    d = [Planes(a) for a in pl]
    s = Planes(np.full(pl[0].shape, SENTINEL, np.float32))
    big = Planes(np.full((1, 2 * H + 1, W), SENTINEL, np.float32))   # for overlapping views
    torch.cuda.synchronize()
    assert (d[0].pitch, d[0].stride) == (B.P, B.S)
    A = SimpleNamespace(d0=d[0].ptr, d1=d[1].ptr, d2=d[2].ptr, d3=d[3].ptr, s=s.ptr, big=big.ptr)
    good = B.defaults("fbcheck", A)

    def score(**kw):
        a = {**good["score"], **kw}
        e.fb_score_batch(*(a[k] for k in ("n", "uf", "vf", "fp", "fs", "ub", "vb", "bp", "bs", "w", "h", "alpha",
                                          "sc", "sp", "ss")), stream=e.stream)

    def zero(**kw):
        a = {**good["zero"], **kw}
        e.zero_above_batch(*(a[k] for k in ("n", "u", "v", "fp", "fs", "sc", "sp", "ss", "w", "h", "beta")),
                           stream=e.stream)

    fns, messages = dict(score=score, zero=zero), []
    for call, kw, status in B.rows("fbcheck", A):
        with pytest.raises(capi.TVL1Error, match=status) as err:
            fns[call](**kw)
        messages.append(str(err.value))
    B.assert_recorded("fbcheck", messages)
    torch.cuda.synchronize()
    # nothing ran: every output is what it was
    assert np.all(s.get()[0] == SENTINEL) and np.all(big.get()[0] == SENTINEL)
    for k in range(4):
        assert same_bits(d[k].get()[0], pl[k])
    # and the same calls with good arguments work
    score()
    zero()
    torch.cuda.synchronize()
    want = np.stack([ref.fb_score(pl[0][b], pl[1][b], pl[2][b], pl[3][b], 0.01) for b in range(2)])
    assert same_bits(s.get()[0], want)


@pytest.mark.parametrize("fast_math", [0, 2], ids=["ieee", "fma"])
def test_calc_consistent_scores_the_oracles_flows(built, fast_math):
    """The engine's flows equal the oracle's in both directions (the parity tests), so the score
    of calc_consistent is the restatement applied to the oracle's flows, bit for bit."""
    from oracle import checker
    I0, I1 = T.patch_pair()
    p = capi.make_params(fast_math=fast_math, **T.PATCH_PARAMS)
    uf, vf = checker.oracle_calc(I0, I1, p)[:2]
    ub, vb = checker.oracle_calc(I1, I0, p)[:2]
    want = ref.fb_score(uf, vf, ub, vb, 0.01)
    wu, wv, wr = ref.zero_above(uf, vf, want, 0.5)
    e = capi.Engine(p)
    try:
        u, v, score, rejected = e.calc_consistent(I0, I1)
    finally:
        e.close()
    assert same_bits(score, want)
    assert rejected == wr and 0 < wr < want.size
    assert same_bits(u, wu) and same_bits(v, wv)


def test_calc_consistent_negates_a_constant_seed(built):
    """init = (dx, dy): the backward solve starts from (-dx, -dy)."""
    from oracle import checker
    I0, I1 = T.patch_pair()
    p = capi.make_params(**T.PATCH_PARAMS)
    dx, dy = 2.0, -1.0
    f = lambda c: np.full(I0.shape, c, np.float32)
    uf, vf = checker.oracle_calc(I0, I1, p, init=(f(dx), f(dy)))[:2]
    ub, vb = checker.oracle_calc(I1, I0, p, init=(f(-dx), f(-dy)))[:2]
    want = ref.fb_score(uf, vf, ub, vb, 0.02)
    e = capi.Engine(p)
    try:
        u, v, score, rejected = e.calc_consistent(I0, I1, alpha=0.02, beta=0.75, init=(dx, dy))
    finally:
        e.close()
    assert same_bits(score, want)
    assert rejected == ref.zero_above(uf, vf, want, 0.75)[2]
