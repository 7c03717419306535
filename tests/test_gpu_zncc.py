"""tvl1_zncc_score*, tvl1_warp_by_flow_u8 and Engine.calc_scored, bit for bit against
tests/zncc_ref.py (numpy) on every case of tests/zncc_cases.py: the sums are integers and the
score is four IEEE f64 operations and one conversion, so every finite value and every +inf must
be equal.  Holds on a ctx with fast_math = 1 and on one with profile = 1 alike.  ROI views lie
in allocations filled with values that would change a sum if they were read, and the score's
allocation must be untouched outside the ROI."""
from types import SimpleNamespace

import numpy as np
import pytest

import flowop_badargs as B
import zncc_cases as T
import zncc_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = {np.dtype(np.float32): np.float32(777.25), np.dtype(np.uint8): np.uint8(173)}
CTXS = {"ieee": dict(), "fast": dict(fast_math=1), "cpu_profile": dict(profile=1)}


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


class Planes:
    """(n, H, W) planes of one dtype on the device: dense, or each a ROI view at element `first`
    of an allocation of AW x AH elements filled with a sentinel (for a flow: a finite value that
    would land somewhere else; for a frame: a grey value that would change every sum)."""

    def __init__(self, a, roi=None):
        a = np.ascontiguousarray(a)
        self.n, self.H, self.W = a.shape
        self.item = a.dtype.itemsize
        self.fill = SENTINEL[a.dtype]
        if roi is None:
            self.AW, self.first, per = self.W, 0, self.W * self.H
        else:
            self.AW, AH, self.first = roi
            per = self.AW * AH
            assert self.first % self.AW + self.W <= self.AW and self.first // self.AW + self.H <= AH
        per += (-per) % 16                           # every pair's allocation starts 16-byte aligned
        host = np.full((self.n, per), self.fill, a.dtype)
        self._view(host)[...] = a
        self.t = torch.from_numpy(host).to(torch.device("cuda", 0))
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.item * self.first
        self.pitch, self.stride = self.item * self.AW, self.item * per

    def _view(self, host):
        v = host[:, self.first:self.first + (self.H - 1) * self.AW + self.W]
        return np.lib.stride_tricks.as_strided(
            v, (self.n, self.H, self.W), (host.strides[0], self.item * self.AW, self.item), writeable=True)

    def get(self):
        """(the planes, True iff every element outside them still holds the sentinel)"""
        host = self.t.cpu().numpy()
        out = self._view(host).copy()
        self._view(host)[...] = self.fill
        return out, bool(np.all(host == self.fill))


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
    """The restatement's J, m and score of every pair of the case, computed once, read-only."""
    if case.name not in _REF:
        I0, I1, u, v = T.planes(case)
        J, m, sc = [], [], []
        for b in range(case.n):
            j, k = ref.warp(I1[b], u[b], v[b])
            J.append(j), m.append(k)
            sc.append(ref.score_from(j, k, I0[0 if case.shared0 else b], case.r))
        out = (np.stack(J), np.stack(m), np.stack(sc))
        for a in out:
            a.setflags(write=False)
        _REF[case.name] = out
    return _REF[case.name]


def score_on_device(eng, case, pl, batch=True):
    """The score planes of the case's pairs `pl` = (I0, I1, u, v), and the device inputs."""
    d = [Planes(a, case.roi) for a in pl]
    n = pl[1].shape[0]
    s = Planes(np.full(pl[2].shape, SENTINEL[np.dtype(F)], F), case.roi)
    torch.cuda.synchronize()
    stride0 = 0 if (case.shared0 and n > 1) else d[0].stride
    if batch:
        eng.zncc_score_batch(n, d[0].ptr, d[0].pitch, stride0, d[1].ptr, d[1].pitch, d[1].stride,
                             d[2].ptr, d[3].ptr, d[2].pitch, d[2].stride, case.W, case.H, case.r,
                             s.ptr, s.pitch, s.stride, stream=eng.stream)
    else:
        assert n == 1
        eng.zncc_score(d[0].ptr, d[0].pitch, d[1].ptr, d[1].pitch, d[2].ptr, d[3].ptr, d[2].pitch,
                       case.W, case.H, case.r, s.ptr, s.pitch, stream=eng.stream)
    torch.cuda.synchronize()
    return s, d


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_score_matches_the_restatement(eng, case):
    pl = T.planes(case)
    _, _, want = reference(case)
    s, d = score_on_device(eng, case, pl, batch=True)
    got, clean = s.get()
    assert clean, "a float outside the score's rows was written"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    for k in range(4):   # no input was written
        assert np.array_equal(d[k].get()[0], pl[k], equal_nan=True)
    if case.n == 1:      # the n = 1 wrapper gives the same plane
        s1, _ = score_on_device(eng, case, pl, batch=False)
        g1, clean = s1.get()
        assert clean and same_bits(g1, want)
    else:                # a pair of the second chunk equals a call of its own
        b = case.n - 1
        assert b == 256
        one = (pl[0] if case.shared0 else pl[0][b:b + 1],) + tuple(a[b:b + 1] for a in pl[1:])
        s1, _ = score_on_device(eng, case, one, batch=True)
        assert same_bits(s1.get()[0][0], got[b]) and same_bits(got[b], want[b])


WARP_CASES = [c for c in T.CASES if c.n == 1 and (c.roi or (c.W, c.H) in ((1, 1), (5, 1), (1, 7), (67, 45), (257, 131)))]


@pytest.mark.parametrize("case", WARP_CASES, ids=[c.name for c in WARP_CASES])
def test_warp_by_flow_matches_step_1(eng0, case):
    _, I1, u, v = T.planes(case)
    wantJ, wantm, _ = reference(case)
    d = [Planes(a, case.roi) for a in (I1, u, v)]
    for with_valid in (True, False):
        J = Planes(np.full(I1.shape, 99, np.uint8), case.roi)
        m = Planes(np.full(I1.shape, 99, np.uint8), case.roi)
        torch.cuda.synchronize()
        eng0.warp_by_flow_u8(d[0].ptr, d[0].pitch, d[1].ptr, d[2].ptr, d[1].pitch, case.W, case.H,
                             J.ptr, J.pitch, m.ptr if with_valid else 0, m.pitch if with_valid else 0,
                             stream=eng0.stream)
        torch.cuda.synchronize()
        (gJ, cJ), (gm, cm) = J.get(), m.get()
        assert cJ and cm, "a byte outside the planes was written"
        assert np.array_equal(gJ, wantJ)
        assert np.array_equal(gm, wantm.astype(np.uint8) if with_valid else np.full(I1.shape, 99, np.uint8))


def test_profiled_calls_count_into_class_2_of_the_next_solve(built):
    from optflow_amd import synth
    case = next(c for c in T.CASES if c.name.startswith("67x45-smooth"))
    pl = T.planes(case)
    I0, I1 = synth.gen_pair(64, 48, seed=3)
    e = capi.Engine(capi.make_params(nscales=2, warps=1, iterations=4))
    try:
        e.set_profiling(True)
        base = e.calc_host(I0, I1)[2]["kernel_launches"][2]
        s, d = score_on_device(e, case, pl)
        J = Planes(np.zeros(pl[1].shape, np.uint8))
        torch.cuda.synchronize()
        e.warp_by_flow_u8(d[1].ptr, d[1].pitch, d[2].ptr, d[3].ptr, d[2].pitch, case.W, case.H, J.ptr,
                          J.pitch, stream=e.stream)
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
    s = Planes(np.full(pl[2].shape, SENTINEL[np.dtype(F)], F))
    big = Planes(np.full((1, 2 * H + 1, W), SENTINEL[np.dtype(F)], F))   # for overlapping views
    J = Planes(np.full((1, H, W), 99, np.uint8))
    torch.cuda.synchronize()
    assert (d[2].pitch, d[2].stride, d[0].pitch, d[0].stride) == (B.P, B.ZS, B.P8, B.S8)
    assert B.ZS >= B.P * H and B.S8 >= B.P8 * H
    A = SimpleNamespace(d0=d[0].ptr, d1=d[1].ptr, d2=d[2].ptr, d3=d[3].ptr, s=s.ptr, big=big.ptr, J=J.ptr)
    good = B.defaults("zncc", A)

    def score(**kw):
        a = {**good["score"], **kw}
        e.zncc_score_batch(*(a[k] for k in ("n", "i0", "p0", "s0", "i1", "p1", "s1", "u", "v", "fp", "fs", "w",
                                            "h", "r", "sc", "sp", "ss")), stream=e.stream)

    def warp(**kw):
        a = {**good["warp"], **kw}
        e.warp_by_flow_u8(*(a[k] for k in ("i1", "p1", "u", "v", "fp", "w", "h", "dst", "dp", "valid", "vp")),
                          stream=e.stream)

    fns, messages = dict(score=score, warp=warp), []
    for call, kw, status in B.rows("zncc", A):
        with pytest.raises(capi.TVL1Error, match=status) as err:
            fns[call](**kw)
        messages.append(str(err.value))
    B.assert_recorded("zncc", messages)
    torch.cuda.synchronize()
    # nothing ran: every output is what it was
    assert np.all(s.get()[0] == SENTINEL[np.dtype(F)]) and np.all(big.get()[0] == SENTINEL[np.dtype(F)])
    assert np.all(J.get()[0] == 99)
    for k in range(4):
        assert np.array_equal(d[k].get()[0], pl[k])
    # and the same calls with good arguments work; a NULL valid is allowed
    score()
    warp()
    torch.cuda.synchronize()
    want = np.stack([ref.zncc_score(pl[0][b], pl[1][b], pl[2][b], pl[3][b], 2) for b in range(2)])
    assert same_bits(s.get()[0], want)
    assert np.array_equal(J.get()[0][0], ref.warp(pl[1][0], pl[2][0], pl[3][0])[0])


@pytest.mark.parametrize("fast_math", [0, 2], ids=["ieee", "fma"])
def test_calc_scored_scores_the_engines_own_flow(built, fast_math):
    """One solve, the score on the raw flow, then tvl1_zero_above: the restatement applied to the
    flow the same ctx's plain solve returns."""
    import fbcheck_cases as FB
    I0, I1 = FB.patch_pair()
    p = capi.make_params(fast_math=fast_math, **FB.PATCH_PARAMS)
    e = capi.Engine(p)
    try:
        uf, vf = e.calc_host(I0, I1)[:2]
        u, v, score, rejected = e.calc_scored(I0, I1)
        u2, v2, score2, rejected2 = e.calc_scored(I0, I1, radius=1, beta=0.5)
    finally:
        e.close()
    for (r, beta, gu, gv, gs, gr) in ((3, 0.25, u, v, score, rejected), (1, 0.5, u2, v2, score2, rejected2)):
        want = ref.zncc_score(I0, I1, uf, vf, r)
        wu, wv, wr = ref.zero_above(uf, vf, want, beta)
        assert same_bits(gs, want)
        assert gr == wr and 0 < wr < want.size
        assert same_bits(gu, wu) and same_bits(gv, wv)


def test_calc_scored_from_a_constant_seed(built):
    import fbcheck_cases as FB
    from oracle import checker
    I0, I1 = FB.patch_pair()
    p = capi.make_params(**FB.PATCH_PARAMS)
    f = lambda c: np.full(I0.shape, c, F)
    uf, vf = checker.oracle_calc(I0, I1, p, init=(f(2.0), f(-1.0)))[:2]
    want = ref.zncc_score(I0, I1, uf, vf, 2)
    e = capi.Engine(p)
    try:
        u, v, score, rejected = e.calc_scored(I0, I1, radius=2, beta=0.3, init=(2.0, -1.0))
    finally:
        e.close()
    assert same_bits(score, want)
    assert rejected == ref.zero_above(uf, vf, want, 0.3)[2]
