"""The oracle's fast branch (fast_math = 1 with orc_set_approx_prims) on the CPU, with stand-in
primitives: ctypes callbacks over numpy that return RN(1/x) and RN(sqrt(x)).  The device's
v_rcp_f32 / v_sqrt_f32 themselves need the GPU (tests/test_gpu_fast_bitwise.py); what is
pinned here is the structure around them:

  * nothing installed, gamma != 0 or tau < 0: fast_math = 1 is the IEEE result, bit for bit;
  * each of the four FAST sites (oracle/tvl1_oracle.c) consumes its primitive: one element of
    one call moved to the next float up changes the result's bits, so no site still divides
    or takes a root on its own;
  * per level and warp the primitives are called on whole planes: rcp(wsum) and rcp(grad) of
    w*h, then per executed iteration one sqrt and one rcp of 2*w*h;
  * identical and constant pairs select around fi = -rho * rcp(0) (inf or NaN): zero flow;
  * correctly rounded primitives are a legal 1-ulp implementation, so with them the branch
    keeps fma mode's per-warp counts and tests/test_gpu_fastmath.py's TOL against IEEE;
  * the seeded and the f32 entry run the same branch.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import test_gpu_batch as gb
import test_gpu_fastmath as fm
from optflow_amd import capi, synth
from oracle import checker
from test_residual_margin_cpu import MIN_MARGIN

ROOT = Path(__file__).resolve().parent.parent


class Prims:
    """Stand-ins of orc_vec_fn's shape.  calls: (kind, n) in call order; inputs: a copy of every
    call's input when record is set; bump = (kind, k, i): element i of the k-th call of that kind
    returns the next float up."""

    def __init__(self, bump=None, record=False, fail=None):
        self.calls, self.inputs, self.count = [], [], {"rcp": 0, "sqrt": 0}
        self.bump, self.record, self.fail = bump, record, fail
        self.rcp = checker.VEC_FN(lambda i, o, n: self._run("rcp", i, o, n))
        self.sqrt = checker.VEC_FN(lambda i, o, n: self._run("sqrt", i, o, n))

    def _run(self, kind, inp, out, n):
        x = np.ctypeslib.as_array(inp, (n,))
        y = np.ctypeslib.as_array(out, (n,))
        k = self.count[kind]
        self.count[kind] += 1
        self.calls.append((kind, n))
        if self.record:
            self.inputs.append(x.copy())
        if self.fail == (kind, k):
            return 7
        with np.errstate(all="ignore"):
            y[:] = np.float32(1.0) / x if kind == "rcp" else np.sqrt(x)
        if self.bump is not None and self.bump[:2] == (kind, k):
            y[self.bump[2]] = np.nextafter(y[self.bump[2]], np.float32(np.inf))
        return 0

    @property
    def pair(self):
        return self.rcp, self.sqrt


def solve(I0, I1, kw, math=1, prims=None, init=None):
    return checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **kw), init=init,
                               approx=prims.pair if prims else None)


def same_bits(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and
            np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[3], b[3]))


def expected_calls(st, wi):
    """The call sequence the array passes prescribe: levels from the coarsest, per warp
    rcp(wsum) and rcp(grad) of w*h, then per executed iteration sqrt and rcp of 2*w*h."""
    out = []
    for s in reversed(range(st["levels"])):
        w, h = st["sizes"][s]
        for n in wi[s]:
            out += [("rcp", w * h), ("rcp", w * h)] + [("sqrt", 2 * w * h), ("rcp", 2 * w * h)] * int(n)
    return out


def test_engine_flags_restated():
    """oracle/Makefile builds fast_prims.hip with the engine's HIPFLAGS, so the primitives run
    in the engine's float mode."""
    flags = [re.search(r"^HIPFLAGS \?= (.*)$", (ROOT / d / "Makefile").read_text(), re.M).group(1)
             for d in ("oracle", "fibsem-optflow_amd")]
    assert flags[0] == flags[1]


def test_default_untouched(built):
    I0, I1 = synth.gen_pair(64, 48, seed=1)
    kw = dict(nscales=4, warps=2)
    assert same_bits(solve(I0, I1, kw, 1), solve(I0, I1, kw, 0))   # nothing installed: IEEE
    for extra in (dict(gamma=0.2), dict(tau=-0.05, epsilon=0.0, iterations=4)):
        p = Prims()
        k2 = dict(kw, **extra)
        a, b = solve(I0, I1, k2, 1, p), solve(I0, I1, k2, 0)
        assert p.calls == []                                         # math_of's rule: IEEE
        ok = np.isfinite(b[0]) & np.isfinite(b[1])
        assert np.array_equal(a[0].view(np.uint32)[ok], b[0].view(np.uint32)[ok])
        assert np.array_equal(a[1].view(np.uint32)[ok], b[1].view(np.uint32)[ok])
        assert np.array_equal(a[3], b[3])
    p = Prims()
    solve(I0, I1, dict(kw, profile=1, nscales=2), 1, p)              # profile 1 ignores fast_math
    assert p.calls == []
    # the primitives do not outlive the call that installed them
    assert same_bits(solve(I0, I1, kw, 1), solve(I0, I1, kw, 0))
    # fma mode is not the fast branch
    p = Prims()
    assert same_bits(solve(I0, I1, kw, 2, p), solve(I0, I1, kw, 2)) and p.calls == []


# one level, one warp, two iterations: rcp 0 = wsum, rcp 1 = grad, sqrt 0 and rcp 2 the first
# iteration's projection (the second iteration's estimateU reads its p)
SITE_KW = dict(nscales=1, warps=1, epsilon=0.0, iterations=2)
SITES = {"wsum": ("rcp", 0), "grad": ("rcp", 1), "sqrt": ("sqrt", 0), "ng": ("rcp", 2)}


@pytest.fixture(scope="module")
def site_case(built):
    """A textured frame against itself + 1 grey level: rho ~ 1 sits inside the TH operator's
    middle branch (|rho| <= l_t * grad) wherever the gradient is steep."""
    I0, _ = synth.gen_pair(40, 24, seed=3)
    I0 = np.minimum(I0, 250)
    I1 = (I0 + 1).astype(np.uint8)
    rec = Prims(record=True)
    base = solve(I0, I1, SITE_KW, 1, rec)
    assert rec.calls == expected_calls(base[2], base[3])
    return I0, I1, base, rec


@pytest.mark.parametrize("site", SITES)
def test_site_consumes_its_primitive(site_case, site):
    I0, I1, base, rec = site_case
    assert same_bits(solve(I0, I1, SITE_KW, 1, Prims()), base)       # plain stand-ins: same bits
    kind, k = SITES[site]
    idx = [j for j, c in enumerate(rec.calls) if c[0] == kind][k]
    x = rec.inputs[idx]
    N = I0.size
    if site == "grad":      # the steepest px: the middle branch, grad > FLT_EPSILON
        i = int(np.argmax(x))
    elif site == "wsum":    # any px consumes coeff
        i = int(np.argmax(rec.inputs[1]))
    else:                   # the px of u1 whose |grad u|^2 is largest: ng = 1 + taut*g well above 1
        i = int(np.argmax(x[:N] if site == "sqrt" else rec.inputs[idx - 1][:N]))
    got = solve(I0, I1, SITE_KW, 1, Prims(bump=(kind, k, i)))
    assert not same_bits(got, base), f"{site}: element {i} of {kind} call {k} is not consumed"
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


def test_primitive_failure_is_ehip(built):
    I0, I1 = synth.gen_pair(32, 24, seed=2)
    for fail in (("rcp", 0), ("rcp", 1), ("sqrt", 0), ("rcp", 2)):
        with pytest.raises(capi.TVL1Error, match="TVL1_EHIP|HIP|3"):
            solve(I0, I1, SITE_KW, 1, Prims(fail=fail))


CENSUS = [(64, 48, 1, dict(nscales=5, warps=3)), (17, 16, 2, dict(nscales=3, warps=2)),
          (33, 19, 4, dict(nscales=2, warps=2, epsilon=0.0, iterations=5)),
          (96, 64, 9, dict(median_filtering=5, nscales=4, warps=3))]


@pytest.mark.parametrize("W,H,seed,kw", CENSUS)
def test_call_census(built, W, H, seed, kw):
    I0, I1 = synth.gen_pair(W, H, seed=seed)
    p = Prims()
    u, v, st, wi = solve(I0, I1, kw, 1, p)
    assert p.calls == expected_calls(st, wi)
    n_iter = sum(1 for c in p.calls if c[0] == "sqrt")
    assert n_iter == st["iterations_total"] == sum(st["level_iterations"])
    for s in range(st["levels"]):
        w, h = st["sizes"][s]
        assert st["level_iterations"][s] == int(wi[s].sum())


def test_degenerate_selections(built):
    """grad = 0 everywhere (a constant I1) or rho = 0 everywhere (an identical pair): fi =
    -rho * rcp(grad) is -rho * inf or -0 * inf, formed and never selected."""
    kw = dict(nscales=3, warps=2)
    I0, _ = synth.gen_pair(48, 40, seed=5)
    with np.errstate(all="ignore"):
        u, v, st, wi = solve(I0, I0, kw, 1, Prims())
        assert not u.any() and not v.any() and np.all(wi == 2)
        c0, c1 = np.full((40, 48), 100, np.uint8), np.full((40, 48), 140, np.uint8)
        u, v, st, wi = solve(c0, c1, kw, 1, Prims())
    assert np.isfinite(u).all() and np.isfinite(v).all()
    assert not u.any() and not v.any()


def close_to_fma(I0, I1, kw, init=None):
    fast = solve(I0, I1, kw, 1, Prims(), init=init)
    assert same_bits(solve(I0, I1, kw, 1, Prims(), init=init), fast)
    fma = solve(I0, I1, kw, 2, init=init)
    ieee = solve(I0, I1, kw, 0, init=init)
    assert fast[2]["sizes"] == fma[2]["sizes"]
    np.testing.assert_array_equal(fast[3], fma[3])
    fm.check_budget(capi.epe(fast[0], fast[1], ieee[0], ieee[1]), 1, f"{I0.shape[1]}x{I0.shape[0]} (stand-ins)")
    assert not same_bits(fast, ieee)
    return fast


@pytest.mark.parametrize("W,H,seed,kw", [c for c in fm.CASES if (c[0], c[1]) != (512, 512)])
def test_standin_result_close_to_fma(built, W, H, seed, kw):
    close_to_fma(*synth.gen_pair(W, H, seed=seed), kw)


def test_seeded_entry(built):
    I0, I1 = synth.gen_pair(61, 47, seed=8)
    kw = dict(nscales=3, warps=2)
    yy, xx = np.mgrid[0:47, 0:61].astype(np.float32)
    init = (0.75 * np.sin(xx / 7) + 0.5, 1.25 * np.cos(yy / 5) - 0.25)
    p = Prims()
    got = solve(I0, I1, kw, 1, p, init=init)
    assert p.calls == expected_calls(got[2], got[3])
    assert same_bits(close_to_fma(I0, I1, kw, init=init), got)
    assert not same_bits(got, solve(I0, I1, kw, 1, Prims()))        # the seed is used
    assert same_bits(solve(I0, I1, kw, 1, init=init), solve(I0, I1, kw, 0, init=init))


def test_f32_entry(built):
    I0, I1 = synth.gen_pair(50, 33, seed=6)
    kw = dict(nscales=3, warps=2)
    F0, F1 = (I0.astype(np.float32) / 255).astype(np.float32), (I1.astype(np.float32) / 255).astype(np.float32)
    p = Prims()
    got = solve(F0, F1, kw, 1, p)
    assert p.calls == expected_calls(got[2], got[3])
    assert same_bits(close_to_fma(F0, F1, kw), got)
    assert same_bits(solve(F0, F1, kw, 1), solve(F0, F1, kw, 0))


def test_check_trace_in_fast_branch(built):
    I0, I1 = synth.gen_pair(64, 48, seed=1)
    p = capi.make_params(fast_math=1, nscales=4, warps=2)
    u, v, st, wi, tr = checker.oracle_check_trace(I0, I1, p, approx=Prims().pair)
    ref = checker.oracle_calc(I0, I1, p, approx=Prims().pair)
    assert same_bits((u, v, st, wi), ref)
    assert len(tr) == st["checks_total"] > 0
    # a warp that stopped before the cap did so at its last record: ratio <= 1 at iteration n - 1
    stopped = 0
    for s in range(st["levels"]):
        for wp in range(2):
            last = tr[(tr[:, 0] == s) & (tr[:, 1] == wp)][-1]
            if wi[s, wp] < 300:
                assert last[2] == wi[s, wp] - 1 and last[3] <= 1
                stopped += 1
    assert stopped > 0


@pytest.mark.parametrize("math", [0, 2, 1], ids=["ieee", "fma", "fast-standin"])
def test_two_chunk_batch_margins(built, math):
    """The compared pairs of test_gpu_batch.TWO_CHUNKS keep every check clear of its thresholds
    (the device's own primitives: tests/test_gpu_fast_bitwise.py)."""
    c = gb.TWO_CHUNKS
    worst = np.inf
    for b in c["sel"]:
        I0, I1 = synth.gen_pair(c["w"], c["h"], seed=c["seed"] + b, z=1 + b % 3)   # gb.pairs' pair b
        p = capi.make_params(fast_math=math, **c["kw"])
        tr = checker.oracle_check_trace(I0, I0 if b == c["identical"] else I1, p,
                                        approx=Prims().pair if math == 1 else None)[4]
        worst = min(worst, checker.check_margins(tr, p.iterations).min())
    print(f"minimum margin {worst:.3g}")
    assert worst >= MIN_MARGIN
