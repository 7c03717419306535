"""k_iterate_stages (a wavefront per iteration of a 2- or 4-iteration pass) on the GPU.

TVL1_STAGES=2 sends every gamma = 0 pass of 2 or 4 iterations, on every level, to the kernel.
Each solve is compared bitwise with the oracle -- u, v, per-warp iteration counts, number of
checks -- and with the same solve under TVL1_STAGES=0 (k_iterate_roll / k_iterate_tb4), in
IEEE and fma arithmetic; the approximate mode is held to tests/test_gpu_fastmath.py's budget
here and, bitwise against the oracle's fast branch, in tests/test_gpu_fast_bitwise.py.

Shapes, the smallest at which the kernel can go wrong (K = 4: 120 output px per 128-px band,
K = 2: 124; TVL1_ROLL_SEG=8 forces 8-row segments; a block runs rows + run-in + 2K - 1 steps in
trips of 3):
  widths   100 one band; 121 a 1-px second band (K = 4); 125 the same for K = 2; 241 a third
           band of 1 px (K = 4) cut by the image edge, K = 2's second band cut at 117 px;
  heights  1, 2, 3 shorter than K; 6, 7, 8 one segment of 3m + 2, 3m, 3m + 1 steps (K = 4);
           9, 17, 18 a last segment of 1, 1, 2 rows; 60 seven seams and a 4-row last segment;
  passes   epsilon = 0, 10 iterations: passes of 4, 4, 2 with no check, the first with p = 0;
           epsilon > 0: a 2-iteration first pass (p = 0) ending in a check, then passes ending
           in checks and passes that do not;
  a 5-level solve of 320 x 200 with epsilon > 0, and a gated launch whose gate is off.
"""
import re

import numpy as np
import pytest

from optflow_amd import capi, synth
from oracle import checker

pytestmark = pytest.mark.gpu

KNOBS = ("TVL1_ROLL_SEG", "TVL1_ROLL_PX4_MIN", "TVL1_ROLL_LONG_MIN", "TVL1_FUSE", "TVL1_FUSE_MIN",
         "TVL1_BUF_LIMIT", "TVL1_POLL", "TVL1_SPEC", "TVL1_WI_NC", "TVL1_TB4", "TVL1_MID",
         "TVL1_MID_MIN", "TVL1_SPEC_TRACE", "TVL1_FILL", "TVL1_FILL_SHARED", "TVL1_STAGES")
FAST_TOL = (1e-3, 2e-2, 0.5)   # mean, p99.9, max EPE (px): tests/test_gpu_fastmath.py
STOP = dict(warps=3, iterations=40, nscales=1)
FIX10 = dict(warps=2, epsilon=0.0, iterations=10, nscales=1)
PSETS = {"stop": STOP, "fix10": FIX10}
SHAPES = [(100, 60), (241, 60), (121, 17), (241, 18), (125, 9), (100, 1), (121, 2), (100, 3),
          (241, 6), (121, 7), (125, 8)]
FULL = (320, 200, 61, dict(nscales=5, warps=5))
_oracle = {}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


def oracle_of(W, H, seed, kw, math):
    """The oracle's result, computed once per case and arithmetic (never modified)."""
    key = (W, H, seed, tuple(sorted(kw.items())), math)
    if key not in _oracle:
        I0, I1 = synth.gen_pair(W, H, seed=seed)
        _oracle[key] = checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **kw))
    return _oracle[key]


def solve(monkeypatch, env, W, H, seed, kw, math):
    set_knobs(monkeypatch, env)
    I0, I1 = synth.gen_pair(W, H, seed=seed)
    eng = capi.Engine(capi.make_params(fast_math=math, **kw))
    try:
        return eng.calc_host(I0, I1)
    finally:
        eng.close()


def assert_same(got, ref, what, checks=True):
    u, v, st, wi = got
    ur, vr, sr, wr = ref
    assert st["levels"] == sr["levels"], what
    np.testing.assert_array_equal(wi, wr, err_msg=what)
    if checks:
        assert st["checks_total"] == sr["checks_total"], what
    bad = (u.view(np.uint32) != ur.view(np.uint32)) | (v.view(np.uint32) != vr.view(np.uint32))
    if bad.any():
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"{what}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} "
                             f"y {ys.min()}..{ys.max()}")


def assert_fast(got, ref, what):
    u, v, st, wi = got
    ur, vr, sr, wr = ref
    assert st["levels"] == sr["levels"], what
    np.testing.assert_array_equal(wi, wr, err_msg=what)
    e = capi.epe(u, v, ur, vr)
    mean, p999, mx = float(e.mean()), float(np.quantile(e, 0.999)), float(e.max())
    print(f"fast vs IEEE {what}: mean {mean:.3g} p99.9 {p999:.3g} max {mx:.3g} px")
    assert np.isfinite(e).all()
    assert mean <= FAST_TOL[0] and p999 <= FAST_TOL[1] and mx <= FAST_TOL[2], what


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_stage_passes_at_band_and_segment_edges(built, monkeypatch, W, H, math):
    for name, kw in PSETS.items():
        seed = 131 * W + H
        what = f"{W}x{H}-{name}"
        on = solve(monkeypatch, "TVL1_STAGES=2,TVL1_ROLL_SEG=8", W, H, seed, kw, math)
        off = solve(monkeypatch, "TVL1_STAGES=0,TVL1_ROLL_SEG=8", W, H, seed, kw, math)
        print(f"{what}: warp iterations {on[3].tolist()} checks {on[2]['checks_total']}")
        assert_same(on, oracle_of(W, H, seed, kw, math), what + " vs oracle")
        assert_same(on, off, what + " vs TVL1_STAGES=0")


@pytest.mark.parametrize("env", ["TVL1_ROLL_SEG=8", ""], ids=["seg8", "auto"])
@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
def test_full_schedule(built, monkeypatch, math, env):
    W, H, seed, kw = FULL
    on = solve(monkeypatch, "TVL1_STAGES=2," + env, W, H, seed, kw, math)
    off = solve(monkeypatch, "TVL1_STAGES=0," + env, W, H, seed, kw, math)
    print(f"warp iterations {on[3].tolist()} checks {on[2]['checks_total']}")
    assert_same(on, oracle_of(W, H, seed, kw, math), "full schedule vs oracle")
    assert_same(on, off, "full schedule vs TVL1_STAGES=0")


def test_default_rule_takes_the_long_passes(built, monkeypatch):
    """TVL1_STAGES=1 (the default): the 4-iteration passes of the blocked levels."""
    W, H, seed, kw = FULL
    on = solve(monkeypatch, "", W, H, seed, kw, 0)
    assert_same(on, oracle_of(W, H, seed, kw, 0), "default dispatch vs oracle")


@pytest.mark.parametrize("case", [(241, 60, 131 * 241 + 60, STOP), (241, 60, 131 * 241 + 60, FIX10), FULL],
                         ids=["stop", "fix10", "full"])
def test_fast_mode_within_tolerance(built, monkeypatch, case):
    W, H, seed, kw = case
    on = solve(monkeypatch, "TVL1_STAGES=2,TVL1_ROLL_SEG=8", W, H, seed, kw, 1)
    assert_fast(on, oracle_of(W, H, seed, kw, 0), f"{W}x{H}")


MISS_RE = re.compile(r"guess ([24])/\d miss")


def test_gated_off_launch_leaves_its_outputs(built, monkeypatch, capfd):
    """TVL1_SPEC=2 enqueues a guessed pass behind every check.  A wrong guess of a 2- or
    4-iteration continuation is a k_iterate_stages launch whose gate is off: had it written
    anything, the flow or the schedule would differ from the solve with nothing enqueued
    ahead."""
    W, H, seed, kw = 320, 240, 31, dict(nscales=4, warps=10)
    set_knobs(monkeypatch, "")
    capfd.readouterr()
    spec = solve(monkeypatch, "TVL1_STAGES=2,TVL1_SPEC=2,TVL1_MID=0,TVL1_SPEC_TRACE=1", W, H, seed, kw, 0)
    err = capfd.readouterr().err
    plain = solve(monkeypatch, "TVL1_STAGES=2,TVL1_SPEC=0,TVL1_MID=0", W, H, seed, kw, 0)
    misses = MISS_RE.findall(err)
    print(f"speculation misses {spec[2]['speculation_misses']}, of a 2- or 4-iteration guess {len(misses)}")
    assert misses, "no gated 2- or 4-iteration pass ran with its gate off"
    assert plain[2]["speculation_misses"] == 0
    assert_same(spec, plain, "TVL1_SPEC=2 vs TVL1_SPEC=0")
    assert_same(spec, oracle_of(W, H, seed, kw, 0), "TVL1_SPEC=2 vs oracle")
