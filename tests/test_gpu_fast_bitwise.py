"""fast_math = 1 held bit for bit: every FM = kFast kernel against the oracle's fast branch
evaluated with the device's own v_rcp_f32 / v_sqrt_f32 (checker.oracle_calc(approx="device"):
oracle/fast_prims.hip's two element-wise kernels supply the instructions, the oracle restates
everything around them; tests/test_oracle_fast_cpu.py pins that structure on the CPU).

Fast mode differs from fma mode in four expressions (csrc/tvl1_kernels.hpp, approx(FM)): the
warp's coeff = rcp(wsum), the TH step's fi = -rho * rcp(grad), the projection's g = sqrt(..)
and p' = fma(taut, du, p) * rcp(ng).  The tables are the other files' own -- frames, seeds,
parameter sets and knob sets are imported, not restated:
  primitives     the two instructions within 1 ulp of the float64-rounded result, and repeatable
  single pair    tests/edge_cases.py, every (group, knob set), every case; the gamma and tau < 0
                 cases, with fast_math = 1 requested, bitwise the IEEE oracle (math_of's rule)
  stages         test_gpu_stages.py's SHAPES x PSETS and FULL on k_iterate_stages, FULL by default
  batch          edge_cases.py's batch table, kb_small_level's on-chip sizes, the 260-pair batch
  warp window    tests/warp_window.py, every row and parameter set, from the seeded reference
  guard paths    test_gpu_guard_paths.py's INPUTS x ENVS
  schedules      test_gpu_fastmath.py's cases but the 512 x 512 one (the reference pays two
                 host-device round trips per iteration), median 3, f32 frames, initflow_ref's
                 strip6 pairs from their seeds
Every comparison: levels and level sizes, per-warp iteration counts, u and v as uint32.

Margins are a condition on the inputs: the engine and the reference sum the residual in
different orders, so a stopping decision is comparable only while every check of the fast
reference's own trace clears test_residual_margin_cpu.MIN_MARGIN.  Each stopping-rule case
asserts that; none is left out.  With TVL1_FAST_MARGINS_OUT=<file> the minimum margin per table
is written there as JSON (profiles/fast_reference/margins.json).
"""
import json
import os

import numpy as np
import pytest

import edge_cases as ec
import initflow_ref as ir
import test_gpu_batch as gb
import test_gpu_edge_cases as ge
import test_gpu_fastmath as fm
import test_gpu_guard_paths as gg
import test_gpu_stages as gs
import test_gpu_warp_window as gw
import warp_window as ww
from optflow_amd import capi, synth
from oracle import checker
from test_gpu_parity import MID_ALL
from test_residual_margin_cpu import MIN_MARGIN

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KNOBS = tuple(sorted(set(ge.KNOBS) | set(gs.KNOBS) | set(gg.KNOBS) | set(fm.KNOBS)))
_ref, _ieee, _margin = {}, {}, {}


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


@pytest.fixture(scope="module", autouse=True)
def margins_out():
    yield
    out = os.environ.get("TVL1_FAST_MARGINS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"min_margin_required": MIN_MARGIN,
                       "tables": {k: {"checks": n, "min_margin": m} for k, (n, m) in sorted(_margin.items())}},
                      f, indent=1)


def stays_ieee(kw):
    """math_of's rule: gamma != 0 and tau / theta < 0 solves run the IEEE kernels."""
    return kw.get("gamma", 0.0) != 0 or kw.get("tau", 0.25) < 0


def fast_ref(table, key, I0, I1, kw, init=None):
    """(u, v, stats, warp_iters, min margin) of the fast reference, computed once per key and
    never modified; its check trace's margins go to the table's minimum."""
    if (table, key) not in _ref:
        p = capi.make_params(fast_math=1, **kw)
        u, v, st, wi, tr = checker.oracle_check_trace(I0, I1, p, init=init, approx="device")
        m = checker.check_margins(tr, p.iterations)
        mm = float(m.min()) if len(m) else float("inf")
        for a in (u, v, wi):
            a.setflags(write=False)
        n0, m0 = _margin.get(table, (0, float("inf")))
        _margin[table] = (n0 + len(m), min(m0, mm))
        _ref[(table, key)] = (u, v, st, wi, mm)
    return _ref[(table, key)]


def ieee_ref(key, I0, I1, kw, init=None):
    if key not in _ieee:
        _ieee[key] = checker.oracle_calc(I0, I1, capi.make_params(**kw), init=init)
    return _ieee[key]


def compare(table, name, kw, got, I0, I1, key=None, init=None):
    """None, or what is wrong: a check of the reference too close to a threshold (the input's
    fault), or ge.mismatch's report -- levels, per-warp counts, how many px differ and their box."""
    u, v, st, wi = got
    key = key if key is not None else name
    if stays_ieee(kw):
        return ge.mismatch(name + " (IEEE)", kw, u, v, st, wi, ieee_ref((table, key), I0, I1, kw, init))
    ur, vr, sr, wr, mm = fast_ref(table, key, I0, I1, kw, init)
    if mm < MIN_MARGIN:
        return f"{name}: a check of the fast reference sits {mm:.3g} from a threshold (< {MIN_MARGIN})"
    return ge.mismatch(name, kw, u, v, st, wi, (ur, vr, sr, wr))


def report(bad, what):
    bad = [b for b in bad if b]
    assert not bad, f"[{what}] {len(bad)} mismatches: " + "; ".join(bad)


# ---------------------------------------------------------------- the two instructions
def sweep():
    """2^16 positive floats: the significand of [1, 2) walked in steps of 2^8 ulp; 399
    significands of every binade 2^-20 .. 2^20; wsum's neighbourhood, 1 +- 8204 ulp."""
    one = np.float32(1.0).view(np.uint32).astype(np.int64)
    walk = one + (np.arange(1 << 15, dtype=np.int64) << 8)
    sig = np.linspace(0, (1 << 23) - 1, 399).astype(np.int64)
    binades = np.concatenate([(np.int64(127 + e) << 23) + sig for e in range(-20, 21)])
    near1 = one + np.arange(-8204, 8205, dtype=np.int64)
    x = np.concatenate([walk, binades, near1]).astype(np.uint32).view(np.float32)
    assert x.size == 1 << 16
    return x


def ulp_diff(a, b):
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64))


def test_device_primitives_within_one_ulp(built):
    rcp, sqrt = checker.device_prims()
    x = sweep()
    for fn, exact in ((rcp, 1.0 / x.astype(np.float64)), (sqrt, np.sqrt(x.astype(np.float64)))):
        got = checker.prim_apply(fn, x)
        d = ulp_diff(got, exact.astype(np.float32))
        print(f"{fn.__name__}: {int((d != 0).sum())} of {x.size} differ from the rounded result, max {int(d.max())} ulp")
        assert np.isfinite(got).all() and (got > 0).all()
        assert d.max() <= 1, x[np.argmax(d)]
        assert np.array_equal(checker.prim_apply(fn, x).view(np.uint32), got.view(np.uint32))
    # the selections' operands: rcp(+0) = +inf (grad = 0), sqrt(+0) = +0 (a constant u)
    z = np.zeros(3, np.float32)
    assert np.all(checker.prim_apply(rcp, z) == np.inf)
    assert np.array_equal(checker.prim_apply(sqrt, z).view(np.uint32), z.view(np.uint32))


# ---------------------------------------------------------------- single-pair edge table
@pytest.mark.parametrize("group,knobs", ge.SINGLE, ids=[f"{g}-{kn or 'default'}" for g, kn in ge.SINGLE])
def test_single_pair_edges(built, monkeypatch, group, knobs):
    set_knobs(monkeypatch, knobs)
    eng, bad = None, []
    try:
        for c in ec.cases_of(group):
            I0, I1 = ec.frames(c)
            p = capi.make_params(fast_math=1, **c.params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            bad.append(compare("edge_cases", c.name, c.params, eng.calc_host(I0, I1), I0, I1))
    finally:
        if eng is not None:
            eng.close()
    report(bad, knobs)


# ---------------------------------------------------------------- k_iterate_stages
STAGES_ON = "TVL1_STAGES=2,TVL1_ROLL_SEG=8"


@pytest.mark.parametrize("W,H", gs.SHAPES, ids=[f"{w}x{h}" for w, h in gs.SHAPES])
def test_stage_passes(built, monkeypatch, W, H):
    bad = []
    for name, kw in gs.PSETS.items():
        seed = 131 * W + H
        I0, I1 = synth.gen_pair(W, H, seed=seed)
        got = gs.solve(monkeypatch, STAGES_ON, W, H, seed, kw, 1)
        bad.append(compare("stages", f"{W}x{H}-{name}", kw, got, I0, I1))
    report(bad, STAGES_ON)


@pytest.mark.parametrize("env", [STAGES_ON, ""], ids=["stages", "default"])
def test_stage_full_schedule(built, monkeypatch, env):
    W, H, seed, kw = gs.FULL
    I0, I1 = synth.gen_pair(W, H, seed=seed)
    report([compare("stages", "full", kw, gs.solve(monkeypatch, env, W, H, seed, kw, 1), I0, I1)], env)


# ---------------------------------------------------------------- batch tables
def batch_compare(table, name, kw, I0s, I1s, u, v, st, sel=None):
    return [compare(table, f"{name} pair {b}", kw, (u[b], v[b], st[b], st[b]["warp_iters"]), I0s[b], I1s[b],
                    key=(name, b)) for b in (sel if sel is not None else range(I0s.shape[0]))]


@pytest.mark.parametrize("knobs", ec.BATCH_KNOBS)
@pytest.mark.parametrize("group", ec.BATCH_GROUPS)
def test_batch_edges(built, monkeypatch, group, knobs):
    set_knobs(monkeypatch, knobs)
    eng, bad = None, []
    try:
        for c in ec.batch_cases_of(group):
            I0s, I1s = ec.batch_frames(c)
            p = capi.make_params(fast_math=1, **c.params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            u, v, st = ge.run_batch(eng, I0s, I1s)
            bad += batch_compare("batch_edges", c.name, c.params, I0s, I1s, u, v, st)
    finally:
        if eng is not None:
            eng.close()
    report(bad, knobs)


def _marks(test):
    return {m.args[0].split(",")[0]: m.args[1] for m in test.pytestmark if m.name == "parametrize"}


ON_CHIP = _marks(gb.test_batch_coarsest_level_on_chip_edges)


@pytest.mark.parametrize("w,h", ON_CHIP["w"])
def test_batch_on_chip_level(built, monkeypatch, w, h):
    set_knobs(monkeypatch, "")
    bad = []
    for i, kw in enumerate(ON_CHIP["kw"]):
        eng = capi.Engine(capi.make_params(fast_math=1, **kw))
        try:
            I0s, I1s = gb.pairs(3, w, h, seed=w * 131 + h)
            u, v, st = gb.run_batch(eng, I0s, I1s)
        finally:
            eng.close()
        bad += batch_compare("batch_on_chip", f"{w}x{h}-{i}", kw, I0s, I1s, u, v, st)
    report(bad, "kb_small_level")


def test_batch_two_chunks(built, monkeypatch):
    """test_gpu_batch.test_batch_larger_than_one_chunk's 260 pairs at its 8 selected pairs."""
    set_knobs(monkeypatch, "")
    kw = gb.TWO_CHUNKS["kw"]
    eng = capi.Engine(capi.make_params(fast_math=1, **kw))
    try:
        I0s, I1s = gb.two_chunk_pairs()
        u, v, st = gb.run_batch(eng, I0s, I1s)
    finally:
        eng.close()
    assert np.all(u[5] == 0) and np.all(st[5]["warp_iters"] == 2)
    report(batch_compare("batch_two_chunks", "260", kw, I0s, I1s, u, v, st, sel=gb.TWO_CHUNKS["sel"]), "260 pairs")


# ---------------------------------------------------------------- warp-window table
@pytest.mark.parametrize("name", [r.name for r in ww.ROWS])
def test_window_edge_seeds(built, monkeypatch, name):
    row = ww.ROW_OF[name]
    set_knobs(monkeypatch, row.knobs)
    eng, bad, ran = None, [], 0
    try:
        for pname, params in row.psets.items():
            p = capi.make_params(fast_math=1, **params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            prs = [ww.frames(row, b) for _, b in ww.solves(row)]
            sds = [ww.make_seed(row.geom, kind, row.W, row.H) for kind, _ in ww.solves(row)]
            if row.batch:
                u, v, st = gw.run_batch(eng, np.stack([a for a, _ in prs]), np.stack([b for _, b in prs]),
                                        np.stack([s[0] for s in sds]), np.stack([s[1] for s in sds]))
            for i, (kind, b) in enumerate(ww.solves(row)):
                if row.batch:
                    got = (u[b], v[b], st[b], st[b]["warp_iters"])
                else:
                    ui, vi, sti = gw.run_single(eng, *prs[i], sds[i])
                    got = (ui, vi, sti, sti["warp_iters"])
                # rows of one geometry and size share the reference
                bad.append(compare("warp_window", f"{pname} {kind}", params, got, *prs[i],
                                   key=(row.geom, row.W, row.H, pname, kind, b), init=sds[i]))
                ran += 1
    finally:
        if eng is not None:
            eng.close()
    assert ran == len(row.psets) * len(row.seeds)
    report(bad, row.knobs)


# ---------------------------------------------------------------- guard-path inputs
@pytest.mark.parametrize("env", gg.ENVS)
@pytest.mark.parametrize("name", list(gg.INPUTS))
def test_guard_path_inputs(built, monkeypatch, name, env):
    set_knobs(monkeypatch, env)
    I0, I1 = gg.pair_of(name)
    kw = gg.INPUTS[name][1]
    eng = capi.Engine(capi.make_params(fast_math=1, **kw))
    try:
        u, v, st, wi = eng.calc_host(I0, I1)
    finally:
        eng.close()
    ur, vr, sr, wr, mm = fast_ref("guard_paths", name, I0, I1, kw)
    assert mm >= MIN_MARGIN, f"a check of the fast reference sits {mm:.3g} from a threshold"
    assert st["sizes"] == sr["sizes"]
    np.testing.assert_array_equal(wi, wr)
    fin = np.isfinite(ur) & np.isfinite(vr)
    assert np.array_equal(fin, np.isfinite(u) & np.isfinite(v))
    bad = fin & ((u.view(np.uint32) != ur.view(np.uint32)) | (v.view(np.uint32) != vr.view(np.uint32)))
    if bad.any():
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"{name}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} "
                             f"y {ys.min()}..{ys.max()}")
    if name == "identical":
        assert np.all(u == 0) and np.all(v == 0)


# ---------------------------------------------------------------- whole schedules
SCHED_ENVS = fm.ENVS + [MID_ALL, "TVL1_STAGES=2"]
SCHED = [c for c in fm.CASES if (c[0], c[1]) != (512, 512)] + [(96, 64, 9, dict(median_filtering=3, nscales=4, warps=3))]


@pytest.mark.parametrize("env", SCHED_ENVS)
@pytest.mark.parametrize("W,H,seed,kw", SCHED, ids=[f"{c[0]}x{c[1]}-m{c[3].get('median_filtering', 1)}" for c in SCHED])
def test_whole_schedule(built, monkeypatch, W, H, seed, kw, env):
    set_knobs(monkeypatch, env)
    I0, I1 = synth.gen_pair(W, H, seed=seed)
    eng = capi.Engine(capi.make_params(fast_math=1, **kw))
    try:
        got = eng.calc_host(I0, I1)
    finally:
        eng.close()
    report([compare("schedules", f"{W}x{H}", kw, got, I0, I1, key=(W, H, seed, tuple(sorted(kw.items()))))], env)


@pytest.mark.parametrize("env", SCHED_ENVS)
def test_whole_schedule_f32_frames(built, monkeypatch, env):
    set_knobs(monkeypatch, env)
    W, H, kw = 150, 67, dict(nscales=4, warps=3)
    I0, I1 = synth.gen_pair(W, H, seed=23)
    F0, F1 = (I0.astype(np.float32) / np.float32(255)), (I1.astype(np.float32) / np.float32(255))
    eng = capi.Engine(capi.make_params(fast_math=1, **kw))
    try:
        d0, d1 = gw.dev(F0), gw.dev(F1)
        du = torch.zeros((H, W), dtype=torch.float32, device=d0.device)
        dv = torch.zeros_like(du)
        torch.cuda.synchronize()
        st = eng.calc_device(d0.data_ptr(), 4 * W, d1.data_ptr(), 4 * W, W, H, du.data_ptr(), dv.data_ptr(), 4 * W,
                             warp_iters=True, f32=True)
        torch.cuda.synchronize()
    finally:
        eng.close()
    report([compare("schedules", "f32", kw, (du.cpu().numpy(), dv.cpu().numpy(), st, st["warp_iters"]), F0, F1)], env)


@pytest.mark.parametrize("env", SCHED_ENVS)
def test_whole_schedule_seeded_strips(built, monkeypatch, env):
    """initflow_ref's strip6 pairs, each solved singly from its own seed."""
    set_knobs(monkeypatch, env)
    case = ir.BATCH["strip6"]
    eng = capi.Engine(capi.make_params(fast_math=1, **case["kw"]))
    bad = []
    try:
        for b in range(case["n"]):
            (I0, I1), (u0, v0) = ir.batch_pair(case, b)
            got = eng.calc_host(I0, I1, init=(u0, v0))
            bad.append(compare("schedules", f"strip6 pair {b}", case["kw"], got, I0, I1, init=(u0, v0)))
    finally:
        eng.close()
    report(bad, env)
