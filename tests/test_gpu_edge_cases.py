"""The solve kernels at band, tile and segment edges and on tiny frames: tests/edge_cases.py's
table on the GPU, bitwise against the oracle (tests/test_edge_cases_cpu.py shows on the CPU
that every size is an edge of the planner and that no stopping decision is close).

Single pair: one test per (group, knob set, arithmetic) -- one engine, every size of the group
through tvl1_calc_host.  A group runs only under the knob sets whose kernels it was built for
(edge_cases.KNOBS_OF):
  x64           k_warp_ring<6,2> (default / TVL1_ROLL_SEG=8), k_warp_img (TVL1_BUF_LIMIT=0)
  x124          k_iterate_roll<G,1|2,2> (default), k_warp_iter<6,.,128,.,2> with two consumer
                wavefronts (TVL1_FUSE_MIN=0) and one (+ TVL1_WI_NC=1)
  x120          k_iterate_roll<G,3|4,2> (TVL1_ROLL_LONG_MIN=0), k_iterate_roll_mid (MID_ALL)
  x248          k_iterate_roll<G,1|2,4> (TVL1_ROLL_PX4_MIN=0)
  x56           k_iterate_tb4 (default, passes of >= 3 iterations; TVL1_BUF_LIMIT=0: every
                pass), k_iterate_tb<false|true,32,1,2> (TVL1_TB4=0 / gamma; with
                TVL1_BUF_LIMIT=0 every pass)
  x248-iterate  k_iterate<false|true,true> (tau < 0, without and with gamma)
  y-stream      all the streaming kernels above with TVL1_ROLL_SEG=8, k_warp_img's 16 rows
  y-tb4, y-tb, y-iterate   the blocked kernels' output rows, k_iterate's 32-row strips
  corner, degenerate, pyramid   both edges at once; frames under a halo; coarse levels on an edge
Batch: three pairs per size through tvl1_calc_batch with TVL1_BATCH_SMALL=0 -- kb_warp_iter and
kb_iterate_roll<K,1> (default), kb_iterate_roll<K,2> (TVL1_BATCH_PX1_W=0), kb_warp_ring
(TVL1_BATCH_FUSE=0; fixed work always), segments of 8 rows (TVL1_BATCH_SEG_MIN=8).

Per case: the oracle's levels and sizes, its per-warp iteration counts, and its u and v bit for
bit (on its finite mask where tau < 0).  fast_math = 1 runs this table bitwise against the
oracle's fast branch in tests/test_gpu_fast_bitwise.py; profile 1 has its own tests.
"""
import re

import numpy as np
import pytest

import edge_cases as ec
from optflow_amd import capi
from oracle import checker

torch = pytest.importorskip("torch")   # device buffers of the batch tests

pytestmark = pytest.mark.gpu

# every knob a set here may touch, cleared first (tests/test_gpu_parity.py's, plus the batch's)
KNOBS = ("TVL1_ROLL_SEG", "TVL1_ROLL_PX4_MIN", "TVL1_ROLL_LONG_MIN", "TVL1_FUSE", "TVL1_FUSE_MIN",
         "TVL1_BUF_LIMIT", "TVL1_BATCH_FUSE", "TVL1_POLL", "TVL1_SPEC", "TVL1_WI_NC", "TVL1_TB4",
         "TVL1_MID", "TVL1_MID_MIN", "TVL1_SPEC_TRACE", "TVL1_BATCH_STORE", "TVL1_BATCH_GROUP",
         "TVL1_BATCH_PX1_W", "TVL1_BATCH_SEG_MIN", "TVL1_BATCH_SMALL", "TVL1_FILL", "TVL1_FILL_SHARED")
MATH_IDS = {0: "ieee", 2: "fma"}
MID_RE = re.compile(r"mid-check passes (\d+),")
_oracle = {}


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


def oracle_of(key, I0, I1, params, math):
    """The oracle's result, computed once per (case[, pair], arithmetic) and never modified."""
    if (key, math) not in _oracle:
        _oracle[(key, math)] = checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **params))
    return _oracle[(key, math)]


def mismatch(name, params, u, v, st, wi, ref):
    """None, or what differs from the oracle's result: levels, per-warp counts, or where the
    flow's bits differ (how many px, and the box that holds them)."""
    ur, vr, sr, wr = ref
    if st["levels"] != sr["levels"] or st["sizes"] != sr["sizes"]:
        return f"{name}: levels {st['sizes']} != {sr['sizes']}"
    if not np.array_equal(wi, wr):
        return f"{name}: per-warp iterations {np.asarray(wi).tolist()} != {wr.tolist()}"
    ok = np.ones(ur.shape, bool)
    if params.get("tau", 0.25) < 0:   # compared on the oracle's finite mask
        ok = np.isfinite(ur) & np.isfinite(vr)
        if not np.array_equal(ok, np.isfinite(u) & np.isfinite(v)):
            return f"{name}: finite mask differs"
    bad = ok & ((u.view(np.uint32) != ur.view(np.uint32)) | (v.view(np.uint32) != vr.view(np.uint32)))
    if bad.any():
        ys, xs = np.nonzero(bad)
        d = max(np.abs(u - ur)[bad].max(), np.abs(v - vr)[bad].max())
        return (f"{name}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} y {ys.min()}..{ys.max()}, "
                f"max |d| {d:.3g}")
    return None


SINGLE = [(g, kn) for g in ec.GROUPS for kn in ec.KNOBS_OF[g]]


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
@pytest.mark.parametrize("group,knobs", SINGLE, ids=[f"{g}-{kn or 'default'}" for g, kn in SINGLE])
def test_single_pair_edges(built, monkeypatch, capfd, group, knobs, math):
    """Fixed-work cases also run with profiling on: kernel_launches[0] counts the iteration
    passes (launch_pass), and with epsilon = 0 nothing is fused, speculated or run as a
    mid-check pass under any knob set, so it must be levels x warps x the passes sched_after
    gives (10 iterations: 4, 4, 2; one iteration per pass where tau < 0) -- the proof that
    passes of the intended lengths ran.  (With epsilon > 0 the count also holds fused, gated
    and repeated passes, so it is not asserted there.)  Under the mid-check knob set the
    engine's trace must show that mid-check passes ran (k_iterate_roll_mid)."""
    mid = "TVL1_MID=1" in knobs.split(",")
    set_knobs(monkeypatch, knobs + (",TVL1_SPEC_TRACE=1" if mid else ""))
    capfd.readouterr()
    eng, bad = None, []
    try:
        for c in ec.cases_of(group):
            I0, I1 = ec.frames(c)
            p = capi.make_params(fast_math=math, **c.params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            fixed = c.params.get("epsilon", 0.01) == 0
            eng.set_profiling(fixed)
            u, v, st, wi = eng.calc_host(I0, I1)
            bad.append(mismatch(c.name, c.params, u, v, st, wi, oracle_of(c.name, I0, I1, c.params, math)))
            if fixed:
                passes = ec.fixed_work_passes(c.params["iterations"], ec.kmax_of(c.params))
                if st["kernel_launches"][0] != st["levels"] * c.params["warps"] * len(passes):
                    bad.append(f"{c.name}: {st['kernel_launches'][0]} iteration passes, schedule {passes} per warp")
    finally:
        if eng is not None:
            eng.close()
    bad = [b for b in bad if b]
    assert not bad, f"[{knobs}] {len(bad)} of {len(ec.cases_of(group))} cases: " + "; ".join(bad)
    if mid:
        n_mid = sum(int(m) for m in MID_RE.findall(capfd.readouterr().err))
        print(f"{group}: {n_mid} mid-check passes")
        assert n_mid > 0, "no mid-check pass ran"


def run_batch(eng, I0s, I1s):
    n, h, w = I0s.shape
    dev = torch.device("cuda", 0)
    d0 = torch.from_numpy(np.ascontiguousarray(I0s)).to(dev)
    d1 = torch.from_numpy(np.ascontiguousarray(I1s)).to(dev)
    du = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    dv = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = eng.calc_batch_device(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h,
                               du.data_ptr(), dv.data_ptr(), 4 * w, 4 * w * h, warp_iters=True)
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
@pytest.mark.parametrize("knobs", ec.BATCH_KNOBS)
@pytest.mark.parametrize("group", ec.BATCH_GROUPS)
def test_batch_edges(built, monkeypatch, group, knobs, math):
    """Each pair of a batch bitwise the oracle's, with its per-warp counts, whatever the other
    pairs of the launch do (batch-mixed: an identical and a constant pair stop at each warp's
    first check while the textured pair runs on)."""
    set_knobs(monkeypatch, knobs)
    eng, bad = None, []
    try:
        for c in ec.batch_cases_of(group):
            I0s, I1s = ec.batch_frames(c)
            p = capi.make_params(fast_math=math, **c.params)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            u, v, st = run_batch(eng, I0s, I1s)
            for b in range(ec.BATCH_N):
                ref = oracle_of((c.name, b), I0s[b], I1s[b], c.params, math)
                bad.append(mismatch(f"{c.name} pair {b}", c.params, u[b], v[b], st[b], st[b]["warp_iters"], ref))
            if group == "batch-mixed":
                assert np.all(st[0]["warp_iters"] == 2) and np.all(st[2]["warp_iters"] == 2), c.name
                assert st[1]["warp_iters"].max() > 2, c.name
    finally:
        if eng is not None:
            eng.close()
    bad = [b for b in bad if b]
    assert not bad, f"[{knobs}] {len(bad)} mismatches: " + "; ".join(bad)
