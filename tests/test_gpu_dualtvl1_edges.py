"""Profile 1's kernels on their geometry edges: tests/dualtvl1_cases.py's table on the GPU, bitwise
against the oracle (tests/test_dualtvl1_edges_cpu.py shows on the CPU that every size sits on the
edge it names, that no stopping decision is close, that the remap group reaches every branch of
k_remap_cubic and that a one-px slip would change the flow).

  iterate-x, iterate-y   k_iterate<G, EXACT, true>: 248-px wave segments, 32-row strips, all four
                         instantiations, with the per-iteration stopping rule and with fixed work
  degenerate             k_remap_cubic's partial branch at every px, k_median's clamps over the
                         whole window, k_gradient on one-px frames
  pyramid                k_resize_hp: the 2x area branch over odd levels (35 -> 18), the copy
                         branch, the bilinear branch with an axis at ratio 1 and with the single-tap
                         last column; u3 resized unscaled; the median inside the outer loop
  remap                  flows that leave the frame: interior, partial on every side, fully outside

Per case: u and v bit for bit where both are finite, equal finiteness masks, the oracle's levels
and per-warp iteration counts, checks_total == iterations_total.  The 0.5 odd cases and the
degenerate group also run after two different earlier solves on the same context: the 2x path
once read the pitch padding and the rows below an odd level, so their flow hung on what the arena
held.  Two cases run through tvl1_calc_f32, two through pitched device views.
"""
import numpy as np
import pytest

import dualtvl1_cases as dc
from optflow_amd import capi
from oracle import checker

torch = pytest.importorskip("torch")   # device buffers of the f32 and pitched tests

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle_of(c):
    """The oracle's result, computed once per case and never modified."""
    if c.name not in _oracle:
        _oracle[c.name] = checker.oracle_calc(*dc.frames(c), dc.params_of(c))
    return _oracle[c.name]


def mismatch(name, u, v, st, wi, ref):
    """None, or what differs from the oracle's result (test_dualtvl1_profile_matches_oracle's
    comparison: levels, per-warp counts, the finiteness masks, the bits where finite)."""
    ur, vr, sr, wr = ref
    if st["levels"] != sr["levels"] or st["sizes"] != sr["sizes"]:
        return f"{name}: levels {st['sizes']} != {sr['sizes']}"
    if not np.array_equal(wi, wr):
        return f"{name}: per-warp iterations {np.asarray(wi).tolist()} != {wr.tolist()}"
    if st["checks_total"] != st["iterations_total"] or st["iterations_total"] != sr["iterations_total"]:
        return f"{name}: {st['checks_total']} checks, {st['iterations_total']} iterations, oracle {sr['iterations_total']}"
    fin = np.isfinite(ur) & np.isfinite(vr)
    if not np.array_equal(fin, np.isfinite(u) & np.isfinite(v)):
        return f"{name}: finite mask differs"
    bad = fin & ((u.view(np.uint32) != ur.view(np.uint32)) | (v.view(np.uint32) != vr.view(np.uint32)))
    if bad.any():
        ys, xs = np.nonzero(bad)
        d = max(np.abs(u - ur)[bad].max(), np.abs(v - vr)[bad].max())
        return (f"{name}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} y {ys.min()}..{ys.max()}, "
                f"max |d| {d:.3g}")
    return None


@pytest.mark.parametrize("group", dc.GROUPS)
def test_every_case_matches_the_oracle(built, group):
    eng, bad = None, []
    try:
        for c in dc.cases_of(group):
            p = dc.params_of(c)
            if eng is None:
                eng = capi.Engine(p)
            else:
                eng.set_params(p)
            u, v, st, wi = eng.calc_host(*dc.frames(c))
            bad.append(mismatch(c.name, u, v, st, wi, oracle_of(c)))
    finally:
        if eng is not None:
            eng.close()
    bad = [b for b in bad if b]
    assert not bad, f"{len(bad)} of {len(dc.cases_of(group))} cases: " + "; ".join(bad)


# ---------------------------------------------------------------- two histories
HIST_W, HIST_H = 256, 192
HISTORY_GROUPS = {"odd-half": [c for c in dc.CASES if dc.is_odd_half(c)], "degenerate": dc.cases_of("degenerate")}


def history_pairs():
    """Earlier solves that leave the context's planes, their pitch padding and the rows below a
    small level non-zero, and different: a constant-250 pair, a noise pair."""
    const = np.full((HIST_H, HIST_W), 250, np.uint8)
    rng = np.random.default_rng(11)
    n0 = rng.integers(1, 256, (HIST_H, HIST_W), dtype=np.uint8)
    n1 = rng.integers(1, 256, (HIST_H, HIST_W), dtype=np.uint8)
    return {"constant": (const, const.copy()), "noise": (n0, n1)}


@pytest.mark.parametrize("group", list(HISTORY_GROUPS))
def test_result_does_not_depend_on_the_contexts_history(built, group):
    cases = HISTORY_GROUPS[group]
    assert len(cases) > 0
    hist = history_pairs()
    phist = capi.make_params(profile=1, nscales=2, warps=1, inner_iterations=2, outer_iterations=1,
                             scale_step=0.5, gamma=0.2, median_filtering=5)
    eng, bad = capi.Engine(phist), []
    try:
        for c in cases:
            for hname, (h0, h1) in hist.items():
                eng.set_params(phist)
                eng.calc_host(h0, h1)
                eng.set_params(dc.params_of(c))
                u, v, st, wi = eng.calc_host(*dc.frames(c))
                bad.append(mismatch(f"{c.name} after {hname}", u, v, st, wi, oracle_of(c)))
    finally:
        eng.close()
    bad = [b for b in bad if b]
    assert not bad, f"{len(bad)} of {2 * len(cases)} solves: " + "; ".join(bad)


# ---------------------------------------------------------------- tvl1_calc_f32
@pytest.mark.parametrize("name", ["pyramid-35x35-step0.5-stop", "iterate-x-249x9-gamma-stop10"])
def test_f32_frames_match_the_oracles_f32_entry(built, name):
    c = dc.case(name)
    p = dc.params_of(c)
    I0, I1 = dc.frames(c)
    rng = np.random.default_rng(5)
    F0 = (I0 / 255.0 + rng.normal(0, 2e-3, I0.shape)).astype(np.float32)   # off the u8 grid
    F1 = (I1 / 255.0 + rng.normal(0, 2e-3, I1.shape)).astype(np.float32)
    ref = checker.oracle_calc(F0, F1, p)
    H, W = I0.shape
    dev = torch.device("cuda", 0)
    eng = capi.Engine(p)
    try:
        d0, d1 = torch.from_numpy(F0).to(dev), torch.from_numpy(F1).to(dev)
        du = torch.zeros((H, W), dtype=torch.float32, device=dev)
        dv = torch.zeros_like(du)
        torch.cuda.synchronize()
        st = eng.calc_device(d0.data_ptr(), 4 * W, d1.data_ptr(), 4 * W, W, H, du.data_ptr(), dv.data_ptr(),
                             4 * W, warp_iters=True, f32=True)
        torch.cuda.synchronize()
        u, v = du.cpu().numpy(), dv.cpu().numpy()
    finally:
        eng.close()
    assert mismatch(name, u, v, st, st["warp_iters"], ref) is None, mismatch(name, u, v, st, st["warp_iters"], ref)
    assert ref[2]["levels"] == (2 if c.group == "pyramid" else 1)


# ---------------------------------------------------------------- pitched views
SENTINEL = -12345.5


@pytest.mark.parametrize("name", ["pyramid-39x67-step0.5-stop", "iterate-y-65x33-plain-stop10"])
def test_pitched_views(built, name):
    """Frames 3 bytes into rows of a wider parent, flows into a wider parent pre-filled with a
    sentinel: the oracle's bits inside the view, the sentinel everywhere else."""
    c = dc.case(name)
    p = dc.params_of(c)
    I0, I1 = dc.frames(c)
    H, W = I0.shape
    ipitch, fcols, top, off = W + 29, W + 7, 2, 3      # bytes per frame row; floats per flow row
    dev = torch.device("cuda", 0)
    parents = []
    for I in (I0, I1):
        par = np.full((H + 2 * top, ipitch), 0xA5, np.uint8)
        par[top:top + H, off:off + W] = I
        parents.append(torch.from_numpy(par).to(dev))
    outs = [torch.full((H + 2 * top, fcols), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    eng = capi.Engine(p)
    try:
        torch.cuda.synchronize()
        st = eng.calc_device(parents[0].data_ptr() + top * ipitch + off, ipitch,
                             parents[1].data_ptr() + top * ipitch + off, ipitch, W, H,
                             outs[0].data_ptr() + 4 * (top * fcols + off), outs[1].data_ptr() + 4 * (top * fcols + off),
                             4 * fcols, warp_iters=True)
        torch.cuda.synchronize()
        pu, pv = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    finally:
        eng.close()
    u, v = pu[top:top + H, off:off + W], pv[top:top + H, off:off + W]
    err = mismatch(name, np.ascontiguousarray(u), np.ascontiguousarray(v), st, st["warp_iters"], oracle_of(c))
    assert err is None, err
    for par in (pu, pv):
        keep = np.ones(par.shape, bool)
        keep[top:top + H, off:off + W] = False
        assert np.all(par[keep] == np.float32(SENTINEL))
    for t, I in zip(parents, (I0, I1)):   # the frames' parents are read-only to the solve
        par = t.cpu().numpy()
        assert np.array_equal(par[top:top + H, off:off + W], I) and (par == 0xA5).sum() == par.size - W * H + (I == 0xA5).sum()
