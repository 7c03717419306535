"""tvl1_calc_init: a solve that starts from a caller-supplied flow must be the
seeded reference bit for bit -- flow and per-warp iteration counts; in IEEE the oracle's stages
composed (tests/initflow_ref.py), in fma mode the oracle's own seeded entry
(checker.oracle_calc(init=...)) -- and must leave tvl1_calc exactly as it was."""
import numpy as np
import pytest

import initflow_ref as ref
from optflow_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def run(eng, I0, I1, seed=None, pitch_extra=0, inplace=False):
    """tvl1_calc (seed None) or tvl1_calc_init on device buffers -> (u, v, stats)."""
    h, w = I0.shape
    d0, d1 = dev(I0), dev(I1)
    du = torch.zeros((h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    init = None
    if seed is not None:
        if inplace:
            du.copy_(dev(seed[0]))
            dv.copy_(dev(seed[1]))
            init = (du.data_ptr(), dv.data_ptr(), 4 * w)
        else:
            ex = pitch_extra // 4
            keep = [torch.full((h, w + ex), float("nan"), dtype=torch.float32, device=d0.device)
                    for _ in range(2)]
            keep[0][:, :w] = dev(seed[0])
            keep[1][:, :w] = dev(seed[1])
            init = (keep[0].data_ptr(), keep[1].data_ptr(), 4 * w + pitch_extra)
    torch.cuda.synchronize()
    st = eng.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, du.data_ptr(), dv.data_ptr(),
                         4 * w, warp_iters=True, init=init)
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


@pytest.mark.parametrize("name", list(ref.SINGLE))
def test_seeded_solve_matches_the_composed_reference(built, name):
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0)
    eng = capi.Engine(capi.make_params(**c["kw"]))
    u, v, st = run(eng, I0, I1, (u0, v0), pitch_extra=c.get("pitch_extra", 0))
    eng.close()
    assert st["levels"] == wr.shape[0]
    np.testing.assert_array_equal(st["warp_iters"], wr)
    assert bits_equal(u, ur) and bits_equal(v, vr)


@pytest.mark.parametrize("name", list(ref.SINGLE))
def test_seeded_solve_matches_the_oracle_in_fma(built, name):
    """fast_math 2: the seed chain (k_flow_down<true>) and every contracted gather under a seed,
    bitwise against the oracle's seeded entry."""
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0, math=2)
    eng = capi.Engine(capi.make_params(fast_math=2, **c["kw"]))
    u, v, st = run(eng, I0, I1, (u0, v0), pitch_extra=c.get("pitch_extra", 0))
    eng.close()
    assert st["levels"] == wr.shape[0]
    np.testing.assert_array_equal(st["warp_iters"], wr)
    assert bits_equal(u, ur) and bits_equal(v, vr)


@pytest.mark.parametrize("name", ["w97_rough", "one_level_pitched"])
def test_in_place_flow_in_fma(built, name):
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    eng = capi.Engine(capi.make_params(fast_math=2, **c["kw"]))
    b = run(eng, I0, I1, (u0, v0), inplace=True)
    eng.close()
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0, math=2)
    np.testing.assert_array_equal(b[2]["warp_iters"], wr)
    assert bits_equal(b[0], ur) and bits_equal(b[1], vr)


@pytest.mark.parametrize("name", ["w97_rough", "one_level_pitched"])
def test_in_place_flow(built, name):
    """u0 is u, v0 is v (OpenCV's in/out flow): the same bits as separate buffers; with more
    than one level and with one (where the seed is copied)."""
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    eng = capi.Engine(capi.make_params(**c["kw"]))
    a = run(eng, I0, I1, (u0, v0))
    b = run(eng, I0, I1, (u0, v0), inplace=True)
    eng.close()
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2]["warp_iters"], b[2]["warp_iters"])
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0)
    assert bits_equal(b[0], ur) and bits_equal(b[1], vr)


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("w,h,kw", [(97, 40, dict(nscales=3, warps=3)), (50, 30, dict(nscales=1))])
def test_zero_seed_is_tvl1_calc(built, math, w, h, kw):
    """The chain of a zero seed is zero in every arithmetic mode, so tvl1_calc_init must give
    tvl1_calc's flow and per-warp counts bitwise."""
    I0, I1 = synth.gen_pair(w, h, seed=77 + w)
    eng = capi.Engine(capi.make_params(fast_math=math, **kw))
    a = run(eng, I0, I1)
    z = np.zeros((h, w), np.float32)
    b = run(eng, I0, I1, (z, z))
    eng.close()
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2]["warp_iters"], b[2]["warp_iters"])
    assert a[2]["iterations_total"] == b[2]["iterations_total"]
    assert a[2]["checks_total"] == b[2]["checks_total"]


@pytest.mark.parametrize("math", [1])
def test_seed_reaches_the_solver_in_every_mode(built, math):
    """fast_math 1 has no seeded reference: the seeded solve is deterministic, the same in
    place, and not the unseeded one.  (fast_math 2 is held to the oracle bitwise above.)"""
    c = ref.SINGLE["w97_smooth"]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    eng = capi.Engine(capi.make_params(fast_math=math, **c["kw"]))
    a = run(eng, I0, I1, (u0, v0))
    b = run(eng, I0, I1, (u0, v0), inplace=True)
    n = run(eng, I0, I1)
    eng.close()
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2]["warp_iters"], b[2]["warp_iters"])
    assert not bits_equal(a[0], n[0])


def test_host_call_and_bad_arguments(built):
    """tvl1_calc_host_init equals the device call; profile 1 and bad seeds are TVL1_EINVAL on a
    live ctx, and the ctx still solves afterwards."""
    c = ref.SINGLE["w97_rough"]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    ur, vr, wr, _ = ref.reference(("single", "w97_rough"), I0, I1, c["kw"], u0, v0)
    eng = capi.Engine(capi.make_params(**c["kw"]))
    h, w = I0.shape
    with pytest.raises(capi.TVL1Error, match="TVL1_EINVAL"):
        eng.calc_host(I0, I1, init=(u0, v0, 4 * w - 4))
    u, v, st, wi = eng.calc_host(I0, I1, init=(u0, v0))
    assert bits_equal(u, ur) and bits_equal(v, vr)
    np.testing.assert_array_equal(wi, wr)
    eng.set_params(capi.make_params(profile=1, **c["kw"]))
    with pytest.raises(capi.TVL1Error, match="profile 1"):
        eng.calc_host(I0, I1, init=(u0, v0))
    eng.close()


def test_no_seed_state_leaks_into_tvl1_calc(built):
    """A tvl1_calc after a tvl1_calc_init on the same ctx equals a fresh ctx's tvl1_calc."""
    c = ref.SINGLE["w97_rough"]
    I0, I1 = ref.frames_of(c)
    p = capi.make_params(**c["kw"])
    fresh = capi.Engine(p)
    a = run(fresh, I0, I1)
    fresh.close()
    eng = capi.Engine(p)
    run(eng, I0, I1, ref.seed_of(c))
    b = run(eng, I0, I1)
    eng.close()
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2]["warp_iters"], b[2]["warp_iters"])
