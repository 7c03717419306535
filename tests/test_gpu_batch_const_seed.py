"""tvl1_calc_batch_const_init and tvl1_calc_batch_auto_init: every pair of a batch seeded by
one constant per pair is the seeded solve from two planes filled with that constant, bit for
bit -- against tests/initflow_ref.py in IEEE, the oracle's seeded entry in fma mode, and
tvl1_calc_batch_init from filled planes (the same kernels after the first step) in fast mode.
tests/test_batch_const_seed_cpu.py holds the cases (tests/const_seed_cases.py) to the
condition that makes this tell kb_flow_down_const from a fill.  The auto route: records equal
to tests/shift_ref.py and tvl1_estimate_shift_batch, flows equal to the const route from them."""
import ctypes as C

import numpy as np
import pytest

import const_seed_cases as cs
import shift_ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENV_KEYS = ("TVL1_BATCH_SMALL", "TVL1_BATCH_FUSE")
ENVS = ["", "TVL1_BATCH_SMALL=0", "TVL1_BATCH_FUSE=0"]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


def run_batch(eng, I0s, I1s, n, **seed):
    """n pairs; a frame stack of one entry is shared by every pair (pair stride 0).  seed:
    init_const=(n, 2) | auto_shift=R | planes=(U0, V0) | nothing."""
    h, w = I0s.shape[1:]
    d0, d1 = dev(I0s), dev(I1s)
    du = torch.zeros((n, h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    keep = None
    if "planes" in seed:
        keep = [dev(a) for a in seed.pop("planes")]
        seed["init"] = (keep[0].data_ptr(), keep[1].data_ptr(), 4 * w, 4 * w * h)
    torch.cuda.synchronize()
    r = eng.calc_batch_device(n, d0.data_ptr(), w, w * h if len(I0s) > 1 else 0, d1.data_ptr(), w,
                              w * h if len(I1s) > 1 else 0, w, h, du.data_ptr(), dv.data_ptr(),
                              4 * w, 4 * w * h, warp_iters=True, **seed)
    torch.cuda.synchronize()
    st, shifts = r if isinstance(r, tuple) else (r, None)
    return du.cpu().numpy(), dv.cpu().numpy(), st, shifts


def run_single(eng, I0, I1, c=None):
    """tvl1_calc_init from planes filled with c (tvl1_calc when c is None)."""
    h, w = I0.shape
    d0, d1 = dev(I0), dev(I1)
    du = torch.zeros((h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    init = None
    if c is not None:
        s0, s1 = dev(np.full((h, w), c[0], np.float32)), dev(np.full((h, w), c[1], np.float32))
        init = (s0.data_ptr(), s1.data_ptr())
    torch.cuda.synchronize()
    st = eng.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, du.data_ptr(), dv.data_ptr(),
                         4 * w, warp_iters=True, init=init)
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


def case_batch(case):
    n = len(case["consts"])
    fr = [cs.frames(case, b) for b in range(n)]
    return (np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]),
            np.array(case["consts"], np.float32), n)


def assert_pairs_equal(u, v, st, ref_of, n):
    for b in range(n):
        ur, vr, wr = ref_of(b)
        assert st[b]["levels"] == wr.shape[0]
        np.testing.assert_array_equal(st[b]["warp_iters"], wr, err_msg=f"pair {b}")
        assert bits_equal(u[b], ur) and bits_equal(v[b], vr), f"pair {b} not bit-exact"


# ------------------------------------------------------------------ constants from the host
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(cs.CASES))
def test_const_batch_matches_the_composed_reference(built, monkeypatch, name, env):
    set_env(monkeypatch, env)
    case = cs.CASES[name]
    I0s, I1s, k, n = case_batch(case)
    eng = capi.Engine(capi.make_params(**case["kw"]))
    u, v, st, _ = run_batch(eng, I0s, I1s, n, init_const=k)
    eng.close()
    assert_pairs_equal(u, v, st, lambda b: cs.reference(name, case, b)[:3], n)


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(cs.CASES))
def test_const_batch_matches_the_oracle_in_fma(built, monkeypatch, name, env):
    """fast_math 2: kb_flow_down_const<true> (the contracted weights and accumulations)."""
    set_env(monkeypatch, env)
    case = cs.CASES[name]
    I0s, I1s, k, n = case_batch(case)
    eng = capi.Engine(capi.make_params(fast_math=2, **case["kw"]))
    u, v, st, _ = run_batch(eng, I0s, I1s, n, init_const=k)
    eng.close()
    assert_pairs_equal(u, v, st, lambda b: cs.reference(name, case, b, math=2)[:3], n)


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("name", list(cs.CASES))
def test_const_batch_is_the_batch_from_filled_planes(built, name, math):
    """The same kernels after step 1; fast_math 1 has no seeded reference, so this equality is
    what holds it.  Pair 0, at (0, 0), is also the unseeded solve."""
    case = cs.CASES[name]
    I0s, I1s, k, n = case_batch(case)
    h, w = I0s.shape[1:]
    U0 = np.broadcast_to(k[:, 0, None, None], (n, h, w)).copy()
    V0 = np.broadcast_to(k[:, 1, None, None], (n, h, w)).copy()
    eng = capi.Engine(capi.make_params(fast_math=math, **case["kw"]))
    a = run_batch(eng, I0s, I1s, n, init_const=k)
    b = run_batch(eng, I0s, I1s, n, planes=(U0, V0))
    z = run_single(eng, I0s[0], I1s[0])
    eng.close()
    assert_pairs_equal(a[0], a[1], a[2], lambda i: (b[0][i], b[1][i], b[2][i]["warp_iters"]), n)
    assert bits_equal(a[0][0], z[0]) and bits_equal(a[1][0], z[1])
    np.testing.assert_array_equal(a[2][0]["warp_iters"], z[2]["warp_iters"])


@pytest.mark.parametrize("math", [0, 2])
def test_shared_frames(built, math):
    """pair_stride 0 for both frames: one frame pair under every pair's own constant."""
    name = "100x37_s3"
    case = cs.CASES[name]
    I0s, I1s, k, n = case_batch(case)
    eng = capi.Engine(capi.make_params(fast_math=math, **case["kw"]))
    u, v, st, _ = run_batch(eng, I0s[1:2], I1s[1:2], n, init_const=k)
    for b in (0, 1, 2, 4):
        us, vs, ss = run_single(eng, I0s[1], I1s[1], k[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], ss["warp_iters"], err_msg=f"pair {b}")
        assert bits_equal(u[b], us) and bits_equal(v[b], vs), f"pair {b}"
    eng.close()
    ur, vr, wr = cs.reference(name, case, 1, math=math)[:3]
    assert bits_equal(u[1], ur) and bits_equal(v[1], vr)


def test_two_chunks_index_the_constants_by_their_first_pair(built):
    """257 pairs: a chunk of 256 and one of 1, whose pair must take constant 256."""
    c = cs.CHUNKS
    n = c["n"]
    I0, I1 = cs.frames(c)
    k = cs.chunk_consts(n)
    eng = capi.Engine(capi.make_params(**c["kw"]))
    u, v, st, _ = run_batch(eng, I0[None], I1[None], n, init_const=k)
    for b in (0, 255, 256):
        us, vs, ss = run_single(eng, I0, I1, k[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], ss["warp_iters"], err_msg=f"pair {b}")
        assert bits_equal(u[b], us) and bits_equal(v[b], vs), f"pair {b}"
    eng.close()
    assert not bits_equal(u[256], u[0]) and not bits_equal(u[256], u[255])


@pytest.mark.parametrize("math", [0, 2])
def test_gamma_takes_the_one_by_one_path(built, math):
    """gamma != 0: tvl1_calc_init's path from planes filled in scratch, pair by pair."""
    case = cs.GAMMA
    I0s, I1s, k, n = case_batch(case)
    eng = capi.Engine(capi.make_params(fast_math=math, **case["kw"]))
    u, v, st, _ = run_batch(eng, I0s, I1s, n, init_const=k)
    for b in range(n):
        us, vs, ss = run_single(eng, I0s[b], I1s[b], k[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], ss["warp_iters"])
        assert bits_equal(u[b], us) and bits_equal(v[b], vs)
    eng.close()
    assert_pairs_equal(u, v, st, lambda b: cs.reference("gamma", case, b, math=math)[:3], n)


def test_bad_seed_arguments(built):
    case = cs.CASES["65x33_s2"]
    I0s, I1s, k, n = case_batch(case)
    h, w = I0s.shape[1:]
    eng = capi.Engine(capi.make_params(**case["kw"]))
    d0, d1 = dev(I0s), dev(I1s)
    du = torch.full((n, h, w), 7.0, dtype=torch.float32, device=d0.device)
    dv = du.clone()
    torch.cuda.synchronize()

    def call(seed, nn=n):
        p = seed.ctypes.data_as(C.POINTER(C.c_float)) if seed is not None else None
        return eng.lib.tvl1_calc_batch_const_init(
            eng.ctx, nn, C.c_void_p(d0.data_ptr()), w, w * h, C.c_void_p(d1.data_ptr()), w, w * h, w,
            h, p, C.c_void_p(du.data_ptr()), C.c_void_p(dv.data_ptr()), 4 * w, 4 * w * h, None, None)

    EINVAL = 1
    assert call(None) == EINVAL and b"null" in eng.lib.tvl1_last_error(eng.ctx)
    for bad in (np.nan, np.inf, -np.inf):
        kk = k.copy()
        kk[3, 1] = bad
        assert call(kk) == EINVAL and b"pair 3" in eng.lib.tvl1_last_error(eng.ctx)
    assert call(k, 0) == EINVAL
    eng.set_params(capi.make_params(profile=1, **case["kw"]))
    assert call(k) == EINVAL and b"profile 1" in eng.lib.tvl1_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert float(du.min()) == 7.0 and float(dv.max()) == 7.0   # nothing was launched
    eng.close()


# ------------------------------------------------------------------ constants from the estimate
@pytest.mark.parametrize("math", [0, 2])
@pytest.mark.parametrize("name", list(cs.AUTO))
def test_auto_batch(built, name, math):
    case = cs.AUTO[name]
    I0s, I1s = cs.auto_batch(case)
    n, w, h, R = len(I1s), case["w"], case["h"], case["R"]
    eng = capi.Engine(capi.make_params(fast_math=math, **case["kw"]))
    u, v, st, shifts = run_batch(eng, I0s, I1s, n, auto_shift=R)
    want = [shift_ref.estimate(I0s[b % len(I0s)], I1s[b], R) for b in range(n)]
    assert shifts == want
    assert shift_ref.levels_of(R) == (0 if R <= 4 else 1)
    d0, d1 = dev(I0s), dev(I1s)
    torch.cuda.synchronize()
    assert shifts == eng.estimate_shift_batch(n, d0.data_ptr(), w, w * h if len(I0s) > 1 else 0,
                                              d1.data_ptr(), w, w * h, w, h, R)
    assert any((s["dx"], s["dy"]) == (0, 0) for s in shifts)
    assert len({(s["dx"], s["dy"]) for s in shifts}) == n
    k = np.array([[s["dx"], s["dy"]] for s in shifts], np.float32)
    uc, vc, sc, _ = run_batch(eng, I0s, I1s, n, init_const=k)
    eng.close()
    assert_pairs_equal(u, v, st, lambda b: (uc[b], vc[b], sc[b]["warp_iters"]), n)


def test_auto_batch_regrows_and_crosses_chunks(built):
    """A second call on the same ctx with more pairs (the shift workspace and the constants'
    block regrow), then 258 pairs: two chunks of the estimate and of the solve, the records of
    the first chunk still seeding it after the second re-laid the workspace."""
    case = cs.AUTO["64x48_R4"]
    w, h, R = case["w"], case["h"], case["R"]
    eng = capi.Engine(capi.make_params(**case["kw"]))
    per = len(case["shifts"])
    for n in (2, 9, 258):
        I0s, I1s = cs.auto_batch(case, n)
        u, v, st, shifts = run_batch(eng, I0s, I1s, n, auto_shift=R)
        want = [shift_ref.estimate(I0s[b], I1s[b], R) for b in range(min(n, per))]
        assert shifts == [want[b % per] for b in range(n)]
        for b in range(per, n):   # the frames repeat with period `per`, and so must the flows
            assert bits_equal(u[b], u[b % per]) and bits_equal(v[b], v[b % per]), (n, b)
            np.testing.assert_array_equal(st[b]["warp_iters"], st[b % per]["warp_iters"])
        k = np.array([[s["dx"], s["dy"]] for s in shifts[:per]], np.float32)
        m = min(n, per)
        uc, vc, sc, _ = run_batch(eng, I0s[:m], I1s[:m], m, init_const=k[:m])
        assert_pairs_equal(u, v, st, lambda b: (uc[b], vc[b], sc[b]["warp_iters"]), m)
    eng.close()


def test_auto_bad_arguments_launch_nothing(built):
    """tvl1_estimate_shift_batch's argument errors, unchanged, before anything is launched."""
    w, h = 64, 48
    eng = capi.Engine(capi.make_params(nscales=2))
    t = dev(np.zeros((2, h, w), np.uint8))
    du = torch.full((2, h, w), 7.0, dtype=torch.float32, device=t.device)
    dv = du.clone()
    torch.cuda.synchronize()
    p = C.c_void_p(t.data_ptr())
    rec = (capi.TVL1Shift * 2)()

    def auto(n=2, I0=p, p0=w, s0=w * h, I1=p, p1=w, R=8, out=rec, ww=w, hh=h):
        return eng.lib.tvl1_calc_batch_auto_init(eng.ctx, n, I0, p0, s0, I1, p1, w * h, ww, hh, R, out,
                                                 C.c_void_p(du.data_ptr()), C.c_void_p(dv.data_ptr()),
                                                 4 * ww, 4 * ww * hh, None, None)

    def est(n=2, I0=p, p0=w, s0=w * h, I1=p, p1=w, R=8, out=rec, ww=w, hh=h):
        return eng.lib.tvl1_estimate_shift_batch(eng.ctx, n, I0, p0, s0, I1, p1, w * h, ww, hh, R, out,
                                                 None)

    def err():
        return eng.lib.tvl1_last_error(eng.ctx)

    for kw in (dict(I0=None), dict(I1=None), dict(out=None), dict(p0=w - 1), dict(p1=w - 1), dict(R=0),
               dict(R=129), dict(R=13), dict(n=0), dict(s0=w), dict(ww=8193, hh=8192, p0=8193, p1=8193)):
        want = est(**kw)
        msg = err()
        assert want != 0
        assert auto(**kw) == want and err() == msg, kw
    torch.cuda.synchronize()
    assert float(du.min()) == 7.0 and float(dv.max()) == 7.0
    assert auto(R=12) == 0
    eng.close()
