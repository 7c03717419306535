"""tvl1_calc_batch_init: every pair of a seeded batch gets the seeded reference
(tests/initflow_ref.py; in fma mode the oracle's own seeded entry) bit for bit, whatever seeds
the other pairs start from, through the on-chip coarsest level (kb_small_level<FM, true>), the
streaming one and the per-pair path."""
import numpy as np
import pytest

import initflow_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENV_KEYS = ("TVL1_BATCH_SMALL", "TVL1_BATCH_FUSE")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def batch_of(case):
    fr, sd = zip(*(ref.batch_pair(case, b) for b in range(case["n"])))
    I0s, I1s = np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
    U0, V0 = np.stack([s[0] for s in sd]), np.stack([s[1] for s in sd])
    return I0s, I1s, U0, V0


def run_batch(eng, I0s, I1s, U0, V0, shared=False):
    n, h, w = I0s.shape
    d0, d1, s0, s1 = dev(I0s), dev(I1s), dev(U0), dev(V0)
    du = torch.zeros((n, h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    torch.cuda.synchronize()
    st = eng.calc_batch_device(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h,
                               du.data_ptr(), dv.data_ptr(), 4 * w, 4 * w * h, warp_iters=True,
                               init=(s0.data_ptr(), s1.data_ptr(), 4 * w, 0 if shared else 4 * w * h))
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


def run_single(eng, I0, I1, u0, v0):
    h, w = I0.shape
    d0, d1, s0, s1 = dev(I0), dev(I1), dev(u0), dev(v0)
    du = torch.zeros((h, w), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    torch.cuda.synchronize()
    st = eng.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, du.data_ptr(), dv.data_ptr(),
                         4 * w, warp_iters=True, init=(s0.data_ptr(), s1.data_ptr()))
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


@pytest.mark.parametrize("env", ["", "TVL1_BATCH_SMALL=0", "TVL1_BATCH_FUSE=0"])
@pytest.mark.parametrize("name", list(ref.BATCH))
def test_seeded_batch_matches_the_composed_reference(built, monkeypatch, name, env):
    set_env(monkeypatch, env)
    case = ref.BATCH[name]
    I0s, I1s, U0, V0 = batch_of(case)
    eng = capi.Engine(capi.make_params(**case["kw"]))
    u, v, st = run_batch(eng, I0s, I1s, U0, V0)
    eng.close()
    for b in range(case["n"]):
        ur, vr, wr, _ = ref.reference(("batch", name, b), I0s[b], I1s[b], case["kw"], U0[b], V0[b])
        assert st[b]["levels"] == wr.shape[0]
        np.testing.assert_array_equal(st[b]["warp_iters"], wr, err_msg=f"pair {b}")
        assert bits_equal(u[b], ur) and bits_equal(v[b], vr), f"pair {b} not bit-exact"


@pytest.mark.parametrize("env", ["", "TVL1_BATCH_SMALL=0", "TVL1_BATCH_FUSE=0"])
@pytest.mark.parametrize("name", list(ref.BATCH))
def test_seeded_batch_matches_the_oracle_in_fma(built, monkeypatch, name, env):
    """fast_math 2: kb_flow_down<true>, kb_small_level<2, true> and the contracted streaming
    kernels under per-pair seeds, bitwise against the oracle's seeded entry."""
    set_env(monkeypatch, env)
    case = ref.BATCH[name]
    I0s, I1s, U0, V0 = batch_of(case)
    eng = capi.Engine(capi.make_params(fast_math=2, **case["kw"]))
    u, v, st = run_batch(eng, I0s, I1s, U0, V0)
    eng.close()
    for b in range(case["n"]):
        ur, vr, wr, _ = ref.reference(("batch", name, b), I0s[b], I1s[b], case["kw"], U0[b], V0[b], math=2)
        assert st[b]["levels"] == wr.shape[0]
        np.testing.assert_array_equal(st[b]["warp_iters"], wr, err_msg=f"pair {b}")
        assert bits_equal(u[b], ur) and bits_equal(v[b], vr), f"pair {b} not bit-exact"


@pytest.mark.parametrize("name", list(ref.BATCH))
def test_shared_seed_is_the_replicated_seed(built, name):
    """init_pair_stride = 0: one seed for every pair."""
    case = ref.BATCH[name]
    I0s, I1s, U0, V0 = batch_of(case)
    k = case["seeds"].index("rough")
    eng = capi.Engine(capi.make_params(**case["kw"]))
    a = run_batch(eng, I0s, I1s, U0[k:k + 1], V0[k:k + 1], shared=True)
    b = run_batch(eng, I0s, I1s, np.repeat(U0[k:k + 1], case["n"], 0), np.repeat(V0[k:k + 1], case["n"], 0))
    eng.close()
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        np.testing.assert_array_equal(x["warp_iters"], y["warp_iters"])
    ur, vr, wr, _ = ref.reference(("batch", name, k), I0s[k], I1s[k], case["kw"], U0[k], V0[k])
    assert bits_equal(a[0][k], ur) and bits_equal(a[1][k], vr)


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("env", ["", "TVL1_BATCH_SMALL=0"])
def test_seeded_batch_pair_is_the_single_seeded_solve(built, monkeypatch, math, env):
    """Each pair of the batch must be tvl1_calc_init of that pair alone, bitwise.  This
    equality is what holds fast_math 1's batched seed chain (its single seeded solves and its
    on-chip level are bitwise the oracle's fast branch in tests/test_gpu_fast_bitwise.py).  IEEE
    and fma mode are also held to their references above."""
    set_env(monkeypatch, env)
    case = ref.BATCH["strip6"]
    I0s, I1s, U0, V0 = batch_of(case)
    eng = capi.Engine(capi.make_params(fast_math=math, **case["kw"]))
    u, v, st = run_batch(eng, I0s, I1s, U0, V0)
    for b in range(case["n"]):
        us, vs, ss = run_single(eng, I0s[b], I1s[b], U0[b], V0[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], ss["warp_iters"], err_msg=f"pair {b}")
        assert bits_equal(u[b], us) and bits_equal(v[b], vs), f"pair {b}"
    eng.close()


def test_gamma_batch_takes_the_seeded_single_path(built):
    case = ref.BATCH_GAMMA
    I0s, I1s, U0, V0 = batch_of(case)
    eng = capi.Engine(capi.make_params(**case["kw"]))
    u, v, st = run_batch(eng, I0s, I1s, U0, V0)
    for b in range(case["n"]):
        us, vs, ss = run_single(eng, I0s[b], I1s[b], U0[b], V0[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], ss["warp_iters"])
        assert bits_equal(u[b], us) and bits_equal(v[b], vs)
        ur, vr, wr, _ = ref.reference(("batch_gamma", b), I0s[b], I1s[b], case["kw"], U0[b], V0[b])
        assert bits_equal(u[b], ur) and bits_equal(v[b], vr)
    eng.close()


def test_gamma_batch_in_fma(built):
    """fast_math 2 with gamma != 0: the engine and the oracle both solve in IEEE, seed chain
    included; each pair bitwise the oracle's seeded entry."""
    case = ref.BATCH_GAMMA
    I0s, I1s, U0, V0 = batch_of(case)
    eng = capi.Engine(capi.make_params(fast_math=2, **case["kw"]))
    u, v, st = run_batch(eng, I0s, I1s, U0, V0)
    eng.close()
    for b in range(case["n"]):
        ur, vr, wr, _ = ref.reference(("batch_gamma", b), I0s[b], I1s[b], case["kw"], U0[b], V0[b], math=2)
        np.testing.assert_array_equal(st[b]["warp_iters"], wr)
        assert bits_equal(u[b], ur) and bits_equal(v[b], vr)


@pytest.mark.parametrize("name", ["one_level_pitched", "one_level_chip"])
def test_one_level_batch_copies_the_seed(built, name):
    """nscales 1: the seed is the coarsest level as it is (kb_flow_copy); 50 x 30 streams,
    130 x 12 is solved on chip."""
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    z = np.zeros_like(u0)
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0)
    eng = capi.Engine(capi.make_params(**c["kw"]))
    u, v, st = run_batch(eng, np.stack([I0, I0, I0]), np.stack([I1, I1, I1]), np.stack([z, u0, z]),
                         np.stack([z, v0, z]))
    eng.close()
    assert bits_equal(u[1], ur) and bits_equal(v[1], vr)
    np.testing.assert_array_equal(st[1]["warp_iters"], wr)
    assert bits_equal(u[0], u[2]) and not bits_equal(u[0], u[1])


@pytest.mark.parametrize("name", ["one_level_pitched", "one_level_chip"])
def test_one_level_batch_copies_the_seed_in_fma(built, name):
    c = ref.SINGLE[name]
    I0, I1 = ref.frames_of(c)
    u0, v0 = ref.seed_of(c)
    z = np.zeros_like(u0)
    ur, vr, wr, _ = ref.reference(("single", name), I0, I1, c["kw"], u0, v0, math=2)
    eng = capi.Engine(capi.make_params(fast_math=2, **c["kw"]))
    u, v, st = run_batch(eng, np.stack([I0, I0, I0]), np.stack([I1, I1, I1]), np.stack([z, u0, z]),
                         np.stack([z, v0, z]))
    eng.close()
    assert bits_equal(u[1], ur) and bits_equal(v[1], vr)
    np.testing.assert_array_equal(st[1]["warp_iters"], wr)
