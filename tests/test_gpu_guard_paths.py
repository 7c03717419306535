"""The iteration kernels' rare-case paths: the long forms of the TH and
projection quotients (numerators under 2^-100, zero included) and of the projection's sqrt
(arguments in (0, 2^-96) when tau/theta > 2^20), each behind a guard that almost no wavefront
of a textured pair takes.

Inputs that send whole wavefronts, and single lanes of a wavefront, through the long forms:
  (a) I1 == I0: rho = 0 and every numerator 0, on every iteration;
  (b) a frame whose left half is identical and whose right half is textured and shifted by
      1.5 px, the seam on a lane boundary (even x) and inside a lane (odd x);
  (c) a textured pair with tau/theta = 2^20 (the sqrt skips its scaled form: taut_small) and
      2.5e6 (it keeps it);
on every iteration kernel the knobs reach (the blocked k_iterate_tb4 for the long passes, the
streaming k_iterate_roll<3|4, 2> and the mid-check pass, both forms of k_warp_iter) and in the
three arithmetic modes.  IEEE and fma mode: bitwise against the oracle, with equal per-warp
iteration counts.  The approximate mode has no guarded forms (v_rcp / v_sqrt on every lane); it
is bitwise the oracle's fast branch on these inputs in tests/test_gpu_fast_bitwise.py, and held
here to tests/test_gpu_fastmath.py's bar against the IEEE oracle (the oracle's iteration
schedule, EPE budget).
"""
import numpy as np
import pytest
from scipy import ndimage

from optflow_amd import capi, synth
from oracle import checker

torch = pytest.importorskip("torch")   # device buffers of the batch test

pytestmark = pytest.mark.gpu

KNOBS = ("TVL1_ROLL_SEG", "TVL1_ROLL_PX4_MIN", "TVL1_ROLL_LONG_MIN", "TVL1_FUSE", "TVL1_FUSE_MIN",
         "TVL1_BUF_LIMIT", "TVL1_BATCH_FUSE", "TVL1_POLL", "TVL1_SPEC", "TVL1_WI_NC", "TVL1_TB4",
         "TVL1_MID", "TVL1_MID_MIN")
# default: k_iterate_tb4 for passes of >= 3 iterations at these sizes; ROLL_LONG_MIN=1: they
# stream (k_iterate_roll<3|4, 2>, k_iterate_roll_mid); FUSE_MIN=0: k_warp_iter, one or two
# consumer wavefronts
ENVS = ["", "TVL1_ROLL_LONG_MIN=1", "TVL1_FUSE_MIN=0,TVL1_WI_NC=1", "TVL1_FUSE_MIN=0,TVL1_WI_NC=2"]
FAST_TOL = (1e-3, 2e-2, 0.5)   # mean, p99.9, max EPE (px): tests/test_gpu_fastmath.py


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def identical(W, H, seed):
    I0, _ = synth.gen_pair(W, H, seed=seed)
    return I0, I0.copy()


def split(W, H, seed, seam):
    """Columns < seam identical, the rest the texture shifted by 1.5 px in x."""
    base = synth.base_texture(W, H, seed=seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    moved = ndimage.map_coordinates(base, [ys, xs + 1.5], order=3, mode="nearest")
    I0 = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    I1 = I0.copy()
    I1[:, seam:] = np.clip(np.rint(moved), 0, 255).astype(np.uint8)[:, seam:]
    return I0, I1


def textured(W, H, seed):
    return synth.gen_pair(W, H, seed=seed)


BASE = dict(nscales=3, warps=3)
# name -> (pair, parameters)
INPUTS = {
    "identical": (lambda: identical(192, 160, 41), BASE),
    "split_even": (lambda: split(192, 160, 42, 96), BASE),
    "split_odd": (lambda: split(192, 160, 43, 97), BASE),
    "split_odd_256": (lambda: split(256, 192, 44, 131), BASE),
    "taut_2p20": (lambda: textured(192, 160, 45), dict(BASE, iterations=12, tau=0.25, theta=2.0 ** -22)),
    "taut_2.5e6": (lambda: textured(192, 160, 46), dict(BASE, iterations=12, tau=0.25, theta=1e-7)),
}
_pairs, _oracle = {}, {}


def pair_of(name):
    if name not in _pairs:
        _pairs[name] = INPUTS[name][0]()
    return _pairs[name]


def oracle_of(name, math):
    """The oracle's result, computed once per input and arithmetic (never modified)."""
    key = (name, math)
    if key not in _oracle:
        I0, I1 = pair_of(name)
        _oracle[key] = checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **INPUTS[name][1]))
    return _oracle[key]


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, env.split(",")):
        monkeypatch.setenv(*kv.split("="))


@pytest.mark.parametrize("math", [0, 2, 1], ids=["ieee", "fma", "fast"])
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_guard_paths(built, monkeypatch, name, env, math):
    set_knobs(monkeypatch, env)
    I0, I1 = pair_of(name)
    eng = capi.Engine(capi.make_params(fast_math=math, **INPUTS[name][1]))
    u, v, st, wi = eng.calc_host(I0, I1)
    eng.close()
    ur, vr, sr, wr = oracle_of(name, 0 if math == 1 else math)
    assert st["levels"] == sr["levels"]
    np.testing.assert_array_equal(wi, wr)
    fin = np.isfinite(ur) & np.isfinite(vr)
    assert np.array_equal(fin, np.isfinite(u) & np.isfinite(v))
    if math == 1:
        e = capi.epe(u, v, ur, vr)[fin]
        mean, p999, mx = float(e.mean()), float(np.quantile(e, 0.999)), float(e.max())
        print(f"fast vs IEEE {name} {env}: mean {mean:.3g} p99.9 {p999:.3g} max {mx:.3g} px")
        assert mean <= FAST_TOL[0] and p999 <= FAST_TOL[1] and mx <= FAST_TOL[2]
    else:
        assert bits_equal(u[fin], ur[fin]) and bits_equal(v[fin], vr[fin])
    if name == "identical":
        assert np.all(u == 0) and np.all(v == 0)


def test_batch_of_guard_strips_equals_lone_solves(built, monkeypatch):
    """One tvl1_calc_batch of three 384 x 100 strips -- identical, split, textured -- each
    bitwise its lone solve (and the oracle), with the same per-warp iteration counts."""
    set_knobs(monkeypatch, "")
    w, h = 384, 100
    prs = [identical(w, h, 51), split(w, h, 52, 193), textured(w, h, 53)]
    I0s = np.stack([a for a, _ in prs])
    I1s = np.stack([b for _, b in prs])
    p = capi.make_params(**BASE)
    eng = capi.Engine(p)
    dev = torch.device("cuda", 0)
    d0 = torch.from_numpy(I0s).to(dev)
    d1 = torch.from_numpy(I1s).to(dev)
    du = torch.zeros((3, h, w), dtype=torch.float32, device=dev)
    dv = torch.zeros((3, h, w), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = eng.calc_batch_device(3, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h,
                               du.data_ptr(), dv.data_ptr(), 4 * w, 4 * w * h, warp_iters=True)
    torch.cuda.synchronize()
    ub, vb = du.cpu().numpy(), dv.cpu().numpy()
    for b in range(3):
        u1, v1, _, w1 = eng.calc_host(I0s[b], I1s[b])
        np.testing.assert_array_equal(st[b]["warp_iters"], w1, err_msg=f"strip {b}")
        assert bits_equal(ub[b], u1) and bits_equal(vb[b], v1), f"strip {b} differs from its lone solve"
        ur, vr, _, wr = checker.oracle_calc(I0s[b], I1s[b], p)
        np.testing.assert_array_equal(w1, wr, err_msg=f"strip {b}")
        assert bits_equal(u1, ur) and bits_equal(v1, vr), f"strip {b} differs from the oracle"
    eng.close()
