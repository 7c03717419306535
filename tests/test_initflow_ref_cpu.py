"""Initial-flow solves (tvl1_calc_init), the part that needs no GPU:
  * the reference the GPU tests compare with (tests/initflow_ref.py, composed from the
    oracle's stage functions) equals the oracle's own whole solve bit for bit when the seed
    is zero -- the composition is pinned before it is trusted;
  * every (case, seed) pair of the GPU tests keeps its stopping decisions at least the
    project's MIN_MARGIN (tests/test_residual_margin_cpu.py) from the thresholds;
  * the oracle's own seeded entry (orc_tvl1_calc_init, checker.oracle_calc(init=...)) equals
    that composition bit for bit in IEEE on every GPU case, and the unseeded oracle under a
    zero seed in IEEE and in fma -- it is the reference of the seeded fma-mode GPU tests;
  * the engine library exports the three entry points and rejects bad seed arguments before
    anything touches a device;
  * the CLI's `initialFlow` key: inert without `useInitialFlow`, an error with `features`."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import initflow_ref as ref
from optflow_amd import capi, synth
from oracle import checker

MIN_MARGIN = 1e-4   # tests/test_residual_margin_cpu.py
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("w,h,kw", [
    (97, 40, dict(nscales=3, warps=3)),
    (64, 48, dict(nscales=5, warps=3)),
    (97, 61, dict(gamma=0.1)),
    (96, 64, dict(median_filtering=5)),
    (40, 24, dict(nscales=5)),            # the pyramid breaks at L = 2 (< 16 px)
], ids=["97x40_s3w3", "64x48_s5w3", "gamma", "median5", "40x24_break"])
def test_zero_seed_composition_is_the_oracle(built, w, h, kw):
    p = capi.make_params(**kw)
    I0, I1 = synth.gen_pair(w, h, seed=w * 7 + h)
    ur, vr, sr, wr, tr = checker.oracle_check_trace(I0, I1, p)
    z = np.zeros((h, w), np.float32)
    for seed in (None, (z, z)):           # no seed, and a zero seed through the chain
        u, v, wi, trace = ref.seeded_calc(I0, I1, p, *(seed or (None, None)))
        assert wi.shape == wr.shape and sr["levels"] == wi.shape[0]
        np.testing.assert_array_equal(wi, wr)
        assert bits_equal(u, ur) and bits_equal(v, vr)
        np.testing.assert_array_equal(trace, tr)
    if (w, h) == (40, 24):
        assert sr["levels"] == 2


def test_seed_pyramid_is_a_chain_of_rounded_levels(built):
    """A.2b: each level from the one before (not from level 0), scaled by float(scaleStep) in a
    rounding of its own; a constant seed c gives c * scaleStep^s up to those roundings."""
    p = capi.make_params(nscales=4)
    u0, v0 = ref.make_seed("rough", 97, 61, rng=5)
    lv = ref.seed_pyramid(u0, v0, p)
    ws, hs = ref.pyramid_sizes(97, 61, p)
    assert [a.shape for a, _ in lv] == list(zip(hs, ws)) and len(lv) == 4
    f = ref._f32(1.0 / p.scale_step)
    direct = ref._resize(ref._resize(u0, ws[1], hs[1], f, f) * np.float32(0.8), ws[2], hs[2], f, f)
    assert bits_equal(lv[2][0], direct * np.float32(0.8))
    c = ref.seed_pyramid(*ref.make_seed("far", 97, 61), p)
    np.testing.assert_allclose(c[3][0], 14 * 0.8 ** 3, rtol=1e-6)
    np.testing.assert_allclose(c[3][1], -11 * 0.8 ** 3, rtol=1e-6)


def oracle_seeded_trace(I0, I1, p, u0, v0):
    return checker.oracle_check_trace(I0, I1, p, init=(u0, v0))


def _gpu_cases():
    out = []
    for name, c in ref.SINGLE.items():
        out.append(pytest.param(lambda c=c: (ref.frames_of(c), ref.seed_of(c), c["kw"]), id=name))
    for name, c in list(ref.BATCH.items()) + [("batch_gamma", ref.BATCH_GAMMA)]:
        for b in range(c["n"]):
            out.append(pytest.param(lambda c=c, b=b: (*ref.batch_pair(c, b), c["kw"]),
                                    id=f"{name}_{b}_{c['seeds'][b]}"))
    return out


@pytest.mark.parametrize("make", _gpu_cases())
def test_gpu_cases_clear_the_residual_margin(built, make):
    (I0, I1), (u0, v0), kw = make()
    p = capi.make_params(**kw)
    _, _, wi, trace = ref.seeded_calc(I0, I1, p, u0, v0)
    if p.epsilon == 0:
        assert len(trace) == 0
        return
    m = checker.check_margins(trace, p.iterations)
    assert m.min() >= MIN_MARGIN, trace[np.argmin(m)]


@pytest.mark.parametrize("make", _gpu_cases())
def test_oracle_seeded_entry_is_the_composition(built, make):
    """IEEE: flow bits and per-warp counts of orc_tvl1_calc_init == seeded_calc."""
    (I0, I1), (u0, v0), kw = make()
    p = capi.make_params(**kw)
    ur, vr, wr, _ = ref.seeded_calc(I0, I1, p, u0, v0)
    u, v, st, wi = checker.oracle_calc(I0, I1, p, init=(u0, v0))
    assert st["levels"] == wr.shape[0]
    np.testing.assert_array_equal(wi, wr)
    assert bits_equal(u, ur) and bits_equal(v, vr)


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("w,h,kw", [
    (97, 40, dict(nscales=3, warps=3)),
    (97, 61, dict(gamma=0.1)),
    (96, 64, dict(median_filtering=5)),
    (200, 60, dict(nscales=4, warps=3, epsilon=0.0, iterations=7)),
    (40, 24, dict(nscales=5)),
], ids=["97x40_s3w3", "gamma", "median5", "fixed_work", "40x24_break"])
def test_oracle_zero_seed_is_the_unseeded_oracle(built, w, h, kw, math):
    p = capi.make_params(fast_math=math, **kw)
    I0, I1 = synth.gen_pair(w, h, seed=w * 7 + h)
    ur, vr, sr, wr = checker.oracle_calc(I0, I1, p)
    z = np.zeros((h, w), np.float32)
    u, v, st, wi = checker.oracle_calc(I0, I1, p, init=(z, z))
    assert st == sr
    np.testing.assert_array_equal(wi, wr)
    assert bits_equal(u, ur) and bits_equal(v, vr)


def test_oracle_seeded_entry_rejects_what_the_engine_rejects(built):
    I0, I1 = synth.gen_pair(40, 24, seed=3)
    z = np.zeros((24, 40), np.float32)
    with pytest.raises(capi.TVL1Error, match="TVL1_EINVAL"):
        checker.oracle_calc(I0, I1, capi.make_params(profile=1, nscales=2), init=(z, z))
    with pytest.raises(ValueError):
        checker.oracle_calc(I0, I1, capi.make_params(), init=(z[:, :39], z[:, :39]))


@pytest.mark.parametrize("make", _gpu_cases())
def test_gpu_cases_clear_the_residual_margin_in_fma(built, make):
    """The fma-mode twin of the margin test above, on the oracle's own seeded entry (the
    reference of the fma-mode GPU tests)."""
    (I0, I1), (u0, v0), kw = make()
    p = capi.make_params(fast_math=2, **kw)
    *_, trace = oracle_seeded_trace(I0, I1, p, u0, v0)
    if p.epsilon == 0:
        assert len(trace) == 0
        return
    m = checker.check_margins(trace, p.iterations)
    assert m.min() >= MIN_MARGIN, trace[np.argmin(m)]


def test_cli_case_clears_the_residual_margin(built):
    c = ref.CLI
    I0, I1 = ref.shifted_pair(c["w"], c["h"], c["rng"], *c["shift"])
    p = capi.make_params()
    u0 = np.full(I0.shape, c["shift"][0], np.float32)
    v0 = np.full(I0.shape, c["shift"][1], np.float32)
    for seed in ((u0, v0), (None, None)):
        _, _, _, trace = ref.seeded_calc(I0, I1, p, *seed)
        m = checker.check_margins(trace, p.iterations)
        assert m.min() >= MIN_MARGIN, trace[np.argmin(m)]


def test_far_seed_is_beyond_the_window_at_the_coarsest_level(built):
    """The 'far' case must start the coarsest level more than 6 px out (the engine's gather
    window margin), so the global-gather path runs from the first warp."""
    c = ref.SINGLE["far_gather"]
    lv = ref.seed_pyramid(*ref.seed_of(c), capi.make_params(**c["kw"]))
    assert len(lv) == 3 and np.abs(lv[2][0]).min() > 6 and np.abs(lv[2][1]).min() > 6


# ---- the C ABI without a GPU
def test_library_exports_and_rejects_bad_seeds(built):
    lib = capi.load_engine()
    for name in ("tvl1_calc_init", "tvl1_calc_host_init", "tvl1_calc_batch_init"):
        assert hasattr(lib, name)
    assert lib.tvl1_abi_version() == 9            # additive under ABI 9
    EINVAL = 1
    w, h = 32, 16
    img = np.zeros((h, w), np.uint8)
    f = np.zeros((h, w), np.float32)
    i, fp = img.ctypes.data, f.ctypes.data
    # no ctx
    assert lib.tvl1_calc_init(None, i, w, i, w, w, h, fp, fp, 4 * w, fp, fp, 4 * w, None, None) == EINVAL
    assert b"ctx" in lib.tvl1_last_error(None)
    # a null seed, then a short and a ragged pitch: reported before the ctx is looked at
    assert lib.tvl1_calc_init(None, i, w, i, w, w, h, None, fp, 4 * w, fp, fp, 4 * w, None, None) == EINVAL
    assert b"initial flow pointer" in lib.tvl1_last_error(None)
    assert lib.tvl1_calc_init(None, i, w, i, w, w, h, fp, None, 4 * w, fp, fp, 4 * w, None, None) == EINVAL
    assert b"initial flow pointer" in lib.tvl1_last_error(None)
    for bad in (4 * w - 4, 4 * w + 2):
        assert lib.tvl1_calc_init(None, i, w, i, w, w, h, fp, fp, bad, fp, fp, 4 * w, None, None) == EINVAL
        assert b"initial flow pitch" in lib.tvl1_last_error(None)
    u8 = C.POINTER(C.c_uint8)
    fl = C.POINTER(C.c_float)
    ip, fpp = img.ctypes.data_as(u8), f.ctypes.data_as(fl)
    assert lib.tvl1_calc_host_init(None, ip, w, ip, w, w, h, None, fpp, 4 * w, fpp, fpp, 4 * w, None) == EINVAL
    assert b"initial flow pointer" in lib.tvl1_last_error(None)
    assert lib.tvl1_calc_host_init(None, ip, w, ip, w, w, h, fpp, fpp, 4 * w - 4, fpp, fpp, 4 * w, None) == EINVAL
    assert b"initial flow pitch" in lib.tvl1_last_error(None)
    assert lib.tvl1_calc_batch_init(None, 2, i, w, w * h, i, w, w * h, w, h, None, fp, 4 * w, 0,
                                    fp, fp, 4 * w, 4 * w * h, None, None) == EINVAL
    assert b"initial flow pointer" in lib.tvl1_last_error(None)
    assert lib.tvl1_calc_batch_init(None, 2, i, w, w * h, i, w, w * h, w, h, fp, fp, 4 * w - 4, 0,
                                    fp, fp, 4 * w, 4 * w * h, None, None) == EINVAL
    assert b"initial flow pitch" in lib.tvl1_last_error(None)
    # a pair stride that does not cover one field
    assert lib.tvl1_calc_batch_init(None, 2, i, w, w * h, i, w, w * h, w, h, fp, fp, 4 * w, 4 * w,
                                    fp, fp, 4 * w, 4 * w * h, None, None) == EINVAL
    assert b"pair stride" in lib.tvl1_last_error(None)


# ---- the CLI's key, resolved without a GPU (optflow --plan)
@pytest.fixture
def cfg(tmp_path, built):
    rng = np.random.default_rng(9)
    for n in ("p", "q"):
        Image.fromarray(rng.integers(0, 256, (61, 83), dtype=np.uint8)).save(tmp_path / f"{n}.png")
    return {"output_dir": str(tmp_path), "scale": 1, "output_type": "flow",
            "rois": {"top": 20, "bottom": 20},
            "images": [{"p": str(tmp_path / "p.png"), "q": str(tmp_path / "q.png"),
                        "output_name": "pq"}]}


def _plan(tmp_path, cfg, name):
    p = tmp_path / name
    p.write_text(json.dumps(cfg))
    return subprocess.run([str(OPTFLOW), "--plan", str(p)], capture_output=True, text=True, timeout=120)


def _plans(r):
    assert r.returncode == 0, r.stderr
    out = r.stdout
    return json.loads(out[out.index("\n[") + 1:] if not out.startswith("[") else out)


def test_cli_initial_flow_needs_use_initial_flow(tmp_path, cfg):
    base = _plans(_plan(tmp_path, cfg, "a.json"))
    assert base[0]["strip_batch"] is True and "initialFlow" not in base[0]
    # the key alone, or the reference's flag alone, changes nothing in the plan
    assert _plans(_plan(tmp_path, {**cfg, "initialFlow": [12, -9]}, "b.json")) == base
    assert _plans(_plan(tmp_path, {**cfg, "useInitialFlow": True}, "c.json")) == base
    # together: the pair is seeded and leaves the strip batch
    (pl,) = _plans(_plan(tmp_path, {**cfg, "useInitialFlow": True, "initialFlow": [12, -9]}, "d.json"))
    assert pl["initialFlow"] == [12, -9] and pl["strip_batch"] is False
    assert {k: v for k, v in pl.items() if k not in ("initialFlow", "strip_batch")} == \
           {k: v for k, v in base[0].items() if k != "strip_batch"}
    # per image entry, over the global value
    c2 = {**cfg, "useInitialFlow": True, "initialFlow": [1, 2]}
    c2["images"] = [{**cfg["images"][0], "initialFlow": [-3.5, 4.25]}]
    (pl,) = _plans(_plan(tmp_path, c2, "e.json"))
    assert pl["initialFlow"] == [-3.5, 4.25]


def test_cli_initial_flow_with_features_fails(tmp_path, cfg):
    r = _plan(tmp_path, {**cfg, "useInitialFlow": True, "initialFlow": [12, -9], "features": 1}, "f.json")
    assert r.returncode != 0 and "initialFlow cannot be combined with feature alignment" in r.stderr
    # ... and without useInitialFlow the same config plans as before
    assert _plans(_plan(tmp_path, {**cfg, "initialFlow": [12, -9], "features": 1}, "g.json"))[0]["features"] is True
