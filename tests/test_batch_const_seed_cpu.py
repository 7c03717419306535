"""Batched solves seeded by one constant per pair (tvl1_calc_batch_const_init,
tvl1_calc_batch_auto_init, the CLI's "seededStripBatch"), the part that needs no GPU:
  * the library exports both entry points under ABI 9 and the binding's signatures load; bad
    seed arguments come back before a device is touched;
  * Engine.calc_batch_device's init / init_const / auto_shift exclude one another;
  * `optflow --plan`: with "seededStripBatch" a globally seeded strip pair stays in the batch,
    a per-image seed does not, and without the key the plan is the parent's, byte for byte
    (tests/golden/plan_seeded_strips.txt, written by the parent commit's binary);
  * every non-integer constant of the GPU cases gives a coarsest seed level of >= 2 bit
    patterns, so the GPU tests can tell the kernel from a fill; every case keeps its stopping
    decisions the project's margin from the thresholds."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import const_seed_cases as cs
import initflow_ref as ref
from optflow_amd import capi
from oracle import checker

MIN_MARGIN = 1e-4   # tests/test_residual_margin_cpu.py
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
GOLDEN_PLAN = Path(__file__).resolve().parent / "golden" / "plan_seeded_strips.txt"


# ------------------------------------------------------------------ ABI and binding
def test_exports_under_abi_9(built):
    lib = capi.load_engine()
    assert lib.tvl1_abi_version() == 9
    for name in ("tvl1_calc_batch_const_init", "tvl1_calc_batch_auto_init"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes
    assert len(lib.tvl1_calc_batch_const_init.argtypes) == 17
    assert len(lib.tvl1_calc_batch_auto_init.argtypes) == 18
    assert lib.tvl1_calc_batch_auto_init.argtypes[11] == C.POINTER(capi.TVL1Shift)


def test_null_ctx_and_null_seed_are_einval(built):
    lib = capi.load_engine()
    seed = (C.c_float * 2)(1.0, 2.0)
    rec = capi.TVL1Shift()
    p = C.c_void_p(4096)   # never dereferenced: the ctx is checked first
    EINVAL = 1
    assert lib.tvl1_calc_batch_const_init(None, 1, p, 8, 0, p, 8, 0, 8, 8, seed, p, p, 32, 0, None,
                                          None) == EINVAL
    assert lib.tvl1_calc_batch_const_init(None, 1, p, 8, 0, p, 8, 0, 8, 8, None, p, p, 32, 0, None,
                                          None) == EINVAL
    assert b"initial flow" in lib.tvl1_last_error(None)
    assert lib.tvl1_calc_batch_auto_init(None, 1, p, 32, 0, p, 32, 0, 32, 32, 4, C.byref(rec), p, p,
                                         128, 0, None, None) == EINVAL


class _NoCtx(capi.Engine):
    """An Engine without a device: calc_batch_device must refuse its keywords before any call."""

    def __init__(self):
        self.params = capi.make_params()
        self.lib = None
        self.ctx = None

    def close(self):
        pass


@pytest.mark.parametrize("kw", [
    dict(init=(1, 2), init_const=np.zeros((2, 2), np.float32)),
    dict(init=(1, 2), auto_shift=4),
    dict(init_const=np.zeros((2, 2), np.float32), auto_shift=4),
    dict(init=(1, 2), init_const=np.zeros((2, 2), np.float32), auto_shift=4),
])
def test_engine_seed_keywords_exclude_one_another(built, kw):
    with pytest.raises(ValueError, match="exclude"):
        _NoCtx().calc_batch_device(2, 0, 8, 64, 0, 8, 64, 8, 8, 0, 0, 32, 256, **kw)


def test_engine_init_const_shape(built):
    with pytest.raises(ValueError, match="shape"):
        _NoCtx().calc_batch_device(2, 0, 8, 64, 0, 8, 64, 8, 8, 0, 0, 32, 256,
                                   init_const=np.zeros((3, 2), np.float32))


# ------------------------------------------------------------------ --plan
def _slices(d):
    rng = np.random.default_rng(3)
    for z in range(3):
        Image.fromarray(rng.integers(0, 256, (61, 83), dtype=np.uint8)).save(d / f"z{z}.png")


def _plan_text(d, cfg):
    """stdout of `optflow --plan` run inside d (relative paths: the same text anywhere)."""
    (d / "cfg.json").write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), "--plan", "cfg.json"], capture_output=True, text=True,
                       timeout=120, cwd=d)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _plan(d, cfg):
    out = _plan_text(d, cfg)
    return json.loads(out[out.index("\n[") + 1:] if not out.startswith("[") else out)


def _base(seed):
    return {"output_dir": ".", "scale": 1, "rois": {"top": 10, "bottom": 12},
            "output_type": "random_points", "useInitialFlow": True, "initialFlow": seed,
            "images": [{"p": "z0.png", "q": "z1.png", "pId": "a", "qId": "b", "output_name": "x"},
                       {"p": "z1.png", "q": "z2.png", "output_name": "y", "initialFlow": [1, 2]},
                       {"p": "z1.png", "q": "z2.png", "output_name": "w", "useInitialFlow": False}]}


@pytest.mark.parametrize("seed", [[2.5, -1.0], "auto"], ids=["numeric", "auto"])
def test_plan_keeps_globally_seeded_pairs_in_the_batch(built, tmp_path, seed):
    _slices(tmp_path)
    pl = _plan(tmp_path, dict(_base(seed), seededStripBatch=True))
    # the per-image seed keys are not production keys: those pairs go the per-pair way
    assert [e["strip_batch"] for e in pl] == [True, False, False]
    if seed == "auto":
        assert pl[0]["initialFlow"] == "auto" and pl[0]["initialFlowMaxShift"] == 32
    else:
        assert pl[0]["initialFlow"] == seed
    assert pl[1]["initialFlow"] == [1, 2] and "initialFlow" not in pl[2]
    # strip_batch 0 and features still switch the batch off
    for extra in ({"strip_batch": 0}, {"rois": {"custom": [0, 0, 20, 20]}}):
        assert not any(e["strip_batch"] for e in _plan(tmp_path, dict(_base(seed), seededStripBatch=True, **extra)))
    # unseeded jobs are untouched by the key
    cfg = dict(_base(seed), seededStripBatch=True, useInitialFlow=False)
    assert [e["strip_batch"] for e in _plan(tmp_path, cfg)] == [True, False, False]


def test_plan_without_the_key_is_the_parents(built, tmp_path):
    """The default changes nothing: the text the parent commit's binary printed for these two
    configs, and the same with the key spelled out as false."""
    _slices(tmp_path)
    text = "".join(_plan_text(tmp_path, _base(seed)) for seed in ([2.5, -1.0], "auto"))
    assert text == GOLDEN_PLAN.read_text()
    assert text == "".join(_plan_text(tmp_path, dict(_base(seed), seededStripBatch=False))
                           for seed in ([2.5, -1.0], "auto"))
    assert '"strip_batch":true' not in text.replace(" ", "")


# ------------------------------------------------------------------ the GPU cases
def _const_cases():
    out = [(n, c) for n, c in cs.CASES.items()] + [("gamma", cs.GAMMA)]
    return [pytest.param(n, c, b, id=f"{n}_{b}") for n, c in out for b in range(len(c["consts"]))]


@pytest.mark.parametrize("name,case,b", _const_cases())
def test_non_integer_constants_do_not_give_a_constant_level(built, name, case, b):
    """The condition the GPU comparison rests on: the composed reference's coarsest seed level
    of every non-integer constant holds >= 2 bit patterns (where a chain exists: nscales 1
    takes the constant as it is, which the fill is held to).  Integer constants of this size
    survive the weights exactly; they are in the cases for the other properties."""
    p = capi.make_params(**case["kw"])
    lv = ref.seed_pyramid(*cs.filled(case, case["consts"][b]), p)
    assert len(lv) == min(p.nscales, len(lv))
    for k, c in enumerate(case["consts"][b]):
        pats = len(np.unique(lv[-1][k].view(np.uint32)))
        print(name, b, "xy"[k], c, "levels", len(lv), "patterns", pats)
        if len(lv) == 1:
            assert pats == 1
        elif not cs.is_integer(c):
            assert pats >= 2, (name, c)


def test_the_cases_reach_every_level_count(built):
    levels = {n: len(ref.pyramid_sizes(c["w"], c["h"], capi.make_params(**c["kw"]))[0])
              for n, c in cs.CASES.items()}
    assert sorted(set(levels.values())) == [1, 2, 3, 4], levels
    c = cs.CHUNKS
    assert len(ref.pyramid_sizes(c["w"], c["h"], capi.make_params(**c["kw"]))[0]) == 2
    k = cs.chunk_consts(c["n"])
    assert len({tuple(r) for r in k.tolist()}) == c["n"] and (k[:, 0] != k[:, 1]).all()


@pytest.mark.parametrize("math", [0, 2], ids=["ieee", "fma"])
@pytest.mark.parametrize("name,case,b", _const_cases())
def test_cases_clear_the_residual_margin(built, name, case, b, math):
    p = capi.make_params(**case["kw"])
    trace = cs.reference(name, case, b, math=math)[3]
    m = checker.check_margins(trace, p.iterations)
    assert m.min() >= MIN_MARGIN, trace[np.argmin(m)]


def test_zero_constant_is_the_unseeded_solve(built):
    """(0, 0) through the chain is 0 on every level: pair 0 of each case equals tvl1_calc."""
    for name, case in cs.CASES.items():
        I0, I1 = cs.frames(case, 0)
        ur, vr, _, wr = checker.oracle_calc(I0, I1, capi.make_params(**case["kw"]))
        u, v, wi, _ = cs.reference(name, case, 0)
        np.testing.assert_array_equal(wi, wr)
        assert np.array_equal(u.view(np.uint32), ur.view(np.uint32))
        assert np.array_equal(v.view(np.uint32), vr.view(np.uint32))
