"""TEST INFRASTRUCTURE: the reference of the initial-flow solves (tvl1_calc_init).

oracle/'s whole-solve entry has no seed, so the seeded solve is composed here out of the
oracle's exported stage functions, through ctypes: the image pyramid, the seed's pyramid
(resize with the image pyramid's step, then a multiply by float(scaleStep), each level from
the rounded one before), and procOneScale's loop in the structure of oracle/tvl1_oracle.c's
calc_in -- the median before each warp, calcError = eps > 0 && (n & 1) && prevError <
scaledEps, prevError -= scaledEps, the upsample with upmul.  test_initflow_ref_cpu.py pins the
composition against checker.oracle_calc (bitwise, zero seed) before anything trusts it.

The stage functions are IEEE only.  The oracle has since grown a seeded whole-solve entry of its
own (orc_tvl1_calc_init, checker.oracle_calc(init=...)) in both of its arithmetics:
test_initflow_ref_cpu.py holds it to this composition bit for bit in IEEE, and it is the
reference of the seeded solves in fma mode (fast_math 2, reference(..., math=2) below).
fast_math 1 has no seeded reference.

Also here: the deterministic seeds and the one table of (case, seed) pairs the GPU tests use,
so the CPU suite can hold every one of them to the project's residual margin."""
from __future__ import annotations

import ctypes as C

import numpy as np

from optflow_amd import capi, synth
from oracle import checker

MAX_LEVELS = capi.TVL1_MAX_LEVELS
_F = C.POINTER(C.c_float)
_lib_cache = []


def _lib():
    if _lib_cache:
        return _lib_cache[0]
    lib = C.CDLL(str(checker.ORACLE_SO))
    lib.orc_pyramid_sizes.restype = C.c_int
    lib.orc_pyramid_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.orc_convert_u8.restype = None
    lib.orc_convert_u8.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.c_int, _F]
    lib.orc_resize_linear.restype = None
    lib.orc_resize_linear.argtypes = [_F, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_float,
                                      C.c_float]
    lib.orc_centered_gradient.restype = None
    lib.orc_centered_gradient.argtypes = [_F, C.c_int, C.c_int, _F, _F]
    lib.orc_median.restype = None
    lib.orc_median.argtypes = [_F, C.c_int, C.c_int, C.c_int, _F]
    lib.orc_warp_backward.restype = None
    lib.orc_warp_backward.argtypes = [_F] * 6 + [C.c_int, C.c_int] + [_F] * 4
    lib.orc_estimate_u.restype = C.c_double
    lib.orc_estimate_u.argtypes = [_F] * 13 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                               C.c_int]
    lib.orc_estimate_dual.restype = None
    lib.orc_estimate_dual.argtypes = [_F] * 9 + [C.c_int, C.c_int, C.c_float, C.c_float]
    lib.orc_postprocess.restype = None
    lib.orc_postprocess.argtypes = [_F, _F, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_int,
                                    C.c_int, C.c_int]
    _lib_cache.append(lib)
    return lib


def _p(a):
    return a.ctypes.data_as(_F) if a is not None else None


def _f32(x):
    return float(np.float32(x))


def pyramid_sizes(w, h, params):
    ws, hs = (C.c_int * MAX_LEVELS)(), (C.c_int * MAX_LEVELS)()
    L = _lib().orc_pyramid_sizes(w, h, min(params.nscales, MAX_LEVELS), params.scale_step, ws, hs)
    return list(ws[:L]), list(hs[:L])


def _resize(src, dw, dh, fx, fy):
    sh, sw = src.shape
    dst = np.empty((dh, dw), np.float32)
    _lib().orc_resize_linear(_p(src), sw, sh, _p(dst), dw, dh, fx, fy)
    return dst


def seed_pyramid(u0, v0, params):
    """[A.2b] the seed's levels, finest first: u[s] = resize(u[s-1]) * float(scaleStep)."""
    h, w = u0.shape
    ws, hs = pyramid_sizes(w, h, params)
    fdown = _f32(1.0 / params.scale_step)
    mul = np.float32(params.scale_step)
    lv = [(np.ascontiguousarray(u0, np.float32), np.ascontiguousarray(v0, np.float32))]
    for s in range(1, len(ws)):
        lv.append(tuple(_resize(a, ws[s], hs[s], fdown, fdown) * mul for a in lv[s - 1]))
    return lv


def seeded_calc(I0, I1, params, u0=None, v0=None):
    """The solve of tvl1_calc_init (profile 0, IEEE) on host u8 frames from the seed (u0, v0)
    (None: zero).  Returns (u, v, warp_iters (levels, warps), trace (n, 4): level, warp, n,
    error / scaledEps)."""
    lib = _lib()
    p = params
    assert p.profile == 0 and p.fast_math == 0
    I0 = np.ascontiguousarray(I0, np.uint8)
    I1 = np.ascontiguousarray(I1, np.uint8)
    h, w = I0.shape
    ws, hs = pyramid_sizes(w, h, p)
    L = len(ws)
    gam = p.gamma != 0.0
    fdown = _f32(1.0 / p.scale_step)
    pyr0, pyr1 = [np.empty((h, w), np.float32)], [np.empty((h, w), np.float32)]
    lib.orc_convert_u8(capi._u8_ptr(I0), w, w, h, _p(pyr0[0]))
    lib.orc_convert_u8(capi._u8_ptr(I1), w, w, h, _p(pyr1[0]))
    for s in range(1, L):
        pyr0.append(_resize(pyr0[s - 1], ws[s], hs[s], fdown, fdown))
        pyr1.append(_resize(pyr1[s - 1], ws[s], hs[s], fdown, fdown))
    if u0 is None:
        u1 = np.zeros((hs[L - 1], ws[L - 1]), np.float32)
        u2 = np.zeros_like(u1)
    else:
        u1, u2 = (np.array(a, np.float32, order="C") for a in seed_pyramid(u0, v0, p)[L - 1])
    u3 = np.zeros_like(u1) if gam else None

    l_t, taut = _f32(p.lambda_ * p.theta), _f32(p.tau / p.theta)
    theta, gamma = _f32(p.theta), _f32(p.gamma)
    upmul = np.float32(1.0 / p.scale_step)
    wi = np.zeros((L, p.warps), np.int32)
    trace = []
    for s in range(L - 1, -1, -1):
        lw, lh = ws[s], hs[s]
        scaled_eps = p.epsilon * p.epsilon * float(lw * lh)
        I1x, I1y = np.empty((lh, lw), np.float32), np.empty((lh, lw), np.float32)
        lib.orc_centered_gradient(_p(pyr1[s]), lw, lh, _p(I1x), _p(I1y))
        pp = [np.zeros((lh, lw), np.float32) for _ in range(6 if gam else 4)] + ([] if gam else [None, None])
        I1wx, I1wy, grad, rho = (np.empty((lh, lw), np.float32) for _ in range(4))
        for wp in range(p.warps):
            if p.median_filtering > 1:
                tmp = np.empty((lh, lw), np.float32)
                lib.orc_median(_p(u1), lw, lh, p.median_filtering, _p(tmp))
                u1[...] = tmp
                lib.orc_median(_p(u2), lw, lh, p.median_filtering, _p(tmp))
                u2[...] = tmp
            lib.orc_warp_backward(_p(pyr0[s]), _p(pyr1[s]), _p(I1x), _p(I1y), _p(u1), _p(u2), lw, lh,
                                  _p(I1wx), _p(I1wy), _p(grad), _p(rho))
            error, prev = np.finfo(np.float64).max, 0.0
            n = 0
            while error > scaled_eps and n < p.iterations:
                calc = p.epsilon > 0 and (n & 1) == 1 and prev < scaled_eps
                e = lib.orc_estimate_u(_p(I1wx), _p(I1wy), _p(grad), _p(rho), *[_p(a) for a in pp],
                                       _p(u1), _p(u2), _p(u3), lw, lh, l_t, theta, gamma, int(calc))
                if calc:
                    error = prev = e
                    trace.append((s, wp, n, error / scaled_eps))
                else:
                    error = np.finfo(np.float64).max
                    prev -= scaled_eps
                lib.orc_estimate_dual(_p(u1), _p(u2), _p(u3), *[_p(a) for a in pp], lw, lh, taut, gamma)
                n += 1
            wi[s, wp] = n
        if s == 0:
            break
        dw, dh = ws[s - 1], hs[s - 1]
        fxu, fyu = _f32(1.0 / (dw / lw)), _f32(1.0 / (dh / lh))
        u1 = _resize(u1, dw, dh, fxu, fyu) * upmul
        u2 = _resize(u2, dw, dh, fxu, fyu) * upmul
        if gam:
            u3 = _resize(u3, dw, dh, fxu, fyu)
    return u1, u2, wi, np.array(trace, np.float64).reshape(-1, 4)


def postprocess(u, v, I1, mode):
    """orc_postprocess (solve_wrapper's post-ops) on copies."""
    uu, vv = np.array(u, np.float32, order="C"), np.array(v, np.float32, order="C")
    i1 = np.ascontiguousarray(I1, np.uint8)
    h, w = uu.shape
    _lib().orc_postprocess(_p(uu), _p(vv), 4 * w, capi._u8_ptr(i1), w, w, h, int(mode))
    return uu, vv


# ---- deterministic float32 seeds
def make_seed(kind, w, h, rng=0):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        return ((3.5 + 2.0 * np.sin(3 * np.pi * ys / h)).astype(np.float32),
                (-2.25 + 1.5 * np.cos(2 * np.pi * xs / w)).astype(np.float32))
    if kind == "rough":   # every bit of the resize chain matters
        g = np.random.default_rng(rng)
        return (g.uniform(-4, 4, (h, w)).astype(np.float32), g.uniform(-4, 4, (h, w)).astype(np.float32))
    if kind == "far":     # > 6 px at the coarsest level of nscales 3: the global gather
        return np.full((h, w), 14, np.float32), np.full((h, w), -11, np.float32)
    if kind == "zero":
        return np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    raise KeyError(kind)


def shifted_pair(w, h, rng, dx, dy):
    """frame1 = frame0 translated by (dx, dy) px (np.roll): the true flow is (dx, dy)."""
    I0 = synth.gen_pair(w, h, seed=rng)[0]
    return I0, np.roll(I0, (dy, dx), axis=(0, 1))


def frames_of(case):
    if case.get("shift"):
        return shifted_pair(case["w"], case["h"], case["rng"], *case["shift"])
    return synth.gen_pair(case["w"], case["h"], seed=case["rng"], z=case.get("z", 1))


def seed_of(case, kind=None):
    return make_seed(kind or case["seed"], case["w"], case["h"], rng=case["rng"] + 1000)


# ---- the (case, seed) pairs of the GPU tests: tests/test_gpu_initflow.py takes SINGLE,
# tests/test_gpu_initflow_batch.py BATCH (per-pair seeds listed in order), the CLI test CLI.
# test_initflow_ref_cpu.py holds each to checker.check_margins >= 1e-4; a case that misses
# gets another rng, never another margin.
SINGLE = {
    "w97_smooth": dict(w=97, h=40, kw=dict(nscales=3, warps=3), seed="smooth", rng=11),
    "w97_rough": dict(w=97, h=40, kw=dict(nscales=3, warps=3), seed="rough", rng=11),
    "far_gather": dict(w=192, h=160, kw=dict(nscales=3, warps=5), seed="far", rng=22, shift=(14, -11)),
    "early_break": dict(w=40, h=24, kw=dict(nscales=5), seed="rough", rng=13),
    "one_level_pitched": dict(w=50, h=30, kw=dict(nscales=1), seed="rough", rng=14, pitch_extra=64),
    "one_level_chip": dict(w=130, h=12, kw=dict(nscales=1), seed="rough", rng=19),   # a batch solves it on chip
    "gamma": dict(w=97, h=61, kw=dict(gamma=0.1), seed="smooth", rng=15),
    "median5": dict(w=96, h=64, kw=dict(median_filtering=5), seed="rough", rng=16),
    "fixed_work": dict(w=200, h=60, kw=dict(nscales=4, warps=3, epsilon=0.0, iterations=7),
                       seed="rough", rng=17),
    "strip9": dict(w=300, h=100, kw=dict(nscales=10, warps=5), seed="smooth", rng=18),
}
BATCH = {
    "strip6": dict(n=6, w=300, h=100, kw=dict(nscales=10, warps=5), rng=130,
                   seeds=["smooth", "rough", "zero", "rough", "smooth", "zero"]),
    "b3": dict(n=3, w=250, h=131, kw=dict(nscales=5, warps=5), rng=210,
               seeds=["rough", "zero", "smooth"]),
}
BATCH_GAMMA = dict(n=3, w=97, h=61, kw=dict(gamma=0.1, nscales=4, warps=3), rng=300,
                   seeds=["smooth", "rough", "zero"])
CLI = dict(w=256, h=192, rng=404, shift=(12, -9))


def batch_pair(case, b):
    """Frames and seed of pair b of a BATCH case."""
    c = dict(w=case["w"], h=case["h"], rng=case["rng"] + b, z=1 + b % 3)
    return frames_of(c), seed_of(c, case["seeds"][b])


_ref_cache = {}


def reference(key, I0, I1, params_kw, u0, v0, math=0):
    """(u, v, warp_iters, trace) of the seeded solve, computed once per key and arithmetic and
    shared (the results are never written to): math 0 seeded_calc, math 2 the oracle's own
    seeded entry in fma mode."""
    if (key, math) not in _ref_cache:
        if math == 0:
            r = seeded_calc(I0, I1, capi.make_params(**params_kw), u0, v0)
        else:
            u, v, _, wi, tr = checker.oracle_check_trace(I0, I1, capi.make_params(fast_math=math, **params_kw),
                                                         init=(u0, v0))
            r = (u, v, wi, tr)
        for a in r:
            a.setflags(write=False)
        _ref_cache[(key, math)] = r
    return _ref_cache[(key, math)]
