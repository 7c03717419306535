"""ctypes mirror of include/tvl1.h (the C-ABI boundary).

This is the binding a Python caller (tests, bench.py) uses; the production
caller is the C++ `optflow` CLI (fibsem-optflow_amd/cli/optflow.cpp), which
links the same library.  Mirrors the reference boundary
/root/reference/src/optflow.cpp:516-520 (TVL1_solve) — see include/tvl1.h.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_ROOT = Path(__file__).resolve().parent.parent          # fibsem-optflow_amd/
REPO_ROOT = PKG_ROOT.parent
ENGINE_SO = PKG_ROOT / "lib" / "libtvl1_hip.so"

TVL1_MAX_LEVELS = 32
ABI_VERSION = 9          # TVL1_ABI_VERSION of include/tvl1.h
STATUS = {0: "TVL1_OK", 1: "TVL1_EINVAL", 2: "TVL1_ESIZE", 3: "TVL1_EHIP",
          4: "TVL1_ENOMEM", 5: "TVL1_ENODEV"}


class TVL1Params(C.Structure):
    _fields_ = [
        ("tau", C.c_double),
        ("lambda_", C.c_double),
        ("theta", C.c_double),
        ("nscales", C.c_int32),
        ("warps", C.c_int32),
        ("epsilon", C.c_double),
        ("iterations", C.c_int32),
        ("scale_step", C.c_double),
        ("gamma", C.c_double),
        ("use_initial_flow", C.c_int32),
        ("median_filtering", C.c_int32),
        ("fast_math", C.c_int32),
        ("profile", C.c_int32),
        ("inner_iterations", C.c_int32),
        ("outer_iterations", C.c_int32),
    ]


class TVL1Stats(C.Structure):
    _fields_ = [
        ("levels", C.c_int32),
        ("level_width", C.c_int32 * TVL1_MAX_LEVELS),
        ("level_height", C.c_int32 * TVL1_MAX_LEVELS),
        ("level_iterations", C.c_int64 * TVL1_MAX_LEVELS),
        ("iterations_total", C.c_int64),
        ("checks_total", C.c_int64),
        ("algorithmic_bytes", C.c_double),
        ("warp_iterations", C.POINTER(C.c_int32)),
        ("warp_iterations_capacity", C.c_int32),
        ("speculation_misses", C.c_int32),
        ("kernel_ms", C.c_double * 4),
        ("kernel_launches", C.c_int64 * 4),
        ("kernel_bytes", C.c_double * 4),
        ("kernel_hbm_bytes", C.c_double * 4),
    ]


class TVL1AlignParams(C.Structure):
    """tvl1_align_params (include/tvl1.h): orb_defaults (features.cpp:19-31) + ratio / homo /
    ransac (:109, :133)."""
    _fields_ = [
        ("nfeatures", C.c_int32),
        ("scale_factor", C.c_float),
        ("nlevels", C.c_int32),
        ("edge_threshold", C.c_int32),
        ("first_level", C.c_int32),
        ("wta_k", C.c_int32),
        ("patch_size", C.c_int32),
        ("fast_threshold", C.c_int32),
        ("blur_for_descriptor", C.c_int32),
        ("ratio", C.c_float),
        ("method", C.c_int32),
        ("ransac_threshold", C.c_double),
    ]


class TVL1Shift(C.Structure):
    """tvl1_shift (include/tvl1.h): the record of tvl1_estimate_shift."""
    _fields_ = [
        ("dx", C.c_int32),
        ("dy", C.c_int32),
        ("levels", C.c_int32),
        ("reserved", C.c_int32),
        ("sad", C.c_uint64),
        ("count", C.c_uint64),
        ("sad_zero", C.c_uint64),
        ("count_zero", C.c_uint64),
    ]


class InvertCounts(C.Structure):
    """tvl1_invert_counts (include/tvl1.h): the per-pair record of tvl1_invert_flow."""
    _fields_ = [("outside", C.c_uint64), ("unconverged", C.c_uint64)]


def shift_dict(r: TVL1Shift) -> dict:
    return dict(dx=int(r.dx), dy=int(r.dy), levels=int(r.levels), sad=int(r.sad),
                count=int(r.count), sad_zero=int(r.sad_zero), count_zero=int(r.count_zero))


# generate_TV_args defaults, /root/reference/src/optflow.cpp:503-512
DEFAULTS = dict(tau=0.25, lambda_=0.05, theta=0.3, nscales=10, warps=5, epsilon=0.01,
                iterations=300, scale_step=0.8, gamma=0.0, use_initial_flow=0,
                median_filtering=1, fast_math=0, profile=0, inner_iterations=30,
                outer_iterations=10)

# JSON key -> struct field (JSON keys are the reference's, optflow.cpp:503-512)
JSON_KEYS = {"tau": "tau", "lambda": "lambda_", "theta": "theta", "nscales": "nscales",
             "warps": "warps", "epsilon": "epsilon", "iterations": "iterations",
             "scaleStep": "scale_step", "gamma": "gamma", "useInitialFlow": "use_initial_flow",
             "medianFiltering": "median_filtering", "fastMath": "fast_math",
             "profile": "profile", "innerIterations": "inner_iterations",
             "outerIterations": "outer_iterations"}


def make_params(**kw) -> TVL1Params:
    d = dict(DEFAULTS)
    for k, v in kw.items():
        k = JSON_KEYS.get(k, k)
        if k == "lambda":
            k = "lambda_"
        if k not in d:
            raise KeyError(f"unknown TV-L1 parameter {k!r}")
        d[k] = v
    p = TVL1Params()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def stats_dict(st: TVL1Stats, warps: int | None = None) -> dict:
    L = st.levels
    out = {
        "levels": L,
        "sizes": [(st.level_width[i], st.level_height[i]) for i in range(L)],
        "level_iterations": [int(st.level_iterations[i]) for i in range(L)],
        "iterations_total": int(st.iterations_total),
        "checks_total": int(st.checks_total),
        "speculation_misses": int(st.speculation_misses),
        "algorithmic_bytes": float(st.algorithmic_bytes),
        "kernel_ms": [float(st.kernel_ms[i]) for i in range(4)],
        "kernel_launches": [int(st.kernel_launches[i]) for i in range(4)],
        "kernel_bytes": [float(st.kernel_bytes[i]) for i in range(4)],
        "kernel_hbm_bytes": [float(st.kernel_hbm_bytes[i]) for i in range(4)],
    }
    return out


def _u8_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f32_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Library:
    """Loads the HIP engine library."""

    def __init__(self, path: Path):
        if not Path(path).exists():
            raise FileNotFoundError(f"{path} not built (run __graft_entry__.build())")
        self.path = Path(path)
        self.lib = C.CDLL(str(path))


def load_engine() -> C.CDLL:
    """The product: libtvl1_hip.so (HIP kernels for gfx950 + C-ABI).  Raises
    if it was not built — there is no CPU fallback."""
    # TVL1_ENGINE_SO: another build of the same engine (A/B runs of tools/ab_lib.sh)
    path = Path(os.environ.get("TVL1_ENGINE_SO", ENGINE_SO))
    lib = Library(path).lib
    lib.tvl1_params_default.argtypes = [C.POINTER(TVL1Params)]
    lib.tvl1_params_default.restype = None
    lib.tvl1_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(TVL1Params)]
    lib.tvl1_create.restype = C.c_int
    lib.tvl1_set_params.argtypes = [C.c_void_p, C.POINTER(TVL1Params)]
    lib.tvl1_set_params.restype = C.c_int
    lib.tvl1_calc.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                              C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                              C.POINTER(TVL1Stats), C.c_void_p]
    lib.tvl1_calc.restype = C.c_int
    lib.tvl1_calc_f32.argtypes = lib.tvl1_calc.argtypes
    lib.tvl1_calc_f32.restype = C.c_int
    lib.tvl1_calc_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t,
                                    C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                    C.POINTER(TVL1Stats), C.c_void_p]
    lib.tvl1_calc_batch.restype = C.c_int
    # solves from a caller-supplied flow (added under ABI 9)
    lib.tvl1_calc_init.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TVL1Stats),
                                   C.c_void_p]
    lib.tvl1_calc_init.restype = C.c_int
    lib.tvl1_calc_host_init.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t,
                                        C.POINTER(C.c_uint8), C.c_size_t, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t,
                                        C.POINTER(TVL1Stats)]
    lib.tvl1_calc_host_init.restype = C.c_int
    lib.tvl1_calc_batch_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.POINTER(TVL1Stats), C.c_void_p]
    lib.tvl1_calc_batch_init.restype = C.c_int
    lib.tvl1_align_params_default.argtypes = [C.POINTER(TVL1AlignParams)]
    lib.tvl1_align_params_default.restype = None
    lib.tvl1_find_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                        C.POINTER(TVL1AlignParams), C.POINTER(C.c_float),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.tvl1_find_alignment.restype = C.c_int
    lib.tvl1_orb_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                    C.POINTER(TVL1AlignParams), C.c_void_p, C.c_void_p, C.c_int32,
                                    C.POINTER(C.c_int32), C.c_void_p]
    lib.tvl1_orb_detect.restype = C.c_int
    lib.tvl1_match_knn2.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tvl1_match_knn2.restype = C.c_int
    lib.tvl1_warp_affine_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_float), C.c_void_p]
    lib.tvl1_warp_affine_u8.restype = C.c_int
    lib.tvl1_find_homography.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                         C.POINTER(C.c_double), C.c_void_p]
    lib.tvl1_find_homography.restype = C.c_int
    lib.tvl1_postprocess_affine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                            C.c_int32, C.POINTER(C.c_float), C.c_void_p]
    lib.tvl1_postprocess_affine.restype = C.c_int
    lib.tvl1_calc_host.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t,
                                   C.POINTER(C.c_uint8), C.c_size_t, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t,
                                   C.POINTER(TVL1Stats)]
    lib.tvl1_calc_host.restype = C.c_int
    lib.tvl1_postprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p]
    lib.tvl1_postprocess.restype = C.c_int
    lib.tvl1_postprocess_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.tvl1_postprocess_batch.restype = C.c_int
    lib.tvl1_gather_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    lib.tvl1_gather_flow.restype = C.c_int
    # average-flow alignment of a slice list (added under ABI 9)
    lib.tvl1_blend6_weights.argtypes = [C.POINTER(C.c_float)]
    lib.tvl1_blend6_weights.restype = None
    lib.tvl1_blend6_u8.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_blend6_u8.restype = C.c_int
    lib.tvl1_half_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_half_u8.restype = C.c_int
    lib.tvl1_remap_flow_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                       C.c_double, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_remap_flow_u8.restype = C.c_int
    # integer drift estimate (added under ABI 9)
    lib.tvl1_estimate_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_int32, C.c_int32, C.c_int32, C.POINTER(TVL1Shift),
                                        C.c_void_p]
    lib.tvl1_estimate_shift.restype = C.c_int
    lib.tvl1_estimate_shift_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(TVL1Shift), C.c_void_p]
    lib.tvl1_estimate_shift_batch.restype = C.c_int
    # batched solves seeded by one constant per pair (added under ABI 9)
    lib.tvl1_calc_batch_const_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                               C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                               C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                               C.POINTER(TVL1Stats), C.c_void_p]
    lib.tvl1_calc_batch_const_init.restype = C.c_int
    lib.tvl1_calc_batch_auto_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(TVL1Shift), C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_size_t, C.POINTER(TVL1Stats),
                                              C.c_void_p]
    lib.tvl1_calc_batch_auto_init.restype = C.c_int
    lib.tvl1_sad_shifts_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p]
    lib.tvl1_sad_shifts_u8.restype = C.c_int
    # forward-backward consistency score (added under ABI 9)
    lib.tvl1_fb_score_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                        C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_size_t,
                                        C.c_size_t, C.c_void_p]
    lib.tvl1_fb_score_batch.restype = C.c_int
    lib.tvl1_fb_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_float,
                                  C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_fb_score.restype = C.c_int
    lib.tvl1_zero_above_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32,
                                          C.c_int32, C.c_float, C.POINTER(C.c_uint64), C.c_void_p]
    lib.tvl1_zero_above_batch.restype = C.c_int
    lib.tvl1_zero_above.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_size_t, C.c_int32, C.c_int32, C.c_float,
                                    C.POINTER(C.c_uint64), C.c_void_p]
    lib.tvl1_zero_above.restype = C.c_int
    # photometric (ZNCC) score of a flow (added under ABI 9)
    lib.tvl1_zncc_score_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.tvl1_zncc_score_batch.restype = C.c_int
    lib.tvl1_zncc_score.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_zncc_score.restype = C.c_int
    lib.tvl1_warp_by_flow_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_size_t, C.c_void_p]
    lib.tvl1_warp_by_flow_u8.restype = C.c_int
    # flow composition (added under ABI 9)
    lib.tvl1_compose_flow_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p]
    lib.tvl1_compose_flow_batch.restype = C.c_int
    lib.tvl1_compose_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p]
    lib.tvl1_compose_flow.restype = C.c_int
    # flow inversion (added under ABI 9)
    lib.tvl1_invert_flow_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_size_t, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                           C.c_int32, C.c_int32, C.POINTER(InvertCounts), C.c_void_p]
    lib.tvl1_invert_flow_batch.restype = C.c_int
    lib.tvl1_invert_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_int32, C.c_int32, C.POINTER(InvertCounts), C.c_void_p]
    lib.tvl1_invert_flow.restype = C.c_int
    lib.tvl1_stream.argtypes = [C.c_void_p]
    lib.tvl1_stream.restype = C.c_void_p
    lib.tvl1_set_profiling.argtypes = [C.c_void_p, C.c_int32]
    lib.tvl1_set_profiling.restype = C.c_int
    lib.tvl1_destroy.argtypes = [C.c_void_p]
    lib.tvl1_destroy.restype = None
    lib.tvl1_last_error.argtypes = [C.c_void_p]
    lib.tvl1_last_error.restype = C.c_char_p
    lib.tvl1_abi_version.restype = C.c_int32
    lib.tvl1_device_count.restype = C.c_int32
    if lib.tvl1_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.tvl1_abi_version()}, binding expects {ABI_VERSION}")
    return lib


class TVL1Error(RuntimeError):
    pass


def align_params(lib, **kw) -> TVL1AlignParams:
    """tvl1_align_params_default (orb_defaults, features.cpp:19-31) with overrides."""
    ap = TVL1AlignParams()
    lib.tvl1_align_params_default(C.byref(ap))
    for k, v in kw.items():
        setattr(ap, k, v)
    return ap


class Engine:
    """Host-side handle on the HIP engine (one ctx per device)."""

    def __init__(self, params: TVL1Params | None = None, device: int = 0):
        self.lib = load_engine()
        self.params = params or make_params()
        self.ctx = C.c_void_p()
        rc = self.lib.tvl1_create(C.byref(self.ctx), int(device), C.byref(self.params))
        if rc != 0:
            raise TVL1Error(f"tvl1_create: {STATUS.get(rc, rc)}: "
                            f"{self.lib.tvl1_last_error(None).decode()}")

    def set_params(self, params: TVL1Params):
        self.params = params
        self._check(self.lib.tvl1_set_params(self.ctx, C.byref(params)), "tvl1_set_params")

    @property
    def stream(self) -> int:
        """The ctx's own non-blocking hipStream_t (as an int handle)."""
        return int(self.lib.tvl1_stream(self.ctx) or 0)

    def set_profiling(self, on: bool):
        self._check(self.lib.tvl1_set_profiling(self.ctx, 1 if on else 0), "tvl1_set_profiling")

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.tvl1_last_error(self.ctx)
            raise TVL1Error(f"{what}: {STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def calc_host(self, I0: np.ndarray, I1: np.ndarray, warp_iters: bool = True, init=None):
        """tvl1_calc_host; init = (u0, v0[, pitch]): tvl1_calc_host_init from that flow (float32
        arrays of the frame's size with unit column stride; pitch in bytes, default their row
        stride)."""
        I0 = np.ascontiguousarray(I0, dtype=np.uint8)
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        h, w = I0.shape
        if I1.shape != I0.shape:
            raise ValueError("I0 and I1 must have the same size")
        u = np.zeros((h, w), np.float32)
        v = np.zeros((h, w), np.float32)
        st = TVL1Stats()
        wi = None
        if warp_iters:
            cap = TVL1_MAX_LEVELS * max(1, self.params.warps)
            wi = np.full(cap, -1, np.int32)
            st.warp_iterations = wi.ctypes.data_as(C.POINTER(C.c_int32))
            st.warp_iterations_capacity = cap
        if init is None:
            rc = self.lib.tvl1_calc_host(self.ctx, _u8_ptr(I0), w, _u8_ptr(I1), w, w, h,
                                         _f32_ptr(u), _f32_ptr(v), 4 * w, C.byref(st))
            self._check(rc, "tvl1_calc_host")
        else:
            u0, v0 = (np.asarray(a, dtype=np.float32) for a in init[:2])
            if u0.shape != (h, w) or v0.shape != (h, w):
                raise ValueError("the initial flow must have the frames' size")
            if u0.strides[1] != 4 or v0.strides[1] != 4 or u0.strides[0] != v0.strides[0]:
                raise ValueError("the initial flow planes need unit column stride and one row pitch")
            ipitch = int(init[2]) if len(init) > 2 else u0.strides[0]
            rc = self.lib.tvl1_calc_host_init(self.ctx, _u8_ptr(I0), w, _u8_ptr(I1), w, w, h,
                                              _f32_ptr(u0), _f32_ptr(v0), ipitch, _f32_ptr(u),
                                              _f32_ptr(v), 4 * w, C.byref(st))
            self._check(rc, "tvl1_calc_host_init")
        sd = stats_dict(st)
        if wi is not None:
            wi = wi[: sd["levels"] * self.params.warps].reshape(sd["levels"], self.params.warps)
        return u, v, sd, wi

    def calc_device(self, dI0: int, pitch0: int, dI1: int, pitch1: int, w: int, h: int,
                    du: int, dv: int, flow_pitch: int, stream: int = 0, stats: bool = True,
                    warp_iters: bool = False, f32: bool = False, init=None):
        """tvl1_calc on device buffers (u8 frames, pitches in bytes), or tvl1_calc_f32 with
        f32=True (float frames in [0, 1], pitches in bytes).  init = (du0, dv0[, pitch]):
        tvl1_calc_init from that flow (device pointers; pitch in bytes, default 4 * w)."""
        if init is not None and f32:
            raise ValueError("tvl1_calc_f32 takes no initial flow")
        st = TVL1Stats() if stats or warp_iters else None
        wi = None
        if warp_iters:
            cap = TVL1_MAX_LEVELS * max(1, self.params.warps)
            wi = np.full(cap, -1, np.int32)
            st.warp_iterations = wi.ctypes.data_as(C.POINTER(C.c_int32))
            st.warp_iterations_capacity = cap
        if init is None:
            fn = self.lib.tvl1_calc_f32 if f32 else self.lib.tvl1_calc
            rc = fn(self.ctx, C.c_void_p(dI0), pitch0, C.c_void_p(dI1), pitch1,
                    w, h, C.c_void_p(du), C.c_void_p(dv), flow_pitch,
                    C.byref(st) if st is not None else None,
                    C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_f32" if f32 else "tvl1_calc")
        else:
            ipitch = int(init[2]) if len(init) > 2 else 4 * w
            rc = self.lib.tvl1_calc_init(self.ctx, C.c_void_p(dI0), pitch0, C.c_void_p(dI1), pitch1,
                                         w, h, C.c_void_p(init[0]), C.c_void_p(init[1]), ipitch,
                                         C.c_void_p(du), C.c_void_p(dv), flow_pitch,
                                         C.byref(st) if st is not None else None,
                                         C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_init")
        if st is None:
            return None
        sd = stats_dict(st)
        if wi is not None:
            sd["warp_iters"] = wi[: sd["levels"] * self.params.warps].reshape(sd["levels"],
                                                                              self.params.warps)
        return sd

    def calc_batch_device(self, n: int, dI0: int, pitch0: int, stride0: int, dI1: int,
                          pitch1: int, stride1: int, w: int, h: int, du: int, dv: int,
                          flow_pitch: int, flow_stride: int, stream: int = 0,
                          warp_iters: bool = False, init=None, init_const=None,
                          auto_shift=None):
        """tvl1_calc_batch on device buffers: n pairs of one size, pair b at base + b*stride
        (bytes).  Returns one stats dict per pair (+ per-warp iterations if asked).  init =
        (du0, dv0[, pitch[, stride]]): tvl1_calc_batch_init from those flows (device pointers;
        bytes, default 4 * w and pitch * h; stride 0 = one seed for every pair).  init_const =
        (n, 2) float32 host array of (dx, dy) per pair: tvl1_calc_batch_const_init.  auto_shift
        = R: tvl1_calc_batch_auto_init with max_shift R; returns (stats dicts, shift dicts).
        At most one of init, init_const and auto_shift."""
        if sum(x is not None for x in (init, init_const, auto_shift)) > 1:
            raise ValueError("init, init_const and auto_shift exclude one another")
        if init_const is not None:
            init_const = np.ascontiguousarray(init_const, np.float32)
            if init_const.shape != (n, 2):
                raise ValueError(f"init_const must have shape ({n}, 2), got {init_const.shape}")
        sts = (TVL1Stats * n)()
        wis = []
        if warp_iters:
            cap = TVL1_MAX_LEVELS * max(1, self.params.warps)
            for b in range(n):
                wi = np.full(cap, -1, np.int32)
                sts[b].warp_iterations = wi.ctypes.data_as(C.POINTER(C.c_int32))
                sts[b].warp_iterations_capacity = cap
                wis.append(wi)
        shifts = None
        if init_const is not None:
            rc = self.lib.tvl1_calc_batch_const_init(
                self.ctx, n, C.c_void_p(dI0), pitch0, stride0, C.c_void_p(dI1), pitch1, stride1, w,
                h, init_const.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(du), C.c_void_p(dv),
                flow_pitch, flow_stride, sts, C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_batch_const_init")
        elif auto_shift is not None:
            rs = (TVL1Shift * max(1, n))()
            rc = self.lib.tvl1_calc_batch_auto_init(
                self.ctx, n, C.c_void_p(dI0 or None), pitch0, stride0, C.c_void_p(dI1 or None),
                pitch1, stride1, w, h, int(auto_shift), rs, C.c_void_p(du), C.c_void_p(dv),
                flow_pitch, flow_stride, sts, C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_batch_auto_init")
            shifts = [shift_dict(rs[b]) for b in range(n)]
        elif init is None:
            rc = self.lib.tvl1_calc_batch(self.ctx, n, C.c_void_p(dI0), pitch0, stride0,
                                          C.c_void_p(dI1), pitch1, stride1, w, h, C.c_void_p(du),
                                          C.c_void_p(dv), flow_pitch, flow_stride, sts,
                                          C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_batch")
        else:
            ipitch = int(init[2]) if len(init) > 2 else 4 * w
            istride = int(init[3]) if len(init) > 3 else ipitch * h
            rc = self.lib.tvl1_calc_batch_init(self.ctx, n, C.c_void_p(dI0), pitch0, stride0,
                                               C.c_void_p(dI1), pitch1, stride1, w, h,
                                               C.c_void_p(init[0]), C.c_void_p(init[1]), ipitch,
                                               istride, C.c_void_p(du), C.c_void_p(dv), flow_pitch,
                                               flow_stride, sts,
                                               C.c_void_p(stream) if stream else None)
            self._check(rc, "tvl1_calc_batch_init")
        out = [stats_dict(sts[b]) for b in range(n)]
        if warp_iters:
            for b in range(n):
                L = out[b]["levels"]
                out[b]["warp_iters"] = wis[b][: L * self.params.warps].reshape(L, self.params.warps)
        return out if shifts is None else (out, shifts)

    def find_alignment(self, d1: int, pitch1: int, w1: int, h1: int, d0: int, pitch0: int,
                       w0: int, h0: int, **kw):
        """tvl1_find_alignment(frame1, frame0) on device frames -> (affine (2, 3), n_good,
        outcome)."""
        ap = align_params(self.lib, **kw)
        aff = (C.c_float * 6)()
        ng, oc = C.c_int32(0), C.c_int32(0)
        rc = self.lib.tvl1_find_alignment(self.ctx, C.c_void_p(d1), pitch1, w1, h1, C.c_void_p(d0),
                                          pitch0, w0, h0, C.byref(ap), aff, C.byref(ng),
                                          C.byref(oc), None)
        self._check(rc, "tvl1_find_alignment")
        return np.array(list(aff), np.float32).reshape(2, 3), int(ng.value), int(oc.value)

    def orb_detect(self, d: int, pitch: int, w: int, h: int, cap: int = 10000, stream: int = 0, **kw):
        """tvl1_orb_detect on a device frame -> (kp (n, 5): x, y, octave, angle, response;
        desc (n, 32) u8)."""
        ap = align_params(self.lib, **kw)
        kp = np.zeros((cap, 5), np.float32)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int32(0)
        self._check(self.lib.tvl1_orb_detect(self.ctx, C.c_void_p(d), pitch, w, h, C.byref(ap),
                                             kp.ctypes.data, desc.ctypes.data, cap, C.byref(n),
                                             C.c_void_p(stream) if stream else None), "tvl1_orb_detect")
        m = min(n.value, cap)
        return kp[:m], desc[:m]

    def match_knn2(self, query: np.ndarray, train: np.ndarray):
        """tvl1_match_knn2 on host descriptor arrays (n, 32) u8 -> (idx (nq, 2), dist (nq, 2))."""
        q = np.ascontiguousarray(query, np.uint8)
        t = np.ascontiguousarray(train, np.uint8)
        idx = np.zeros((len(q), 2), np.int32)
        dist = np.zeros((len(q), 2), np.int32)
        self._check(self.lib.tvl1_match_knn2(self.ctx, q.ctypes.data, len(q), t.ctypes.data,
                                             len(t), idx.ctypes.data, dist.ctypes.data, None),
                    "tvl1_match_knn2")
        return idx, dist

    def warp_affine_u8(self, src: int, sp: int, sw: int, sh: int, dst: int, dp: int, dw: int,
                       dh: int, affine) -> None:
        a = (C.c_float * 6)(*[float(x) for x in np.asarray(affine, np.float32).ravel()])
        self._check(self.lib.tvl1_warp_affine_u8(self.ctx, C.c_void_p(src), sp, sw, sh,
                                                 C.c_void_p(dst), dp, dw, dh, a, None),
                    "tvl1_warp_affine_u8")

    def postprocess_batch(self, n: int, du: int, dv: int, fpitch: int, fstride: int, dI1: int,
                          pitch1: int, stride1: int, w: int, h: int, mode: int, stream: int = 0):
        """tvl1_postprocess_batch: solve_wrapper's map grid + I1 <= 1 mask on n pairs."""
        self._check(self.lib.tvl1_postprocess_batch(self.ctx, n, du, dv, fpitch, fstride, dI1,
                                                    pitch1, stride1, w, h, mode, stream),
                    "tvl1_postprocess_batch")

    def gather_flow(self, du: int, dv: int, plane_elems: int, offsets, stream: int = 0):
        """tvl1_gather_flow: (u[off], v[off]) for element offsets in [0, plane_elems) into
        device planes (any other offset raises, TVL1_EINVAL)."""
        off = np.ascontiguousarray(offsets, np.int64)
        ou = np.zeros(len(off), np.float32)
        ov = np.zeros(len(off), np.float32)
        self._check(self.lib.tvl1_gather_flow(self.ctx, du, dv, plane_elems, off.ctypes.data,
                                              len(off),
                                              ou.ctypes.data, ov.ctypes.data, stream),
                    "tvl1_gather_flow")
        return ou, ov

    # ---- average-flow alignment of a slice list (tvl1_blend6_u8 ... tvl1_remap_flow_u8) ----
    def blend6_u8(self, frames, pitches, w: int, h: int, dst: int, dst_pitch: int,
                  stream: int = 0) -> None:
        """tvl1_blend6_u8: six device u8 planes (pointers, pitches in bytes; the neighbours
        i-3, i-2, i-1, i+1, i+2, i+3) -> their weighted mean, rounded half-to-even."""
        if len(frames) != 6 or len(pitches) != 6:
            raise ValueError("blend6_u8 takes six frames and six pitches")
        fr = (C.c_void_p * 6)(*[C.c_void_p(int(f) or None) for f in frames])
        pt = (C.c_size_t * 6)(*[int(p) for p in pitches])
        self._check(self.lib.tvl1_blend6_u8(self.ctx, fr, pt, w, h, C.c_void_p(dst or None),
                                            dst_pitch, C.c_void_p(stream) if stream else None),
                    "tvl1_blend6_u8")

    def half_u8(self, src: int, pitch: int, w: int, h: int, dst: int, dst_pitch: int,
                stream: int = 0) -> None:
        """tvl1_half_u8: the 2x2 mean of a w x h device plane (both even) -> w/2 x h/2."""
        self._check(self.lib.tvl1_half_u8(self.ctx, C.c_void_p(src or None), pitch, w, h,
                                          C.c_void_p(dst or None), dst_pitch,
                                          C.c_void_p(stream) if stream else None), "tvl1_half_u8")

    def remap_flow_u8(self, frame: int, pitch: int, w: int, h: int, du: int, dv: int,
                      flow_pitch: int, fw: int, fh: int, gain: float, border: int, dst: int,
                      dst_pitch: int, stream: int = 0) -> None:
        """tvl1_remap_flow_u8: warp a w x h device frame by the fw x fh flow (times gain) onto a
        (w + 2 border) x (h + 2 border) canvas."""
        self._check(self.lib.tvl1_remap_flow_u8(self.ctx, C.c_void_p(frame or None), pitch, w, h,
                                                C.c_void_p(du or None), C.c_void_p(dv or None),
                                                flow_pitch, fw, fh, float(gain), border,
                                                C.c_void_p(dst or None), dst_pitch,
                                                C.c_void_p(stream) if stream else None),
                    "tvl1_remap_flow_u8")

    def align_slice_host(self, frames7, scale: float = 0.5, border: int = 0):
        """One slice of the average-flow alignment on host arrays: frames7 = slices i-3 .. i+3
        (u8, one size).  Uploads them, blends the six neighbours, pre-scales slice and blend
        (scale 1: not at all; 0.5 with even sizes: tvl1_half_u8), solves slice -> blend and
        warps the slice by the flow.  Returns (aligned (h + 2 border, w + 2 border) u8, u, v at
        the solve's size).  Any other pre-scale is not done on the device: it raises."""
        import torch
        if len(frames7) != 7:
            raise ValueError("align_slice_host takes the seven slices i-3 .. i+3")
        fr = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames7]
        h, w = fr[3].shape
        if any(f.shape != (h, w) for f in fr):
            raise ValueError("the seven slices must have one size")
        if scale == 1:
            halve = False
        elif scale == 0.5 and w % 2 == 0 and h % 2 == 0:
            halve = True
        else:
            raise ValueError(f"pre-scale {scale} of a {w}x{h} slice is not done on the device "
                             "(scale 1, or 0.5 with even sizes)")
        if border < 0:
            raise ValueError("border must be >= 0")
        dev = torch.device("cuda", torch.cuda.current_device())
        d = [torch.from_numpy(f).to(dev) for f in fr]
        fw, fh = (w // 2, h // 2) if halve else (w, h)
        blend = torch.empty((h, w), dtype=torch.uint8, device=dev)
        du = torch.empty((fh, fw), dtype=torch.float32, device=dev)
        dv = torch.empty_like(du)
        out = torch.empty((h + 2 * border, w + 2 * border), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        st = self.stream
        nb = [d[k] for k in (0, 1, 2, 4, 5, 6)]
        self.blend6_u8([t.data_ptr() for t in nb], [w] * 6, w, h, blend.data_ptr(), w, stream=st)
        i0, i1 = d[3], blend
        if halve:
            i0 = torch.empty((fh, fw), dtype=torch.uint8, device=dev)
            i1 = torch.empty_like(i0)
            self.half_u8(d[3].data_ptr(), w, w, h, i0.data_ptr(), fw, stream=st)
            self.half_u8(blend.data_ptr(), w, w, h, i1.data_ptr(), fw, stream=st)
        self.calc_device(i0.data_ptr(), fw, i1.data_ptr(), fw, fw, fh, du.data_ptr(), dv.data_ptr(),
                         4 * fw, stream=st, stats=False)
        self.remap_flow_u8(d[3].data_ptr(), w, w, h, du.data_ptr(), dv.data_ptr(), 4 * fw, fw, fh,
                           1.0 / scale, border, out.data_ptr(), w + 2 * border, stream=st)
        torch.cuda.synchronize()
        return out.cpu().numpy(), du.cpu().numpy(), dv.cpu().numpy()

    # ---- integer drift estimate (tvl1_estimate_shift ... tvl1_sad_shifts_u8) ----
    def estimate_shift(self, dI0: int, pitch0: int, dI1: int, pitch1: int, w: int, h: int,
                       max_shift: int, stream: int = 0) -> dict:
        """tvl1_estimate_shift on device u8 frames (pitches in bytes): the integer (dx, dy) with
        I1(x + d) ~= I0(x), |dx|, |dy| <= max_shift, and the sums behind it, as a dict."""
        r = TVL1Shift()
        self._check(self.lib.tvl1_estimate_shift(self.ctx, C.c_void_p(dI0 or None), pitch0,
                                                 C.c_void_p(dI1 or None), pitch1, w, h, max_shift,
                                                 C.byref(r), C.c_void_p(stream) if stream else None),
                    "tvl1_estimate_shift")
        return shift_dict(r)

    def estimate_shift_batch(self, n: int, dI0: int, pitch0: int, stride0: int, dI1: int,
                             pitch1: int, stride1: int, w: int, h: int, max_shift: int,
                             stream: int = 0) -> list:
        """tvl1_estimate_shift_batch: n pairs of one size, pair b at base + b*stride (bytes; 0 =
        one frame for every pair).  One dict per pair."""
        rs = (TVL1Shift * max(1, n))()
        self._check(self.lib.tvl1_estimate_shift_batch(self.ctx, n, C.c_void_p(dI0 or None), pitch0,
                                                       stride0, C.c_void_p(dI1 or None), pitch1,
                                                       stride1, w, h, max_shift, rs,
                                                       C.c_void_p(stream) if stream else None),
                    "tvl1_estimate_shift_batch")
        return [shift_dict(rs[b]) for b in range(n)]

    def sad_shifts_u8(self, dI0: int, pitch0: int, dI1: int, pitch1: int, w: int, h: int,
                      cx: int, cy: int, radius: int, stream: int = 0) -> np.ndarray:
        """tvl1_sad_shifts_u8: S(cx + dx, cy + dy) for dx, dy in [-radius, radius] as a
        (2r + 1, 2r + 1) uint64 array indexed [dy + r, dx + r]."""
        d = 2 * max(1, min(4, int(radius))) + 1
        out = np.zeros((d, d), np.uint64)
        self._check(self.lib.tvl1_sad_shifts_u8(self.ctx, C.c_void_p(dI0 or None), pitch0,
                                                C.c_void_p(dI1 or None), pitch1, w, h, cx, cy,
                                                radius, out.ctypes.data,
                                                C.c_void_p(stream) if stream else None),
                    "tvl1_sad_shifts_u8")
        return out

    def estimate_shift_host(self, I0: np.ndarray, I1: np.ndarray, max_shift: int) -> dict:
        """estimate_shift on host u8 arrays of one size: uploads them and calls."""
        import torch
        I0 = np.array(I0, dtype=np.uint8, order="C")   # copies: torch wants writable arrays
        I1 = np.array(I1, dtype=np.uint8, order="C")
        if I1.shape != I0.shape:
            raise ValueError("I0 and I1 must have the same size")
        h, w = I0.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
        torch.cuda.synchronize()
        return self.estimate_shift(d0.data_ptr(), w, d1.data_ptr(), w, w, h, max_shift,
                                   stream=self.stream)

    # ---- forward-backward consistency score (tvl1_fb_score ... tvl1_zero_above_batch) ----
    def fb_score_batch(self, n: int, duf: int, dvf: int, f_pitch: int, f_stride: int, dub: int,
                       dvb: int, b_pitch: int, b_stride: int, w: int, h: int, alpha: float,
                       dscore: int, s_pitch: int, s_stride: int, stream: int = 0) -> None:
        """tvl1_fb_score_batch on device f32 planes (pitches and pair strides in bytes): the
        score of n pairs' forward flows (uf, vf) against their backward flows (ub, vb)."""
        self._check(self.lib.tvl1_fb_score_batch(
            self.ctx, n, C.c_void_p(duf or None), C.c_void_p(dvf or None), f_pitch, f_stride,
            C.c_void_p(dub or None), C.c_void_p(dvb or None), b_pitch, b_stride, w, h, float(alpha),
            C.c_void_p(dscore or None), s_pitch, s_stride, C.c_void_p(stream) if stream else None),
            "tvl1_fb_score_batch")

    def fb_score(self, duf: int, dvf: int, f_pitch: int, dub: int, dvb: int, b_pitch: int, w: int,
                 h: int, alpha: float, dscore: int, s_pitch: int, stream: int = 0) -> None:
        """tvl1_fb_score: one pair."""
        self._check(self.lib.tvl1_fb_score(
            self.ctx, C.c_void_p(duf or None), C.c_void_p(dvf or None), f_pitch,
            C.c_void_p(dub or None), C.c_void_p(dvb or None), b_pitch, w, h, float(alpha),
            C.c_void_p(dscore or None), s_pitch, C.c_void_p(stream) if stream else None),
            "tvl1_fb_score")

    def zero_above_batch(self, n: int, du: int, dv: int, f_pitch: int, f_stride: int, dscore: int,
                         s_pitch: int, s_stride: int, w: int, h: int, beta: float,
                         stream: int = 0, count: bool = True):
        """tvl1_zero_above_batch: u = v = 0 where !(score <= beta), in place.  Returns the
        rejected px of each pair (uint64 array of n), or None with count=False (the call then
        stays asynchronous)."""
        rej = np.zeros(max(1, n), np.uint64) if count else None
        self._check(self.lib.tvl1_zero_above_batch(
            self.ctx, n, C.c_void_p(du or None), C.c_void_p(dv or None), f_pitch, f_stride,
            C.c_void_p(dscore or None), s_pitch, s_stride, w, h, float(beta),
            rej.ctypes.data_as(C.POINTER(C.c_uint64)) if count else None,
            C.c_void_p(stream) if stream else None), "tvl1_zero_above_batch")
        return rej[:max(0, n)] if count else None

    def zero_above(self, du: int, dv: int, f_pitch: int, dscore: int, s_pitch: int, w: int, h: int,
                   beta: float, stream: int = 0) -> int:
        """tvl1_zero_above: one pair; returns its rejected px."""
        rej = C.c_uint64(0)
        self._check(self.lib.tvl1_zero_above(
            self.ctx, C.c_void_p(du or None), C.c_void_p(dv or None), f_pitch,
            C.c_void_p(dscore or None), s_pitch, w, h, float(beta), C.byref(rej),
            C.c_void_p(stream) if stream else None), "tvl1_zero_above")
        return int(rej.value)

    def calc_consistent(self, I0: np.ndarray, I1: np.ndarray, alpha: float = 0.01,
                        beta: float = 0.5, init=None):
        """Forward solve I0 -> I1, backward solve I1 -> I0 (the frames swapped), their score,
        and the forward flow zeroed where !(score <= beta).  Host u8 arrays of one size in;
        returns (u, v, score, rejected): float32 arrays and the number of zeroed px.  init =
        (dx, dy): both solves start from a constant flow (tvl1_calc_batch_const_init), the
        forward one from (dx, dy), the backward one from (-dx, -dy)."""
        import torch
        I0 = np.array(I0, dtype=np.uint8, order="C")   # copies: torch wants writable arrays
        I1 = np.array(I1, dtype=np.uint8, order="C")
        if I1.shape != I0.shape:
            raise ValueError("I0 and I1 must have the same size")
        h, w = I0.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
        fl = torch.zeros((5, h, w), dtype=torch.float32, device=dev)   # uf, vf, ub, vb, score
        torch.cuda.synchronize()
        st = self.stream
        p = [fl[k].data_ptr() for k in range(5)]
        for (a, b, pu, pv, sign) in ((d0, d1, p[0], p[1], 1.0), (d1, d0, p[2], p[3], -1.0)):
            if init is None:
                self.calc_device(a.data_ptr(), w, b.data_ptr(), w, w, h, pu, pv, 4 * w, stream=st,
                                 stats=False)
            else:
                seed = np.array([[sign * float(init[0]), sign * float(init[1])]], np.float32)
                self.calc_batch_device(1, a.data_ptr(), w, w * h, b.data_ptr(), w, w * h, w, h,
                                       pu, pv, 4 * w, 4 * w * h, stream=st, init_const=seed)
        self.fb_score(p[0], p[1], 4 * w, p[2], p[3], 4 * w, w, h, alpha, p[4], 4 * w, stream=st)
        rejected = self.zero_above(p[0], p[1], 4 * w, p[4], 4 * w, w, h, beta, stream=st)
        torch.cuda.synchronize()
        out = fl.cpu().numpy()
        return out[0], out[1], out[4], rejected

    # ---- photometric (ZNCC) score of a flow (tvl1_zncc_score*, tvl1_warp_by_flow_u8) ----
    def zncc_score_batch(self, n: int, dI0: int, pitch0: int, stride0: int, dI1: int, pitch1: int,
                         stride1: int, du: int, dv: int, f_pitch: int, f_stride: int, w: int, h: int,
                         radius: int, dscore: int, s_pitch: int, s_stride: int, stream: int = 0) -> None:
        """tvl1_zncc_score_batch on device planes (pitches and pair strides in bytes): 1 - ZNCC of
        a (2 radius + 1)^2 window of frame0 against frame1 warped back along the flow (du, dv),
        for n pairs; a frame pair stride 0 is one frame shared by every pair."""
        self._check(self.lib.tvl1_zncc_score_batch(
            self.ctx, n, C.c_void_p(dI0 or None), pitch0, stride0, C.c_void_p(dI1 or None), pitch1,
            stride1, C.c_void_p(du or None), C.c_void_p(dv or None), f_pitch, f_stride, w, h, radius,
            C.c_void_p(dscore or None), s_pitch, s_stride, C.c_void_p(stream) if stream else None),
            "tvl1_zncc_score_batch")

    def zncc_score(self, dI0: int, pitch0: int, dI1: int, pitch1: int, du: int, dv: int, f_pitch: int,
                   w: int, h: int, radius: int, dscore: int, s_pitch: int, stream: int = 0) -> None:
        """tvl1_zncc_score: one pair."""
        self._check(self.lib.tvl1_zncc_score(
            self.ctx, C.c_void_p(dI0 or None), pitch0, C.c_void_p(dI1 or None), pitch1,
            C.c_void_p(du or None), C.c_void_p(dv or None), f_pitch, w, h, radius,
            C.c_void_p(dscore or None), s_pitch, C.c_void_p(stream) if stream else None),
            "tvl1_zncc_score")

    def warp_by_flow_u8(self, dI1: int, pitch1: int, du: int, dv: int, f_pitch: int, w: int, h: int,
                        ddst: int, d_pitch: int, dvalid: int = 0, v_pitch: int = 0,
                        stream: int = 0) -> None:
        """tvl1_warp_by_flow_u8: frame1 warped back along the flow into the u8 plane ddst (0 where
        the flow leaves the frame) and, with dvalid, the 0/1 plane of px that stay inside."""
        self._check(self.lib.tvl1_warp_by_flow_u8(
            self.ctx, C.c_void_p(dI1 or None), pitch1, C.c_void_p(du or None), C.c_void_p(dv or None),
            f_pitch, w, h, C.c_void_p(ddst or None), d_pitch, C.c_void_p(dvalid or None), v_pitch,
            C.c_void_p(stream) if stream else None), "tvl1_warp_by_flow_u8")

    def calc_scored(self, I0: np.ndarray, I1: np.ndarray, radius: int = 3, beta: float = 0.25,
                    init=None):
        """One forward solve I0 -> I1, its ZNCC score against the two frames, and the flow zeroed
        where !(score <= beta): calc_consistent's sibling with one solve.  Host u8 arrays of one
        size in; returns (u, v, score, rejected).  init = (dx, dy): the solve starts from that
        constant flow (tvl1_calc_batch_const_init)."""
        import torch
        I0 = np.array(I0, dtype=np.uint8, order="C")   # copies: torch wants writable arrays
        I1 = np.array(I1, dtype=np.uint8, order="C")
        if I1.shape != I0.shape:
            raise ValueError("I0 and I1 must have the same size")
        h, w = I0.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        d0, d1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
        fl = torch.zeros((3, h, w), dtype=torch.float32, device=dev)   # u, v, score
        torch.cuda.synchronize()
        st = self.stream
        p = [fl[k].data_ptr() for k in range(3)]
        if init is None:
            self.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, p[0], p[1], 4 * w, stream=st,
                             stats=False)
        else:
            seed = np.array([[float(init[0]), float(init[1])]], np.float32)
            self.calc_batch_device(1, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h,
                                   p[0], p[1], 4 * w, 4 * w * h, stream=st, init_const=seed)
        self.zncc_score(d0.data_ptr(), w, d1.data_ptr(), w, p[0], p[1], 4 * w, w, h, radius, p[2],
                        4 * w, stream=st)
        rejected = self.zero_above(p[0], p[1], 4 * w, p[2], 4 * w, w, h, beta, stream=st)
        torch.cuda.synchronize()
        out = fl.cpu().numpy()
        return out[0], out[1], out[2], rejected

    # ---- flow composition (tvl1_compose_flow*): c(x) = a(x) + b(x + a(x)) ----
    def compose_flow_batch(self, n: int, dua: int, dva: int, a_pitch: int, a_stride: int, dub: int,
                           dvb: int, b_pitch: int, b_stride: int, w: int, h: int, duc: int, dvc: int,
                           c_pitch: int, c_stride: int, stream: int = 0, count: bool = True):
        """tvl1_compose_flow_batch on device f32 planes (pitches and pair strides in bytes): the
        flows A -> C of n pairs from their flows a: A -> B and b: B -> C.  c may be a exactly (in
        place).  Returns the px of each pair that a takes out of the frame (uint64 array of n), or
        None with count=False (the call then stays asynchronous)."""
        out = np.zeros(max(1, n), np.uint64) if count else None
        self._check(self.lib.tvl1_compose_flow_batch(
            self.ctx, n, C.c_void_p(dua or None), C.c_void_p(dva or None), a_pitch, a_stride,
            C.c_void_p(dub or None), C.c_void_p(dvb or None), b_pitch, b_stride, w, h,
            C.c_void_p(duc or None), C.c_void_p(dvc or None), c_pitch, c_stride,
            out.ctypes.data_as(C.POINTER(C.c_uint64)) if count else None,
            C.c_void_p(stream) if stream else None), "tvl1_compose_flow_batch")
        return out[:max(0, n)] if count else None

    def compose_flow(self, dua: int, dva: int, a_pitch: int, dub: int, dvb: int, b_pitch: int, w: int,
                     h: int, duc: int, dvc: int, c_pitch: int, stream: int = 0, count: bool = True):
        """tvl1_compose_flow: one pair; returns its px outside the frame (None with count=False)."""
        out = C.c_uint64(0)
        self._check(self.lib.tvl1_compose_flow(
            self.ctx, C.c_void_p(dua or None), C.c_void_p(dva or None), a_pitch,
            C.c_void_p(dub or None), C.c_void_p(dvb or None), b_pitch, w, h,
            C.c_void_p(duc or None), C.c_void_p(dvc or None), c_pitch,
            C.byref(out) if count else None, C.c_void_p(stream) if stream else None),
            "tvl1_compose_flow")
        return int(out.value) if count else None

    def compose_chain_host(self, links):
        """The flow A -> Z of a chain of links A -> B, B -> C, ..., each a (u, v) pair of host
        float32 planes of one size, composed left to right on the device, in place on the
        accumulator.  Returns (u, v, outside_counts): the composed flow and, per composition
        (len(links) - 1 of them), the px the accumulated flow took out of the frame.  The planes
        travel through torch, as calc_consistent's do: import torch before the first Engine."""
        import torch
        links = [(np.asarray(u, np.float32), np.asarray(v, np.float32)) for u, v in links]
        if not links:
            raise ValueError("a chain needs at least one link")
        h, w = links[0][0].shape
        for u, v in links:
            if u.shape != (h, w) or v.shape != (h, w):
                raise ValueError("every link must have the same size")
        dev = torch.device("cuda", torch.cuda.current_device())
        fl = torch.from_numpy(np.stack([np.stack(l) for l in links])).to(dev)   # (links, 2, h, w)
        torch.cuda.synchronize()
        st = self.stream
        acc = fl[0]
        counts = []
        for k in range(1, len(links)):
            counts.append(self.compose_flow(acc[0].data_ptr(), acc[1].data_ptr(), 4 * w,
                                            fl[k, 0].data_ptr(), fl[k, 1].data_ptr(), 4 * w, w, h,
                                            acc[0].data_ptr(), acc[1].data_ptr(), 4 * w, stream=st))
        torch.cuda.synchronize()
        out = acc.cpu().numpy()
        return out[0], out[1], counts

    def calc_chained_host(self, I0: np.ndarray, I1: np.ndarray, links, warp_iters: bool = True,
                          inverse: bool = False, inverse_iterations: int = 8,
                          inverse_tolerance: float = 0.01):
        """compose_chain_host(links) followed by calc_host(I0, I1, init=(u, v)): the pair solved
        from the chain of the shorter flows that connect its two frames.  Returns calc_host's
        (u, v, stats, warp_iterations) and the compositions' outside counts.  With inverse=True
        the links are those of the opposite pair (they walk from I1 to I0), the seed is
        invert_flow_host of their composition, and the inversion's counts are returned last."""
        u0, v0, counts = self.compose_chain_host(links)
        if not inverse:
            return self.calc_host(I0, I1, warp_iters=warp_iters, init=(u0, v0)) + (counts,)
        u0, v0, inv = self.invert_flow_host(u0, v0, inverse_iterations, inverse_tolerance)
        return self.calc_host(I0, I1, warp_iters=warp_iters, init=(u0, v0)) + (counts, inv)

    # ---- flow inversion (tvl1_invert_flow*): g(y) = -f(y + g(y)) ----
    def invert_flow_batch(self, n: int, duf: int, dvf: int, f_pitch: int, f_stride: int,
                          iterations: int, tol: float, dug: int, dvg: int, g_pitch: int, g_stride: int,
                          dresid: int, r_pitch: int, r_stride: int, w: int, h: int, stream: int = 0,
                          counts: bool = True):
        """tvl1_invert_flow_batch on device f32 planes (pitches and pair strides in bytes): the
        flows B -> A of n pairs from their flows f: A -> B, by `iterations` fixed-point steps;
        dresid may be 0 (no residual plane).  Returns an (n, 2) uint64 array of each pair's
        (outside, unconverged) px, or None with counts=False (the call then stays asynchronous)."""
        out = (InvertCounts * max(1, n))() if counts else None
        self._check(self.lib.tvl1_invert_flow_batch(
            self.ctx, n, C.c_void_p(duf or None), C.c_void_p(dvf or None), f_pitch, f_stride,
            iterations, tol, C.c_void_p(dug or None), C.c_void_p(dvg or None), g_pitch, g_stride,
            C.c_void_p(dresid or None), r_pitch, r_stride, w, h, out,
            C.c_void_p(stream) if stream else None), "tvl1_invert_flow_batch")
        if not counts:
            return None
        return np.array([(out[b].outside, out[b].unconverged) for b in range(max(0, n))],
                        np.uint64).reshape(-1, 2)

    def invert_flow(self, duf: int, dvf: int, f_pitch: int, iterations: int, tol: float, dug: int,
                    dvg: int, g_pitch: int, dresid: int, r_pitch: int, w: int, h: int, stream: int = 0,
                    counts: bool = True):
        """tvl1_invert_flow: one pair; returns {"outside", "unconverged"} (None with
        counts=False)."""
        out = InvertCounts()
        self._check(self.lib.tvl1_invert_flow(
            self.ctx, C.c_void_p(duf or None), C.c_void_p(dvf or None), f_pitch, iterations, tol,
            C.c_void_p(dug or None), C.c_void_p(dvg or None), g_pitch, C.c_void_p(dresid or None),
            r_pitch, w, h, C.byref(out) if counts else None,
            C.c_void_p(stream) if stream else None), "tvl1_invert_flow")
        return dict(outside=int(out.outside), unconverged=int(out.unconverged)) if counts else None

    def invert_flow_host(self, u, v, iterations: int = 8, tol: float = 0.01, resid: bool = False):
        """The flow B -> A of the host float32 flow (u, v) of A -> B.  Returns (ug, vg, counts), or
        (ug, vg, resid, counts) with resid=True; counts is invert_flow's record.  The planes
        travel through torch, as compose_chain_host's do: import torch before the first Engine."""
        import torch
        u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
        if u.ndim != 2 or u.shape != v.shape:
            raise ValueError("u and v must be two planes of one size")
        h, w = u.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        f = torch.from_numpy(np.stack([u, v])).to(dev)
        g = torch.empty((3 if resid else 2, h, w), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        counts = self.invert_flow(f[0].data_ptr(), f[1].data_ptr(), 4 * w, iterations, tol,
                                  g[0].data_ptr(), g[1].data_ptr(), 4 * w,
                                  g[2].data_ptr() if resid else 0, 4 * w, w, h, stream=self.stream)
        torch.cuda.synchronize()
        out = g.cpu().numpy()
        return tuple(out) + (counts,)

    def close(self):
        if self.ctx:
            self.lib.tvl1_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def epe(u, v, u_ref, v_ref) -> np.ndarray:
    """Per-pixel end-point error."""
    return np.sqrt((u.astype(np.float64) - u_ref) ** 2 + (v.astype(np.float64) - v_ref) ** 2)


def blend6_weights() -> np.ndarray:
    """tvl1_blend6_weights (host only): the six float32 weights of tvl1_blend6_u8, in
    neighbour order i-3, i-2, i-1, i+1, i+2, i+3."""
    w = (C.c_float * 6)()
    load_engine().tvl1_blend6_weights(w)
    return np.array(list(w), np.float32)


def find_homography(src: np.ndarray, dst: np.ndarray, method: int = 8, thresh: float = 5.0):
    """tvl1_find_homography (cv::findHomography restated, host only): src, dst (n, 2) point
    arrays; returns (H 3x3, inlier mask) or raises TVL1Error."""
    lib = load_engine()
    a = np.ascontiguousarray(src, dtype=np.float32)
    b = np.ascontiguousarray(dst, dtype=np.float32)
    n = a.shape[0]
    H = (C.c_double * 9)()
    mask = np.zeros(n, np.uint8)
    rc = lib.tvl1_find_homography(a.ctypes.data, b.ctypes.data, n, method, thresh, H,
                                  mask.ctypes.data)
    if rc != 0:
        raise TVL1Error(f"tvl1_find_homography: {STATUS.get(rc, rc)}: "
                        f"{lib.tvl1_last_error(None).decode()}")
    return np.array(H[:], dtype=np.float64).reshape(3, 3), mask.astype(bool)
