"""The reference of the average-flow alignment (tests/avgflow_ref.py) pinned on the CPU: the
blend's weights against the library's, the blend's rounding, known answers of the remap, and
the condition on the GPU tests' end-to-end inputs (every solve clear of its stopping
thresholds, as tests/test_residual_margin_cpu.py asks of the golden fixtures)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
from PIL import Image

import avgflow_ref as ref
from optflow_amd import capi
from oracle import checker
from test_residual_margin_cpu import MIN_MARGIN

OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


# ------------------------------------------------------------------ weights and the ABI
def test_weights_match_the_library_bit_for_bit(built):
    lib = capi.load_engine()
    w = (C.c_float * 6)()
    lib.tvl1_blend6_weights(w)
    got = np.array(list(w), np.float32)
    want = ref.weights()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(capi.blend6_weights().view(np.uint32), want.view(np.uint32))
    assert [float(x).hex() for x in want[:3]] == ["0x1.58cc700000000p-5", "0x1.2cddc80000000p-3",
                                                  "0x1.3e778e0000000p-2"]
    assert np.array_equal(want, want[::-1])


def test_weights_sum_to_one_in_double():
    w = ref.weights().astype(np.float64)
    assert w.sum() == 1.0 and sum(w[::-1]) == 1.0
    assert np.array_equal(w * 2.0 ** 28, np.rint(w * 2.0 ** 28))   # multiples of 2^-28


def test_abi_is_still_9_and_the_new_symbols_resolve(built):
    lib = capi.load_engine()
    assert lib.tvl1_abi_version() == 9 == capi.ABI_VERSION
    for name in ("tvl1_blend6_weights", "tvl1_blend6_u8", "tvl1_half_u8", "tvl1_remap_flow_u8"):
        assert getattr(lib, name)
    for name in ("blend6_u8", "half_u8", "remap_flow_u8", "align_slice_host"):
        assert callable(getattr(capi.Engine, name))


# ------------------------------------------------------------------ blend
def test_six_equal_frames_give_that_frame():
    f = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(ref.blend6([f] * 6), f)


def test_summation_order_changes_nothing():
    rng = np.random.default_rng(1)
    fr = list(rng.integers(0, 256, (6, 64, 257), dtype=np.uint8))
    a = ref.blend6(fr)
    assert np.array_equal(a, ref.blend6(fr, order=range(5, -1, -1)))
    assert np.array_equal(a, ref.blend6(fr, order=(2, 5, 0, 3, 1, 4)))


def test_exact_ties_round_to_even():
    fr, floors = ref.tie_frames()
    assert len(floors) >= 8 and (floors % 2 == 0).any() and (floors % 2 == 1).any()
    w = ref.weights().astype(np.float64)
    acc = sum(w[k] * fr[k].astype(np.float64) for k in range(6))
    assert np.array_equal(acc, floors + 0.5)                       # exact ties
    out = ref.blend6(list(fr))
    assert np.array_equal(out, floors + (floors & 1)) and (out % 2 == 0).all()


def test_extremes_survive():
    z, f = np.zeros((3, 5), np.uint8), np.full((3, 5), 255, np.uint8)
    assert (ref.blend6([z] * 6) == 0).all() and (ref.blend6([f] * 6) == 255).all()


def test_half_is_the_rounded_2x2_mean():
    a = np.array([[255, 255, 0, 1], [255, 254, 1, 0]], np.uint8)
    assert ref.half(a).tolist() == [[255, 1]]          # (1019 + 2) >> 2, (2 + 2) >> 2


def test_half_against_the_cli_prescale(tmp_path, built):
    """The CLI's host resize_u8 at exactly 1/2 (through its --decode hook) restates OpenCV's 8u
    kernel: (s + 2) >> 2 in blocks of 8 output columns, and cvRound(s / 4) -- half to even -- in
    the scalar tail of the last (w / 2) % 8 columns.  `half` is (s + 2) >> 2 everywhere: the
    same bytes when w is a multiple of 16, and in the tail different only at the ties."""
    for w in (80, 66):
        a = np.random.default_rng(w).integers(0, 256, (40, w), dtype=np.uint8)
        a[:, -2:] = np.array([[1, 0], [1, 0]], np.uint8).repeat(20, 0)   # s = 2 or 0 in the last column
        Image.fromarray(a).save(tmp_path / "a.png")
        subprocess.run([str(OPTFLOW), "--decode", str(tmp_path / "a.png"), str(tmp_path / "a.tiff"), "0.5"],
                       check=True, timeout=60)
        cli, h = np.array(Image.open(tmp_path / "a.tiff")), ref.half(a)
        vec = (w // 2) // 8 * 8
        assert np.array_equal(cli[:, :vec], h[:, :vec])
        if w % 16 == 0:
            assert np.array_equal(cli, h)
        else:
            s = a.astype(np.int32)
            s = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
            assert np.array_equal(cli[:, vec:], np.rint(s[:, vec:] / 4.0).astype(np.uint8))
            assert (cli[:, -1] == 0).all() and (h[:, -1] == 1).all()     # s = 2: 0.5 -> 0 / 1


# ------------------------------------------------------------------ remap: known answers
def frame():
    rng = np.random.default_rng(4)
    return rng.integers(1, 256, (21, 67), dtype=np.uint8)


def const(shape, val):
    return np.full(shape, val, np.float32)


def test_zero_flow_returns_the_frame_and_an_empty_band():
    f = frame()
    z = const(f.shape, 0)
    assert np.array_equal(ref.remap(f, z, z), f)
    out = ref.remap(f, z, z, border=5)
    assert out.shape == (31, 77) and np.array_equal(out[5:-5, 5:-5], f)
    out[5:-5, 5:-5] = 0
    assert not out.any()
    zs = const((10, 34), 0)                               # a coarser flow, brought to the frame's size
    assert np.array_equal(ref.remap(f, zs, zs, gain=2.0), f)


def test_integer_shift_fills_with_zero():
    f = frame()
    out = ref.remap(f, const(f.shape, 3), const(f.shape, -2))    # out(x, y) = f(x - 3, y + 2)
    want = np.zeros_like(f)
    want[:-2, 3:] = f[2:, :-3]
    assert np.array_equal(out, want)


def test_shifted_edge_lands_in_the_band():
    """The band takes the nearest frame px's flow, so content shifted out of the frame is kept."""
    f = frame()
    out = ref.remap(f, const(f.shape, 3), const(f.shape, -2), border=5)
    H, W = f.shape
    want = np.zeros((H + 10, W + 10), np.uint8)
    want[5 - 2:5 - 2 + H, 5 + 3:5 + 3 + W] = f
    assert np.array_equal(out, want)
    assert out[3:5].any() and out[:, 5 + W:].any()            # rows above and columns right of the frame


def test_half_pixel_flow_is_the_rounded_mean():
    f = frame()
    out = ref.remap(f, const(f.shape, 0.5), const(f.shape, 0))   # samples x - 0.5: taps x-1 and x
    a, b = f[:, :-1].astype(np.int32), f[:, 1:].astype(np.int32)
    assert np.array_equal(out[:, 1:], ((a + b + 1) >> 1).astype(np.uint8))
    assert np.array_equal(out[:, 0], ((f[:, 0].astype(np.int32) + 1) >> 1).astype(np.uint8))


def test_negative_map_coordinates():
    """x - U < 0: >> 5 floors and & 31 wraps on negative ints (a sample at -0.25 px is 3/4 of
    column 0 and 1/4 of nothing; at -1.25 px nothing)."""
    f = frame()
    assert ref.round_map(np.float32(-8.0)) >> 5 == -1 and ref.round_map(np.float32(-8.0)) & 31 == 24
    out = ref.remap(f, const(f.shape, 0.25), const(f.shape, 0))
    assert np.array_equal(out[:, 0], ((f[:, 0].astype(np.int32) * 24 * 32 + 512) >> 10).astype(np.uint8))
    out = ref.remap(f, const(f.shape, 1.25), const(f.shape, 0))
    assert not out[:, 0].any()
    out = ref.remap(f, const(f.shape, 0), const(f.shape, 0.25), border=2)
    assert np.array_equal(out[2, 2:-2], ((f[0].astype(np.int32) * 32 * 24 + 512) >> 10).astype(np.uint8))


def test_nan_and_infinite_flow_give_zero():
    f = frame()
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        u = const(f.shape, 0)
        u[4, 7] = bad
        out = ref.remap(f, u, const(f.shape, 0))
        assert out[4, 7] == 0
        out[4, 7] = f[4, 7]
        assert np.array_equal(out, f)
        assert ref.remap(f, const(f.shape, 0), u)[4, 7] == 0
    assert ref.round_map(np.float32(np.nan)) == ref.INT_MIN == ref.round_map(np.float32(2.0 ** 31))
    assert ref.round_map(np.float32(2.5)) == 2 and ref.round_map(np.float32(-3.5)) == -4


def test_flow_up_is_the_engines_resize():
    """k_resize_hp's bilinear branch: constant planes stay constant, a ramp is interpolated at
    half-pixel centres and clamped at the edges, the last column is a single tap."""
    assert np.array_equal(ref.flow_up(const((10, 34), 1.5), 67, 21, 2.0), const((21, 67), 3.0))
    ramp = np.tile(np.arange(4, dtype=np.float32), (2, 1))
    up = ref.flow_up(ramp, 8, 4, 1.0)
    assert up.shape == (4, 8)
    assert up[0].tolist() == [0.0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.0]


# ------------------------------------------------------------------ the GPU cases' inputs
def prescaled_by_cli(tmp_path, F, B):
    out = []
    for k, a in enumerate((F, B)):
        Image.fromarray(a).save(tmp_path / f"{k}.png")
        subprocess.run([str(OPTFLOW), "--decode", str(tmp_path / f"{k}.png"),
                        str(tmp_path / f"{k}.tiff"), "0.5"], check=True, timeout=60)
        out.append(np.array(Image.open(tmp_path / f"{k}.tiff")))
    return tuple(out)


@pytest.mark.parametrize("name", list(ref.STACKS))
def test_end_to_end_inputs_clear_the_residual_margin(built, tmp_path, name):
    c, st = ref.STACKS[name], ref.stack_of(name)
    p = capi.make_params(**ref.TV)
    for i in ref.outputs_of(name):
        F = st[i]
        B = ref.blend6([st[i + d] for d in (-3, -2, -1, 1, 2, 3)])
        path = ref.prescale_path(c["w"], c["h"], c["scale"])
        I0, I1 = {"none": lambda: (F, B), "device": lambda: (ref.half(F), ref.half(B)),
                  "host": lambda: prescaled_by_cli(tmp_path, F, B)}[path]()
        u, v, s, wi, tr = checker.oracle_check_trace(I0, I1, p)
        assert len(tr) > 0
        m = checker.check_margins(tr, p.iterations)
        assert m.min() >= MIN_MARGIN, (name, i, tr[np.argmin(m)])
        assert np.abs(u).max() > 0.05 or np.abs(v).max() > 0.05      # the remap has something to do
