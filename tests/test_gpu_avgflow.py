"""The three device stages of the average-flow alignment (tvl1_blend6_u8, tvl1_half_u8,
tvl1_remap_flow_u8) and Engine.align_slice_host, bitwise against tests/avgflow_ref.py (numpy).
Small planes inside wider, misaligned parents: every lane width, the byte-wise fall-backs, more
than one block, and the padding that must stay untouched."""
import numpy as np
import pytest

import avgflow_ref as ref
from optflow_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAD = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


class Plane:
    """A w x h u8 (or f32) view at column offset `off` of a parent with `pitch` elements per
    row, the parent filled with `fill` first."""

    def __init__(self, a=None, shape=None, pitch=None, off=0, dtype=np.uint8, fill=PAD):
        h, w = a.shape if a is not None else shape
        pitch = pitch or w + off
        host = np.full((h, pitch), fill, dtype)
        if a is not None:
            host[:, off:off + w] = a
        self.h, self.w, self.off, self.host0 = h, w, off, host
        self.t = dev(host)
        self.item = host.itemsize
        self.pitch = pitch * self.item
        self.ptr = self.t.data_ptr() + off * self.item

    def get(self):
        """(the view, True if the parent outside the view is unchanged)"""
        torch.cuda.synchronize()
        now = self.t.cpu().numpy()
        m = np.ones(now.shape, bool)
        m[:, self.off:self.off + self.w] = False
        same = np.array_equal(now[m].view(np.uint8), self.host0[m].view(np.uint8))
        return now[:, self.off:self.off + self.w].copy(), same


@pytest.fixture(scope="module")
def eng(built):
    e = capi.Engine(capi.make_params(**ref.TV))
    yield e
    e.close()


# ------------------------------------------------------------------ blend
@pytest.mark.parametrize("w,h", [(67, 9), (517, 5)])
def test_blend6(eng, w, h):
    """67 px: nine 8-px lanes, the last one partial; 517 px: past one block's 64 lanes.  Six
    pitches and six column offsets (aligned and not); ties, 0 and 255 in the first rows."""
    rng = np.random.default_rng(w)
    fr = rng.integers(0, 256, (6, h, w), dtype=np.uint8)
    ties, floors = ref.tie_frames()
    fr[:, 0, :ties.shape[1]] = ties
    fr[:, 1, :] = 0
    fr[:, 2, :] = 255
    planes = [Plane(fr[k], pitch=w + 8 + 5 * k, off=(0, 1, 8, 3, 16, 7)[k]) for k in range(6)]
    for off in (0, 3):
        dst = Plane(shape=(h, w), pitch=w + 24, off=off)
        eng.blend6_u8([p.ptr for p in planes], [p.pitch for p in planes], w, h, dst.ptr, dst.pitch)
        got, clean = dst.get()
        want = ref.blend6(list(fr))
        assert np.array_equal(want[0, :len(floors)], floors + (floors & 1))   # ties went to even
        assert (want[1] == 0).all() and (want[2] == 255).all()
        assert np.array_equal(got, want)
        assert clean


# ------------------------------------------------------------------ half
@pytest.mark.parametrize("w,h", [(66, 10), (130, 6), (1040, 4)])
def test_half(eng, w, h):
    rng = np.random.default_rng(w + h)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a[0, :8] = (255, 255, 0, 0, 255, 254, 1, 0)
    a[1, :8] = (255, 255, 0, 0, 254, 254, 0, 0)
    for soff, doff in ((0, 0), (16, 8), (5, 3)):
        src = Plane(a, pitch=w + 32 + (soff & 1), off=soff)
        dst = Plane(shape=(h // 2, w // 2), pitch=w // 2 + 16, off=doff)
        eng.half_u8(src.ptr, src.pitch, w, h, dst.ptr, dst.pitch)
        got, clean = dst.get()
        assert np.array_equal(got, ref.half(a))
        assert clean


def test_half_odd_sizes_are_einval(eng):
    src = Plane(shape=(10, 66))
    dst = Plane(shape=(5, 33))
    for w, h in ((65, 10), (66, 9)):
        with pytest.raises(capi.TVL1Error, match="TVL1_EINVAL"):
            eng.half_u8(src.ptr, src.pitch, w, h, dst.ptr, dst.pitch)
    got, clean = dst.get()
    assert (got == PAD).all() and clean


# ------------------------------------------------------------------ remap
W, H = 67, 21


def frame_of():
    rng = np.random.default_rng(67)
    f = rng.integers(1, 256, (H, W), dtype=np.uint8)
    f[0, :] = 255
    f[:, 0] = 200
    return f


def flows_of(kind, fw, fh, gain):
    """Flow planes (u, v) in solve units: `gain` times them is the displacement in frame px."""
    rng = np.random.default_rng(fw * 31 + fh)
    if kind == "rand":
        # inside (|d| small), astride each edge (|d| up to the frame's size) and wholly outside
        amp = rng.choice([1.5, 12.0, 40.0, 150.0], size=(2, fh, fw))
        f = (rng.uniform(-1, 1, (2, fh, fw)) * amp / gain).astype(np.float32)
        f[0, 3, 5] = np.nan
        f[1, 7, 11] = np.inf
        f[0, fh - 1, fw - 1] = -np.inf
        return f[0], f[1]
    k = {"c64a": (33, -95), "c64b": (-1, 1), "c64c": (64 * 3 + 1, 64 * 2 - 1), "zero": (0, 0)}[kind]
    # exact multiples of 1/64 px in frame units: the map times 32 lands on .5 (rint's ties)
    return (np.full((fh, fw), k[0] / 64.0 / gain, np.float32),
            np.full((fh, fw), k[1] / 64.0 / gain, np.float32))


@pytest.mark.parametrize("border", [0, 5])
@pytest.mark.parametrize("kind", ["rand", "c64a", "c64b", "c64c", "zero"])
@pytest.mark.parametrize("fw,fh,gain", [(67, 21, 1.0), (34, 10, 2.0)])
def test_remap(eng, fw, fh, gain, kind, border):
    f = frame_of()
    u, v = flows_of(kind, fw, fh, gain)
    want = ref.remap(f, u, v, gain, border)
    if kind == "zero":
        inner = want[border:border + H, border:border + W]
        assert np.array_equal(inner, f) and want.sum() == inner.sum()   # the band is 0
    fr = Plane(f, pitch=W + 13, off=3)
    pu = Plane(u, pitch=fw + 5, off=2, dtype=np.float32, fill=np.nan)
    pv = Plane(v, pitch=fw + 5, off=1, dtype=np.float32, fill=np.nan)
    for doff in (0, 2):
        dst = Plane(shape=(H + 2 * border, W + 2 * border), pitch=W + 2 * border + 11, off=doff)
        eng.remap_flow_u8(fr.ptr, fr.pitch, W, H, pu.ptr, pv.ptr, pu.pitch, fw, fh, gain, border,
                          dst.ptr, dst.pitch)
        got, clean = dst.get()
        assert np.array_equal(got, want)
        assert clean


# ------------------------------------------------------------------ errors and isolation
def test_bad_arguments_launch_nothing(eng):
    f = Plane(frame_of())
    u = Plane(np.zeros((H, W), np.float32), dtype=np.float32)
    dst = Plane(shape=(H + 10, W + 10))
    ok = dict(frame=f.ptr, pitch=f.pitch, w=W, h=H, du=u.ptr, dv=u.ptr, flow_pitch=u.pitch, fw=W,
              fh=H, gain=1.0, border=5, dst=dst.ptr, dst_pitch=dst.pitch)
    bad = [("TVL1_EINVAL", dict(frame=0)), ("TVL1_EINVAL", dict(du=0)), ("TVL1_EINVAL", dict(dv=0)),
           ("TVL1_EINVAL", dict(dst=0)), ("TVL1_EINVAL", dict(pitch=W - 1)),
           ("TVL1_EINVAL", dict(dst_pitch=W + 9)), ("TVL1_EINVAL", dict(flow_pitch=4 * W + 2)),
           ("TVL1_EINVAL", dict(flow_pitch=4 * W - 4)), ("TVL1_EINVAL", dict(border=-1)),
           ("TVL1_EINVAL", dict(fw=0)), ("TVL1_EINVAL", dict(fh=0)),
           ("TVL1_EINVAL", dict(dst=f.ptr + 8, border=0, dst_pitch=f.pitch)),
           ("TVL1_ESIZE", dict(border=16351)), ("TVL1_ESIZE", dict(w=32768, pitch=32768, border=0))]
    for status, kw in bad:
        with pytest.raises(capi.TVL1Error, match=status):
            eng.remap_flow_u8(**{**ok, **kw})
    six = [f.ptr] * 6
    for status, fr, pt, dp, d in [("TVL1_EINVAL", [f.ptr] * 5 + [0], [f.pitch] * 6, dst.pitch, dst.ptr),
                                  ("TVL1_EINVAL", six, [f.pitch] * 5 + [W - 1], dst.pitch, dst.ptr),
                                  ("TVL1_EINVAL", six, [f.pitch] * 6, W - 1, dst.ptr),
                                  ("TVL1_EINVAL", six, [f.pitch] * 6, dst.pitch, 0)]:
        with pytest.raises(capi.TVL1Error, match=status):
            eng.blend6_u8(fr, pt, W, H, d, dp)
    for kw in (dict(src=0), dict(dst=0), dict(pitch=65), dict(dst_pitch=32)):
        a = dict(src=f.ptr, pitch=f.pitch, w=66, h=20, dst=dst.ptr, dst_pitch=dst.pitch)
        with pytest.raises(capi.TVL1Error, match="TVL1_EINVAL"):
            eng.half_u8(**{**a, **kw})
    got, clean = dst.get()
    assert (got == PAD).all() and clean
    assert np.array_equal(f.get()[0], frame_of())


def test_solver_scratch_is_not_touched(eng):
    """A tvl1_calc before and after the three calls returns identical bits."""
    I0, I1 = synth.gen_pair(96, 64, seed=5)
    a = eng.calc_host(I0, I1)
    f = Plane(frame_of())
    u = Plane(np.full((H, W), 0.75, np.float32), dtype=np.float32)
    dst = Plane(shape=(H + 4, W + 4))
    eng.blend6_u8([f.ptr] * 6, [f.pitch] * 6, W, H, dst.ptr, dst.pitch)
    eng.half_u8(f.ptr, f.pitch, 66, 20, dst.ptr, dst.pitch)
    eng.remap_flow_u8(f.ptr, f.pitch, W, H, u.ptr, u.ptr, u.pitch, W, H, 1.0, 2, dst.ptr, dst.pitch)
    torch.cuda.synchronize()
    b = eng.calc_host(I0, I1)
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    np.testing.assert_array_equal(a[3], b[3])


def test_calls_count_into_profiling_class_2(built):
    """With profiling on, the three calls are added to class 2 of the ctx's next solve."""
    I0, I1 = synth.gen_pair(96, 64, seed=5)
    d0, d1 = dev(I0), dev(I1)
    du = torch.zeros((64, 96), dtype=torch.float32, device=d0.device)
    dv = torch.zeros_like(du)
    e = capi.Engine(capi.make_params(**ref.TV))
    e.set_profiling(True)

    def solve():
        torch.cuda.synchronize()
        return e.calc_device(d0.data_ptr(), 96, d1.data_ptr(), 96, 96, 64, du.data_ptr(), dv.data_ptr(), 4 * 96)

    a = solve()
    f = Plane(frame_of())
    u = Plane(np.zeros((H, W), np.float32), dtype=np.float32)
    dst = Plane(shape=(H, W))
    e.blend6_u8([f.ptr] * 6, [f.pitch] * 6, W, H, dst.ptr, dst.pitch)
    e.half_u8(f.ptr, f.pitch, 66, 20, dst.ptr, dst.pitch)
    e.remap_flow_u8(f.ptr, f.pitch, W, H, u.ptr, u.ptr, u.pitch, W, H, 1.0, 0, dst.ptr, dst.pitch)
    b = solve()
    c = solve()
    e.half_u8(f.ptr, f.pitch, 66, 20, dst.ptr, dst.pitch)
    e.set_profiling(False)                                         # discards the waiting mark
    e.set_profiling(True)
    d = solve()
    e.close()
    assert b["kernel_launches"][2] == a["kernel_launches"][2] + 3
    assert c["kernel_launches"][2] == a["kernel_launches"][2]      # counted once, not kept
    assert d["kernel_launches"][2] == a["kernel_launches"][2]      # none survives the switch
    assert b["kernel_hbm_bytes"][2] > a["kernel_hbm_bytes"][2] == c["kernel_hbm_bytes"][2]


# ------------------------------------------------------------------ the composed call
def test_align_slice_host(eng):
    name = "half_96x64"
    c, st = ref.STACKS[name], ref.stack_of(name)
    aligned, u, v = eng.align_slice_host([st[k] for k in range(7)], c["scale"], c["border"])
    ra, ru, rv, *_ = ref.reference(name, 3)
    assert np.array_equal(u.view(np.uint32), ru.view(np.uint32))
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert aligned.shape == (c["h"] + 2 * c["border"], c["w"] + 2 * c["border"])
    assert np.array_equal(aligned, ra)
    with pytest.raises(ValueError, match="not done on the device"):
        eng.align_slice_host([s[:63, :95] for s in st[:7]], 0.5, 0)
