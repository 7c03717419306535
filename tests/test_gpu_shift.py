"""tvl1_sad_shifts_u8, tvl1_estimate_shift and tvl1_estimate_shift_batch, exact against
tests/shift_ref.py (numpy): the estimate is integer arithmetic end to end, so every table
entry and every field of the record must be equal -- sums, counts and ties.  Small frames: sizes
that are no multiple of the 4-px word or the 256-px band, more than one band, ROI views at
every byte offset, and the shifts at the corners of the search range."""
import ctypes as C

import numpy as np
import pytest

import initflow_ref
import shift_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


class View:
    """A frame as a ROI view at byte offset `off` of a parent with `pitch` bytes per row, one
    spare row above and below, everything outside the view filled with `fill`."""

    def __init__(self, a, pitch=None, off=0, fill=0):
        h, w = a.shape
        pitch = pitch or w + off
        host = np.full((h + 2, pitch), fill, np.uint8)
        host[1:h + 1, off:off + w] = a
        self.t = dev(host)
        self.pitch = pitch
        self.ptr = self.t.data_ptr() + pitch + off


@pytest.fixture(scope="module")
def eng(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


def estimate(eng, I0, I1, R, **kw):
    a, b = View(I0, **kw), View(I1, **kw)
    torch.cuda.synchronize()
    return eng.estimate_shift(a.ptr, a.pitch, b.ptr, b.pitch, I0.shape[1], I0.shape[0], R)


# ------------------------------------------------------------------ the cost kernel
@pytest.mark.parametrize("w,h", [(64, 48), (67, 45), (33, 32), (130, 70), (3072, 100)])
def test_sad_tables(eng, w, h):
    """Radius 1 and 4, centred and off-centre (odd and even centres: the I1 words aligned and
    not), packed and as views at odd offsets; 3072 px: twelve bands along x."""
    I0, I1 = ref.window_pair(w, h, 3, -2, rng=w)
    for off, pitch in ((0, None), (3, w + 7)):
        a, b = View(I0, pitch, off, fill=255), View(I1, pitch, off, fill=255)
        torch.cuda.synchronize()
        for cx, cy, r in ((0, 0, 1), (0, 0, 4), (3, -2, 1), (-5, 6, 4), (4, 1, 2), (-2, -3, 3)):
            got = eng.sad_shifts_u8(a.ptr, a.pitch, b.ptr, b.pitch, w, h, cx, cy, r)
            want = ref.sad_table(I0, I1, cx, cy, r).reshape(2 * r + 1, 2 * r + 1)
            assert np.array_equal(got, want), (off, cx, cy, r)


def test_sad_table_empty_overlaps(eng):
    """Shifts whose overlap is empty report 0, the ones beside them their sums."""
    w, h = 33, 32
    I0, I1 = ref.window_pair(w, h, 0, 0, rng=5)
    a, b = View(I0), View(I1)
    torch.cuda.synchronize()
    for cx, cy in ((w - 2, 0), (0, -(h - 1)), (10 ** 6, 3), (-w - 20, -h - 20)):
        got = eng.sad_shifts_u8(a.ptr, a.pitch, b.ptr, b.pitch, w, h, cx, cy, 4)
        want = ref.sad_table(I0, I1, cx, cy, 4).reshape(9, 9)
        assert np.array_equal(got, want), (cx, cy)
    assert (ref.sad_table(I0, I1, w - 2, 0, 4).reshape(9, 9)[:, 6:] == 0).all()


# ------------------------------------------------------------------ the estimate
SMALL = [i for i, k in enumerate(ref.KNOWN) if k[:2] != (1024, 768)]   # 512x384 and smaller, 3072x100


@pytest.mark.parametrize("i", SMALL, ids=lambda i: "%dx%d_%+d%+d_R%d" % (*ref.KNOWN[i][:2], *ref.KNOWN[i][2],
                                                                         ref.KNOWN[i][3]))
def test_estimate_known(eng, i):
    """Every field of the record on the known-answer table (corner shifts (+-R, +-R) included:
    67x45 at R = 8, 3072x100 at R = 25)."""
    I0, I1, want = ref.known_pair(i)
    w, h, d, R = ref.KNOWN[i]
    assert (want["dx"], want["dy"]) == d
    assert estimate(eng, I0, I1, R) == want


def test_estimate_identical_constant_and_ties(eng):
    I0, _ = ref.window_pair(96, 40, 0, 0, rng=3)
    cases = [(I0, I0, 10), (np.full((40, 96), 77, np.uint8),) * 2 + (10,),
             ref.stripes(64, 48) + (8,), ref.stripes(64, 48, roll=2) + (8,)]
    want_d = [(0, 0), (0, 0), (0, 0), (-2, 0)]
    for (a, b, R), d in zip(cases, want_d):
        want = ref.estimate(a, b, R)
        assert (want["dx"], want["dy"]) == d
        got = estimate(eng, a, b, R)
        assert got == want
        assert got["sad"] == 0


@pytest.mark.parametrize("off", [1, 2, 3])
def test_estimate_roi_views(eng, off):
    """A view at a 1-, 2- or 3-byte offset and an odd pitch: no byte outside the rows enters a
    sum, whether the outside is all 0 or all 255."""
    i = next(k for k, c in enumerate(ref.KNOWN) if c[:2] == (257, 131))
    I0, I1, want = ref.known_pair(i)
    R = ref.KNOWN[i][3]
    got = [estimate(eng, I0, I1, R, pitch=257 + 14, off=off, fill=f) for f in (0, 255)]
    assert got[0] == got[1] == want
    assert estimate(eng, I0, I1, R) == want


# ------------------------------------------------------------------ the batch
def _batch(n, w, h, R, shifts):
    prs = [ref.window_pair(w, h, *shifts[b % len(shifts)], rng=100 + b % 7) for b in range(n)]
    return np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])


def test_batch_of_five(eng):
    n, w, h, R = 5, 96, 40, 10
    A, B = _batch(n, w, h, R, [(-10, 9), (0, 0), (3, -7), (10, 10), (-1, 2)])
    dA, dB = dev(A), dev(B)
    torch.cuda.synchronize()
    got = eng.estimate_shift_batch(n, dA.data_ptr(), w, w * h, dB.data_ptr(), w, w * h, w, h, R)
    for b in range(n):
        assert got[b] == ref.estimate(A[b], B[b], R), b
        assert got[b] == estimate(eng, A[b], B[b], R), b
    # one frame0 for every pair
    got = eng.estimate_shift_batch(n, dA.data_ptr(), w, 0, dB.data_ptr(), w, w * h, w, h, R)
    for b in range(n):
        assert got[b] == ref.estimate(A[0], B[b], R), b


def test_batch_of_two_chunks(eng):
    """260 pairs: a chunk of 256 and one of 4."""
    n, w, h, R = 260, 64, 48, 8
    A, B = _batch(n, w, h, R, [(1, -1), (8, -8), (-3, 5), (0, 0), (-8, 7), (2, 2), (5, 0)])
    dA, dB = dev(A), dev(B)
    torch.cuda.synchronize()
    got = eng.estimate_shift_batch(n, dA.data_ptr(), w, w * h, dB.data_ptr(), w, w * h, w, h, R)
    want = {}
    for b in range(n):
        k = b % 7   # _batch repeats with period 7
        if k not in want:
            want[k] = ref.estimate(A[b], B[b], R)
        assert got[b] == want[k], b
    for b in (0, 255, 256, 259):
        assert got[b] == estimate(eng, A[b], B[b], R), b


# ------------------------------------------------------------------ arguments
def test_bad_arguments(eng):
    lib, ctx = eng.lib, eng.ctx
    w, h = 64, 48
    t = dev(np.zeros((h, w), np.uint8))
    p = C.c_void_p(t.data_ptr())
    rec = capi.TVL1Shift()
    sad = (C.c_uint64 * 81)()

    def est(I0=p, p0=w, I1=p, p1=w, ww=w, hh=h, R=8, out=C.byref(rec)):
        return lib.tvl1_estimate_shift(ctx, I0, p0, I1, p1, ww, hh, R, out, None)

    def err():
        return lib.tvl1_last_error(ctx).decode()

    EINVAL, ESIZE = 1, 2
    assert est(I0=None) == EINVAL and "I0" in err()
    assert est(I1=None) == EINVAL and "I1" in err()
    assert est(out=None) == EINVAL and "out" in err()
    assert est(p0=w - 1) == EINVAL and "pitch0" in err()
    assert est(p1=w - 1) == EINVAL and "pitch1" in err()
    assert est(R=0) == EINVAL and "max_shift" in err()
    assert est(R=129) == EINVAL and "max_shift" in err()
    assert est(R=13) == EINVAL and "max_shift" in err()       # 4 * 13 > 48
    assert est(R=12) == 0
    assert est(ww=8193, hh=8192, p0=8193, p1=8193, R=8) == ESIZE and "w*h" in err()
    assert lib.tvl1_estimate_shift_batch(ctx, 0, p, w, 0, p, w, 0, w, h, 8, C.byref(rec), None) == EINVAL
    assert "n must" in err()
    for r in (0, 5):
        assert lib.tvl1_sad_shifts_u8(ctx, p, w, p, w, w, h, 0, 0, r, sad, None) == EINVAL
        assert "radius" in err()
    assert lib.tvl1_sad_shifts_u8(ctx, p, w, p, w, w, h, 0, 0, 1, None, None) == EINVAL
    assert lib.tvl1_sad_shifts_u8(ctx, p, w - 1, p, w, w, h, 0, 0, 1, sad, None) == EINVAL and "pitch0" in err()
    assert lib.tvl1_sad_shifts_u8(ctx, p, 8193, p, 8193, 8193, 8192, 0, 0, 1, sad, None) == ESIZE
    assert lib.tvl1_estimate_shift(None, p, w, p, w, w, h, 8, C.byref(rec), None) == EINVAL


def test_profile_1_ctx(built):
    """No float in the estimate: a ctx of the CPU DualTVL1 profile gives the same record."""
    e = capi.Engine(capi.make_params(profile=1))
    try:
        i = next(k for k, c in enumerate(ref.KNOWN) if c[:2] == (130, 70))
        I0, I1, want = ref.known_pair(i)
        assert e.estimate_shift_host(I0, I1, ref.KNOWN[i][3]) == want
    finally:
        e.close()


def test_cli_pair(eng):
    """tests/initflow_ref.py's CLI pair (np.roll by (12, -9)): the whole frame at R = 32 and its
    top and bottom 48-row strips at R = 12, sad 0."""
    c = initflow_ref.CLI
    I0, I1 = initflow_ref.frames_of(c)
    for a, b, R in ((I0, I1, 32), (I0[:48], I1[:48], 12), (I0[-48:], I1[-48:], 12)):
        want = ref.estimate(a, b, R)
        assert (want["dx"], want["dy"], want["sad"]) == (12, -9, 0)
        assert eng.estimate_shift_host(a, b, R) == want
