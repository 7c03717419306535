"""tests/align_edges.py on the GPU, bitwise: the pre-alignment kernels (csrc/tvl1_align.hpp) at
their tile, level, segment and budget edges.

  detect     keypoint x, y, octave, response bits and descriptors against the oracle (angles
             only lie in [0, 360)); a pitched view against its contiguous copy; short and
             null outputs
  select     the periodic frame's tie groups cut by the budget
  budget     the quota sum above nfeatures, through tvl1_orb_detect and tvl1_find_alignment
  match      against the numpy brute force (tests/align_ref.py), planted duplicates in order
  alignment  affine bits, n_good and outcome against the oracle, contiguous and pitched
  warps      against the numpy restatements, the padding's sentinels intact

One engine serves the whole module, and one test walks a single fresh engine through frames
that shrink and grow again.  tests/test_align_edges_cpu.py keeps the table from going
vacuous.  Nothing here has a tolerance: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_edges as ae
import align_ref as ar
from optflow_amd import capi
from oracle import checker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KP_COLS = [0, 1, 2, 4]   # x, y, octave, response (3: the angle, not restated)


@pytest.fixture(scope="module")
def eng(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def detect_ref(name):
    case = next(d for d in ae.DETECT + ae.DETECT_EMPTY if d.name == name)
    return checker.oracle_orb_detect(case.frame(), **case.kw)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def gpu_detect(eng, frame, **kw):
    d = dev(frame)
    return eng.orb_detect(d.data_ptr(), frame.shape[1], frame.shape[1], frame.shape[0], **kw)


def same_detect(got, want):
    kp, desc = got
    kr, dr = want
    assert len(kp) == len(kr) and len(desc) == len(dr)
    assert np.array_equal(kp[:, KP_COLS].view(np.uint32), kr[:, KP_COLS].view(np.uint32))
    assert np.array_equal(desc, dr)
    assert np.all((kp[:, 3] >= 0) & (kp[:, 3] < 360))


# ---------------------------------------------------------------- detect
@pytest.mark.parametrize("case", ae.DETECT, ids=[d.name for d in ae.DETECT])
def test_detect_bitwise(eng, case):
    want = detect_ref(case.name)
    assert len(want[0]) > 0
    same_detect(gpu_detect(eng, case.frame(), **case.kw), want)


@pytest.mark.parametrize("case", ae.DETECT_EMPTY, ids=[d.name for d in ae.DETECT_EMPTY])
def test_detect_no_candidate_px(eng, case):
    kp, desc = gpu_detect(eng, case.frame(), **case.kw)   # TVL1_OK (orb_detect raises otherwise)
    assert len(kp) == 0 and len(desc) == 0


@pytest.mark.parametrize("nlevels", [1, 8])
def test_detect_pitched_view_equals_contiguous_copy(eng, nlevels):
    r = ae.ROI
    parent, view = ae.in_parent(ae.noise(r["W"], r["H"], r["seed"]), r["ox"], r["oy"], r["PW"], r["PH"])
    kw = dict(edge_threshold=ae.ET, nlevels=nlevels)
    dp = dev(parent)
    got = eng.orb_detect(dp.data_ptr() + r["oy"] * r["PW"] + r["ox"], r["PW"], r["W"], r["H"], **kw)
    same_detect(got, gpu_detect(eng, view.copy(), **kw))
    same_detect(got, detect_ref(f"129x97-L{nlevels}"))


def _raw_detect(eng, frame, cap, null=False, **kw):
    """tvl1_orb_detect into sentinel-filled host rows: (n, kp, desc)"""
    ap = capi.align_params(eng.lib, **kw)
    rows = max(cap, 1) + ae.CAP_SHORT
    kp = np.full((rows, 5), -7.0, np.float32)
    desc = np.full((rows, 32), 0xEE, np.uint8)
    n = C.c_int32(-1)
    d = dev(frame)
    rc = eng.lib.tvl1_orb_detect(eng.ctx, C.c_void_p(d.data_ptr()), frame.shape[1], frame.shape[1], frame.shape[0],
                                 C.byref(ap), None if null else kp.ctypes.data,
                                 None if null else desc.ctypes.data, cap, C.byref(n), None)
    assert rc == 0, eng.lib.tvl1_last_error(eng.ctx)
    return n.value, kp, desc


def test_detect_short_and_null_outputs(eng):
    case = next(d for d in ae.DETECT if d.name == "129x97-L8")
    kr, dr = detect_ref(case.name)
    full = len(kr)
    cap = full - ae.CAP_SHORT
    n, kp, desc = _raw_detect(eng, case.frame(), cap, **case.kw)
    assert n == full
    same_detect((kp[:cap], desc[:cap]), (kr[:cap], dr[:cap]))
    assert np.all(kp[cap:] == -7.0) and np.all(desc[cap:] == 0xEE)   # rows past cap untouched
    n, kp, desc = _raw_detect(eng, case.frame(), 0, null=True, **case.kw)
    assert n == full and np.all(kp == -7.0) and np.all(desc == 0xEE)


def test_ctx_reuse_shrinking_and_growing(built):
    """One fresh engine over frames that shrink, then grow: stale score / key / count scratch
    of a larger level or an earlier frame would show."""
    e = capi.Engine(capi.make_params())
    try:
        for name in ae.REUSE_ORDER:
            case = next(d for d in ae.DETECT if d.name == name)
            same_detect(gpu_detect(e, case.frame(), **case.kw), detect_ref(name))
    finally:
        e.close()


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("nfeatures", ae.SELECT_NFEATURES)
def test_select_cuts_tie_groups(eng, nfeatures):
    f = ae.periodic()
    want = checker.oracle_orb_detect(f, nfeatures=nfeatures, cap=100000, **ae.SELECT_KW)
    assert len(want[0]) == min(nfeatures, ae.PERIODIC_COUNT)
    same_detect(gpu_detect(eng, f, nfeatures=nfeatures, **ae.SELECT_KW), want)
    ref, _ = ar.level0_keypoints(f, nfeatures, ae.ET)      # and the numpy restatement
    assert np.array_equal(want[0][:, [0, 1, 4]].view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------- budget
@pytest.mark.parametrize("case", ae.BUDGET, ids=[b.name for b in ae.BUDGET])
def test_budget_quota_sum_above_nfeatures(eng, case):
    for frame in case.frames:
        f = frame()
        want = checker.oracle_orb_detect(f, **case.kw)
        assert len(want[0]) == case.count == case.kw["nfeatures"] + 1
        same_detect(gpu_detect(eng, f, **case.kw), want)


# ---------------------------------------------------------------- match
@pytest.mark.parametrize("nt", ae.MATCH_NT)
def test_match_random(eng, nt):
    t = ae.descriptors(nt, 200 + nt)
    for nq in ae.MATCH_NQ:
        q = ae.descriptors(nq, 100 + nq)
        idx, dist = eng.match_knn2(q, t)
        ri, rd = ar.match_knn2(q, t)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd), (nq, nt)


def test_match_planted_duplicates_identical_and_complement(eng):
    q, t, dups = ae.match_dup_case()
    idx, dist = eng.match_knn2(q, t)
    assert np.array_equal(idx, np.array(dups)) and np.all(dist == 0)   # the lower index first
    # the same rows as queries 0..2 of a 65-query list, among random ones
    q65 = np.concatenate([q, ae.descriptors(62, 77)])
    idx, dist = eng.match_knn2(q65, t)
    ri, rd = ar.match_knn2(q65, t)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    same = np.repeat(ae.descriptors(1, 5), 300, axis=0)                # all distances 0
    idx, dist = eng.match_knn2(same[:65], same)
    assert np.all(idx == [0, 1]) and np.all(dist == 0)
    idx, dist = eng.match_knn2(~same[:1], same[:1])                    # distance 256, no second
    assert idx.tolist() == [[0, -1]] and dist.tolist() == [[256, ar.NO_DIST]]
    # 4097 train rows: the nearest is row 4096, alone in the last used segment's fifth tile
    # (three empty segments after it), and the farthest its complement in the first segment
    t = ae.descriptors(4097, 9)
    t[0] = ~t[4096]
    q = t[4096:].copy()
    q[0, 7] ^= 0x10
    idx, dist = eng.match_knn2(q, t)
    ri, rd = ar.match_knn2(q, t)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    assert idx[0, 0] == 4096 and dist[0, 0] == 1 and idx[0, 1] != 0


def test_match_no_query_touches_nothing(eng):
    t = ae.descriptors(5, 1)
    idx = np.full((2, 2), -99, np.int32)
    dist = np.full((2, 2), -99, np.int32)
    rc = eng.lib.tvl1_match_knn2(eng.ctx, None, 0, t.ctypes.data, 5, idx.ctypes.data, dist.ctypes.data, None)
    assert rc == 0 and np.all(idx == -99) and np.all(dist == -99)
    rc = eng.lib.tvl1_match_knn2(eng.ctx, None, 0, None, 0, None, None, None)
    assert rc == 0


# ---------------------------------------------------------------- alignment
@functools.lru_cache(maxsize=None)
def align_ref(name):
    case = next(a for a in ae.ALIGN if a.name == name)
    f1, f0 = case.frames()
    return checker.oracle_find_alignment(f1, f0, **case.kw)


def same_alignment(got, want):
    A, ng, oc = got
    Ar, ngr, ocr = want
    assert (ng, oc) == (ngr, ocr)
    assert np.array_equal(A.view(np.uint32), Ar.view(np.uint32)), (A, Ar)


@pytest.mark.parametrize("case", ae.ALIGN, ids=[a.name for a in ae.ALIGN])
def test_alignment_bitwise(eng, case):
    f1, f0 = case.frames()
    want = align_ref(case.name)
    assert (want[2], want[1]) == (case.outcome, case.n_good)
    d1, d0 = dev(f1), dev(f0)
    got = eng.find_alignment(d1.data_ptr(), f1.shape[1], f1.shape[1], f1.shape[0], d0.data_ptr(), f0.shape[1],
                             f0.shape[1], f0.shape[0], **case.kw)
    same_alignment(got, want)


@pytest.mark.parametrize("name", ae.ALIGN_PITCHED)
def test_alignment_pitched_views(eng, name):
    case = next(a for a in ae.ALIGN if a.name == name)
    f1, f0 = case.frames()
    (x1, y1, pw1, ph1), (x0, y0, pw0, ph0) = ae.ALIGN_PARENTS
    p1, _ = ae.in_parent(f1, x1, y1, pw1, ph1, fill=1)
    p0, _ = ae.in_parent(f0, x0, y0, pw0, ph0, fill=2)
    d1, d0 = dev(p1), dev(p0)
    got = eng.find_alignment(d1.data_ptr() + y1 * pw1 + x1, pw1, f1.shape[1], f1.shape[0],
                             d0.data_ptr() + y0 * pw0 + x0, pw0, f0.shape[1], f0.shape[0], **case.kw)
    same_alignment(got, align_ref(name))


# ---------------------------------------------------------------- warps
@pytest.mark.parametrize("case", ae.WARP, ids=[w.name for w in ae.WARP])
def test_warp_affine_u8_pitched(eng, case):
    (sw, sh), (dw, dh) = case.ssize, case.dsize
    src = ae.noise(sw, sh, 40 + sw + sh)
    sp, dp = sw + case.spad, dw + case.dpad
    sparent = ae.noise(sp, sh, 41)
    sparent[:, :sw] = src
    ds = dev(sparent)
    dd = torch.full((dh, dp), ae.WARP_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.warp_affine_u8(ds.data_ptr(), sp, sw, sh, dd.data_ptr(), dp, dw, dh, np.asarray(case.M, np.float32))
    torch.cuda.synchronize()
    out = dd.cpu().numpy()
    want = ar.warp_affine_u8(src, dw, dh, case.M)
    assert np.array_equal(out[:, :dw], want)
    assert np.all(out[:, dw:] == ae.WARP_SENTINEL)
    if case.name == "singular":
        assert np.all(want == src[0, 0])
    if case.name.startswith("far"):
        assert np.all(want == 0)


@pytest.mark.parametrize("flow_output", [0, 1])
@pytest.mark.parametrize("case", ae.POST, ids=[p.name for p in ae.POST])
def test_postprocess_affine_pitched(eng, case, flow_output):
    u, v, I1 = ae.post_inputs(case)
    h, w = u.shape
    fp, ip = w + case.fpad, w + case.ipad
    pu = np.full((h, fp), ae.POST_SENTINEL, np.float32)
    pv = np.full((h, fp), ae.POST_SENTINEL, np.float32)
    pi = np.full((h, ip), 200, np.uint8)
    pu[:, :w], pv[:, :w], pi[:, :w] = u, v, I1
    du, dv, di = dev(pu), dev(pv), dev(pi)
    aff = (C.c_float * 6)(*[float(x) for x in np.asarray(case.M, np.float32).ravel()])
    rc = eng.lib.tvl1_postprocess_affine(eng.ctx, C.c_void_p(du.data_ptr()), C.c_void_p(dv.data_ptr()), 4 * fp,
                                         C.c_void_p(di.data_ptr()), ip, w, h, flow_output, aff, None)
    assert rc == 0
    torch.cuda.synchronize()
    gu, gv = du.cpu().numpy(), dv.cpu().numpy()
    wu, wv = ar.postprocess_affine(u, v, I1, flow_output, case.M)
    assert np.array_equal(gu[:, :w].view(np.uint32), wu.view(np.uint32))
    assert np.array_equal(gv[:, :w].view(np.uint32), wv.view(np.uint32))
    assert np.all(gu[:, w:] == ae.POST_SENTINEL) and np.all(gv[:, w:] == ae.POST_SENTINEL)
