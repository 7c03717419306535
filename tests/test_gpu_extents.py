"""Every entry point at the far end of the sizes its header accepts: tests/extent_cases.py's table
on the GPU, bit for bit against the project's references (tests/test_extent_cases_cpu.py shows
on the CPU that each reference has content in the rows that matter).

  A. Row walk.  k_fb_score, k_zero_above, k_compose_flow, k_invert_flow<false|true> and
     k_warp_flow_u8 cap their grid at 65535 row groups of 4 rows and walk the rest: at
     5 x 262149 a second step of 9 rows runs (two full row groups and one of a single row).
     Every output is pre-filled with a sentinel; the whole plane is compared, the rows
     y >= ROWS_CAP once more on their own, and those rows must have been written.  A row walk
     cut to its first step fails both, and its count.
  B. At the arithmetic bounds: 2^19 px for the 1/32-px map (32 mx reaches 2^24 - 32), a canvas
     of exactly 32767 px with a map that saturates to short, 65535 pairs in one launch.
  C. Rows over 4 x 65535 in every other 2-D launch, which puts rows / 4 straight into the grid
     (the runtime runs such grids): a size the header accepts gives the reference's
     bits, and TVL1_EHIP is never the answer to a frame size.
"""
import ctypes as C

import numpy as np
import pytest

import align_ref
import avgflow_ref
import compose_ref
import extent_cases as X
import fbcheck_ref
import initflow_ref
import invert_ref
import shift_ref
import zncc_ref
from optflow_amd import capi
from oracle import checker
from test_gpu_zncc import SENTINEL, Planes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
CAP = X.ROWS_CAP
FSENT = SENTINEL[np.dtype(F)]
MATH_IDS = {0: "ieee", 2: "fma"}
WALK_IDS = [c.name for c in X.WALK_CASES]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def assert_same(got, want, what):
    """Bit for bit, a NaN for a NaN; the rows of the second step once more on their own."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if got.dtype == F:
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    if got.shape[-2] > CAP:
        assert not X.second_step(bad).any(), what


def assert_second_step_written(got, what):
    """The output was pre-filled with the sentinel: the second step's rows no longer hold it."""
    tail = X.second_step(np.asarray(got))
    assert tail.shape[-2] == got.shape[-2] - CAP > 0
    fill = SENTINEL[tail.dtype]
    if tail.dtype == F:
        assert not (bits(tail) == bits(np.array(fill))).any(), what
    else:   # a u8 value may equal the fill; not every one of them
        assert (tail != fill).any(), what


def blank(shape, dtype=F):
    return np.full(shape, SENTINEL[np.dtype(dtype)], dtype)


@pytest.fixture(scope="module")
def eng(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


def make_engine(params, env=None):
    """An engine created under knobs that tvl1_create reads."""
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        return capi.Engine(params)
    finally:
        mp.undo()


# ================================================================== A. the row walk
_REF = {}


def walk_ref(b):
    """Pair b's planes and every reference of section A, computed once and never changed."""
    if b not in _REF:
        uf, vf, ub, vb = X.walk_planes(b)
        score = fbcheck_ref.fb_score(uf, vf, ub, vb, X.ALPHA)
        zu, zv, rejected = fbcheck_ref.zero_above(uf, vf, score, X.BETA)
        cu, cv, outside = compose_ref.compose(uf, vf, ub, vb)
        gu, gv, rs, inv_out, inv_unc = invert_ref.invert(uf, vf, X.INV_K, X.INV_TOL)
        J, m = zncc_ref.warp(X.walk_frame(b), uf, vf)
        r = dict(score=score, zero=(zu, zv, rejected), compose=(cu, cv, outside),
                 invert=(gu, gv, rs, (inv_out, inv_unc)), warp=(J, m.astype(np.uint8)))
        for a in (score, zu, zv, cu, cv, gu, gv, rs, J):
            a.setflags(write=False)
        _REF[b] = r
    return _REF[b]


def stacked(case, j):
    """Plane j (uf, vf, ub, vb) of the case's pairs, (n, H, W)."""
    return np.stack([X.walk_planes(b)[j] for b in range(case.n)])


def want_of(case, pick):
    return np.stack([pick(walk_ref(b)) for b in range(case.n)])


@pytest.mark.parametrize("case", X.WALK_CASES, ids=WALK_IDS)
def test_fb_score_walks_past_the_row_cap(eng, case):
    d = [Planes(stacked(case, j), case.roi) for j in range(4)]
    s = Planes(blank((case.n, X.H_TALL, X.W_THIN)), case.roi)
    torch.cuda.synchronize()
    if case.n == 1:
        eng.fb_score(d[0].ptr, d[1].ptr, d[0].pitch, d[2].ptr, d[3].ptr, d[2].pitch, X.W_THIN, X.H_TALL,
                     X.ALPHA, s.ptr, s.pitch, stream=eng.stream)
    else:
        eng.fb_score_batch(case.n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, d[2].ptr, d[3].ptr,
                           d[2].pitch, d[2].stride, X.W_THIN, X.H_TALL, X.ALPHA, s.ptr, s.pitch,
                           s.stride, stream=eng.stream)
    torch.cuda.synchronize()
    got, clean = s.get()
    assert clean, "a float outside the score's rows was written"
    assert_second_step_written(got, "score")
    assert_same(got, want_of(case, lambda r: r["score"]), "score")


@pytest.mark.parametrize("case", X.WALK_CASES, ids=WALK_IDS)
def test_zero_above_walks_past_the_row_cap_and_counts_there(eng, case):
    u, v = Planes(stacked(case, 0), case.roi), Planes(stacked(case, 1), case.roi)
    s = Planes(want_of(case, lambda r: r["score"]), case.roi)
    torch.cuda.synchronize()
    if case.n == 1:
        rej = [eng.zero_above(u.ptr, v.ptr, u.pitch, s.ptr, s.pitch, X.W_THIN, X.H_TALL, X.BETA,
                              stream=eng.stream)]
    else:
        rej = eng.zero_above_batch(case.n, u.ptr, v.ptr, u.pitch, u.stride, s.ptr, s.pitch, s.stride,
                                   X.W_THIN, X.H_TALL, X.BETA, stream=eng.stream)
    torch.cuda.synchronize()
    (gu, cu), (gv, cv) = u.get(), v.get()
    assert cu and cv, "a float outside the flow's rows was written"
    assert [int(r) for r in rej] == [walk_ref(b)["zero"][2] for b in range(case.n)]
    assert_same(gu, want_of(case, lambda r: r["zero"][0]), "u")
    assert_same(gv, want_of(case, lambda r: r["zero"][1]), "v")
    # the second step zeroed px: its rows are no longer the input's
    assert (bits(X.second_step(gu)) != bits(X.second_step(stacked(case, 0)))).any()


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in-place"])
@pytest.mark.parametrize("case", X.WALK_CASES, ids=WALK_IDS)
def test_compose_flow_walks_past_the_row_cap(eng, case, in_place):
    d = [Planes(stacked(case, j), case.roi) for j in range(4)]
    shape = (case.n, X.H_TALL, X.W_THIN)
    cu, cv = (d[0], d[1]) if in_place else (Planes(blank(shape), case.roi), Planes(blank(shape), case.roi))
    torch.cuda.synchronize()
    if case.n == 1:
        out = [eng.compose_flow(d[0].ptr, d[1].ptr, d[0].pitch, d[2].ptr, d[3].ptr, d[2].pitch, X.W_THIN,
                                X.H_TALL, cu.ptr, cv.ptr, cu.pitch, stream=eng.stream)]
    else:
        out = eng.compose_flow_batch(case.n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, d[2].ptr, d[3].ptr,
                                     d[2].pitch, d[2].stride, X.W_THIN, X.H_TALL, cu.ptr, cv.ptr, cu.pitch,
                                     cu.stride, stream=eng.stream)
    torch.cuda.synchronize()
    (gu, clean_u), (gv, clean_v) = cu.get(), cv.get()
    assert clean_u and clean_v, "a float outside the output rows was written"
    assert [int(o) for o in out] == [walk_ref(b)["compose"][2] for b in range(case.n)]
    if in_place:
        assert (bits(X.second_step(gu)) != bits(X.second_step(stacked(case, 0)))).any()
    else:
        assert_second_step_written(gu, "uc")
        assert_second_step_written(gv, "vc")
    assert_same(gu, want_of(case, lambda r: r["compose"][0]), "uc")
    assert_same(gv, want_of(case, lambda r: r["compose"][1]), "vc")


@pytest.mark.parametrize("arm", ["0", "1"], ids=["global", "window"])
@pytest.mark.parametrize("case", X.WALK_CASES, ids=WALK_IDS)
def test_invert_flow_walks_past_the_row_cap(built, case, arm):
    e = make_engine(capi.make_params(), {"TVL1_INVERT_WINDOW": arm})
    try:
        d = [Planes(stacked(case, j), case.roi) for j in range(2)]
        shape = (case.n, X.H_TALL, X.W_THIN)
        gu, gv, rs = (Planes(blank(shape), case.roi) for _ in range(3))
        torch.cuda.synchronize()
        if case.n == 1:
            c = e.invert_flow(d[0].ptr, d[1].ptr, d[0].pitch, X.INV_K, X.INV_TOL, gu.ptr, gv.ptr, gu.pitch,
                              rs.ptr, rs.pitch, X.W_THIN, X.H_TALL, stream=e.stream)
            cnt = [(c["outside"], c["unconverged"])]
        else:
            c = e.invert_flow_batch(case.n, d[0].ptr, d[1].ptr, d[0].pitch, d[0].stride, X.INV_K, X.INV_TOL,
                                    gu.ptr, gv.ptr, gu.pitch, gu.stride, rs.ptr, rs.pitch, rs.stride,
                                    X.W_THIN, X.H_TALL, stream=e.stream)
            cnt = [tuple(int(x) for x in row) for row in c]
        torch.cuda.synchronize()
        got = [p.get() for p in (gu, gv, rs)]
        kept = [p.get() for p in d]
    finally:
        e.close()
    assert all(clean for _, clean in got), "a float outside the output rows was written"
    assert cnt == [walk_ref(b)["invert"][3] for b in range(case.n)]
    for j, name in enumerate(("ug", "vg", "resid")):
        assert_second_step_written(got[j][0], name)
        assert_same(got[j][0], want_of(case, lambda r: r["invert"][j]), name)
    for j in range(2):   # f is what it was
        assert kept[j][1]
        assert_same(kept[j][0], stacked(case, j), "f")


@pytest.mark.parametrize("valid", [False, True], ids=["dst", "dst+valid"])
@pytest.mark.parametrize("b,roi", [(0, None), (1, None), (0, X.VIEW), (1, X.VIEW)],
                         ids=["dense-pair0", "dense-pair1", "view-pair0", "view-pair1"])
def test_warp_by_flow_walks_past_the_row_cap(eng, b, roi, valid):
    """One pair per call (the call has no batch): both pairs of the table, dense and as views."""
    uf, vf = X.walk_planes(b)[:2]
    I1 = Planes(X.walk_frame(b)[None], roi)
    u, v = Planes(uf[None], roi), Planes(vf[None], roi)
    dst = Planes(blank((1, X.H_TALL, X.W_THIN), np.uint8), roi)
    val = Planes(blank((1, X.H_TALL, X.W_THIN), np.uint8), roi)
    torch.cuda.synchronize()
    eng.warp_by_flow_u8(I1.ptr, I1.pitch, u.ptr, v.ptr, u.pitch, X.W_THIN, X.H_TALL, dst.ptr, dst.pitch,
                        val.ptr if valid else 0, val.pitch if valid else 0, stream=eng.stream)
    torch.cuda.synchronize()
    J, m = walk_ref(b)["warp"]
    (gd, clean_d), (gm, clean_m) = dst.get(), val.get()
    assert clean_d and clean_m
    assert_second_step_written(gd, "dst")
    assert_same(gd[0], J, "dst")
    if valid:
        assert_second_step_written(gm, "valid")
        assert_same(gm[0], m, "valid")
    else:
        assert np.all(gm == SENTINEL[np.dtype(np.uint8)])


# ================================================================== B. at the arithmetic bounds
@pytest.mark.parametrize("case", X.ZNCC_CASES, ids=[c.name for c in X.ZNCC_CASES])
def test_zncc_and_warp_at_the_map_bound(eng, case):
    """2^19 px one way: rint(32 mx) reaches 2^24 - 32 at the far edge.  Step 1 is shared, so the
    warp is held to it beside the score; the tall case walks rows in k_warp_flow_u8 as well."""
    I0, I1, u, v = X.zncc_planes(case)
    W, H = case.W, case.H
    J, m = zncc_ref.warp(I1, u, v)
    d = [Planes(a[None]) for a in (I0, I1, u, v)]
    dst, val = Planes(blank((1, H, W), np.uint8)), Planes(blank((1, H, W), np.uint8))
    torch.cuda.synchronize()
    eng.warp_by_flow_u8(d[1].ptr, d[1].pitch, d[2].ptr, d[3].ptr, d[2].pitch, W, H, dst.ptr, dst.pitch,
                        val.ptr, val.pitch, stream=eng.stream)
    torch.cuda.synchronize()
    assert_same(dst.get()[0][0], J, "dst")
    assert_same(val.get()[0][0], m.astype(np.uint8), "valid")
    for r in X.ZNCC_RADII:
        s = Planes(blank((1, H, W)))
        torch.cuda.synchronize()
        eng.zncc_score(d[0].ptr, d[0].pitch, d[1].ptr, d[1].pitch, d[2].ptr, d[3].ptr, d[2].pitch, W, H, r,
                       s.ptr, s.pitch, stream=eng.stream)
        torch.cuda.synchronize()
        got = s.get()[0][0]
        assert not (bits(got) == bits(np.array(FSENT))).any()
        assert_same(got, zncc_ref.score_from(J, m, I0, r), f"score r={r}")


@pytest.mark.parametrize("case", X.REMAP_CASES, ids=[c.name for c in X.REMAP_CASES])
def test_remap_on_the_largest_canvas(eng, case):
    frame, u, v = X.remap_planes(case)
    b = X.REMAP_BORDER
    CW, CH = case.W + 2 * b, case.H + 2 * b
    assert max(CW, CH) == X.CANVAS_MAX
    df, du, dv = Planes(frame[None]), Planes(u[None]), Planes(v[None])
    out = Planes(blank((1, CH, CW), np.uint8))
    torch.cuda.synchronize()
    eng.remap_flow_u8(df.ptr, df.pitch, case.W, case.H, du.ptr, dv.ptr, du.pitch, case.W, case.H, 1.0, b,
                      out.ptr, out.pitch, stream=eng.stream)
    torch.cuda.synchronize()
    assert_same(out.get()[0][0], avgflow_ref.remap(frame, u, v, 1.0, b), "canvas")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_postprocess_batch_of_the_most_pairs(eng, mode):
    """n = 65535 pairs of 1 x 1: the pair index reaches the last block of grid z."""
    u, v, I1 = X.post_batch_planes()
    n = X.POST_BATCH_MAX
    du, dv, dI = (torch.from_numpy(a.copy()).to("cuda:0") for a in (u, v, I1))
    torch.cuda.synchronize()
    eng.postprocess_batch(n, du.data_ptr(), dv.data_ptr(), 4, 4, dI.data_ptr(), 1, 1, 1, 1, mode,
                          stream=eng.stream)
    torch.cuda.synchronize()
    wu, wv = X.postprocess_numpy(u, v, I1, mode)
    assert_same(du.cpu().numpy(), wu, "u")
    assert_same(dv.cpu().numpy(), wv, "v")
    assert (wu[-8:] != u[-8:]).any()   # the last pairs are among the masked ones


# ================================================================== C. rows over the cap in every 2-D launch
def dev(a):
    """A device copy (through a writable host copy: the table's arrays are read-only)."""
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def mismatch(name, u, v, st, wi, ref):
    """None, or what differs from the reference (u, v, levels or None, per-warp counts)."""
    ur, vr, sizes, wr = ref
    if sizes is not None and st["sizes"] != sizes:
        return f"{name}: levels {st['sizes']} != {sizes}"
    if not np.array_equal(wi, wr):
        return f"{name}: per-warp iterations {np.asarray(wi).tolist()} != {np.asarray(wr).tolist()}"
    fin = np.isfinite(ur) & np.isfinite(vr)
    if not np.array_equal(fin, np.isfinite(u) & np.isfinite(v)):
        return f"{name}: finite mask differs"
    bad = fin & ((bits(u) != bits(ur)) | (bits(v) != bits(vr)))
    if bad.any():
        ys, xs = np.nonzero(bad)
        return (f"{name}: not bit-exact at {bad.sum()} px, x {xs.min()}..{xs.max()} y {ys.min()}..{ys.max()}, "
                f"{int(X.second_step(bad).sum()) if bad.shape[0] > CAP else 0} of them at y >= {CAP}")
    return None


_oracle = {}


def oracle_of(key, I0, I1, params, math, init=None):
    """(u, v, sizes, warp_iters) of the oracle, computed once per case and arithmetic."""
    if (key, math) not in _oracle:
        u, v, st, wi = checker.oracle_calc(I0, I1, capi.make_params(fast_math=math, **params), init=init)
        _oracle[(key, math)] = (u, v, st["sizes"], wi)
    return _oracle[(key, math)]


def seeded_ref(key, I0, I1, params, math, u0, v0):
    """tests/initflow_ref.py's seeded solve (IEEE) or the oracle's seeded entry (fma)."""
    u, v, wi, _ = initflow_ref.reference(("extent", key), I0, I1, params, u0, v0, math=math)
    return u, v, None, wi


def solve_device(e, I0, I1, f32=False, init=None):
    h, w = I0.shape
    d0, d1 = dev(I0), dev(I1)
    du = torch.full((h, w), float(FSENT), dtype=torch.float32, device=d0.device)
    dv = torch.full_like(du, float(FSENT))
    keep = [dev(a) for a in init] if init is not None else None
    torch.cuda.synchronize()
    item = 4 if f32 else 1
    st = e.calc_device(d0.data_ptr(), item * w, d1.data_ptr(), item * w, w, h, du.data_ptr(), dv.data_ptr(),
                       4 * w, warp_iters=True, f32=f32,
                       init=(keep[0].data_ptr(), keep[1].data_ptr()) if keep else None)
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
@pytest.mark.parametrize("name", ["fix", "stop", "median", "wide"])
def test_calc_on_a_pyramid_over_the_cap(built, name, math):
    """tvl1_calc at 20 x 327685 (both levels over 4 x 65535 rows): fixed work, the stopping rule,
    median 5 with gamma; and the transposed frame, the same table's x direction."""
    c = X.SOLVE_CASES[name]
    I0, I1 = X.solve_frames(c)
    ref = oracle_of(name, I0, I1, c.params, math)
    assert ref[2] == (X.PYR_LEVELS if name != "wide" else [(h, w) for w, h in X.PYR_LEVELS])
    e = capi.Engine(capi.make_params(fast_math=math, **c.params))
    try:
        u, v, st = solve_device(e, I0, I1)
    finally:
        e.close()
    err = mismatch(name, u, v, st, st["warp_iters"], ref)
    assert err is None, err
    if name == "stop":
        assert (st["warp_iters"] < c.params["iterations"]).any()


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
def test_calc_f32_over_the_cap(built, math):
    c = X.SOLVE_CASES["f32"]
    I0, I1 = X.solve_frames(c)
    rng = np.random.default_rng(c.seed)
    F0 = (I0 / 255.0 + rng.normal(0, 2e-3, I0.shape)).astype(F)   # off the u8 grid
    F1 = (I1 / 255.0 + rng.normal(0, 2e-3, I1.shape)).astype(F)
    ref = oracle_of("f32", F0, F1, c.params, math)
    e = capi.Engine(capi.make_params(fast_math=math, **c.params))
    try:
        u, v, st = solve_device(e, F0, F1, f32=True)
    finally:
        e.close()
    err = mismatch("f32", u, v, st, st["warp_iters"], ref)
    assert err is None, err
    assert st["sizes"] == [(X.W_PYR, X.H_TALL)]


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
def test_calc_init_from_a_seed_over_the_cap(built, math):
    """A non-constant seed: kb_flow_copy and k_flow_down build its pyramid."""
    c = X.SOLVE_CASES["init"]
    I0, I1 = X.solve_frames(c)
    u0, v0 = X.solve_seed(c)
    ref = seeded_ref("init", I0, I1, c.params, math, u0, v0)
    e = capi.Engine(capi.make_params(fast_math=math, **c.params))
    try:
        u, v, st = solve_device(e, I0, I1, init=(u0, v0))
    finally:
        e.close()
    err = mismatch("init", u, v, st, st["warp_iters"], ref)
    assert err is None, err
    assert st["sizes"] == X.PYR_LEVELS


def run_batch(e, I0s, I1s, **seed):
    n, h, w = I0s.shape
    d0, d1 = dev(I0s), dev(I1s)
    du = torch.full((n, h, w), float(FSENT), dtype=torch.float32, device=d0.device)
    dv = torch.full_like(du, float(FSENT))
    torch.cuda.synchronize()
    st = e.calc_batch_device(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h, du.data_ptr(),
                             dv.data_ptr(), 4 * w, 4 * w * h, warp_iters=True, **seed)
    torch.cuda.synchronize()
    return du.cpu().numpy(), dv.cpu().numpy(), st


@pytest.mark.parametrize("math", [0, 2], ids=MATH_IDS.get)
@pytest.mark.parametrize("name", ["batch", "const"])
def test_calc_batch_over_the_cap(built, name, math):
    """tvl1_calc_batch against the oracle per pair; tvl1_calc_batch_const_init against the seeded
    solve from two planes filled with the pair's constant."""
    c = X.SOLVE_CASES[name]
    prs = [X.solve_frames(c, b) for b in range(X.BATCH_N)]
    I0s, I1s = np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])
    e = capi.Engine(capi.make_params(fast_math=math, **c.params))
    try:
        u, v, st = run_batch(e, I0s, I1s, **(dict(init_const=X.CONST_SEEDS) if name == "const" else {}))
    finally:
        e.close()
    bad = []
    for b in range(X.BATCH_N):
        if name == "const":
            k = X.CONST_SEEDS[b]
            full = lambda x: np.full(I0s[b].shape, x, F)
            ref = seeded_ref((name, b), I0s[b], I1s[b], c.params, math, full(k[0]), full(k[1]))
        else:
            ref = oracle_of((name, b), I0s[b], I1s[b], c.params, math)
        assert st[b]["sizes"] == X.PYR_LEVELS
        bad.append(mismatch(f"{name} pair {b}", u[b], v[b], st[b], st[b]["warp_iters"], ref))
    bad = [x for x in bad if x]
    assert not bad, "; ".join(bad)


def test_profile_1_over_the_cap(built):
    """The DualTVL1 schedule: k_resize_hp, k_gradient, k_remap_cubic and k_median at both levels."""
    c = X.SOLVE_CASES["profile1"]
    I0, I1 = X.solve_frames(c)
    ref = oracle_of("profile1", I0, I1, c.params, 0)
    assert ref[2] == X.PYR_LEVELS
    e = capi.Engine(capi.make_params(**c.params))
    try:
        u, v, st = solve_device(e, I0, I1)
    finally:
        e.close()
    err = mismatch("profile1", u, v, st, st["warp_iters"], ref)
    assert err is None, err


# ---------------------------------------------------------------- stand-alone calls
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2])
def test_postprocess_over_the_cap(eng, n, mode):
    pl = [X.post_planes(b) for b in range(n)]
    u, v, I1 = (np.stack([p[j] for p in pl]) for j in range(3))
    W, H = X.W_THIN, X.H_TALL
    du, dv, dI = dev(u), dev(v), dev(I1)
    torch.cuda.synchronize()
    if n == 1:
        rc = eng.lib.tvl1_postprocess(eng.ctx, du.data_ptr(), dv.data_ptr(), 4 * W, dI.data_ptr(), W, W, H,
                                      mode, eng.stream)
        eng._check(rc, "tvl1_postprocess")
    else:
        eng.postprocess_batch(n, du.data_ptr(), dv.data_ptr(), 4 * W, 4 * W * H, dI.data_ptr(), W, W * H, W, H,
                              mode, stream=eng.stream)
    torch.cuda.synchronize()
    gu, gv = du.cpu().numpy(), dv.cpu().numpy()
    for b in range(n):
        wu, wv = initflow_ref.postprocess(u[b], v[b], I1[b], mode)
        assert_same(gu[b], wu, "u")
        assert_same(gv[b], wv, "v")
        assert (bits(X.second_step(wu)) != bits(X.second_step(u[b]))).any()   # the mask bites there


@pytest.mark.parametrize("flow_output", [0, 1])
def test_postprocess_affine_over_the_cap(eng, flow_output):
    """Against the oracle and against tests/align_ref.py, which shares no code with it."""
    u, v, I1 = X.post_planes(0)
    W, H = X.W_THIN, X.H_TALL
    du, dv, dI = dev(u), dev(v), dev(I1)
    aff = (C.c_float * 6)(*[float(x) for x in X.AFFINE.ravel()])
    torch.cuda.synchronize()
    rc = eng.lib.tvl1_postprocess_affine(eng.ctx, C.c_void_p(du.data_ptr()), C.c_void_p(dv.data_ptr()), 4 * W,
                                         C.c_void_p(dI.data_ptr()), W, W, H, flow_output, aff, None)
    eng._check(rc, "tvl1_postprocess_affine")
    torch.cuda.synchronize()
    gu, gv = du.cpu().numpy(), dv.cpu().numpy()
    for name, (wu, wv) in (("oracle", checker.oracle_postprocess_affine(u, v, I1, flow_output, X.AFFINE)),
                           ("align_ref", align_ref.postprocess_affine(u, v, I1, flow_output, X.AFFINE))):
        assert_same(gu, wu, f"u ({name})")
        assert_same(gv, wv, f"v ({name})")
    assert np.count_nonzero(X.second_step(gu)) > 0


def test_warp_affine_over_the_cap(eng):
    src = X.walk_frame(0)
    W, H = X.W_THIN, X.H_TALL
    ds = dev(src)
    dd = torch.full((H, W), int(SENTINEL[np.dtype(np.uint8)]), dtype=torch.uint8, device=ds.device)
    torch.cuda.synchronize()
    eng.warp_affine_u8(ds.data_ptr(), W, W, H, dd.data_ptr(), W, W, H, X.AFFINE)
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert_second_step_written(got, "dst")
    assert_same(got, checker.oracle_warp_affine_u8(src, W, H, X.AFFINE), "dst (oracle)")
    assert_same(got, align_ref.warp_affine_u8(src, W, H, X.AFFINE), "dst (align_ref)")
    assert np.count_nonzero(X.second_step(got)) > 0


def test_blend6_over_the_cap(eng):
    fr = X.blend_frames()
    W, H = X.W_BLEND, X.H_TALL
    d = [dev(f) for f in fr]
    dst = torch.full((H, W), int(SENTINEL[np.dtype(np.uint8)]), dtype=torch.uint8, device=d[0].device)
    torch.cuda.synchronize()
    eng.blend6_u8([t.data_ptr() for t in d], [W] * 6, W, H, dst.data_ptr(), W, stream=eng.stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert_second_step_written(got, "blend")
    assert_same(got, avgflow_ref.blend6(list(fr)), "blend")


def test_half_over_the_cap(eng):
    src = X.half_frame()
    H, W = src.shape
    ds = dev(src)
    dst = torch.full((H // 2, W // 2), int(SENTINEL[np.dtype(np.uint8)]), dtype=torch.uint8, device=ds.device)
    torch.cuda.synchronize()
    eng.half_u8(ds.data_ptr(), W, W, H, dst.data_ptr(), W // 2, stream=eng.stream)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got.shape[0] > CAP
    assert_second_step_written(got, "half")
    assert_same(got, avgflow_ref.half(src), "half")


def test_estimate_shift_over_the_cap(eng):
    """20 x 524296, max_shift 5: one level of 262148 rows through k_shift_half's grid z; every
    field of the record, single and as a batch of two."""
    w, h = X.SHIFT_SIZE
    prs = [X.shift_pair(b) for b in range(2)]
    want = [shift_ref.estimate(a, b, X.SHIFT_R) for a, b in prs]
    assert (want[0]["dx"], want[0]["dy"]) == X.SHIFT_TRUE
    dA, dB = dev(np.stack([p[0] for p in prs])), dev(np.stack([p[1] for p in prs]))
    torch.cuda.synchronize()
    assert eng.estimate_shift(dA.data_ptr(), w, dB.data_ptr(), w, w, h, X.SHIFT_R, stream=eng.stream) == want[0]
    assert eng.estimate_shift_batch(2, dA.data_ptr(), w, w * h, dB.data_ptr(), w, w * h, w, h, X.SHIFT_R,
                                    stream=eng.stream) == want
