"""tests/align_edges.py held to the headers, the planner and the oracle, with no GPU.

tests/test_gpu_align_edges.py runs that table bitwise on the GPU.  It would be vacuous if a
size no longer sat on a kernel's edge, if no keypoint lay next to a tile seam, or if no score
tied where ka_select's low passes are meant to decide.  So here

  * the table's periods are the constants of csrc/tvl1_align.hpp and tvl1_align_plan.hpp, and
    every size steps a tile count exactly where the table says;
  * tests/align_plan_dump.cpp (built as tests/test_plan_cpu.py builds plan_dump: g++, ASan +
    UBSan) sweeps the per-keypoint capacity against the quota sum -- 304 of the 72000
    combinations overflowed while the buffers were sized by nfeatures alone -- and confirms
    the match segmentation, the skipped levels and the budget cases;
  * a census of the oracle's keypoints finds them on the border lines and on both sides of
    every seam a case names, finds the tie groups the select cases cut, 17 and 25 keypoints in
    the budget cases, empty upper levels in the level-drop case and the listed outcomes of the
    alignment cases;
  * numpy restatements that share no code with the oracle (tests/align_ref.py) reproduce its
    match lists, its warps and post-process, and its level-0 keypoints.
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import align_edges as ae
import align_ref as ar
from oracle import checker

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fibsem-optflow_amd" / "csrc"


@pytest.fixture(scope="module")
def align_dump(tmp_path_factory):
    """Runs align_plan_dump on a list of query lines and returns its output lines."""
    d = tmp_path_factory.mktemp("align_plan")
    exe = d / "align_plan_dump"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "align_plan_dump.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        cases = d / "cases.txt"
        cases.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a sanitizer report fails here
        out = r.stdout.splitlines()
        assert len(out) == len(lines), (len(out), len(lines))
        return out, r.stderr

    return run


def geom(align_dump, W, H, nfeatures=5000, scale_factor=1.2, nlevels=8, edge_threshold=31, **_):
    """(kcap, quota sum, border, [(w, h, quota, skipped) per level]) from the planner."""
    out, _ = align_dump([f"geom {W} {H} {nfeatures} {scale_factor} {nlevels} {edge_threshold}"])
    head, levels = out[0].split("|")
    L, kcap, qsum, border = (int(x) for x in head.split())
    v = [int(x) for x in levels.split()]
    assert len(v) == 4 * L
    return kcap, qsum, border, [tuple(v[4 * l:4 * l + 4]) for l in range(L)]


# ---------------------------------------------------------------- constants
def test_plan_header_is_plain_cxx():
    text = (CSRC / "tvl1_align_plan.hpp").read_text()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text


def test_table_periods_are_the_kernels():
    align = (CSRC / "tvl1_align.hpp").read_text()
    plan = (CSRC / "tvl1_align_plan.hpp").read_text()
    eng = (CSRC / "tvl1_engine.hip").read_text()
    m = re.search(r"constexpr int kFhW = (\d+), kFhH = (\d+),", align)
    assert m and (int(m.group(1)), int(m.group(2))) == (ae.FH_W, ae.FH_H)
    m = re.search(r"constexpr int kNmsRows = (\d+);", align)
    assert m and int(m.group(1)) == ae.NMS_ROWS
    m = re.search(r"constexpr int kMatchSegs = (\d+), kMatchSegPx = (\d+), kMatchTile = (\d+);", plan)
    assert m and tuple(int(x) for x in m.groups()) == (ae.MATCH_SEGS, ae.MATCH_SEG_PX, ae.MATCH_TILE)
    # the launches and kernels that use them
    assert "dim3((g.w[l] + kFhW - 1) / kFhW, (g.h[l] + kFhH - 1) / kFhH)" in eng
    assert "dim3((g.w[l] + 63) / 64, (g.h[l] + kNmsRows - 1) / kNmsRows)" in eng
    assert "const int x = blockIdx.x * 64 + tx;" in align and ae.NMS_W == 64
    assert "__shared__ uint32_t tile[64 * 8];" in align and "const int nj = min(64, j1 - jt);" in align
    assert "const int i = blockIdx.x * 64 + lane;" in align and ae.QUERY_GROUP == 64
    assert "dim3((nq + 63) / 64, mp.nseg)" in eng


def _tiles(n, period):
    return -(-n // period)


def test_sizes_step_the_tile_counts():
    sizes = {d.name.rsplit("-L", 1)[0]: d.frame().shape for d in ae.DETECT}
    h, w = sizes["129x97"]
    assert (_tiles(w, ae.FH_W), _tiles(w - 1, ae.FH_W)) == (3, 2)          # a third column, one px wide
    assert (_tiles(h, ae.NMS_ROWS), _tiles(h, ae.FH_H)) == (2, 7)
    assert sizes["64x64"] == (64, 64) and sizes["65x65"] == (65, 65)
    assert (_tiles(64, ae.FH_W), _tiles(65, ae.FH_W)) == (1, 2) == (_tiles(64, ae.NMS_ROWS), _tiles(65, ae.NMS_ROWS))
    h, w = sizes["63x130"]
    assert _tiles(w, ae.FH_W) == 1 and w % ae.FH_W == ae.FH_W - 1
    assert (_tiles(h, ae.NMS_ROWS), _tiles(h - 2, ae.NMS_ROWS)) == (3, 2)
    assert sizes["33x33"] == (2 * ae.ET + 1,) * 2                          # one candidate px
    for d in ae.DETECT_EMPTY:
        assert min(d.frame().shape) == 2 * ae.ET                           # none
    for d in ae.DETECT:                                                    # the seams a case names are seams
        for x in d.xs:
            assert x % ae.FH_W in (ae.FH_W - 1, 0)
        for y in d.ys:
            assert y % ae.FH_H in (ae.FH_H - 1, 0)
    assert set(ae.REUSE_ORDER) <= {d.name for d in ae.DETECT}
    for nq in ae.MATCH_NQ:
        assert nq == 1 or abs(nq - ae.QUERY_GROUP) <= 1
    assert {1, 63, 64, 65} == set(ae.MATCH_NQ)
    assert {0, 1, 2, 63, 64, 65, 256, 257, 769, 4096, 4097} == set(ae.MATCH_NT)
    for w in ae.WARP[:16]:
        assert w.dsize[0] in (1, 63, 64, 65) and w.dsize[1] in (1, 3, 4, 5)
    assert len({w.dsize for w in ae.WARP[:16]}) == 16


# ---------------------------------------------------------------- planner
def test_per_keypoint_capacity_holds_the_quota_sum(align_dump):
    """nfeatures 1..3000 x nlevels {2, 3, 4, 8, 12, 16} x scale_factor {1.1, 1.2, 1.5, 2.0}:
    every per-keypoint buffer of the carve holds the quota sum."""
    out, err = align_dump(["sweep 1 3000"])
    cases, bad = (int(x) for x in out[0].split())
    assert cases == 3000 * 6 * 4
    assert bad == 0, err


def test_budget_cases_overrun_nfeatures(align_dump):
    for b in ae.BUDGET:
        for f in b.frames:
            h, w = f().shape
            kcap, qsum, _, _ = geom(align_dump, w, h, **b.kw)
            assert qsum == b.count == b.kw["nfeatures"] + 1 and kcap == qsum
    # the first case's overrun would land on desc[0]: the carve keeps it out
    b = ae.BUDGET[0]
    out, _ = align_dump([f"carve 400 300 {b.kw['nfeatures']} {b.kw['scale_factor']} {b.kw['nlevels']} 0"])
    _, kps, d0, d1, best, _, _, _ = (int(x) for x in out[0].split())
    assert d0 - kps >= 16 * b.count and d1 - d0 >= 32 * b.count and best - d1 >= 32 * b.count


def test_match_segmentation(align_dump):
    nts = sorted(ae.MATCH_PLAN)
    out, _ = align_dump([f"match {nt}" for nt in nts])
    for nt, o in zip(nts, out):
        assert tuple(int(x) for x in o.split()) == ae.MATCH_PLAN[nt], (nt, o)
    assert ae.MATCH_PLAN[769][3] == 1          # a one-descriptor last segment
    assert ae.MATCH_PLAN[4097][2] == 3         # three empty trailing segments
    out, _ = align_dump([f"match {nt}" for nt in range(0, 6000)])
    for nt, o in enumerate(out):               # every plan covers its train set, in whole tiles
        nseg, seg, empty, last = (int(x) for x in o.split())
        assert 1 <= nseg <= ae.MATCH_SEGS and seg % ae.MATCH_TILE == 0 and nseg * seg >= nt
        assert 0 <= empty < nseg and (nseg - empty - 1) * seg + last == nt and 0 <= last <= seg
    out, _ = align_dump([f"match {ae.MATCH_DUP_NT}"])
    nseg, seg, _, _ = (int(x) for x in out[0].split())
    assert (nseg, seg) == (3, 256)
    (a, b), (c, d), (e, f) = ae.MATCH_DUPS
    assert a // 64 == b // 64 and c // 64 + 1 == d // 64 and c // seg == d // seg
    assert e // seg + 1 == f // seg


def test_level_drop_case_skips_upper_levels(built, align_dump):
    d = next(d for d in ae.DETECT if d.name == "129x97-et31-L8")
    f = d.frame()
    _, _, border, levels = geom(align_dump, f.shape[1], f.shape[0], **d.kw)
    assert border == 31 and [l[3] for l in levels] == [0, 0, 0, 1, 1, 1, 1, 1]
    kp, _ = checker.oracle_orb_detect(f, **d.kw)
    counts = np.bincount(kp[:, 2].astype(int), minlength=8)
    assert np.all(counts[:3] > 0) and np.all(counts[3:] == 0), counts
    # with the 16-px threshold the same frame keeps them
    _, _, border, levels = geom(align_dump, f.shape[1], f.shape[0], edge_threshold=ae.ET)
    assert border == 16 and [l[3] for l in levels][:5] == [0] * 5


# ---------------------------------------------------------------- census, by the oracle
@pytest.mark.parametrize("case", ae.DETECT, ids=[d.name for d in ae.DETECT])
def test_census_keypoints_on_borders_and_seams(built, case):
    f = case.frame()
    H, W = f.shape
    kp, _ = checker.oracle_orb_detect(f, **case.kw)
    k0 = kp[kp[:, 2] == 0]
    b = max(case.kw.get("edge_threshold", 31), 16)   # the case's own border
    assert len(k0) > 0
    assert k0[:, 0].min() >= b and k0[:, 0].max() <= W - 1 - b
    assert k0[:, 1].min() >= b and k0[:, 1].max() <= H - 1 - b
    assert all(b <= x <= W - 1 - b for x in case.xs) and all(b <= y <= H - 1 - b for y in case.ys)
    for x in (b, W - 1 - b) + tuple(case.xs):
        assert np.any(k0[:, 0] == x), ("no keypoint in column", x)
    for y in (b, H - 1 - b) + tuple(case.ys):
        assert np.any(k0[:, 1] == y), ("no keypoint in row", y)
    if case.kw["nlevels"] > 1 and W > 2 * b + 20:
        assert np.any(kp[:, 2] > 0)


@pytest.mark.parametrize("case", ae.DETECT_EMPTY, ids=[d.name for d in ae.DETECT_EMPTY])
def test_census_no_candidate_px(built, case):
    kp, desc = checker.oracle_orb_detect(case.frame(), **case.kw)
    assert len(kp) == 0 and len(desc) == 0


def test_census_mirror_frame_has_equal_neighbours(built):
    """Both halves of the tie rule's position test decide something: pairs of equal scores side
    by side (the right one goes) and one above the other (the lower one goes)."""
    f = ae.mirror()
    assert f.shape == (ae.MIRROR_H, ae.MIRROR_W) and f.max() < 96
    score = ar.harris_scores(f, ae.ET)
    with_rule, without = ar.nms3(score), ar.nms3(score, position_rule=False)
    ys, xs = np.nonzero(without & ~with_rule)
    cx, cy = ae.MIRROR_W // 2, ae.MIRROR_H // 2
    side = [(x, y) for x, y in zip(xs, ys) if x == cx and score[y, x - 1] == score[y, x] and with_rule[y, x - 1]]
    below = [(x, y) for x, y in zip(xs, ys) if y == cy and score[y - 1, x] == score[y, x] and with_rule[y - 1, x]]
    assert len(side) >= 2 and len(below) >= 2, (side, below)
    kp, _ = checker.oracle_orb_detect(f, edge_threshold=ae.ET, nlevels=1)
    ref, _ = ar.level0_keypoints(f, 5000, ae.ET)
    _same_keypoints(kp, ref)
    assert len(kp) == with_rule.sum() < without.sum()


def _tie_groups(resp):
    """sizes of the groups of equal responses, best first, and their running total"""
    u, c = np.unique(resp, return_counts=True)
    c = c[::-1]
    return c, np.cumsum(c)


def test_census_select_cases_cut_tie_groups(built):
    f = ae.periodic()
    assert f.shape == (ae.PERIODIC_H, ae.PERIODIC_W)
    kp, _ = checker.oracle_orb_detect(f, nfeatures=100000, cap=100000, **ae.SELECT_KW)
    sizes, total = _tie_groups(kp[:, 4])
    assert (len(kp), len(sizes), sizes.max()) == (ae.PERIODIC_COUNT, ae.PERIODIC_DISTINCT, ae.PERIODIC_MAX_TIE)
    for nf in ae.SELECT_TIE_CUTS:
        g = int(np.searchsorted(total, nf, side="left"))     # the group the cut falls in
        before = total[g - 1] if g else 0
        assert before < nf < total[g], (nf, before, total[g])  # strictly inside it
    for nf in ae.SELECT_NFEATURES:
        k, _ = checker.oracle_orb_detect(f, nfeatures=nf, cap=100000, **ae.SELECT_KW)
        assert len(k) == min(nf, ae.PERIODIC_COUNT)


def test_census_budget_cases(built):
    for b in ae.BUDGET:
        for f in b.frames:
            kp, desc = checker.oracle_orb_detect(f(), **b.kw)
            assert len(kp) == len(desc) == b.count == b.kw["nfeatures"] + 1


@pytest.mark.parametrize("case", ae.ALIGN, ids=[a.name for a in ae.ALIGN])
def test_census_alignment_outcomes(built, case):
    f1, f0 = case.frames()
    assert max(f1.shape + f0.shape) <= 400
    A, ng, oc = checker.oracle_find_alignment(f1, f0, **case.kw)
    assert (oc, ng) == (case.outcome, case.n_good)
    ident = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    assert np.array_equal(A, ident) == (oc != 0)
    if case.name in ae.ALIGN_SWAPPED:      # the loop bound bites: queries past train rows - 1
        kw = {k: v for k, v in case.kw.items() if k != "method"}
        nq = len(checker.oracle_orb_detect(f1, **kw)[0])
        nt = len(checker.oracle_orb_detect(f0, **kw)[0])
        assert nq > nt - 1 > 10
    if case.name.startswith("shift"):
        assert abs(A[0, 2] - 14.5) < 1 and abs(A[1, 2] - 9.25) < 1


# ---------------------------------------------------------------- references sharing no code
def test_match_reference_equals_oracle(built):
    for nq in ae.MATCH_NQ:
        q = ae.descriptors(nq, 100 + nq)
        for nt in ae.MATCH_NT:
            t = ae.descriptors(nt, 200 + nt)
            got, want = checker.oracle_match_knn2(q, t), ar.match_knn2(q, t)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (nq, nt)
    q, t, dups = ae.match_dup_case()
    idx, dist = ar.match_knn2(q, t)
    assert np.array_equal(idx, np.array(dups)) and np.all(dist == 0)
    oi, od = checker.oracle_match_knn2(q, t)
    assert np.array_equal(oi, idx) and np.array_equal(od, dist)
    same = np.repeat(ae.descriptors(1, 5), 300, axis=0)
    for fn in (ar.match_knn2, checker.oracle_match_knn2):
        idx, dist = fn(same[:3], same)
        assert np.all(idx == [0, 1]) and np.all(dist == 0)
        idx, dist = fn(~same[:1], same[:1])
        assert idx.tolist() == [[0, -1]] and dist.tolist() == [[256, ar.NO_DIST]]


def _warp_src(case):
    sw, sh = case.ssize
    return ae.noise(sw, sh, 40 + sw + sh)


@pytest.mark.parametrize("case", ae.WARP, ids=[w.name for w in ae.WARP])
def test_warp_reference_equals_oracle(built, case):
    src = _warp_src(case)
    dw, dh = case.dsize
    want = ar.warp_affine_u8(src, dw, dh, case.M)
    assert np.array_equal(checker.oracle_warp_affine_u8(src, dw, dh, case.M), want)
    if case.name == "singular":
        assert np.all(want == src[0, 0])
    if case.name.startswith("far"):
        assert np.all(want == 0)
    if case.name == "shift-int":
        assert np.array_equal(want[:-2, 3:], src[2:, :-3]) and np.all(want[:, :3] == 0) and np.all(want[-2:] == 0)


@pytest.mark.parametrize("flow_output", [0, 1])
@pytest.mark.parametrize("case", ae.POST, ids=[p.name for p in ae.POST])
def test_postprocess_reference_equals_oracle(built, case, flow_output):
    u, v, I1 = ae.post_inputs(case)
    wu, wv = ar.postprocess_affine(u, v, I1, flow_output, case.M)
    gu, gv = checker.oracle_postprocess_affine(u, v, I1, flow_output, case.M)
    assert np.array_equal(gu.view(np.uint32), wu.view(np.uint32))
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32))
    assert np.all(wu[I1 <= 1] == 0) and np.all(wv[I1 <= 1] == 0) and np.any(I1 <= 1)
    if I1.shape[1] > 1:
        assert np.any(wu[I1 > 1] != 0)


def _same_keypoints(kp, ref):
    assert len(kp) == len(ref)
    assert np.array_equal(kp[:, [0, 1, 4]].view(np.uint32), ref.view(np.uint32))


def test_detector_reference_equals_oracle_on_noise(built):
    case = next(d for d in ae.DETECT if d.name == "129x97-L1")
    f = case.frame()
    kp, _ = checker.oracle_orb_detect(f, **case.kw)
    ref, _ = ar.level0_keypoints(f, 5000, ae.ET)
    assert len(ref) > 500
    _same_keypoints(kp, ref)


def test_detector_reference_equals_oracle_on_ties(built):
    """The periodic frame at every budget; where the cut falls inside a tie group, the kept
    members of that group are its first in raster order."""
    f = ae.periodic()
    for nf in ae.SELECT_NFEATURES:
        kp, _ = checker.oracle_orb_detect(f, nfeatures=nf, cap=100000, **ae.SELECT_KW)
        ref, allk = ar.level0_keypoints(f, nf, ae.ET)
        _same_keypoints(kp, ref)
        if nf in ae.SELECT_TIE_CUTS:
            cut = kp[-1, 4]
            group = allk[allk[:, 2] == cut]
            kept = kp[kp[:, 4] == cut]
            assert 0 < len(kept) < len(group)
            pos = group[:, 1] * ae.PERIODIC_W + group[:, 0]
            assert np.all(np.diff(pos) > 0)                     # the group in raster order
            assert np.array_equal(kept[:, :2], group[:len(kept), :2])
    # without the position half of the rule, equal neighbours would both survive: the frame has none
    score = ar.harris_scores(f, ae.ET)
    assert ar.nms3(score).sum() == ae.PERIODIC_COUNT
