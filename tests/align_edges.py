"""TEST INFRASTRUCTURE: the one table of cases that sit on the pre-alignment kernels' edges
(csrc/tvl1_align.hpp, planned by csrc/tvl1_align_plan.hpp) -- pure data and frame builders, no
GPU.

  ka_fast_harris            64 x 16 px tiles (kFhW x kFhH) with LDS aprons
  ka_nms                    64 x 64 px tiles (64 x kNmsRows), one global atomic per block
  ka_select                 8-pass radix select; the low four passes (the position half of a
                            key) decide only where scores tie
  ka_match2 / _merge        64-query groups, 64-descriptor LDS tiles, <= 16 train segments of
                            about 256 (kMatchSegs, kMatchSegPx), trailing segments empty when
                            rounding the segment up overshoots
  ka_warp_u8, ka_map_*      64 x 4 px blocks over pitched planes
  tvl1_find_alignment       the min(nt - 1, nq) loop bound, outcome 2, pitched frames
  align_carve               per-keypoint buffers sized by max(nfeatures, sum of the quotas)

tests/test_align_edges_cpu.py checks on the CPU that every case still sits where this table
says (the constants read from the headers, a census of the oracle's keypoints, numpy
restatements that share no code with the oracle); tests/test_gpu_align_edges.py runs the
table on the GPU, bitwise.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
from scipy import ndimage

from optflow_amd import synth

# the periods this table is built on; test_align_edges_cpu.py reads them from the headers
FH_W, FH_H, NMS_W, NMS_ROWS = 64, 16, 64, 64
MATCH_SEGS, MATCH_SEG_PX, MATCH_TILE, QUERY_GROUP = 16, 256, 64, 64
ET = 16   # the edge threshold of the small frames: ORB's least border (patch radius 15 + 1)


# ---------------------------------------------------------------- frame builders
def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def texture(W, H, seed):
    return np.clip(np.rint(synth.base_texture(W, H, seed=seed)), 0, 255).astype(np.uint8)


PERIODIC_SEED, PERIODIC_W, PERIODIC_H = 1, 190, 150


def periodic():
    """A 32 x 32 random tile repeated and cropped to 190 x 150: corners 32 px apart see the
    same neighbourhood and score the same, in tie groups of up to 20."""
    tile = np.random.default_rng(PERIODIC_SEED).integers(0, 256, (32, 32)).astype(np.uint8)
    return np.tile(tile, (5, 6))[:PERIODIC_H, :PERIODIC_W].copy()


MIRROR_SEED, MIRROR_W, MIRROR_H = 2, 66, 66


def mirror():
    """A random quadrant (values below 96) mirrored about both axes of a 66 x 66 frame.  The
    Sobel gradients stay below 2^9 and the 49-term Harris sums below 2^24: they are exact
    integers whatever the order of the sum, so mirrored px score exactly the same -- and the
    px either side of an axis (columns 32|33, rows 32|33) are NEIGHBOURS with equal scores:
    only the position half of the suppression's tie rule decides between them."""
    q = np.random.default_rng(MIRROR_SEED).integers(0, 96, (MIRROR_H // 2, MIRROR_W // 2)).astype(np.uint8)
    top = np.concatenate([q, q[:, ::-1]], axis=1)
    return np.concatenate([top, top[::-1]], axis=0)


def sampled(base, X, Y):
    """u8 frame of a float image sampled bilinearly at (X, Y), 0 outside."""
    return np.clip(np.rint(ndimage.map_coordinates(np.asarray(base, np.float64), [Y, X], order=1,
                                                   cval=0.0)), 0, 255).astype(np.uint8)


def in_parent(frame, ox, oy, PW, PH, fill=7):
    """(parent, view): the frame as a pitched view at (ox, oy) of a PW x PH parent filled with
    `fill` noise (seeded by it), so a read past a row's end meets something else."""
    h, w = frame.shape
    assert ox + w <= PW and oy + h <= PH
    parent = noise(PW, PH, 1000 + fill)
    parent[oy:oy + h, ox:ox + w] = frame
    return parent, parent[oy:oy + h, ox:ox + w]


# ---------------------------------------------------------------- detect cases
# name, frame builder, ORB parameters; xs / ys: level-0 columns / rows that must hold a keypoint
# besides the four border lines (both sides of each tile seam inside the candidate area).
Detect = namedtuple("Detect", "name frame kw xs ys")


def _both_levels(name, frame, kw, xs=(), ys=()):
    return [Detect(f"{name}-L{nl}", frame, dict(kw, nlevels=nl), xs, ys) for nl in (1, 8)]


DETECT = (
    # x seam 63|64 of both tilings, a third tile column one px wide (all border, its scores
    # must still be written 0), ka_fast_harris rows 31|32, 47|48, 63|64 (the row seam 15|16
    # is the border line y = 16 itself), two ka_nms block rows
    _both_levels("129x97", lambda: noise(129, 97, 0), dict(edge_threshold=ET), (63, 64), (31, 32, 47, 48, 63, 64))
    + _both_levels("64x64", lambda: noise(64, 64, 1), dict(edge_threshold=ET), (), (31, 32))
    + _both_levels("65x65", lambda: noise(65, 65, 1), dict(edge_threshold=ET), (), (31, 32, 47, 48))
    # three ka_nms block rows (the third two rows high), a partial tile in x
    + _both_levels("63x130", lambda: noise(63, 130, 3), dict(edge_threshold=ET), (), (63, 64, 95, 96, 111, 112))
    # one candidate px, (16, 16); seed 7 makes it a corner
    + _both_levels("33x33", lambda: noise(33, 33, 7), dict(edge_threshold=ET))
    # the default threshold of 31 px: levels >= 3 of 129 x 97 (75 x 56 and smaller) drop out
    # (border lines x = 31 | 97, y = 31 | 65; the seams inside them: x 63|64, y 47|48, 63|64)
    + [Detect("129x97-et31-L8", lambda: noise(129, 97, 0), dict(nlevels=8), (63, 64), (47, 48, 63, 64))]
    # equal scores next to each other, left-right and up-down: the suppression's tie rule
    + _both_levels("mirror66", mirror, dict(edge_threshold=ET))
    + _both_levels("129x97-blur", lambda: noise(129, 97, 2), dict(edge_threshold=ET, blur_for_descriptor=1),
                   (63, 64), (31, 32, 47, 48, 63, 64))
)
# no candidate px at all: n == 0 and TVL1_OK
DETECT_EMPTY = _both_levels("32x40", lambda: noise(32, 40, 0), dict(edge_threshold=ET)) + \
    _both_levels("40x32", lambda: noise(40, 32, 0), dict(edge_threshold=ET))
# a pitched view at (3, 5) of a 200 x 150 parent must equal its contiguous copy
ROI = dict(ox=3, oy=5, PW=200, PH=150, W=129, H=97, seed=0)
# output capacity: cap = n - CAP_SHORT rows written, the rest keep a sentinel; cap = 0 with null
# outputs; *n is the full count either way
CAP_SHORT = 10
# one engine is reused over these in this order: the frame shrinks, then grows, so stale score
# and key scratch of a larger level would show
REUSE_ORDER = ("129x97-L8", "64x64-L8", "33x33-L1", "63x130-L8", "129x97-blur-L8", "65x65-L1", "mirror66-L1",
               "129x97-et31-L8", "129x97-L1")

# ---------------------------------------------------------------- select cases
# the periodic frame at nlevels = 1: PERIODIC_COUNT survivors in PERIODIC_DISTINCT distinct
# scores.  50, 51, 64 and 200 cut strictly inside a tie group: the kept members of the cut
# group are decided by position alone (the low passes of ka_select).  count - 1 runs the
# select with one key to drop, count and count + 1 the copy-all path (n == quota, n < quota).
PERIODIC_COUNT, PERIODIC_DISTINCT, PERIODIC_MAX_TIE = 1818, 100, 20
SELECT_TIE_CUTS = (50, 51, 64, 200)
SELECT_NFEATURES = SELECT_TIE_CUTS + (PERIODIC_COUNT - 1, PERIODIC_COUNT, PERIODIC_COUNT + 1)
SELECT_KW = dict(edge_threshold=ET, nlevels=1)

# ---------------------------------------------------------------- budget cases
# ORB's quota rule rounds each level's share: the shares add up to nfeatures + 1 here, and
# that many keypoints come back.
Budget = namedtuple("Budget", "name frames kw count")
BUDGET = (
    Budget("16-levels", (lambda: texture(400, 300, 5), lambda: texture(200, 150, 5)),
           dict(nlevels=16, scale_factor=1.1, nfeatures=16, edge_threshold=ET), 17),
    Budget("12-levels", (lambda: texture(400, 300, 5),),
           dict(nlevels=12, scale_factor=1.2, nfeatures=24, edge_threshold=ET), 25),
)

# ---------------------------------------------------------------- match cases
MATCH_NQ = (1, 63, 64, 65)
MATCH_NT = (0, 1, 2, 63, 64, 65, 256, 257, 769, 4096, 4097)
# what the planner must say: nt -> (nseg, seg, empty trailing segments, size of the last used one)
MATCH_PLAN = {769: (4, 256, 0, 1), 4097: (16, 320, 3, 257), 4096: (16, 256, 0, 256), 257: (2, 192, 0, 65),
              256: (1, 256, 0, 256), 0: (1, 64, 0, 0)}


def descriptors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32)).astype(np.uint8)


MATCH_DUP_NT = 600   # 3 segments of 256: tiles end at 64, 128, ...; segments at 256, 512
# (lower, higher) train rows made equal: inside one LDS tile, across a tile boundary, across a
# segment boundary
MATCH_DUPS = ((5, 40), (63, 64), (255, 256))


def match_dup_case():
    """(query, train, dups): train rows `higher` copy rows `lower`; query i is that row."""
    t = descriptors(MATCH_DUP_NT, 31)
    for lo, hi in MATCH_DUPS:
        t[hi] = t[lo]
    return np.stack([t[lo] for lo, _ in MATCH_DUPS]), t, MATCH_DUPS


# ---------------------------------------------------------------- alignment cases
Align = namedtuple("Align", "name frames kw outcome n_good")


def shift_pair():
    """(frame1 200 x 160, frame0 260 x 190): frame1(p) = frame0(p + (14.5, 9.25))."""
    base = synth.base_texture(400, 300, seed=77)
    f0 = np.clip(np.rint(base[:190, :260]), 0, 255).astype(np.uint8)
    ys, xs = np.mgrid[0:160, 0:200].astype(np.float64)
    return sampled(base, xs + 14.5, ys + 9.25), f0


def swapped_pair():
    """The same frames the other way round: more queries than train rows - 1, so the
    reference's min(train rows - 1, queries) loop bound leaves the last queries out."""
    f1, f0 = shift_pair()
    return f0, f1


def zoom_pair():
    """frame1 = a 1.3 x zoom of frame0: the homography's scale fails the 20 % check."""
    base = synth.base_texture(400, 300, seed=77)
    ys, xs = np.mgrid[0:300, 0:400].astype(np.float64)
    return sampled(base, xs * 1.3, ys * 1.3), np.clip(np.rint(base), 0, 255).astype(np.uint8)


def budget_pair():
    b = BUDGET[0]
    return b.frames[1](), b.frames[0]()


def budget_same():
    f = BUDGET[0].frames[0]()
    return f, f


ALIGN = (
    Align("shift-ransac", shift_pair, dict(method=8), 0, 472),
    Align("shift-lmeds", shift_pair, dict(method=4), 0, 472),
    Align("shift-ransac-et16", shift_pair, dict(method=8, edge_threshold=ET), 0, 1029),
    Align("shift-lmeds-et16", shift_pair, dict(method=4, edge_threshold=ET), 0, 1029),
    Align("swapped-ransac", swapped_pair, dict(method=8), 0, 258),
    Align("swapped-lmeds", swapped_pair, dict(method=4), 0, 258),
    Align("swapped-ransac-et16", swapped_pair, dict(method=8, edge_threshold=ET), 0, 633),
    Align("swapped-lmeds-et16", swapped_pair, dict(method=4, edge_threshold=ET), 0, 633),
    Align("zoom", zoom_pair, dict(), 2, 953),
    # the 16-level budget set: 17 keypoints a frame where nfeatures is 16
    Align("budget-16-levels", budget_pair, BUDGET[0].kw, 1, 1),
    Align("budget-16-levels-same", budget_same, BUDGET[0].kw, 0, 16),
)
ALIGN_SWAPPED = tuple(a.name for a in ALIGN if a.name.startswith("swapped"))
# the shift and swapped pairs again as pitched views: (ox, oy, PW, PH) of frame1's and frame0's parent
ALIGN_PITCHED = tuple(a.name for a in ALIGN if a.name.startswith(("shift", "swapped")))
ALIGN_PARENTS = ((5, 3, 300, 200), (2, 7, 277, 211))

# ---------------------------------------------------------------- warp cases
# name, (sw, sh), (dw, dh), M (2x3), src row padding, dst row padding
Warp = namedtuple("Warp", "name ssize dsize M spad dpad")
_HALF = [[1, 0, 0.5], [0, 1, -0.5]]
_ROTZOOM = [[1.02 * np.cos(0.05), -1.02 * np.sin(0.05), 2.25], [1.02 * np.sin(0.05), 1.02 * np.cos(0.05), -1.5]]
WARP = tuple(
    # every block edge of the 64 x 4 launch: dw in {1, 63, 64, 65} x dh in {1, 3, 4, 5}
    [Warp(f"{dw}x{dh}", (70, 9), (dw, dh), _ROTZOOM, 3, 5) for dw in (1, 63, 64, 65) for dh in (1, 3, 4, 5)]
    + [Warp("src-1x1", (1, 1), (5, 3), [[1, 0, 2], [0, 1, 1]], 2, 1),
       Warp("src-1x1-half", (1, 1), (5, 3), [[1, 0, 1.5], [0, 1, 0.5]], 2, 1),
       Warp("shift-int", (65, 17), (65, 17), [[1, 0, 3], [0, 1, -2]], 7, 1),
       Warp("shift-half", (65, 17), (65, 17), _HALF, 7, 1),
       Warp("rot-zoom", (129, 67), (131, 70), _ROTZOOM, 0, 13),
       # det = 0: the inverse is all zero and every px samples src(0, 0)
       Warp("singular", (33, 9), (65, 5), [[1, 2, 3], [2, 4, -1]], 1, 3),
       Warp("far+", (33, 9), (65, 5), [[1, 0, 1e6], [0, 1, 1e6]], 1, 3),
       Warp("far-", (33, 9), (65, 5), [[1, 0, -1e6], [0, 1, -1e6]], 1, 3)])
WARP_SENTINEL = 0xA5

# tvl1_postprocess_affine: name, (W, H), M, flow row padding (floats), I1 row padding; each runs
# with flow_output 0 and 1.  I1 rows 0 and 1 (where H allows) are all 0 and all 1: masked; every
# row has scattered 0 and 1 px besides.
Post = namedtuple("Post", "name size M fpad ipad")
_PM = [[1.01, 0.02, 1.75], [-0.015, 0.99, -0.5]]
POST = tuple([Post(f"{w}x{h}", (w, h), _PM if w > 1 else _HALF, 3, 2) for w in (1, 65) for h in (1, 5)]
             + [Post("pitched-uv", (65, 5), _PM, 9, 0), Post("pitched-I1", (65, 5), _PM, 0, 11),
                Post("67x9-half", (67, 9), _HALF, 1, 1)])
POST_SENTINEL = np.float32(-12345.5)


def post_inputs(case):
    """(u, v, I1) of a post-process case, contiguous."""
    w, h = case.size
    rng = np.random.default_rng(19 + w + 7 * h)
    u = rng.normal(0, 1.5, (h, w)).astype(np.float32)
    v = rng.normal(0, 1.5, (h, w)).astype(np.float32)
    I1 = rng.integers(2, 256, (h, w)).astype(np.uint8)
    I1[:, ::7] = 1
    I1[:, 3::7] = 0
    if h > 2:
        I1[0, :] = 0
        I1[1, :] = 1
    return u, v, I1
