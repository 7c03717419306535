"""The planner of k_iterate_stages (csrc/tvl1_plan.hpp: plan_stages, stages_r0, stages_steps,
stages_hbm) pinned on the CPU.

tests/stages_plan_dump.cpp, a stand-alone program that includes only tvl1_plan.hpp, is built
with g++ and the host sanitizers.  For every level size of the grid, K = 2 and 4, several
resident-slot counts and TVL1_ROLL_SEG settings:
  * the bands' output lanes (the kernel's rule: lanes of the 128-px band inside its halo,
    first px inside the image) cover every column exactly once;
  * the segments cover every row exactly once;
  * a block starts K rows above its segment (clipped) and runs enough steps, in whole trips of
    3, for stage 1 to pass row ye - 1 + K and the last stage -- 2 (K - 1) steps behind -- row
    ye, and no whole trip more;
  * the HBM bytes equal a direct count over bands, segments and planes;
  * the blocks fit the residual partials a frame reserves.
"""
from __future__ import annotations

import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fibsem-optflow_amd" / "csrc"
WIDTHS = [1, 119, 120, 121, 124, 128, 240, 241, 2517]
HEIGHTS = [1, 2, 3, 4, 7, 47, 1678]
SLOTS = [0, 768, 1280]      # 0: unknown (the planner's default), 60 % and all of 5 blocks x 256 CUs
ROLL_SEGS = [0, 8, 34]
BW = 128


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("stages_plan")
    exe = d / "stages_plan_dump"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "stages_plan_dump.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = list(itertools.product(WIDTHS, HEIGHTS, (2, 4), SLOTS, ROLL_SEGS, (0, 1)))
    (d / "cases.txt").write_text("".join(" ".join(map(str, c)) + "\n" for c in cases))
    r = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a sanitizer report fails here
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    res = []
    for c, line in zip(cases, out):
        v = [int(x) for x in line.split()]
        head, segs = v[:8], v[8:]
        assert len(segs) == 4 * head[7]
        res.append((c, head, [tuple(segs[i:i + 4]) for i in range(0, len(segs), 4)]))
    return res


def test_bands_cover_every_column_once(plans):
    for (W, H, K, slots, rs, pz), (bands, seg, waves, out_w, halo, *_), _ in plans:
        assert halo == (K + 1) // 2 * 2 and out_w == BW - 2 * halo
        hits = [0] * W
        for b in range(bands):
            x0 = b * out_w - halo
            for lane in range(64):
                X = x0 + 2 * lane
                if 2 * lane >= halo and 2 * lane < BW - halo and X < W:   # RollLane::out
                    for j in range(2):
                        if X + j < W:   # a second px at x = W lands in the pitch padding
                            assert X + j >= 0
                            hits[X + j] += 1
        assert hits == [1] * W, (W, K, bands)
        assert bands == -(-W // out_w)   # no empty band


def test_segments_cover_every_row_once(plans):
    for (W, H, K, slots, rs, pz), (bands, seg, waves, *_), segs in plans:
        assert seg >= 1
        rows = [0] * H
        for ys, ye, r0, steps in segs:
            assert 0 <= ys < ye <= H
            for y in range(ys, ye):
                rows[y] += 1
        assert rows == [1] * H, (H, seg)
        assert waves == bands * len(segs)
        if rs:
            assert seg == max(rs, 8)   # TVL1_ROLL_SEG, never below the shortest segment


def test_steps_reach_the_last_rows(plans):
    for (W, H, K, slots, rs, pz), _, segs in plans:
        for ys, ye, r0, steps in segs:
            assert r0 == max(ys - K, 0)
            assert steps % 3 == 0
            last = r0 + steps - 1                 # stage 1's last input row
            assert last >= ye - 1 + K             # u^K(ye - 1) ... p^K(ye - 1) depend on it
            assert last - 2 * (K - 1) >= ye       # the last stage's row: p^K(ye - 1) is stored at ye
            assert last - 3 - 2 * (K - 1) < ye    # ... and not a whole trip later


def test_byte_accounting_equals_a_direct_count(plans):
    for (W, H, K, slots, rs, pz), (bands, seg, waves, out_w, halo, hbm, cap, nseg), segs in plans:
        loaded = 0
        for ys, ye, r0, steps in segs:
            first, last = max(ys - K, 0), min(ye - 1 + K, H - 1)   # input rows a stored cell needs
            loaded += bands * BW * (last - first + 1)
        ld_planes = 3 + 2 + (0 if pz else 4)   # constants, u, and p unless it is +0
        st_planes = 2 + 4
        assert hbm == 4 * loaded * ld_planes + 4 * W * H * st_planes, (W, H, K, slots, rs, pz)


def test_blocks_fit_the_partials(plans):
    for (W, H, K, slots, rs, pz), (bands, seg, waves, out_w, halo, hbm, cap, nseg), _ in plans:
        assert waves <= cap, (W, H, K, slots, rs)
