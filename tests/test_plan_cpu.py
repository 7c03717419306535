"""The host planner (csrc/tvl1_plan.hpp) pinned on the CPU.

Segmentation and speculation never change a result, so the GPU parity tests cannot see a slip
in roll_segment, a bands formula or the schedule: it would only make the engine slower.  Here
tests/plan_dump.cpp, a stand-alone program that includes only tvl1_plan.hpp, is built with g++
and the host sanitizers (ASan + UBSan) and must

  * reproduce tests/golden/plan_table.json, the launch-plan numbers recorded from the engine's
    own functions before the header existed (every launch site, blocked-pass geometry,
    partial capacities, pyramid sizes; the 11232 + 1920 site and roll_segment cases as one
    SHA-256 per site and level size, with a readable part spelled out);
  * schedule a warp's residual checks exactly where a direct transcription of OpenCV's
    procOneScale loop (below, in Python) evaluates the residual;
  * give the batched solve the pass lengths and prevError of the open-coded loop it replaced;
  * never plan more wavefronts or blocks than the partial capacity reserved for the frame.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import math
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fibsem-optflow_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "plan_table.json"
DBL_MAX = 1.7976931348623157e308


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """Runs plan_dump on a list of case lines and returns its output lines."""
    d = tmp_path_factory.mktemp("plan")
    exe = d / "plan_dump"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "plan_dump.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        cases = d / "cases.txt"
        cases.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a sanitizer report fails here
        out = r.stdout.splitlines()
        assert len(out) == len(lines), (len(out), len(lines))
        return out

    return run


@pytest.fixture(scope="module")
def table():
    return json.loads(GOLDEN.read_text())


def _ints(line):
    return [int(x) for x in line.split()]


def test_plan_header_is_plain_cxx():
    """No HIP header: the planner and the level walkers compile with any C++17 compiler."""
    for name in ("tvl1_plan.hpp", "tvl1_walk.hpp", "tvl1_batch_walk.hpp"):
        text = (CSRC / name).read_text()
        assert "hip/" not in text and "__global__" not in text


def _digest(lines):
    return hashlib.sha256(("\n".join(sorted(lines)) + "\n").encode()).hexdigest()


def test_roll_segment_matches_golden(dump, table):
    d = table["dims"]
    cases = [(b, h, k, s) for _, h in d["sizes"] for b in d["roll_segment_bands"] for k in d["roll_segment_k"]
             for s in d["slots"]]
    assert len(cases) == 1920
    out = dump(["seg %d %d %d %d" % c for c in cases])
    got = {c: int(o) for c, o in zip(cases, out)}
    for r in table["roll_segment_rows"]:
        assert got[tuple(r[:4])] == r[4], r
    groups = {}
    for c, o in got.items():
        groups.setdefault(f"rows {c[1]}", []).append("%d %d %d %d " % c + str(o))
    assert {g: _digest(v) for g, v in groups.items()} == table["roll_segment_digests"]


def _site_cases(d):
    """Every launch site over the table's dimensions: (site, w, h, k, px, slots, fill, roll_seg,
    pairs, seg_min).  A single-pair site takes fill and TVL1_ROLL_SEG; the batched gathers and
    fused passes take neither; the batched passes take TVL1_ROLL_SEG and TVL1_BATCH_SEG_MIN."""
    for (w, h), sl in itertools.product(d["sizes"], d["slots"]):
        for fill, seg in itertools.product(d["fill"], d["roll_seg"]):
            yield ("warp_ring", w, h, 6, 0, sl, fill, seg, 1, 0)
            yield ("warp_iter", w, h, 8, 0, sl, fill, seg, 1, 0)
            for k, px in itertools.product(d["k"], d["px"]):   # k_iterate_roll_mid: k 4, px 2
                yield ("roll", w, h, k, px, sl, fill, seg, 1, 0)
        for n in d["pairs"]:
            yield ("kb_warp_iter", w, h, 8, 0, sl, 100, 0, n, 0)
            yield ("kb_warp_ring", w, h, 6, 0, sl, 100, 0, n, 0)
            for seg, k, px, mn in itertools.product(d["roll_seg"], d["k"], d["batched_px"], d["seg_min"]):
                yield ("kb_roll", w, h, k, px, sl, 100, seg, n, mn)


def test_launch_sites_match_golden(dump, table):
    """bands, segment rows and wavefronts of every launch site: sizes x slots x fill x
    TVL1_ROLL_SEG x k x px x batch size (x TVL1_BATCH_SEG_MIN for the batched passes)."""
    cases = list(_site_cases(table["dims"]))
    assert len(cases) == len(set(cases)) == 11232
    out = dump(["site " + " ".join(str(x) for x in c) for c in cases])
    got = {c: _ints(o) for c, o in zip(cases, out)}
    assert len(table["site_rows"]) == 96
    for r in table["site_rows"]:   # the readable part first: a mismatch names its case
        assert got[tuple(r[:10])] == r[10:], r
    groups = {}
    for c, o in got.items():
        groups.setdefault(f"{c[0]} {c[1]}x{c[2]}", []).append(" ".join(str(x) for x in c + tuple(o)))
    bad = {g: sorted(v)[:3] for g, v in groups.items() if _digest(v) != table["site_digests"].get(g)}
    assert not bad and len(groups) == len(table["site_digests"]) == 48, bad


def test_blocked_capacity_pyramid_match_golden(dump, table):
    out = dump([f"blocked {r[0]} {r[1]} {r[2]}" for r in table["blocked"]])
    assert [_ints(o) for o in out] == [r[3:] for r in table["blocked"]]
    out = dump([f"cap {r[0]} {r[1]}" for r in table["capacity"]])
    assert [_ints(o) for o in out] == [r[2:] for r in table["capacity"]]
    sizes = {(r[0], r[1]) for r in table["pyramid"]}
    for p in (ROOT / "tests" / "golden").glob("pair_*.npz"):   # every golden pair's size is covered
        w, h = p.name.split("_")[1].split("x")
        assert (int(w), int(h)) in sizes, p.name
    out = dump([f"pyr {r[0]} {r[1]} {r[2]} {r[3]}" for r in table["pyramid"]])
    assert [_ints(o) for o in out] == [r[4:] for r in table["pyramid"]]


# ---- sched_after against procOneScale

def proc_one_scale_checks(res, thr, iterations, eps_pos):
    """OpenCV 3.4.1 OpticalFlowDual_TVL1 procOneScale's inner loop, transcribed:
        for (n = 0; error > scaledEpsilon && n < iterations; ++n) {
            calcError = epsilon > 0 && (n & 1) && prevError < scaledEpsilon;
            estimateU(..., calcError);
            if (calcError) { error = sum(diff); prevError = error; }
            else { error = DBL_MAX; prevError -= scaledEpsilon; }
            estimateDualVariables(...);
        }
    res[m]: the residual after m iterations.  Returns the iteration counts at which the
    residual was evaluated, and the iterations run."""
    error, prev, checks, n = DBL_MAX, 0.0, [], 0
    while error > thr and n < iterations:
        calc = bool(eps_pos) and bool(n & 1) and prev < thr
        if calc:
            error = res[n + 1]
            prev = error
            checks.append(n + 1)
        else:
            error = DBL_MAX
            prev -= thr
        n += 1
    return checks, n


def _residual_sequences(n):
    """Synthetic residuals in units of the threshold, by iteration count 1..n."""
    seqs = []
    for e0, f in itertools.product((50.0, 3.7, 1.5, 1.0000001, 0.5), (0.5, 0.9, 0.97, 1.0)):
        seqs.append([e0 * f ** m for m in range(1, n + 1)])
    seqs.append([1.3 if m % 4 else 0.99 for m in range(1, n + 1)])       # dips below now and then
    seqs.append([2.0 + math.sin(m) for m in range(1, n + 1)])            # never converges
    seqs.append([6.5 if m < 40 else 0.2 for m in range(1, n + 1)])       # long unchecked runs, then a stop
    return seqs


def test_sched_after_checks_where_procOneScale_does(dump):
    thr = 0.01 * 0.01 * 97 * 61   # eps^2 W H (inexact in binary)
    cases, want = [], []
    for iterations, kmax, eps_pos in itertools.product((0, 1, 2, 3, 7, 300), (1, 4), (0, 1)):
        for seq in _residual_sequences(max(iterations, 1)):
            res = [0.0] + [r * thr for r in seq]
            cases.append(f"warp {thr.hex()} {iterations} {kmax} {eps_pos} " + " ".join(r.hex() for r in seq))
            want.append(proc_one_scale_checks(res, thr, iterations, eps_pos))
    assert len(cases) == 6 * 2 * 2 * 23
    out = dump(cases)
    for c, o, (checks, n) in zip(cases, out, want):
        left, right = o.split("|")
        assert (_ints(left), int(right)) == (checks, n), c[:80]
    assert any(len(w[0]) > 3 for w in want) and any(not w[0] for w in want)


def removed_batch_rule(prev, thr, nit, iterations, eps_pos, kmax, kmin=None):
    """The batched solve's open-coded pass rule, as it stood before it called sched_after:
    a pair's pass length, whether it ends in a check, and prevError after the pass.  kmin: the
    lock-step clip of TVL1_BATCH_GROUP=0 (the pass cut to the shortest of the batch)."""
    k, ends, ps = 0, False, prev
    while k < kmax and nit + k < iterations:
        ce = bool(eps_pos) and bool((nit + k) & 1) and ps < thr
        k += 1
        if ce:
            ends = True
            break
        ps -= thr
    if kmin is not None and k > kmin:
        k, ends = kmin, False
    for i in range(k):
        if not (ends and i == k - 1):
            prev -= thr
    return k, ends, prev


def test_batched_rule_equals_the_removed_loop(dump):
    thr = 0.01 * 0.01 * 128 * 96 + 1e-13   # repeated subtraction of it is inexact
    prevs = [0.0, 0.3, thr, thr * 1.7 + 1e-3, thr * 2.9999999, thr * 3.1, 50.3 * thr, -thr, 0.1 + 0.2]
    prevs += [thr * (7.3 + 0.37 * i) + 0.1 for i in range(24)] + [1e3 * thr + 0.1, 1e9 * thr + 0.7]
    cases, want = [], []
    for prev, nit, iterations, eps_pos in itertools.product(prevs, (0, 1, 2, 5, 298), (1, 2, 3, 7, 300), (0, 1)):
        if nit >= iterations:
            continue   # an active pair has iterations left
        k, ends, pe = removed_batch_rule(prev, thr, nit, iterations, eps_pos, 4)
        cases.append(f"sched {prev.hex()} {thr.hex()} {nit} {iterations} 4 {eps_pos}")
        want.append((k, int(ends), pe))
        for kmin in range(1, k):   # lock step: sched_after with kmax = kmin
            kc, ec, pc = removed_batch_rule(prev, thr, nit, iterations, eps_pos, 4, kmin)
            assert (kc, ec) == (kmin, False)
            cases.append(f"sched {prev.hex()} {thr.hex()} {nit} {iterations} {kmin} {eps_pos}")
            want.append((kc, 0, pc))
    out = dump(cases)
    inexact = 0
    for c, o, (k, ends, pe) in zip(cases, out, want):
        ko, eo, po = o.split()
        assert (int(ko), int(eo)) == (k, ends), c
        assert float.fromhex(po) == pe, (c, po, pe.hex())
        prev = float.fromhex(c.split()[1])
        inexact += pe != prev - (k - ends) * thr
    assert inexact > 0   # the order of the subtractions mattered in some case


# ---- capacity

def test_plans_stay_within_the_reserved_partials(dump):
    """Every wavefront / block count (the mid-check pass: 2 x wavefronts) of every launch site,
    k, px and TVL1_ROLL_SEG, single and batched, for every frame of 1..700 x 1..200 px and the
    large sizes of the golden table, against partials_capacity / batch_partials_capacity of
    that frame: the condition behind the engine's `internal: ... > partials capacity` errors."""
    large = [(1573, 51), (2048, 1536), (6144, 4096)]
    out = dump(["capsweep 1 700 1 200"] + [f"capsweep {w} {w} {h} {h}" for w, h in large])
    per_size = 1 + 8 + 9 * (2 + 12 + 1 + 2 * (2 + 16))
    assert _ints(out[0]) == [700 * 200 * per_size, 0]
    for o in out[1:]:
        assert _ints(o) == [per_size, 0]
