"""The warp loop of the single-pair solve (csrc/tvl1_walk.hpp) on a CPU model of the device.

walk_level decides which buffer sets every launch reads, which constants are current and which
check the host waits for, with speculation and mid-check passes interleaved: a slip changes bits
or hangs, and on the GPU shows only for the residuals a test image happens to produce.  Here
tests/walk_model.cpp, a stand-alone program built with g++ and the host sanitizers (ASan +
UBSan), runs the same template over a symbolic device that follows every buffer set (and exits
non-zero on a stale read, a wait for a check that never ran, or a missed guess not rolled back)
through scripted residuals, for the product of residual scripts x warps x iterations x kmax x
epsilon > 0 x fusion x median x speculation x mid-check passes.  Every run must

  * give each warp the iterations, and read the residuals at the iteration counts, of OpenCV's
    procOneScale loop (test_plan_cpu.proc_one_scale_checks, transcribed in Python);
  * without mid-check passes, run exactly the passes of the plain schedule (the open-coded rule
    of test_plan_cpu.removed_batch_rule), whatever was enqueued ahead and ran empty;
  * count what the device saw: checks, wrong guesses, mid-check passes.

and over all runs every branch is reached (asserted at the end, so the test cannot pass by
never speculating).
"""
from __future__ import annotations

import itertools
import subprocess

import pytest

from test_plan_cpu import CSRC, ROOT, _residual_sequences, proc_one_scale_checks, removed_batch_rule

THR = 0.01 * 0.01 * 97 * 61   # eps^2 W H (inexact in binary)
WARPS = (1, 2, 5)
ITERATIONS = (1, 2, 3, 7, 300)
# kmax, eps_pos, fuse, median, speculation (0 off, 1 alone, 2 not alone), (mid, mid_min)
CONFIGS = list(itertools.product((1, 4), (0, 1), (0, 1), (0, 1), (0, 1, 2), ((0, 1.1), (1, 1.0), (1, 1.1))))
EVENTS = ("stop_right", "stop_wrong", "stop_wrong_regather", "cont_right", "cont_wrong", "chain_same",
          "chain_next", "mid", "mid_continued", "mid_retaken", "mid_speculating")


def _scripts(n):
    """Residuals of 5 warps by iteration count 1..n, in units of the threshold: every sequence
    for all warps alike (the predictor's "as the previous warp did" holds), and scaled per warp
    so that consecutive warps stop at other counts (it does not)."""
    out = []
    for seq in _residual_sequences(n):
        out.append([seq] * 5)
        out.append([[r * f for r in seq] for f in (1.0, 0.6, 1.5, 1.5, 0.45)])
    return out


def plain_passes(res, thr, iterations, eps_pos, kmax):
    """The passes of a warp without speculation or mid-check passes: 'k' or 'kc' (ends in a check)."""
    error, prev, n, out = 1.7976931348623157e308, 0.0, 0, []
    while error > thr and n < iterations:
        k, ends, prev = removed_batch_rule(prev, thr, n, iterations, eps_pos, kmax)
        n += k
        out.append(f"{k}c" if ends else str(k))
        error = 1.7976931348623157e308
        if ends:
            error = prev = res[n]
    return ",".join(out)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk")
    exe = d / "walk_model"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "walk_model.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        cases = d / "cases.txt"
        cases.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a model or sanitizer report
        return r.stdout.splitlines()

    return run


def test_walk_level_follows_procOneScale_through_every_branch(model):
    lines, want = [], []
    for iterations in ITERATIONS:
        for script in _scripts(iterations):
            lines.append(f"script {THR.hex()} 5 {iterations} " + " ".join(r.hex() for s in script for r in s))
            res = [[0.0] + [r * THR for r in s] for s in script]
            for warps, eps_pos in itertools.product(WARPS, (0, 1)):
                per_warp = [proc_one_scale_checks(res[w], THR, iterations, eps_pos) for w in range(warps)]
                iters = " ".join(str(n) for _, n in per_warp)
                reads = " ".join(f"{w}:{n}" for w, (checks, _) in enumerate(per_warp) for n in checks)
                total = sum(n for _, n in per_warp)
                nchecks = sum(len(c) for c, _ in per_warp)
                for kmax in (1, 4):
                    passes = " ".join(plain_passes(res[w], THR, iterations, eps_pos, kmax) for w in range(warps))
                    for cfg in CONFIGS:
                        if cfg[0] != kmax or cfg[1] != eps_pos:
                            continue
                        _, _, fuse, median, spec, (mid, mid_min) = cfg
                        lines.append(f"run {warps} {kmax} {eps_pos} {fuse} {median} {spec} {mid} {mid_min.hex()}")
                        want.append((iters, reads, total, nchecks, passes))
    assert len(want) == len(ITERATIONS) * 46 * len(WARPS) * len(CONFIGS)
    out = model(lines)
    assert len(out) == len(want)
    runs = [ln for ln in lines if ln.startswith("run")]
    seen = dict.fromkeys(EVENTS, 0)
    for ln, o, (iters, reads, total, nchecks, passes) in zip(runs, out, want):
        flags, o_iters, o_reads, o_total, o_counts, o_passes, o_ev = (f.strip() for f in o.split("|"))
        spec, mid = (int(x) for x in flags.split())
        assert (o_iters, o_reads, int(o_total)) == (iters, reads, total), ln
        ev = dict(zip(EVENTS, (int(x) for x in o_ev.split())))
        checks, misses, mid_passes, mid_taken = (int(x) for x in o_counts.split())
        assert checks == nchecks, ln
        assert misses == ev["stop_wrong"] + ev["cont_wrong"], ln
        assert (mid_passes, mid_taken) == (ev["mid"], ev["mid_retaken"]), ln
        assert ev["mid"] == ev["mid_continued"] + ev["mid_retaken"], ln
        if not spec:
            assert misses == 0 and not any(ev[k] for k in EVENTS[:7]), ln
        if not mid:
            assert mid_passes == 0 and o_passes == passes, ln
        for k in EVENTS:
            seen[k] += ev[k]
    print(seen)
    # a right stop guess; a wrong one followed by a re-gather; a right and a wrong continue guess;
    # a chained speculative check that became the next pending one (of the same warp, and of the
    # next); a mid pass that continued, one that ended on its mid state, one in a speculating run
    assert all(seen[k] > 0 for k in EVENTS), seen
