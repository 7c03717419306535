"""The warp loop of the batched solve (csrc/tvl1_batch_walk.hpp) on a CPU model of the device.

walk_batch_level decides, for every pair of a chunk, which u / p set each launch reads, whether p
is still zero, whether the fused first pass stores its constants and who is re-gathered after a
wrong guess, how pairs are grouped by pass length (or clipped to lock step), which partials a
reduce sums and when a residual slot may be read: a slip changes bits or reads a stale residual,
and on the GPU shows only for the residuals a test image happens to produce.  Here
tests/batch_walk_model.cpp, a stand-alone program built with g++ and the host sanitizers (ASan +
UBSan), runs the same template over a symbolic device that follows every pair's buffers (and
exits non-zero on a stale read, a missing constant, a pair listed twice, a reduce over other
partials, a residual read early or twice) through scripted residuals that agree and disagree
from pair to pair and from warp to warp, for the product of scripts x warps x iterations x
epsilon > 0 x fusion x median x grouping x store prediction x chunk size, two levels per run
with the state carried across.  Every pair of every run must

  * run the iterations per warp, and read the residuals at the iteration counts, of OpenCV's
    procOneScale loop on its own script (test_plan_cpu.proc_one_scale_checks), whatever the
    other pairs do;
  * with grouping, run exactly the passes of the single-pair schedule
    (test_walk_cpu.plain_passes with kmax 4); without, those of a lock-step simulation built
    from the open-coded rule the batched solve once had (test_plan_cpu.removed_batch_rule);
  * count as many checks as it read residuals, and as many re-gathers as it has warps > 0 that
    go on past their first check after a warp of exactly 2 iterations (none without fusion or
    store prediction);

and over all runs every branch is reached (asserted at the end).
"""
from __future__ import annotations

import itertools
import subprocess

import numpy as np
import pytest

import batch_walk_cases
from test_plan_cpu import CSRC, DBL_MAX, ROOT, proc_one_scale_checks, removed_batch_rule
from test_residual_margin_cpu import MIN_MARGIN
from test_walk_cpu import ITERATIONS, THR, WARPS, _scripts, plain_passes

KMAX = 4   # kTbMax
NW = 5     # warps per script
# eps_pos, fuse, median, group, store prediction
CONFIGS = list(itertools.product((0, 1), repeat=5))
EVENTS = ("guess_held", "regather", "multi_k_round", "round_without_check", "pair_idle", "non_fused_gather",
          "median")


def _sets(base):
    """Pair scripts of a chunk (pair b reads set[b % len(set)]): every pair alike, and 7 that
    differ, so pairs leave a warp's loop at different iterations and land in different groups."""
    agree = [[base[j]] for j in (3, 9, 21, 41)]
    differ = [[base[(j + 7 * i) % len(base)] for i in range(7)] for j in range(0, 46, 6)]
    return agree + differ


def _rle(tokens):
    out = []
    for tok, grp in itertools.groupby(tokens):
        k = len(list(grp))
        out.append(tok if k == 1 else f"{tok}x{k}")
    return ",".join(out) or "-"


def lock_step(res, thr, iterations, eps_pos):
    """One warp of TVL1_BATCH_GROUP=0 over pairs with the residuals res[i]: every round is one
    launch of the shortest pass any active pair allows; a pair whose own pass is longer runs that
    many iterations without a check.  Returns each pair's passes and how many checks were clipped."""
    m = len(res)
    error, prev, n = [DBL_MAX] * m, [0.0] * m, [0] * m
    out = [[] for _ in range(m)]
    clipped = 0
    while True:
        act = [i for i in range(m) if error[i] > thr and n[i] < iterations]
        if not act:
            return out, clipped
        own = {i: removed_batch_rule(prev[i], thr, n[i], iterations, eps_pos, KMAX) for i in act}
        kmin = min(k for k, _, _ in own.values())
        for i in act:
            k, ends, pe = removed_batch_rule(prev[i], thr, n[i], iterations, eps_pos, KMAX, kmin)
            assert k == kmin
            clipped += own[i][1] and not ends
            n[i] += k
            out[i].append(f"{k}c" if ends else str(k))
            error[i], prev[i] = DBL_MAX, pe
            if ends:
                error[i] = prev[i] = res[i][n[i]]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_walk")
    exe = d / "batch_walk_model"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "batch_walk_model.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        cases = d / "cases.txt"
        cases.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a model or sanitizer report
        return r.stdout.splitlines()

    return run


def _expect(pset, n, warps, iterations, eps_pos, fuse, group, store):
    """Per pair class (pair b is class b % len(pset)): what the model must print for it, and the
    checks the lock step clipped."""
    m = min(n, len(pset))
    res = [[[0.0] + [r * THR for r in s] for s in pset[i]] for i in range(m)]
    fused = fuse and eps_pos and iterations >= 2
    iters, reads, passes = [[] for _ in range(m)], [[] for _ in range(m)], [[] for _ in range(m)]
    clipped = 0
    for lw in range(2 * warps):   # two levels
        w = lw % NW
        if not group:
            ls, c = lock_step([res[i][w] for i in range(m)], THR, iterations, eps_pos)
            clipped += c
        for i in range(m):
            checks, nit = proc_one_scale_checks(res[i][w], THR, iterations, eps_pos)
            iters[i].append(nit)
            reads[i].append(_rle(str(b - a) for a, b in zip([0] + checks, checks)))
            if group:
                p = plain_passes(res[i][w], THR, iterations, eps_pos, KMAX)
                passes[i].append(_rle(p.split(",")) if p else "-")
            else:
                passes[i].append(_rle(ls[i]))
    out = []
    for i in range(m):
        nchecks = sum(len(proc_one_scale_checks(res[i][lw % NW], THR, iterations, eps_pos)[0])
                      for lw in range(2 * warps))
        regathers = sum(iters[i][lv * warps + wp - 1] == 2 and iters[i][lv * warps + wp] > 2
                        for lv in range(2) for wp in range(1, warps)) if fused and store else 0
        out.append(" | ".join((" ".join(map(str, iters[i])), " ".join(reads[i]), " ".join(passes[i]),
                               f"{nchecks} {regathers}")))
    return out, clipped


def test_walk_batch_level_follows_procOneScale_for_every_pair_through_every_branch(model):
    lines, want = [], []

    def add(pset, n, warps, cfg, iterations):
        eps_pos, fuse, median, group, store = cfg
        lines.append(f"run {n} {warps} {eps_pos} {fuse} {median} {group} {store}")
        want.append((n, len(pset)) + _expect(pset, n, warps, iterations, eps_pos, fuse, group, store))

    for iterations in ITERATIONS:
        sets = _sets(_scripts(iterations))
        for k, pset in enumerate(sets):
            lines.append(f"script {THR.hex()} {len(pset)} {NW} {iterations} " +
                         " ".join(r.hex() for sc in pset for s in sc for r in s))
            # 65 pairs (a second BatchMask word) with sets whose pairs differ
            for n in (1, 3, 65) if k in (4, 7, 10) else (1, 3):
                for warps, cfg in itertools.product(WARPS, CONFIGS):
                    add(pset, n, warps, cfg, iterations)
            if k == 5 and iterations == 7:   # index 255 of idx, and the last mask word
                add(pset, 256, 2, (1, 1, 0, 1, 1), iterations)
    assert len(want) == len(ITERATIONS) * (12 * 2 + 3) * len(WARPS) * len(CONFIGS) + 1
    out = model(lines)
    assert len(out) == len(want)
    runs = [ln for ln in lines if ln.startswith("run")]
    seen = dict.fromkeys(EVENTS + ("clipped_check",), 0)
    for ln, o, (n, ns, pairs, clipped) in zip(runs, out, want):
        head, *got = (f.strip() for f in o.split(";"))
        assert len(got) == n, ln
        for b, g in enumerate(got):
            assert g == pairs[b % ns], (ln, b)
        ev = dict(zip(EVENTS, (int(x) for x in head.split())))
        _, _, _, fuse, median, group, store = (int(x) for x in ln.split()[1:])
        if not (fuse and store):
            assert ev["guess_held"] == 0 and ev["regather"] == 0, ln
        assert ev["regather"] == sum(int(g.rsplit(" ", 1)[1]) for g in got), ln
        assert (ev["median"] > 0) == bool(median), ln
        if group:
            assert clipped == 0
        seen["clipped_check"] += clipped
        for k in EVENTS:
            seen[k] += ev[k]
    print(seen)
    # a store guess that held; one that missed and was re-gathered; a round of two or more pass
    # lengths; a lock-step clip that removed a check; a round without any check; a pair idle
    # while others run; the non-fused path; the median
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("ch", batch_walk_cases.CHUNKS, ids=batch_walk_cases.chunk_id)
def test_recorded_chunks_disagree_regather_and_clear_their_thresholds(built, ch):
    """What the chunks of tests/golden/batch_walk_sequence.json were picked for, with the oracle:
    at least two pairs with different per-warp iteration counts, a pair with a warp > 0 that goes
    on after a warp of exactly 2 iterations (the re-gather), and every stopping decision at least
    MIN_MARGIN from its threshold, so that the engine's sums decide every check as the oracle's."""
    from optflow_amd import capi
    from oracle import checker
    p = capi.make_params(**ch["params"])
    I0s, I1s = batch_walk_cases.chunk_pairs(ch)
    counts, regathers = set(), 0
    for b in range(len(I0s)):
        _, _, st, wi, tr = checker.oracle_check_trace(I0s[b], I1s[b], p)
        assert checker.check_margins(tr, p.iterations).min() >= MIN_MARGIN, (b, ch["seeds"][b])
        wi = np.asarray(wi)[: st["levels"]]
        counts.add(tuple(int(x) for x in wi.ravel()))
        regathers += int(((wi[:, :-1] == 2) & (wi[:, 1:] > 2)).sum())
    assert len(counts) >= 2 and regathers >= 1, (counts, regathers)
