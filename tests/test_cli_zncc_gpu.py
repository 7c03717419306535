"""The CLI's "zncc": every ROI's raw flow is scored by 1 - ZNCC of frame0 against frame1 warped
back along the flow, in the one solve, the flow is zeroed where the score is above beta, and
random_points emits accepted candidates only.  A strip job writes the same bytes batched and
pair by pair, unseeded and seeded; the score plane it writes is tests/zncc_ref.py applied to the
strips and the raw flow; and without the key nothing changes.  "debug" keeps the exact shuffle,
so every run is reproducible."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import zncc_ref as ref
from optflow_amd import capi, synth

pytestmark = pytest.mark.gpu
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
W, H, Z = 200, 120, 4
TOP, BOTTOM = 40, 32
DRIFT = (1, -1)
PAIRS = [(z, z + 1) for z in range(Z - 1)]
PATCH = (60, 6, 96, 30)   # x0, y0, x1, y1 of slice 2's top strip: texture no other slice has
NPOINTS, OVER = 10, 4
RADIUS, BETA = 3, 0.25


@pytest.fixture(scope="module")
def stack(tmp_path_factory, built):
    """Windows of one texture that drift by DRIFT per slice, noise of their own, no px <= 1 (the
    I1 <= 1 mask stays out of the way); slice 2 carries a patch of unrelated texture."""
    d = tmp_path_factory.mktemp("znstack")
    pad = (Z - 1) * max(abs(DRIFT[0]), abs(DRIFT[1]))
    base = synth.base_texture(W + 2 * pad, H + 2 * pad, seed=0xFBC)
    other = synth.base_texture(PATCH[2] - PATCH[0], PATCH[3] - PATCH[1], seed=0x0DD)
    g = np.random.default_rng(7)
    for z in range(Z):
        ox, oy = pad - z * DRIFT[0], pad - z * DRIFT[1]
        a = base[oy:oy + H, ox:ox + W] + g.normal(0.0, 2.0, size=(H, W)).astype(np.float32)
        if z == 2:
            a[PATCH[1]:PATCH[3], PATCH[0]:PATCH[2]] = other
        a = np.clip(np.rint(a), 2, 255).astype(np.uint8)
        Image.fromarray(a).save(d / f"s{z}.tif")
    return d


def job(d, otype, out, pairs=PAIRS, **kw):
    cfg = {"output_dir": str(out), "scale": 1, "output_type": otype, "nscales": 4, "warps": 3,
           "rois": {"top": TOP, "bottom": BOTTOM}, "stats_json": str(out / "stats.json"),
           "npoints": NPOINTS, "debug": True, "inflight": 1,
           "images": [{"p": str(d / f"s{a}.tif"), "q": str(d / f"s{b}.tif"), "pId": f"t{a}",
                       "qId": f"t{b}", "output_name": f"z{a}_{b}"} for a, b in pairs]}
    cfg.update(kw)
    return cfg


def run(cfg, out):
    out.mkdir(exist_ok=True)
    p = out / "cfg.json"
    p.write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads((out / "stats.json").read_text())


def outputs(out):
    return {f.name: f.read_bytes() for f in sorted(out.iterdir())
            if f.suffix == ".tiff" or f.name.startswith("point_matches")}


def tif(path):
    a = np.array(Image.open(path))
    assert a.dtype == np.float32
    return a


def strip(d, z, key):
    a = np.array(Image.open(d / f"s{z}.tif"))
    return a[:TOP] if key == "top" else a[H - BOTTOM:]


def same_bits(a, b):
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


ON = dict(zncc=True, znccOutput=True, znccOversample=OVER)
SEEDS = {"unseeded": {}, "numeric": dict(useInitialFlow=True, initialFlow=[1.0, -1.0], seededStripBatch=True),
         "auto": dict(useInitialFlow=True, initialFlow="auto", seededStripBatch=True)}
COMBOS = [(s, o) for s in SEEDS for o in ("flow", "map", "random_points")]


@pytest.mark.parametrize("seed,otype", COMBOS, ids=[f"{s}-{o}" for s, o in COMBOS])
def test_batched_strips_write_what_the_per_pair_path_writes(stack, tmp_path, seed, otype):
    tj = tmp_path / "timing.json"
    sb = run(job(stack, otype, tmp_path / "b", timing_json=str(tj), **ON, **SEEDS[seed]), tmp_path / "b")
    su = run(job(stack, otype, tmp_path / "u", strip_batch=0, **ON, **SEEDS[seed]), tmp_path / "u")
    ob, ou = outputs(tmp_path / "b"), outputs(tmp_path / "u")
    # per pair and strip: the score plane, and for flow / map the two flow planes
    assert ob.keys() == ou.keys()
    assert len(ob) == (len(PAIRS) * 6 if otype != "random_points" else len(PAIRS) * 2 + 1)
    assert sum(k.endswith("_zncc.tiff") for k in ob) == len(PAIRS) * 2
    for k in ob:
        assert ob[k] == ou[k], k
    rejected = 0
    for eb, eu in zip(sb, su):
        assert eb["ok"] and eu["ok"] and len(eb["solves"]) == len(eu["solves"]) == 2
        for x, y in zip(eb["solves"], eu["solves"]):
            assert x["batch"] == len(PAIRS) and "batch" not in y and x["roi"] == y["roi"]
            assert x["zncc"] == y["zncc"] and "consistency" not in x and "consistency" not in y
            c = x["zncc"]
            assert c["radius"] == RADIUS and c["beta"] == BETA
            assert c["px"] == x["roi"][2] * x["roi"][3] and 0 <= c["rejected_px"] <= c["px"]
            assert ("candidates" in c) == (otype == "random_points")
            assert x.get("initial_flow") == y.get("initial_flow")
            assert ("initial_flow" in x) == (seed != "unseeded")
            rejected += c["rejected_px"]
    assert rejected > 0   # the patch, at least
    assert '"zncc_score"' in tj.read_text() and '"solve_backward"' not in tj.read_text()


def test_score_plane_is_the_restatement_on_the_raw_flow(stack, tmp_path):
    """Raw flows: the same job without the key (no px <= 1, so "flow" output is the solve's own).
    The job with the key must write the restatement's score of the strips under that flow, the
    flow zeroed where it is above beta, and count those px."""
    on = dict(zncc={"radius": 2, "beta": 0.3}, znccOutput=True)
    s = run(job(stack, "flow", tmp_path / "c", **on), tmp_path / "c")
    run(job(stack, "flow", tmp_path / "f"), tmp_path / "f")
    total = inside = 0
    for (a, b), e in zip(PAIRS, s):
        for sv in e["solves"]:
            key = "top" if sv["roi"][1] == 0 else "bottom"
            uf, vf = (tif(tmp_path / "f" / f"z{a}_{b}_1.00_{key}_{c}.tiff") for c in "xy")
            want = ref.zncc_score(strip(stack, a, key), strip(stack, b, key), uf, vf, 2)
            assert same_bits(tif(tmp_path / "c" / f"z{a}_{b}_1.00_{key}_zncc.tiff"), want), (a, b, key)
            wu, wv, wr = ref.zero_above(uf, vf, want, 0.3)
            assert same_bits(tif(tmp_path / "c" / f"z{a}_{b}_1.00_{key}_x.tiff"), wu)
            assert same_bits(tif(tmp_path / "c" / f"z{a}_{b}_1.00_{key}_y.tiff"), wv)
            assert sv["zncc"] == {"radius": 2, "beta": pytest.approx(0.3), "px": want.size, "rejected_px": wr}
            total += wr
            if key == "top" and 2 in (a, b):   # the patch exists in one slice of the pair only
                rej = ~ref.accepted(want, 0.3)
                inside += int(rej[PATCH[1]:PATCH[3], PATCH[0]:PATCH[2]].sum())
    assert total > 0 and inside > 0
    # "map": a rejected px is 0 there too (zeroed after the grid is added)
    run(job(stack, "map", tmp_path / "m", **on), tmp_path / "m")
    for (a, b) in PAIRS:
        for key in ("top", "bottom"):
            rej = ~ref.accepted(tif(tmp_path / "m" / f"z{a}_{b}_1.00_{key}_zncc.tiff"), 0.3)
            mx, my = (tif(tmp_path / "m" / f"z{a}_{b}_1.00_{key}_{c}.tiff") for c in "xy")
            fx = tif(tmp_path / "c" / f"z{a}_{b}_1.00_{key}_x.tiff")
            assert np.all(mx[rej] == 0) and np.all(my[rej] == 0)
            xs = np.arange(W, dtype=np.float32)[None, :]
            assert same_bits(mx[~rej], (fx + xs)[~rej])


def matches(out):
    """Per pair: the emitted points [(x, y, qx, qy)] of point_matches_0.json."""
    recs = json.loads((out / "point_matches_0.json").read_text())
    res = []
    for r in recs:
        m = r["matches"]
        res.append([(int(x), int(y), qx, qy) for x, y, qx, qy, w in
                    zip(m["p"][0], m["p"][1], m["q"][0], m["q"][1], m["w"]) if w])
    return res


def test_random_points_emits_the_first_accepted_candidates(stack, tmp_path):
    """The candidates are the first npoints x oversample px of the shuffle a job without the key
    draws (the same job asked for that many points); the first npoints of them with score <=
    beta are emitted, in order, with the flow they have there."""
    beta = 0.004   # tight enough that candidates fail all over the strips
    on = dict(zncc={"radius": RADIUS, "beta": beta}, znccOutput=True, znccOversample=OVER)
    s = run(job(stack, "random_points", tmp_path / "c", **on), tmp_path / "c")
    run(job(stack, "random_points", tmp_path / "a", npoints=NPOINTS * OVER), tmp_path / "a")
    got, cand = matches(tmp_path / "c"), matches(tmp_path / "a")
    assert len(got) == len(cand) == len(PAIRS)
    dropped = 0
    for (a, b), e, g, c in zip(PAIRS, s, got, cand):
        want = []
        for sv in e["solves"]:   # in the order the strips are drawn
            key, y0 = ("top", 0) if sv["roi"][1] == 0 else ("bottom", H - BOTTOM)
            score = tif(tmp_path / "c" / f"z{a}_{b}_1.00_{key}_zncc.tiff")
            mine = [p for p in c if y0 <= p[1] < y0 + sv["roi"][3]]
            assert len(mine) == NPOINTS * OVER == sv["zncc"]["candidates"]
            ok = [p for p in mine if score[p[1] - y0, p[0]] <= np.float32(beta)]
            assert sv["zncc"]["kept"] == min(NPOINTS, len(ok))
            dropped += len(mine) - len(ok)
            want += ok[:NPOINTS]
        # an accepted px is not zeroed, so its flow is the job's without the key
        assert g == want
    assert dropped > 0


def test_without_the_key_nothing_changes(stack, tmp_path):
    for otype in ("flow", "random_points"):
        run(job(stack, otype, tmp_path / f"n_{otype}"), tmp_path / f"n_{otype}")
        s = run(job(stack, otype, tmp_path / f"o_{otype}", zncc=False, znccOutput=True, znccOversample=9),
                tmp_path / f"o_{otype}")
        a, b = outputs(tmp_path / f"n_{otype}"), outputs(tmp_path / f"o_{otype}")
        assert a.keys() == b.keys() and not any(k.endswith("_zncc.tiff") for k in a)
        assert a == b
        assert all("zncc" not in sv for e in s for sv in e["solves"])


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "per_pair"])
def test_sampled_random_points_gathers_flow_and_score(stack, tmp_path, batched):
    """Without "debug" the px are drawn from the time-seeded generator and only their flow and
    score are read back: whichever px are drawn, each emitted one is accepted and carries the
    flow the dense job writes there."""
    beta = 0.004
    on = dict(zncc={"radius": RADIUS, "beta": beta}, znccOversample=OVER)
    kw = {} if batched else dict(strip_batch=0)
    s = run(job(stack, "random_points", tmp_path / "p", debug=False, **on, **kw), tmp_path / "p")
    run(job(stack, "flow", tmp_path / "d", znccOutput=True, **on), tmp_path / "d")
    assert not any(f.name.endswith("_zncc.tiff") for f in (tmp_path / "p").iterdir())
    got = matches(tmp_path / "p")
    for (a, b), e, g in zip(PAIRS, s, got):
        assert sum(sv["zncc"]["kept"] for sv in e["solves"]) == len(g)
        for sv in e["solves"]:
            c = sv["zncc"]
            assert c["candidates"] == NPOINTS * OVER and 0 <= c["kept"] <= NPOINTS
            key, y0 = ("top", 0) if sv["roi"][1] == 0 else ("bottom", H - BOTTOM)
            score, fx, fy = (tif(tmp_path / "d" / f"z{a}_{b}_1.00_{key}_{n}.tiff") for n in ("zncc", "x", "y"))
            mine = [p for p in g if y0 <= p[1] < y0 + sv["roi"][3]]
            assert len(mine) == c["kept"]
            for x, y, qx, qy in mine:
                assert score[y - y0, x] <= np.float32(beta)
                assert np.float32(qx) == np.float32(x) + fx[y - y0, x]
                assert np.float32(qy) == np.float32(y) + fy[y - y0, x]
