"""The CLI's "seededStripBatch": a strip job whose global config seeds its solves ("initialFlow":
[dx, dy] or "auto" with "useInitialFlow") stays in the strip batch -- tvl1_calc_batch_const_init
/ tvl1_calc_batch_auto_init per ROI key -- and writes what the per-pair seeded path
("strip_batch": 0: tvl1_estimate_shift and tvl1_calc_init per strip) writes: every output file
byte for byte, and per solve the same seed, estimate sums and per-warp iteration counts."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

from optflow_amd import capi, synth

pytestmark = pytest.mark.gpu
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
W, H, Z = 200, 120, 5
TOP, BOTTOM = 40, 32          # "auto" searches 10 px in the top strips, 8 in the bottom ones
DRIFT = (3, -2)               # per slice: inside both ranges for the pairs (z, z + 1), (0, 2)
PAIRS = [(z, z + 1) for z in range(Z - 1)] + [(0, 2)]


@pytest.fixture(scope="module")
def stack(tmp_path_factory, built):
    """Windows of one texture that drift by DRIFT per slice, with noise of their own."""
    d = tmp_path_factory.mktemp("drift")
    pad = (Z - 1) * max(abs(DRIFT[0]), abs(DRIFT[1]))
    base = synth.base_texture(W + 2 * pad, H + 2 * pad, seed=0xD21F7)
    g = np.random.default_rng(99)
    for z in range(Z):
        ox, oy = pad - z * DRIFT[0], pad - z * DRIFT[1]
        a = base[oy:oy + H, ox:ox + W] + g.normal(0.0, 2.0, size=(H, W)).astype(np.float32)
        Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8)).save(d / f"s{z}.tif")
    return d


def job(d, otype, out, seed, **kw):
    cfg = {"output_dir": str(out), "scale": 1, "output_type": otype, "nscales": 5, "warps": 3,
           "rois": {"top": TOP, "bottom": BOTTOM}, "stats_json": str(out / "stats.json"),
           "useInitialFlow": True, "initialFlow": seed, "npoints": 12, "debug": True, "inflight": 1,
           "images": [{"p": str(d / f"s{a}.tif"), "q": str(d / f"s{b}.tif"), "pId": f"t{a}",
                       "qId": f"t{b}", "output_name": f"z{a}_{b}"} for a, b in PAIRS]}
    cfg.update(kw)
    return cfg


def run(cfg, out):
    out.mkdir(exist_ok=True)
    p = out / "cfg.json"
    p.write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r, json.loads((out / "stats.json").read_text())


def outputs(out):
    return {f.name: f.read_bytes() for f in sorted(out.iterdir())
            if f.suffix == ".tiff" or f.name.startswith("point_matches")}


@pytest.mark.parametrize("otype", ["flow", "random_points"])
@pytest.mark.parametrize("seed", [[2.5, -1.75], "auto"], ids=["numeric", "auto"])
def test_seeded_strip_batch_is_the_per_pair_seeded_path(stack, tmp_path, seed, otype):
    rb, sb = run(job(stack, otype, tmp_path / "b", seed, seededStripBatch=True), tmp_path / "b")
    ru, su = run(job(stack, otype, tmp_path / "u", seed, strip_batch=0), tmp_path / "u")
    ob, ou = outputs(tmp_path / "b"), outputs(tmp_path / "u")
    assert ob.keys() == ou.keys() and len(ob) == (len(PAIRS) * 4 if otype == "flow" else 1)
    for k in ob:
        assert ob[k] == ou[k], k
    assert len(sb) == len(su) == len(PAIRS)
    for (a, b), eb, eu in zip(PAIRS, sb, su):
        assert eb["ok"] and eu["ok"] and len(eb["solves"]) == len(eu["solves"]) == 2
        for x, y in zip(eb["solves"], eu["solves"]):
            assert x["batch"] == len(PAIRS) and "batch" not in y
            assert x["roi"] == y["roi"]
            assert x["initial_flow"] == y["initial_flow"]
            assert x.get("initial_flow_auto") == y.get("initial_flow_auto")
            assert x["warp_iterations"] == y["warp_iterations"]
            assert x["iterations"] == y["iterations"] and x["levels"] == y["levels"]
            if seed == "auto":
                assert x["initial_flow_auto"]["max_shift"] == min(32, x["roi"][3] // 4)
                assert x["initial_flow"] == [DRIFT[0] * (b - a), DRIFT[1] * (b - a)]
            else:
                assert x["initial_flow"] == seed and "initial_flow_auto" not in x
    assert sorted(rb.stdout.splitlines()) == sorted(ru.stdout.splitlines())


def test_without_the_key_a_seeded_job_leaves_the_batch(stack, tmp_path):
    _, s = run(job(stack, "flow", tmp_path, "auto"), tmp_path)
    assert all("batch" not in x for e in s for x in e["solves"])
    assert all("initial_flow_auto" in x for e in s for x in e["solves"])


def test_auto_range_below_one_solves_unseeded(stack, tmp_path):
    """initialFlowMaxShift 0: R < 1, tvl1_calc_batch, and the per-pair path's stats entry."""
    kw = dict(initialFlowMaxShift=0)
    _, sb = run(job(stack, "flow", tmp_path / "b", "auto", seededStripBatch=True, **kw), tmp_path / "b")
    _, su = run(job(stack, "flow", tmp_path / "u", "auto", strip_batch=0, **kw), tmp_path / "u")
    assert outputs(tmp_path / "b") == outputs(tmp_path / "u")
    for eb, eu in zip(sb, su):
        for x, y in zip(eb["solves"], eu["solves"]):
            assert x["batch"] == len(PAIRS)
            assert "initial_flow" not in x and "initial_flow" not in y
            assert x["initial_flow_auto"] == y["initial_flow_auto"] == {"max_shift": 0}
