"""The optflow CLI's `initialFlow` key end to end: a pair whose frame1 is frame0 shifted by
(12, -9) px, solved from that drift as the seed.  The written TIFFs must be the seeded
reference (tests/initflow_ref.py) plus the reference's post-ops, bit for bit; the same config
without the key must write what it always wrote (the oracle's unseeded solve)."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import initflow_ref as ref
from optflow_amd import capi
from oracle import checker

pytestmark = pytest.mark.gpu
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
C = ref.CLI


@pytest.fixture
def pair(tmp_path, built):
    I0, I1 = ref.shifted_pair(C["w"], C["h"], C["rng"], *C["shift"])
    Image.fromarray(I0).save(tmp_path / "p.png")
    Image.fromarray(I1).save(tmp_path / "q.png")
    return I0, I1


def config(tmp_path, **extra):
    """The shape of the reference's docs/example.json (tests/golden/reference_example.json):
    its global keys and one image entry; feature alignment off and the frame as one ROI, since
    a seeded pair is not pre-aligned."""
    return {"debug": False, "style": 1, "features": False, "homo": 4, "ratio": 0.7, "ransac": 5.0,
            "hessianThreshold": 1600,
            "images": [{"p": str(tmp_path / "p.png"), "q": str(tmp_path / "q.png"),
                        "output_name": "json_test", "hessianThreshold": 1600}],
            "output_type": "flow", "scale": 1, "output_dir": str(tmp_path),
            "rois": {"custom": [0, 0, C["w"], C["h"]]}, "stats_json": str(tmp_path / "stats.json"),
            **extra}


def run_cli(cfg, tmp_path):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Error" not in r.stderr, r.stderr
    tif = lambda s: np.array(Image.open(tmp_path / f"json_test_1.00_{s}.tiff")).astype(np.float32)
    return tif("x"), tif("y"), json.loads((tmp_path / "stats.json").read_text())


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def test_seeded_cli_writes_the_seeded_reference(tmp_path, pair):
    I0, I1 = pair
    dx, dy = C["shift"]
    x, y, stats = run_cli(config(tmp_path, useInitialFlow=True, initialFlow=[dx, dy]), tmp_path)
    p = capi.make_params()
    u, v, wr, _ = ref.seeded_calc(I0, I1, p, np.full(I0.shape, dx, np.float32),
                                  np.full(I0.shape, dy, np.float32))
    ur, vr = ref.postprocess(u, v, I1, 0)
    assert bits_equal(x, ur) and bits_equal(y, vr)
    solve = stats[0]["solves"][0]
    assert solve["initial_flow"] == [dx, dy]
    assert solve["warp_iterations"] == wr.ravel().tolist()
    # the seed is the true translation: away from the wrapped border the flow stays on it
    assert abs(float(np.median(x)) - dx) < 0.5 and abs(float(np.median(y)) - dy) < 0.5


@pytest.mark.parametrize("extra", [dict(useInitialFlow=True), dict(initialFlow=[12, -9]), {}],
                         ids=["flag_alone", "key_alone", "neither"])
def test_unseeded_cli_is_unchanged(tmp_path, pair, extra):
    I0, I1 = pair
    x, y, stats = run_cli(config(tmp_path, **extra), tmp_path)
    u, v, _, wr = checker.oracle_calc(I0, I1, capi.make_params())
    ur, vr = ref.postprocess(u, v, I1, 0)
    assert bits_equal(x, ur) and bits_equal(y, vr)
    assert "initial_flow" not in stats[0]["solves"][0]
    assert stats[0]["solves"][0]["warp_iterations"] == wr.ravel().tolist()
