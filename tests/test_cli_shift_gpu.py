"""The optflow CLI's `"initialFlow": "auto"` end to end, on tests/initflow_ref.py's CLI pair
(frame1 = frame0 rolled by (12, -9) px): the drift is found on the GPU (tvl1_estimate_shift) and
the ROI is solved from it exactly as from `"initialFlow": [12, -9]`."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import initflow_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
C = ref.CLI


@pytest.fixture
def pair(tmp_path, built):
    I0, I1 = ref.shifted_pair(C["w"], C["h"], C["rng"], *C["shift"])
    Image.fromarray(I0).save(tmp_path / "p.png")
    Image.fromarray(I1).save(tmp_path / "q.png")
    return I0, I1


def config(tmp_path, out, **extra):
    (tmp_path / out).mkdir(exist_ok=True)
    return {"debug": False, "style": 1, "features": False,
            "images": [{"p": str(tmp_path / "p.png"), "q": str(tmp_path / "q.png"),
                        "output_name": "json_test"}],
            "output_type": "flow", "scale": 1, "output_dir": str(tmp_path / out),
            "rois": {"custom": [0, 0, C["w"], C["h"]]},
            "stats_json": str(tmp_path / out / "stats.json"), **extra}


def run_cli(cfg, tmp_path, out):
    p = tmp_path / out / "cfg.json"
    p.write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Error" not in r.stderr, r.stderr
    return json.loads((tmp_path / out / "stats.json").read_text())


def tiffs(tmp_path, out):
    return {f.name: f.read_bytes() for f in sorted((tmp_path / out).glob("*.tiff"))}


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def test_auto_is_the_numeric_seed(tmp_path, pair):
    I0, I1 = pair
    dx, dy = C["shift"]
    sa = run_cli(config(tmp_path, "auto", useInitialFlow=True, initialFlow="auto"), tmp_path, "auto")
    run_cli(config(tmp_path, "num", useInitialFlow=True, initialFlow=[dx, dy]), tmp_path, "num")
    ta, tn = tiffs(tmp_path, "auto"), tiffs(tmp_path, "num")
    assert len(ta) == 2 and ta == tn
    u, v, _, _ = ref.reference("cli_seeded", I0, I1, {}, np.full(I0.shape, dx, np.float32),
                               np.full(I0.shape, dy, np.float32))
    ur, vr = ref.postprocess(u, v, I1, 0)
    tif = lambda s: np.array(Image.open(tmp_path / "auto" / f"json_test_1.00_{s}.tiff")).astype(np.float32)
    assert bits_equal(tif("x"), ur) and bits_equal(tif("y"), vr)
    solve = sa[0]["solves"][0]
    assert solve["initial_flow"] == [dx, dy]
    auto = solve["initial_flow_auto"]
    assert auto["max_shift"] == 32 and auto["sad"] == 0
    assert auto["count"] == (C["w"] - abs(dx)) * (C["h"] - abs(dy))
    assert auto["count_zero"] == C["w"] * C["h"] and auto["sad_zero"] > 0


def test_auto_per_roi(tmp_path, pair):
    """Explicit top / bottom strips (the production job's shape): each ROI has its own estimate,
    searched within min(32, 48 / 4) px."""
    cfg = config(tmp_path, "rois", useInitialFlow=True, initialFlow="auto")
    cfg["rois"] = {"top": 48, "bottom": 48}
    solves = run_cli(cfg, tmp_path, "rois")[0]["solves"]
    assert len(solves) == 2
    for s in solves:
        assert s["initial_flow"] == list(C["shift"])
        assert s["initial_flow_auto"]["max_shift"] == 12 and s["initial_flow_auto"]["sad"] == 0


def test_auto_without_the_flag_is_inert(tmp_path, pair):
    s0 = run_cli(config(tmp_path, "plain"), tmp_path, "plain")
    s1 = run_cli(config(tmp_path, "key", initialFlow="auto", initialFlowMaxShift=16), tmp_path, "key")
    t0, t1 = tiffs(tmp_path, "plain"), tiffs(tmp_path, "key")
    assert len(t0) == 2 and t0 == t1
    for s in (s0, s1):
        assert "initial_flow" not in s[0]["solves"][0] and "initial_flow_auto" not in s[0]["solves"][0]
    assert s0[0]["solves"][0]["warp_iterations"] == s1[0]["solves"][0]["warp_iterations"]
