"""The CLI side of an inverted "initialFlow" chain without a GPU: `--plan` on configs that carry
"inverse", "inverseIterations", "inverseTolerance" and "backward", and the config errors of
those keys, each of which ends the job with exit status 1 and its message before a slice is read
(the slices named here do not exist).  Runs on the release binary and on the stand-alone ASan +
UBSan build of the CLI (`make -C fibsem-optflow_amd asan`), as tests/test_compose_cli_cpu.py does."""
import fcntl
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from optflow_amd import capi

BINS = {"release": capi.PKG_ROOT / "bin" / "optflow",
        "asan": capi.PKG_ROOT / "bin" / "optflow_asan"}   # make -C fibsem-optflow_amd asan
_bin = [str(BINS["release"])]


@pytest.fixture(autouse=True, params=["release", "asan"])
def optflow_bin(request, built):
    path = BINS[request.param]
    if request.param == "asan":
        # one build at a time (pytest-xdist workers): a worker must not run the binary
        # while another is still linking it
        with open(capi.PKG_ROOT / "bin" / ".asan.lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if not path.exists() or path.stat().st_mtime < BINS["release"].stat().st_mtime:
                r = subprocess.run(["make", "-C", str(capi.PKG_ROOT), "asan"], capture_output=True,
                                   text=True)
                if r.returncode != 0:
                    pytest.skip("ASan/UBSan build unavailable: " + r.stderr[-300:])
    _bin[0] = os.environ.get("OPTFLOW_BIN", str(path))
    yield


def run(*args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([_bin[0], *map(str, args)], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode not in (98, 99), r.stderr
    assert r.returncode >= 0, f"optflow killed by signal {-r.returncode}: {r.stderr}"
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r


def _slices(tmp_path, n=3, w=48, h=40):
    rng = np.random.default_rng(8)
    out = []
    for k in range(n):
        p = tmp_path / f"s{k}.tif"
        Image.fromarray(rng.integers(2, 255, (h, w), dtype=np.uint8)).save(p)
        out.append(str(p))
    return out


def _plan(tmp_path, cfg):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return run("--plan", p)


def _entries(r):
    """The plan: the JSON list after the pair lines the pair loop prints."""
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    return json.loads("\n".join(lines[lines.index("["):]))


def _cfg(tmp_path, s, init, **pair):
    links = [str(tmp_path / "z0_1.00"), str(tmp_path / "z1_1.00")]
    return {"output_dir": str(tmp_path), "scale": 1, "output_type": "flow", "rois": {"top": 16, "bottom": 16},
            "images": [
                {"p": s[0], "q": s[1], "output_name": "z0"},
                {"p": s[1], "q": s[2], "output_name": "z1"},
                dict({"p": s[2], "q": s[0], "output_name": "back", "useInitialFlow": True,
                      "initialFlow": dict({"chain": links}, **init)}, **pair)]}, links


def test_plan_lists_inverse_and_backward(tmp_path):
    s = _slices(tmp_path)
    cfg, links = _cfg(tmp_path, s, {"inverse": True})
    plan = _entries(_plan(tmp_path, cfg))
    assert [p["strip_batch"] for p in plan] == [True, True, False]
    assert plan[2]["initialFlow"] == {"chain": links, "links": 2, "inverse": True, "inverseIterations": 8,
                                      "inverseTolerance": pytest.approx(0.01)}
    cfg, links = _cfg(tmp_path, s, {"inverse": True, "inverseIterations": 32, "inverseTolerance": 0.25,
                                    "backward": "inverse"}, consistency=True)
    plan = _entries(_plan(tmp_path, cfg))
    assert plan[2]["initialFlow"] == {"chain": links, "links": 2, "inverse": True, "inverseIterations": 32,
                                      "inverseTolerance": 0.25, "backward": "inverse"}
    assert plan[2]["consistency"]["alpha"] == pytest.approx(0.01)
    cfg, links = _cfg(tmp_path, s, {"backward": "inverse", "inverseIterations": 1, "inverseTolerance": 0},
                      consistency=True)
    plan = _entries(_plan(tmp_path, cfg))
    assert plan[2]["initialFlow"] == {"chain": links, "links": 2, "inverse": False, "inverseIterations": 1,
                                      "inverseTolerance": 0, "backward": "inverse"}
    # without the new keys, and with the default spelled out, the plan is what it was
    cfg, links = _cfg(tmp_path, s, {})
    plan = _entries(_plan(tmp_path, cfg))
    assert plan[2]["initialFlow"] == {"chain": links, "links": 2}
    cfg, links = _cfg(tmp_path, s, {"inverse": False})
    assert _entries(_plan(tmp_path, cfg)) == plan


BAD = [
    ({"inverse": 1}, '"inverse" must be true or false'),
    ({"inverse": "true"}, '"inverse" must be true or false'),
    ({"inverse": None}, '"inverse" must be true or false'),
    ({"inverse": [True]}, '"inverse" must be true or false'),
    ({"inverseIterations": 0}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseIterations": 33}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseIterations": -8}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseIterations": 8.5}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseIterations": "8"}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseIterations": True}, '"inverseIterations" must be an integer from 1 to 32'),
    ({"inverseTolerance": "0.01"}, '"inverseTolerance" must be a finite number'),
    ({"inverseTolerance": 1e60}, '"inverseTolerance" must be a finite number'),
    ({"inverseTolerance": None}, '"inverseTolerance" must be a finite number'),
    ({"inverseTolerance": [0.01]}, '"inverseTolerance" must be a finite number'),
    ({"backward": "negation"}, '"backward" must be "inverse"'),
    ({"backward": True}, '"backward" must be "inverse"'),
    ({"backward": ""}, '"backward" must be "inverse"'),
    ({"backward": ["inverse"]}, '"backward" must be "inverse"'),
]


@pytest.mark.parametrize("init,message", BAD, ids=[json.dumps(b[0]) for b in BAD])
def test_a_malformed_key_ends_the_job_before_a_slice_is_read(tmp_path, init, message):
    # the slices do not exist: a job that got as far as reading one would say so instead
    s = [str(tmp_path / f"missing{k}.tif") for k in range(3)]
    cfg, _ = _cfg(tmp_path, s, init)
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    for args in (("--plan", p), (p,)):
        r = run(*args)
        assert r.returncode == 1, (r.returncode, r.stderr)
        assert "pair 2: initialFlow: " + message in r.stderr, r.stderr
        assert "missing" not in r.stderr, r.stderr
    # the limits themselves are fine
    s = _slices(tmp_path)
    for good in ({"inverseIterations": 1}, {"inverseIterations": 32}, {"inverseTolerance": 0},
                 {"inverseTolerance": 3.0e38}, {"inverse": False}, {"backward": "inverse"}):
        cfg, _ = _cfg(tmp_path, s, good)
        assert _plan(tmp_path, cfg).returncode == 0, good
