"""`optflow` with "style": 2 (the average-flow alignment of a slice list) without a GPU: what
--plan resolves, and every configuration error that must end the job with rc 2 before the GPU
is touched."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

from optflow_amd import capi

OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


def run(tmp_path, cfg, *flags):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return subprocess.run([str(OPTFLOW), *flags, str(p)], capture_output=True, text=True, timeout=120)


def make_slices(tmp_path, n, w, h):
    rng = np.random.default_rng(n * w + h)
    paths = []
    for z in range(n):
        p = tmp_path / f"s{z}.png"
        Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8)).save(p)
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("w,h,scale,path", [(96, 64, 0.5, "device"), (67, 45, 0.5, "host"),
                                            (96, 64, 0.25, "host"), (67, 45, 1, "none")])
def test_plan(tmp_path, built, w, h, scale, path):
    names = make_slices(tmp_path, 9, w, h)
    out = tmp_path / "out"
    r = run(tmp_path, {"style": 2, "slices": names, "output_dir": str(out), "scale": scale,
                       "border": 4}, "--plan")
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines()]
    assert [l["index"] for l in lines] == [3, 4, 5]
    for l in lines:
        i = l["index"]
        assert l["input"] == names[i]
        assert l["neighbours"] == [names[i + d] for d in (-3, -2, -1, 1, 2, 3)]
        assert l["output"] == f"{out}/{i}.tiff"
        assert l["prescale"] == path
    assert not out.exists()


def test_plan_reads_a_file_list(tmp_path, built):
    names = make_slices(tmp_path, 7, 20, 10)
    (tmp_path / "list.txt").write_text("\n".join(names[:3]) + "\n\n" + "\n".join(names[3:]) + "\n\n")
    r = run(tmp_path, {"style": 2, "file_list": str(tmp_path / "list.txt"),
                       "output_dir": str(tmp_path)}, "--plan")
    assert r.returncode == 0, r.stderr
    (l,) = [json.loads(x) for x in r.stdout.splitlines()]
    assert l["index"] == 3 and l["input"] == names[3] and l["prescale"] == "device"
    assert l["neighbours"] == names[:3] + names[4:]


@pytest.mark.parametrize("flags", [(), ("--plan",)])
def test_configuration_errors_are_rc_2(tmp_path, built, flags):
    names = make_slices(tmp_path, 7, 20, 10)
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    ok = {"style": 2, "slices": names, "output_dir": str(tmp_path / "o"), "device": 99}
    cases = [({**ok, "slices": names[:6]}, "at least 7 slices"),
             ({**ok, "file_list": str(tmp_path / "list.txt")}, "exactly one of"),
             ({k: v for k, v in ok.items() if k != "slices"}, "exactly one of"),
             ({k: v for k, v in ok.items() if k != "output_dir"}, "output_dir"),
             ({**ok, "border": -1}, "border")]
    for cfg, what in cases:
        r = run(tmp_path, cfg, *flags)
        assert r.returncode == 2, (cfg, r.stderr)
        assert what in r.stderr
        assert not (tmp_path / "o").exists()


def test_other_styles_keep_their_message(tmp_path, built):
    r = run(tmp_path, {"style": 3, "slices": [], "output_dir": str(tmp_path)})
    assert r.returncode == 2
    assert r.stderr.strip() == "style 3 is not implemented (only style 1, optflow.cpp:62-66)"
