"""`optflow` with "style": 2 end to end on the GPU: the aligned slices, the saved flows and the
per-warp iteration counts must be those of tests/avgflow_ref.py (numpy + the oracle's solve),
byte for byte, for the device pre-scale, no pre-scale and the host pre-scale, with 1 and 3
outputs in flight; a slice of another size costs exactly the outputs that need it."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import avgflow_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


def write_stack(tmp_path, name, replace=None):
    st = ref.stack_of(name)
    paths = []
    for z, a in enumerate(st):
        if replace and z in replace:
            a = replace[z]
        p = tmp_path / f"z{z:02d}.png"
        Image.fromarray(a).save(p)
        paths.append(str(p))
    return paths


def run_cli(tmp_path, name, paths, **kw):
    c = ref.STACKS[name]
    out = tmp_path / "out"
    out.mkdir()
    cfg = {"style": 2, "slices": paths, "output_dir": str(out), "scale": c["scale"],
           "border": c["border"], "stats_json": str(tmp_path / "stats.json"),
           "timing_json": str(tmp_path / "timing.json"), **ref.TV, **kw}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(tmp_path / "cfg.json")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return out, r


def numbered(out):
    return sorted(p.name for p in out.glob("*.tiff"))


def prescaled_by_cli(tmp_path, name, i):
    """The pre-scaled slice and blend of a host-path job, from the CLI's --decode hook."""
    st = ref.stack_of(name)
    res = []
    for tag, a in (("f", st[i]), ("b", ref.blend6([st[i + d] for d in (-3, -2, -1, 1, 2, 3)]))):
        src, dst = tmp_path / f"pre_{tag}{i}.png", tmp_path / f"pre_{tag}{i}.tiff"
        Image.fromarray(a).save(src)
        subprocess.run([str(OPTFLOW), "--decode", str(src), str(dst), "0.5"], check=True, timeout=60)
        res.append(np.array(Image.open(dst)))
    return tuple(res)


def check_outputs(tmp_path, name, out, r, prescale, path):
    c = ref.STACKS[name]
    idx = ref.outputs_of(name)
    stats = {s["index"]: s for s in json.loads((tmp_path / "stats.json").read_text())}
    assert sorted(stats) == idx
    want_files = []
    for i in idx:
        pre = prescaled_by_cli(tmp_path, name, i) if prescale else None
        ra, ru, rv, rw, rs, _ = ref.reference(name, i, pre)
        got = np.array(Image.open(out / f"{i}.tiff"))
        assert got.dtype == np.uint8 and got.shape == (c["h"] + 2 * c["border"], c["w"] + 2 * c["border"])
        assert np.array_equal(got, ra), i
        for suf, want in (("x", ru), ("y", rv)):
            f = np.array(Image.open(out / f"{i}_{suf}.tiff"))
            assert f.dtype == np.float32
            assert np.array_equal(f.view(np.uint32), want.view(np.uint32)), (i, suf)
        s = stats[i]
        assert s["levels"] == rs["levels"] and s["prescale"] == path
        assert s["warp_iterations"] == rw.ravel().tolist()
        assert s["output"] == str(out / f"{i}.tiff")
        assert f"N: {i} " in r.stdout
        want_files += [f"{i}.tiff", f"{i}_x.tiff", f"{i}_y.tiff"]
    assert numbered(out) == sorted(want_files)                 # no other numbered TIFF


@pytest.mark.parametrize("inflight", [1, 3])
def test_nine_slices_device_prescale(tmp_path, built, inflight):
    name = "half_96x64"
    out, r = run_cli(tmp_path, name, write_stack(tmp_path, name), save_flow=True, inflight=inflight)
    check_outputs(tmp_path, name, out, r, False, "device")
    t = json.loads((tmp_path / "timing.json").read_text())
    assert t["slices"] == 3 and t["ring_slots"] == 7 + inflight - 1


def test_file_list_and_no_flow_files(tmp_path, built):
    name = "half_96x64"
    paths = write_stack(tmp_path, name)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    c = ref.STACKS[name]
    out = tmp_path / "out"
    out.mkdir()
    cfg = {"style": 2, "file_list": str(tmp_path / "list.txt"), "output_dir": str(out),
           "border": c["border"], **ref.TV}                    # scale: the default, 0.5
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(tmp_path / "cfg.json")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert numbered(out) == ["3.tiff", "4.tiff", "5.tiff"]
    for i in (3, 4, 5):
        assert np.array_equal(np.array(Image.open(out / f"{i}.tiff")), ref.reference(name, i)[0])


def test_scale_1(tmp_path, built):
    name = "full_80x48"
    out, r = run_cli(tmp_path, name, write_stack(tmp_path, name), save_flow=True, inflight=2)
    check_outputs(tmp_path, name, out, r, False, "none")


def test_host_prescale(tmp_path, built):
    name = "host_67x45"
    out, r = run_cli(tmp_path, name, write_stack(tmp_path, name), save_flow=True, inflight=3)
    check_outputs(tmp_path, name, out, r, True, "host")


def test_a_slice_of_another_size_costs_the_outputs_that_need_it(tmp_path, built):
    name = "half_96x64"
    odd = np.zeros((64, 94), np.uint8)
    paths = write_stack(tmp_path, name, replace={8: odd})      # outputs 3, 4 do not read slice 8
    out, r = run_cli(tmp_path, name, paths, inflight=3)
    assert "Error:" in r.stderr and paths[8] in r.stderr
    assert all(p not in r.stderr for p in paths[:8])
    assert numbered(out) == ["3.tiff", "4.tiff"]
    for i in (3, 4):
        assert np.array_equal(np.array(Image.open(out / f"{i}.tiff")), ref.reference(name, i)[0])
    # an unreadable slice likewise
    (tmp_path / "z00.png").write_bytes(b"not a png")
    (out / "3.tiff").unlink()
    (out / "4.tiff").unlink()
    out.rmdir()
    out, r = run_cli(tmp_path, name, paths, inflight=1)
    assert paths[0] in r.stderr and paths[8] in r.stderr
    assert numbered(out) == ["4.tiff"]
