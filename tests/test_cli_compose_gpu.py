"""The optflow CLI's "initialFlow": {"chain": [...]} end to end.  One job writes the four
stride-1 flows of a five-frame stack ("output_type": "flow", the whole frame as one ROI); a
second job solves the stride-4 pair from their chain.  Its TIFFs must be the Python path's
(Engine.calc_chained_host on the same link planes, then the reference's post-ops) byte for byte,
stats_json must carry the chain and its outside counts, a pair whose link is missing or of
another size must fail alone with a line that names the file, and a chain beside "consistency"
must fail with its own message."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import compose_cases as T
import compose_ref
import initflow_ref as ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")   # before the engine library loads: one HIP runtime in the process
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
W, H = ref.CLI["w"], ref.CLI["h"]
N = T.CHAIN_FRAMES


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


def run_cli(cfg, path):
    path.write_text(json.dumps(cfg))
    r = subprocess.run([str(OPTFLOW), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def errors(r):
    """The failed pairs' lines by pair index (the workers' order is not the pairs')."""
    out = {}
    for l in r.stderr.splitlines():
        if l.startswith("Error: pair "):
            out[int(l.split()[2])] = l
    return out


def tif(path):
    a = np.array(Image.open(path))
    assert a.dtype == np.float32
    return a


@pytest.fixture(scope="module")
def jobs(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("chain")
    frames = T.chain_frames(w=W, h=H)
    for k, f in enumerate(frames):
        Image.fromarray(f).save(d / f"f{k}.png")
    base = {"style": 1, "features": False, "output_type": "flow", "scale": 1, "output_dir": str(d),
            "rois": {"custom": [0, 0, W, H]}}
    # job 1: the links
    r1 = run_cli(dict(base, images=[{"p": str(d / f"f{k}.png"), "q": str(d / f"f{k + 1}.png"),
                                     "output_name": f"z{k}"} for k in range(N - 1)]), d / "links.json")
    assert "Error" not in r1.stderr, r1.stderr
    links = [str(d / f"z{k}_1.00") for k in range(N - 1)]
    Image.fromarray(np.zeros((H - 1, W), np.float32)).save(d / "tooshort_1.00_x.tiff")
    Image.fromarray(np.zeros((H - 1, W), np.float32)).save(d / "tooshort_1.00_y.tiff")
    far = {"p": str(d / "f0.png"), "q": str(d / f"f{N - 1}.png"), "useInitialFlow": True}
    images = [
        dict(far, output_name="far", initialFlow={"chain": links}),
        dict(far, output_name="missing", initialFlow={"chain": links[:2] + [str(d / "nothing_1.00")] + links[3:]}),
        dict(far, output_name="short", initialFlow={"chain": links[:1] + [str(d / "tooshort_1.00")]}),
        dict(far, output_name="checked", initialFlow={"chain": links}, consistency=True),
        dict(far, output_name="scored", initialFlow={"chain": links}, zncc=True),
        dict(far, output_name="one", initialFlow={"chain": links[:1]}),
        dict(far, output_name="unseeded"),
    ]
    images[-1].pop("useInitialFlow")
    r2 = run_cli(dict(base, images=images, stats_json=str(d / "stats.json")), d / "far.json")
    return d, frames, links, r2, json.loads((d / "stats.json").read_text())


def test_the_chained_pair_is_the_python_paths_flow(jobs):
    d, frames, links, r2, stats = jobs
    e = capi.Engine(capi.make_params())
    try:
        planes = []
        for k in range(N - 1):
            u, v = e.calc_host(frames[k], frames[k + 1])[:2]
            planes.append(ref.postprocess(u, v, frames[k + 1], 0))
        u, v, st, wi, counts = e.calc_chained_host(frames[0], frames[-1], planes)
    finally:
        e.close()
    for k in range(N - 1):   # the link files are the flows the Python path chains
        assert bits_equal(tif(links[k] + "_x.tiff"), planes[k][0])
        assert bits_equal(tif(links[k] + "_y.tiff"), planes[k][1])
    ur, vr = ref.postprocess(u, v, frames[-1], 0)
    x, y = tif(d / "far_1.00_x.tiff"), tif(d / "far_1.00_y.tiff")
    assert bits_equal(x, ur) and bits_equal(y, vr)
    assert x.tobytes() == ur.tobytes() and y.tobytes() == vr.tobytes()
    # the chain is the restatement's
    su, sv, want = compose_ref.compose_chain(planes)
    assert counts == want
    solve = stats[0]["solves"][0]
    assert stats[0]["ok"] is True
    assert solve["initial_flow_chain"] == {"links": N - 1, "outside": want}
    assert "initial_flow" not in solve
    assert solve["warp_iterations"] == wi.ravel().tolist()
    assert stats[6]["ok"] is True and "initial_flow_chain" not in stats[6]["solves"][0]


def test_a_bad_link_fails_only_its_pair_and_names_the_file(jobs):
    d, _, links, r2, stats = jobs
    err = errors(r2)
    assert sorted(err) == [1, 2, 3], r2.stderr
    assert str(d / "nothing_1.00_x.tiff") in err[1]
    assert str(d / "tooshort_1.00_x.tiff") in err[2] and f"{W}x{H - 1}" in err[2]
    assert [s["ok"] for s in stats] == [True, False, False, False, True, True, True]
    for name in ("missing", "short", "checked"):
        assert not (d / f"{name}_1.00_x.tiff").exists()


def test_a_chain_beside_consistency_fails_with_its_message(jobs):
    _, _, _, r2, stats = jobs
    assert "chain cannot be combined with consistency" in errors(r2)[3]
    assert "solves" not in stats[3] or not stats[3]["solves"]


def test_a_chain_combines_with_zncc_and_one_link_is_a_seed_from_a_file(jobs):
    d, frames, links, _, stats = jobs
    s = stats[4]["solves"][0]
    assert s["initial_flow_chain"]["links"] == N - 1 and s["zncc"]["px"] == W * H
    assert s["warp_iterations"] == stats[0]["solves"][0]["warp_iterations"]
    x, x0 = tif(d / "scored_1.00_x.tiff"), tif(d / "far_1.00_x.tiff")
    keep = x != 0   # the score only zeroes
    assert bits_equal(x[keep], x0[keep]) and keep.any()
    one = stats[5]["solves"][0]["initial_flow_chain"]
    assert one["links"] == 1 and not one["outside"]
    e = capi.Engine(capi.make_params())
    try:
        seed = (tif(links[0] + "_x.tiff"), tif(links[0] + "_y.tiff"))
        u, v = e.calc_host(frames[0], frames[-1], init=seed)[:2]
    finally:
        e.close()
    ur, vr = ref.postprocess(u, v, frames[-1], 0)
    assert bits_equal(tif(d / "one_1.00_x.tiff"), ur) and bits_equal(tif(d / "one_1.00_y.tiff"), vr)
