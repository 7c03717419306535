"""The optflow CLI's inverted chains end to end ("initialFlow": {"chain": [...], "inverse": true}
and "backward": "inverse").  One job writes the four stride-1 flows of the zoom stack
("output_type": "flow", the whole frame as one ROI); a second job solves the reverse pair (4 -> 0)
from the inverse of their chain, and the forward pair (0 -> 4) from the chain with "consistency",
its backward solve seeded by the chain's inverse.  The TIFFs must be those of the same sequence
of Engine calls (then the reference's post-ops) byte for byte, stats_json must carry the
inversion's record with the restatement's counts, the checked pair without "backward" must still
fail alone with the old message, and a job without any new key must equal one that spells the
defaults out."""
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import compose_ref
import fbcheck_ref
import initflow_ref as ref
import invert_cases as T
import invert_ref
from optflow_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")   # before the engine library loads: one HIP runtime in the process
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"
W, H, N = T.ZOOM_W, T.ZOOM_H, T.ZOOM_FRAMES
ALPHA, BETA = 0.01, 0.5   # "consistency": true


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
    d = tmp_path_factory.mktemp("invert")
    frames = T.zoom_frames()
    for k, f in enumerate(frames):
        Image.fromarray(f).save(d / f"f{k}.png")
    base = {"style": 1, "features": False, "output_type": "flow", "scale": 1, "output_dir": str(d),
            "rois": {"custom": [0, 0, W, H]}}
    # job 1: the links
    r1 = run_cli(dict(base, images=[{"p": str(d / f"f{k}.png"), "q": str(d / f"f{k + 1}.png"),
                                     "output_name": f"z{k}"} for k in range(N - 1)]), d / "links.json")
    assert "Error" not in r1.stderr, r1.stderr
    links = [str(d / f"z{k}_1.00") for k in range(N - 1)]
    fwd = {"p": str(d / "f0.png"), "q": str(d / f"f{N - 1}.png"), "useInitialFlow": True}
    rev = {"p": str(d / f"f{N - 1}.png"), "q": str(d / "f0.png"), "useInitialFlow": True}
    check = dict(consistency=True, consistencyOutput=True)
    images = [
        dict(rev, output_name="back", initialFlow={"chain": links, "inverse": True}),
        dict(fwd, output_name="checked", initialFlow={"chain": links, "backward": "inverse"}, **check),
        dict(fwd, output_name="refused", initialFlow={"chain": links}, **check),
        dict(fwd, output_name="plain", initialFlow={"chain": links}),
        dict(fwd, output_name="spelled", initialFlow={"chain": links, "inverse": False, "inverseIterations": 8,
                                                      "inverseTolerance": 0.01}),
        dict(rev, output_name="both", initialFlow={"chain": links, "inverse": True, "backward": "inverse",
                                                   "inverseIterations": 4, "inverseTolerance": 0.25}, **check),
    ]
    r2 = run_cli(dict(base, images=images, stats_json=str(d / "stats.json")), d / "far.json")
    planes = [(tif(l + "_x.tiff"), tif(l + "_y.tiff")) for l in links]
    return d, frames, planes, r2, json.loads((d / "stats.json").read_text())


@pytest.fixture(scope="module")
def eng(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


def checked(eng, I0, I1, seed_f, seed_b):
    """The CLI's sequence for a checked ROI on Engine calls: both solves, the score of the raw
    flows, the post-process of the forward flow, the rejection."""
    u, v, _, wi = eng.calc_host(I0, I1, init=seed_f)
    ub, vb = eng.calc_host(I1, I0, init=seed_b)[:2]
    dev = torch.device("cuda", 0)
    fl = torch.from_numpy(np.stack([u, v, ub, vb, np.zeros_like(u)])).to(dev)
    torch.cuda.synchronize()
    p = [fl[k].data_ptr() for k in range(5)]
    eng.fb_score(p[0], p[1], 4 * W, p[2], p[3], 4 * W, W, H, ALPHA, p[4], 4 * W, stream=eng.stream)
    torch.cuda.synchronize()
    score = fl[4].cpu().numpy()
    uu, vv = ref.postprocess(u, v, I1, 0)
    uu, vv, rejected = fbcheck_ref.zero_above(uu, vv, score, BETA)
    return uu, vv, score, rejected, wi


def test_the_reverse_pair_is_the_python_paths_flow(jobs, eng):
    d, frames, planes, r2, stats = jobs
    u, v, st, wi, counts, inv = eng.calc_chained_host(frames[4], frames[0], planes, inverse=True)
    ur, vr = ref.postprocess(u, v, frames[0], 0)
    x, y = tif(d / "back_1.00_x.tiff"), tif(d / "back_1.00_y.tiff")
    assert x.tobytes() == ur.tobytes() and y.tobytes() == vr.tobytes()
    # the chain and its inverse are the restatement's
    cu, cv, want = compose_ref.compose_chain(planes)
    gu, gv, _, outside, unconv = invert_ref.invert(cu, cv, 8, 0.01)
    assert counts == want and inv == dict(outside=outside, unconverged=unconv)
    solve = stats[0]["solves"][0]
    assert stats[0]["ok"] is True
    rec = solve["initial_flow_chain"]
    assert rec["links"] == N - 1 and rec["outside"] == want
    assert rec["inverse"] == {"iterations": 8, "tolerance": pytest.approx(0.01), "outside": outside,
                              "unconverged": unconv}
    assert solve["warp_iterations"] == wi.ravel().tolist()
    assert T.zoom_epe(x, y, 4, 0) < 0.5


def test_the_checked_pair_seeds_its_backward_solve_with_the_inverse(jobs, eng):
    d, frames, planes, r2, stats = jobs
    cu, cv, _ = eng.compose_chain_host(planes)
    gu, gv, inv = eng.invert_flow_host(cu, cv, 8, 0.01)
    uu, vv, score, rejected, wi = checked(eng, frames[0], frames[4], (cu, cv), (gu, gv))
    assert tif(d / "checked_1.00_x.tiff").tobytes() == uu.tobytes()
    assert tif(d / "checked_1.00_y.tiff").tobytes() == vv.tobytes()
    assert tif(d / "checked_1.00_fb.tiff").tobytes() == score.tobytes()
    solve = stats[1]["solves"][0]
    assert stats[1]["ok"] is True
    assert solve["initial_flow_chain"]["inverse"]["outside"] == inv["outside"]
    assert solve["initial_flow_chain"]["inverse"]["unconverged"] == inv["unconverged"]
    assert solve["consistency"]["rejected_px"] == rejected
    assert solve["warp_iterations"] == wi.ravel().tolist()
    # most of the interior passes the check: the backward solve found the forward flow's inverse
    m = T.ZOOM_MARGIN
    assert fbcheck_ref.consistent(score, BETA)[m:-m, m:-m].mean() > 0.9
    # with "inverse" too, the forward seed is the inverse and the backward seed the chain itself
    gu4, gv4, inv4 = eng.invert_flow_host(cu, cv, 4, 0.25)
    uu, vv, score, rejected, wi = checked(eng, frames[4], frames[0], (gu4, gv4), (cu, cv))
    assert tif(d / "both_1.00_x.tiff").tobytes() == uu.tobytes()
    assert tif(d / "both_1.00_y.tiff").tobytes() == vv.tobytes()
    assert tif(d / "both_1.00_fb.tiff").tobytes() == score.tobytes()
    rec = stats[5]["solves"][0]["initial_flow_chain"]["inverse"]
    assert rec == {"iterations": 4, "tolerance": 0.25, "outside": inv4["outside"],
                   "unconverged": inv4["unconverged"]}


def test_without_backward_the_checked_pair_still_fails_alone(jobs):
    d, _, _, r2, stats = jobs
    err = errors(r2)
    assert sorted(err) == [2], r2.stderr
    assert ("an initialFlow chain cannot be combined with consistency: the backward solve's seed would be the "
            "chain's inverse, not its negation") in err[2]
    assert [s["ok"] for s in stats] == [True, True, False, True, True, True]
    assert not (d / "refused_1.00_x.tiff").exists()


def test_a_job_without_the_new_keys_equals_one_that_spells_the_defaults(jobs):
    d, _, _, _, stats = jobs
    for axis in ("x", "y"):
        assert (d / f"plain_1.00_{axis}.tiff").read_bytes() == (d / f"spelled_1.00_{axis}.tiff").read_bytes()
    a, b = stats[3]["solves"][0], stats[4]["solves"][0]
    a.pop("seconds"), b.pop("seconds")
    assert a == b and "inverse" not in a["initial_flow_chain"]
