"""The forward-backward score without a GPU: the case table's census (so the GPU comparison
cannot pass vacuously), the header and the library, and what the score is for: on the oracle's
flows it rejects a region that exists in one slice only and keeps the rest."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import fbcheck_cases as T
import fbcheck_ref as ref
from optflow_amd import capi

F = np.float32
HEADER = Path(__file__).resolve().parents[1] / "include" / "tvl1.h"
SYMBOLS = ("tvl1_fb_score", "tvl1_fb_score_batch", "tvl1_zero_above", "tvl1_zero_above_batch")

# Measured with the oracle (IEEE and fma modes alike) on T.patch_pair(), nscales 3, warps 3, alpha
# 0.01, beta 0.5: 0.6254 of the patch's 2304 px are rejected, 0.0 of the 14080 px at least 16 px
# away from the patch and from the frame edge.  The test asks for half that gap.
SHARE_IN, SHARE_OUT = 0.6254, 0.0
MARGIN = 0.5 * (SHARE_IN - SHARE_OUT)


def test_case_table_has_every_class_of_px():
    n = dict.fromkeys(("inside", "left", "right", "top", "bottom", "nan_landing", "nan_score", "edge",
                       "edge_clamped", "tie", "ulp_over", "ax0", "ay0", "inf", "kept", "rejected",
                       "neg_zero"), 0)
    for case in T.CASES:
        pl = T.planes(case)
        assert all(a.shape == (case.n, case.H, case.W) and a.dtype == F for a in pl)
        for b in range(case.n):
            uf, vf, ub, vb = (a[b] for a in pl)
            X, Y, ins = ref.landing(uf, vf)
            s = ref.fb_score(uf, vf, ub, vb, case.alpha)
            assert np.all(np.isposinf(s[~ins]))
            with np.errstate(invalid="ignore"):
                n["inside"] += int(ins.sum())
                n["left"] += int((X < 0).sum())
                n["right"] += int((X > F(case.W - 1)).sum())
                n["top"] += int((Y < 0).sum())
                n["bottom"] += int((Y > F(case.H - 1)).sum())
                n["nan_landing"] += int((np.isnan(X) | np.isnan(Y)).sum())
                n["nan_score"] += int(np.isnan(s).sum())
                edge = ins & ((X == 0) | (X == F(case.W - 1)) | (Y == 0) | (Y == F(case.H - 1)))
                n["edge"] += int(edge.sum())
                # landed on the last column or row of a frame that has another one: x1, y1 clamped
                n["edge_clamped"] += int((ins & (((X == F(case.W - 1)) & (case.W > 1)) |
                                                 ((Y == F(case.H - 1)) & (case.H > 1)))).sum())
                fx, fy = X - np.floor(X), Y - np.floor(Y)
                n["ax0"] += int((ins & (fx == 0) & (fy != 0)).sum())
                n["ay0"] += int((ins & (fy == 0) & (fx != 0)).sum())
                n["inf"] += int(np.isposinf(s).sum())
                n["tie"] += int((s == F(case.beta)).sum())
                n["ulp_over"] += int((s == np.nextafter(F(case.beta), F(np.inf))).sum())
                ok = ref.consistent(s, case.beta)
                n["kept"] += int(ok.sum())
                n["rejected"] += int((~ok).sum())
                n["neg_zero"] += sum(int((np.signbit(a) & (a == 0)).sum()) for a in (uf, vf, ub, vb))
            if case.kind == "integer":   # b = -f exactly: the score is exactly 0
                assert np.all(s[ins] == 0)
            if case.kind == "edges":
                assert ins.all()
            if case.kind == "tie":       # the tie counts as consistent, its neighbour does not
                k = np.arange(case.W * case.H).reshape(case.H, case.W)
                assert np.all(s[k % 2 == 0] == T.TIE_BETA) and np.all(ok[k % 2 == 0])
                assert np.all(s[k % 2 == 1] == np.nextafter(T.TIE_BETA, F(1))) and not np.any(ok[k % 2 == 1])
    empty = [k for k, v in n.items() if v == 0]
    assert not empty, (empty, n)


def test_special_values_sit_in_each_of_the_four_planes():
    case = next(c for c in T.CASES if c.name == "67x45-special")
    for a in T.planes(case):
        a = a[0]
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
        assert (a == F(1e30)).any() and (a == F(-1e30)).any()
        assert (np.signbit(a) & (a == 0)).any()


def test_table_covers_the_sizes_and_layouts():
    sizes = {(c.W, c.H) for c in T.CASES if c.roi is None and c.n == 1}
    assert sizes == set(T.SIZES) == {(1, 1), (1, 7), (5, 1), (3, 256), (67, 45), (257, 131)}
    roi = [c for c in T.CASES if c.roi]
    assert roi and all((c.W, c.H) == (130, 70) and c.roi[:2] == (160, 80) for c in roi)
    assert all((4 * c.roi[2]) % 16 == 4 and (4 * c.roi[0]) % 16 == 0 for c in roi)   # every row off by 1 float
    assert [(c.n, c.W, c.H) for c in T.CASES if c.n > 1] == [(257, 130, 20)]


def test_header_declares_and_library_exports_the_calls(built):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"#define\s+TVL1_ABI_VERSION\s+9\b", text)
    lib = C.CDLL(str(capi.ENGINE_SO))
    for name in SYMBOLS:
        assert re.search(rf"\btvl1_status\s+{name}\s*\(", text), name
        assert hasattr(lib, name), name
    eng_lib = capi.load_engine()
    assert eng_lib.tvl1_abi_version() == 9
    # argument checks need no device: a NULL ctx is TVL1_EINVAL
    assert eng_lib.tvl1_fb_score(None, None, None, 0, None, None, 0, 1, 1, 0.0, None, 0, None) == 1
    assert eng_lib.tvl1_zero_above(None, None, None, 0, None, 0, 1, 1, 0.0, None, None) == 1
    for name in ("fb_score", "fb_score_batch", "zero_above", "zero_above_batch", "calc_consistent"):
        assert callable(getattr(capi.Engine, name))


@pytest.mark.parametrize("fast_math", [0, 2], ids=["ieee", "fma"])
def test_score_rejects_a_region_of_one_slice_only(built, fast_math):
    from oracle import checker
    I0, I1 = T.patch_pair()
    p = capi.make_params(fast_math=fast_math, **T.PATCH_PARAMS)
    uf, vf = checker.oracle_calc(I0, I1, p)[:2]
    ub, vb = checker.oracle_calc(I1, I0, p)[:2]
    rej = ~ref.consistent(ref.fb_score(uf, vf, ub, vb, 0.01), 0.5)
    inp, far = T.patch_masks(16)
    assert (int(inp.sum()), int(far.sum())) == (2304, 14080)
    share_in, share_out = float(rej[inp].mean()), float(rej[far].mean())
    print(f"rejected share inside the patch {share_in:.4f}, outside {share_out:.4f}")
    assert share_in - share_out > MARGIN, (share_in, share_out)


# ---- the CLI's keys, resolved without a GPU (optflow --plan)
OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


@pytest.fixture
def cfg(tmp_path, built):
    from PIL import Image
    rng = np.random.default_rng(9)
    for n in ("p", "q"):
        Image.fromarray(rng.integers(0, 256, (61, 83), dtype=np.uint8)).save(tmp_path / f"{n}.png")
    return {"output_dir": str(tmp_path), "scale": 1, "output_type": "flow",
            "rois": {"top": 20, "bottom": 20},
            "images": [{"p": str(tmp_path / "p.png"), "q": str(tmp_path / "q.png"),
                        "output_name": "pq"}]}


def _plan(tmp_path, cfg, name):
    import json
    import subprocess
    p = tmp_path / name
    p.write_text(json.dumps(cfg))
    return subprocess.run([str(OPTFLOW), "--plan", str(p)], capture_output=True, text=True, timeout=120)


def _plans(r):
    import json
    assert r.returncode == 0, r.stderr
    out = r.stdout
    return json.loads(out[out.index("\n[") + 1:] if not out.startswith("[") else out)


def test_cli_plan_lists_the_consistency_keys(tmp_path, cfg):
    base = _plans(_plan(tmp_path, cfg, "a.json"))
    assert "consistency" not in base[0]
    # off, and the other two keys without it, change nothing
    assert _plans(_plan(tmp_path, {**cfg, "consistency": False, "consistencyOversample": 9,
                                   "consistencyOutput": True}, "b.json")) == base
    (pl,) = _plans(_plan(tmp_path, {**cfg, "consistency": True}, "c.json"))
    assert pl["consistency"] == {"alpha": pytest.approx(0.01), "beta": 0.5, "oversample": 4, "output": False}
    assert pl["strip_batch"] is True   # the global key stays in the strip batch
    assert {k: v for k, v in pl.items() if k != "consistency"} == base[0]
    (pl,) = _plans(_plan(tmp_path, {**cfg, "consistency": {"alpha": 0.25, "beta": 2.0},
                                   "consistencyOversample": 7, "consistencyOutput": True}, "d.json"))
    assert pl["consistency"] == {"alpha": 0.25, "beta": 2.0, "oversample": 7, "output": True}
    # per image over global, and an oversample below 1 is 1
    c2 = {**cfg, "consistency": True, "consistencyOversample": 0}
    c2["images"] = [{**cfg["images"][0], "consistency": {"beta": 0.125}}]
    (pl,) = _plans(_plan(tmp_path, c2, "e.json"))
    assert pl["consistency"] == {"alpha": pytest.approx(0.01), "beta": 0.125, "oversample": 1, "output": False}
    assert pl["strip_batch"] is False   # a per-image key is not a production key
    c2["images"] = [{**cfg["images"][0], "consistency": False}]
    assert "consistency" not in _plans(_plan(tmp_path, c2, "f.json"))[0]


def test_cli_consistency_with_features_is_a_config_error(tmp_path, cfg):
    r = _plan(tmp_path, {**cfg, "consistency": True, "features": 1}, "g.json")
    assert r.returncode != 0 and "consistency cannot be combined with feature alignment" in r.stderr
    c2 = {**cfg, "features": 1}
    c2["images"] = [{**cfg["images"][0], "consistency": {"alpha": 0.0}}]
    r = _plan(tmp_path, c2, "h.json")
    assert r.returncode != 0 and "consistency cannot be combined with feature alignment" in r.stderr
    assert _plans(_plan(tmp_path, {**cfg, "consistency": False, "features": 1}, "i.json"))[0]["features"] is True
