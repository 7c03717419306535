"""The ZNCC score without a GPU: the header and the library, the case table's census (so the
GPU comparison cannot pass vacuously), the restatement's vectorised sums against a loop per px,
and what the score is for: on the oracle's forward flow alone it rejects a region that exists in
one slice only and keeps the rest."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import fbcheck_cases as FB
import zncc_cases as T
import zncc_ref as ref
from optflow_amd import capi

F = np.float32
HEADER = Path(__file__).resolve().parents[1] / "include" / "tvl1.h"
SYMBOLS = ("tvl1_zncc_score", "tvl1_zncc_score_batch", "tvl1_warp_by_flow_u8")

# Measured with the oracle's forward flow (IEEE and fma modes alike) on fbcheck_cases.patch_pair(),
# nscales 3, warps 3, radius 3, beta 0.25: 0.8043 of the patch's 2304 px are rejected, 0.0 of the
# 14080 px at least 16 px away from the patch and from the frame edge.  The test asks for half
# that gap.
SHARE_IN, SHARE_OUT = 0.8043, 0.0
MARGIN = 0.5 * (SHARE_IN - SHARE_OUT)


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
    assert eng_lib.tvl1_zncc_score_batch(None, 1, None, 0, 0, None, 0, 0, None, None, 0, 0, 1, 1, 3,
                                         None, 0, 0, None) == 1
    assert eng_lib.tvl1_zncc_score(None, None, 0, None, 0, None, None, 0, 1, 1, 3, None, 0, None) == 1
    assert eng_lib.tvl1_warp_by_flow_u8(None, None, 0, None, None, 0, 1, 1, None, 0, None, 0, None) == 1
    for name in ("zncc_score", "zncc_score_batch", "warp_by_flow_u8", "calc_scored"):
        assert callable(getattr(capi.Engine, name))


def _frac32(a):
    """The fraction of a * 32 (exact in float32 for the table's sizes)."""
    a32 = a * F(32)
    return a32, a32 - np.floor(a32)


def test_case_table_has_every_class_of_px():
    keys = ("valid", "left", "right", "top", "bottom", "nan", "pos_inf", "neg_inf", "huge", "neg_zero",
            "edge_x0", "edge_x1", "edge_y0", "edge_y1", "clamped_tap", "tie_x", "tie_x_below",
            "tie_x_above", "tie_y", "tie_y_below", "tie_y_above", "tie_even_down", "tie_odd_up",
            "score_0", "score_2", "score_inf_invalid", "score_inf_B0", "score_inf_C0", "finite",
            "truncated_by_m", "shared0", "roi", "second_chunk")
    n = dict.fromkeys(keys, 0)
    per_r = {r: dict(truncated=0, full=0) for r in (1, 2, 3, 4)}
    for case in T.CASES:
        I0, I1, u, v = T.planes(case)
        assert I1.shape == u.shape == v.shape == (case.n, case.H, case.W)
        assert I0.shape == ((1 if case.shared0 else case.n), case.H, case.W)
        assert I0.dtype == I1.dtype == np.uint8 and u.dtype == v.dtype == F
        n["shared0"] += int(case.shared0)
        n["roi"] += int(case.roi is not None)
        n["second_chunk"] += int(case.n > 256)
        W, H, r = case.W, case.H, case.r
        for b in range(min(case.n, 3)):   # the batch's pairs are alike: three stand for all
            a0 = I0[0 if case.shared0 else b]
            J, m = ref.warp(I1[b], u[b], v[b])
            sums = ref.window_sums(a0, J, m, r)
            A, B, Cc = ref.abc(sums)
            s = ref.score_from(J, m, a0, r)
            with np.errstate(all="ignore"):
                mx = np.arange(W, dtype=F)[None, :] + u[b]
                my = np.arange(H, dtype=F)[:, None] + v[b]
                n["valid"] += int(m.sum())
                n["left"] += int((mx < 0).sum())
                n["right"] += int((mx > F(W - 1)).sum())
                n["top"] += int((my < 0).sum())
                n["bottom"] += int((my > F(H - 1)).sum())
                for p in (u[b], v[b]):
                    n["nan"] += int(np.isnan(p).sum())
                    n["pos_inf"] += int(np.isposinf(p).sum())
                    n["neg_inf"] += int(np.isneginf(p).sum())
                    n["huge"] += int((np.abs(p) == F(1e30)).sum())
                    n["neg_zero"] += int((np.signbit(p) & (p == 0)).sum())
                n["edge_x0"] += int((m & (mx == 0) & (u[b] != 0)).sum())
                n["edge_x1"] += int((m & (mx == F(W - 1)) & (u[b] != 0)).sum())
                n["edge_y0"] += int((m & (my == 0) & (v[b] != 0)).sum())
                n["edge_y1"] += int((m & (my == F(H - 1)) & (v[b] != 0)).sum())
                n["clamped_tap"] += int((m & (((mx == F(W - 1)) & (W > 1)) | ((my == F(H - 1)) & (H > 1)))).sum())
                for key, a in (("tie_x", mx), ("tie_y", my)):
                    a32, fr = _frac32(a)
                    tp = np.floor(a32) + F(0.5)
                    n[key] += int((m & (fr == F(0.5))).sum())
                    n[key + "_below"] += int((m & (a32 == np.nextafter(tp, F(-np.inf)))).sum())
                    n[key + "_above"] += int((m & (a32 == np.nextafter(tp, F(np.inf)))).sum())
                    odd = np.floor(a32).astype(np.int64) % 2 == 1
                    n["tie_even_down"] += int((m & (fr == F(0.5)) & ~odd).sum())   # rint goes down
                    n["tie_odd_up"] += int((m & (fr == F(0.5)) & odd).sum())       # rint goes up
            n["score_0"] += int((s == 0).sum())
            n["score_2"] += int((s == 2).sum())
            n["score_inf_invalid"] += int((~m).sum())
            n["score_inf_B0"] += int((m & (B == 0) & (Cc != 0)).sum())
            n["score_inf_C0"] += int((m & (Cc == 0) & (B != 0)).sum())
            n["finite"] += int(np.isfinite(s).sum())
            assert np.all(np.isposinf(s[~m])) and not np.isnan(s).any()
            # the window of a valid px: cut by the frame or by an invalid px, or complete
            ys, xs = np.mgrid[0:H, 0:W]
            in_frame = ((np.minimum(xs + r, W - 1) - np.maximum(xs - r, 0) + 1) *
                        (np.minimum(ys + r, H - 1) - np.maximum(ys - r, 0) + 1))
            per_r[r]["truncated"] += int((m & (sums[0] < (2 * r + 1) ** 2)).sum())
            per_r[r]["full"] += int((m & (sums[0] == (2 * r + 1) ** 2)).sum())
            n["truncated_by_m"] += int((m & (sums[0] < in_frame)).sum())
            fin = np.isfinite(s)
            if case.kind == "identical":
                assert m.all() and np.all(s[B > 0] == 0) and np.all(np.isposinf(s[B == 0]))
            if case.kind == "negative":
                assert m.all() and np.all(s[B > 0] == 2)
            if case.kind == "shift":   # 0 wherever the whole window moved with the flow
                dx, dy = int(u[b][0, 0]), int(v[b][0, 0])
                assert np.array_equal(m, (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H))
                assert np.all(s[fin] == 0)
            if case.kind == "const0":
                assert (B == 0).all() and not fin.any()
            if case.kind == "const1":
                assert (Cc[m] == 0).all() and not fin.any()
            if case.kind == "edges":
                assert m.all()
    empty = [k for k, c in n.items() if c == 0]
    assert not empty, (empty, n)
    assert all(c["truncated"] > 0 and c["full"] > 0 for c in per_r.values()), per_r


def test_table_covers_the_sizes_layouts_and_radii():
    sizes = {(c.W, c.H) for c in T.CASES if c.roi is None and c.n == 1}
    assert sizes == set(T.SIZES) == {(1, 1), (1, 7), (5, 1), (3, 256), (67, 45), (257, 131)}
    for size in T.SIZES:
        assert {c.kind for c in T.CASES if (c.W, c.H) == size and c.n == 1 and not c.roi} == set(T.KINDS)
    assert {c.r for c in T.CASES} == {1, 2, 3, 4}
    for kind in T.KINDS:   # every kind meets more than one radius over the sizes
        assert len({c.r for c in T.CASES if c.kind == kind}) == 4, kind
    roi = [c for c in T.CASES if c.roi]
    assert roi and all((c.W, c.H) == (130, 70) and c.roi[:2] == (160, 80) for c in roi)
    assert all(c.roi[2] % 2 == 1 and (4 * c.roi[2]) % 16 == 4 and (4 * c.roi[0]) % 16 == 0 for c in roi)
    assert {c.r for c in roi} == {1, 2, 3, 4}
    batch = [c for c in T.CASES if c.n > 1]
    assert [(c.n, c.W, c.H, c.shared0) for c in batch] == [(257, 130, 20, False), (257, 130, 20, True)]


@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_vectorised_sums_equal_a_loop_per_px(r):
    seen = 0
    for case in T.CASES:
        if (case.W, case.H) not in ((1, 1), (1, 7), (5, 1)) or case.roi:
            continue
        I0, I1, u, v = T.planes(case)
        J, m = ref.warp(I1[0], u[0], v[0])
        fast = ref.window_sums(I0[0], J, m, r)
        slow = ref.window_sums_bruteforce(I0[0], J, m, r)
        for a, b in zip(fast, slow):
            assert np.array_equal(a, b), case.name
        seen += 1
    assert seen >= 3 * len(T.KINDS)
    # and on a frame larger than the window, with invalid px inside it
    case = next(c for c in T.CASES if c.name.startswith("67x45-special"))
    I0, I1, u, v = T.planes(case)
    J, m = ref.warp(I1[0][:20, :24], u[0][:20, :24], v[0][:20, :24])
    assert not m.all()
    for a, b in zip(ref.window_sums(I0[0][:20, :24], J, m, r), ref.window_sums_bruteforce(I0[0][:20, :24], J, m, r)):
        assert np.array_equal(a, b)


def test_step_1_on_hand_made_px():
    I1 = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    z = np.zeros((2, 3), F)
    J, m = ref.warp(I1, z, z)
    assert m.all() and np.array_equal(J, I1)
    u = z.copy()
    u[0, 0] = 0.5                     # halfway between 10 and 20
    u[0, 1] = F(1) / F(64)            # ix = rint(32.5) = 32 (half to even): exactly px 1
    u[0, 2] = np.nextafter(F(0), F(1))   # inside (mx = 2 after rounding)
    u[1, 2] = F(2.0 ** -20)           # 2 + 2^-20 is above 2: outside
    u[1, 0] = -0.0
    v = z.copy()
    v[1, 1] = np.nan
    J, m = ref.warp(I1, u, v)
    assert J[0, 0] == 15 and J[0, 1] == 20 and J[0, 2] == 30 and J[1, 0] == 40
    assert m.tolist() == [[True, True, True], [True, False, False]] and J[1, 1] == 0 and J[1, 2] == 0
    u[0, 1] = F(3) / F(64)            # ix = rint(33.5) = 34: 2/32 of the way from 20 to 30
    assert ref.warp(I1, u, v)[0][0, 1] == (20 * 30 * 32 + 30 * 2 * 32 + 512) >> 10


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


def test_cli_plan_lists_the_zncc_keys(tmp_path, cfg):
    base = _plans(_plan(tmp_path, cfg, "a.json"))
    assert "zncc" not in base[0]
    # off, and the other two keys without it, change nothing
    assert _plans(_plan(tmp_path, {**cfg, "zncc": False, "znccOversample": 9, "znccOutput": True}, "b.json")) == base
    (pl,) = _plans(_plan(tmp_path, {**cfg, "zncc": True}, "c.json"))
    assert pl["zncc"] == {"radius": 3, "beta": 0.25, "oversample": 4, "output": False}
    assert pl["strip_batch"] is True   # the global key stays in the strip batch
    assert {k: v for k, v in pl.items() if k != "zncc"} == base[0]
    (pl,) = _plans(_plan(tmp_path, {**cfg, "zncc": {"radius": 1, "beta": 0.5}, "znccOversample": 7,
                                   "znccOutput": True}, "d.json"))
    assert pl["zncc"] == {"radius": 1, "beta": 0.5, "oversample": 7, "output": True}
    # per image over global, and an oversample below 1 is 1
    c2 = {**cfg, "zncc": True, "znccOversample": 0}
    c2["images"] = [{**cfg["images"][0], "zncc": {"beta": 0.125}}]
    (pl,) = _plans(_plan(tmp_path, c2, "e.json"))
    assert pl["zncc"] == {"radius": 3, "beta": 0.125, "oversample": 1, "output": False}
    assert pl["strip_batch"] is False   # a per-image key is not a production key
    c2["images"] = [{**cfg["images"][0], "zncc": False}]
    assert "zncc" not in _plans(_plan(tmp_path, c2, "f.json"))[0]
    # "consistency" alone is listed as before
    (pl,) = _plans(_plan(tmp_path, {**cfg, "consistency": True, "zncc": False}, "g.json"))
    assert "zncc" not in pl and pl["consistency"] == {"alpha": pytest.approx(0.01), "beta": 0.5,
                                                      "oversample": 4, "output": False}


def test_cli_zncc_config_errors(tmp_path, cfg):
    msg = "zncc cannot be combined with feature alignment"
    r = _plan(tmp_path, {**cfg, "zncc": True, "features": 1}, "g.json")
    assert r.returncode != 0 and msg in r.stderr
    c2 = {**cfg, "features": 1}
    c2["images"] = [{**cfg["images"][0], "zncc": {"radius": 2}}]
    r = _plan(tmp_path, c2, "h.json")
    assert r.returncode != 0 and msg in r.stderr
    assert _plans(_plan(tmp_path, {**cfg, "zncc": False, "features": 1}, "i.json"))[0]["features"] is True
    # together with "consistency", globally or per image
    r = _plan(tmp_path, {**cfg, "zncc": True, "consistency": True}, "j.json")
    assert r.returncode != 0 and "zncc cannot be combined with consistency" in r.stderr
    c3 = {**cfg, "consistency": {"alpha": 0.0}}
    c3["images"] = [{**cfg["images"][0], "zncc": True}]
    r = _plan(tmp_path, c3, "k.json")
    assert r.returncode != 0 and "zncc cannot be combined with consistency" in r.stderr
    for bad in (0, 5):
        r = _plan(tmp_path, {**cfg, "zncc": {"radius": bad}}, f"r{bad}.json")
        assert r.returncode != 0 and "radius must be 1..4" in r.stderr


@pytest.mark.parametrize("fast_math", [0, 2], ids=["ieee", "fma"])
def test_score_rejects_a_region_of_one_slice_only(built, fast_math):
    from oracle import checker
    I0, I1 = FB.patch_pair()
    p = capi.make_params(fast_math=fast_math, **FB.PATCH_PARAMS)
    uf, vf = checker.oracle_calc(I0, I1, p)[:2]
    score = ref.zncc_score(I0, I1, uf, vf, 3)
    rej = ~ref.accepted(score, 0.25)
    inp, far = FB.patch_masks(16)
    assert (int(inp.sum()), int(far.sum())) == (2304, 14080)
    share_in, share_out = float(rej[inp].mean()), float(rej[far].mean())
    print(f"rejected share inside the patch {share_in:.4f}, outside {share_out:.4f}, "
          f"+inf share {float(np.isposinf(score).mean()):.4f}")
    assert share_in - share_out > MARGIN, (share_in, share_out)
