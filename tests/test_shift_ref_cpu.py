"""The integer drift estimate without a GPU: tests/shift_ref.py (the numpy restatement the GPU
is held to, tests/test_gpu_shift.py) on its known-answer table, the tie rules and the range and
depth of every result; the library's symbols and argument checks; and the CLI's
`"initialFlow": "auto"` as `optflow --plan` resolves it."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
from PIL import Image

import avgflow_ref
import initflow_ref
import shift_ref as ref
from optflow_amd import capi

OPTFLOW = capi.PKG_ROOT / "bin" / "optflow"


# ---- the specification
@pytest.mark.parametrize("i", range(len(ref.KNOWN)))
def test_known_answers(i):
    w, h, d, R = ref.KNOWN[i]
    I0, I1, e = ref.known_pair(i)
    assert (e["dx"], e["dy"]) == d
    assert e["levels"] == ref.levels_of(R) + 1
    assert e["count"] == (w - abs(d[0])) * (h - abs(d[1])) and e["count_zero"] == w * h
    assert e["sad"] == ref.sad(I0, I1, *d)[0] and e["sad_zero"] == ref.sad(I0, I1, 0, 0)[0]


def test_levels():
    want = {1: 0, 4: 0, 5: 1, 8: 1, 9: 2, 16: 2, 17: 3, 25: 3, 32: 3, 33: 4, 64: 4, 65: 5, 128: 5}
    for R, L in want.items():
        assert ref.levels_of(R) == L
        assert ref.ceil_div_pow2(R, L) <= 4 and (L == 0 or ref.ceil_div_pow2(R, L - 1) > 4)


def test_cli_pair_whole_and_strips():
    I0, I1 = initflow_ref.frames_of(initflow_ref.CLI)
    for a, b, R in ((I0, I1, 32), (I0[:48], I1[:48], 12), (I0[-48:], I1[-48:], 12)):
        e = ref.estimate(a, b, R)
        assert (e["dx"], e["dy"], e["sad"]) == (12, -9, 0)


def test_ties_and_constant_frames():
    s0, s1 = ref.stripes(64, 48)
    assert np.array_equal(s0, s1)
    e = ref.estimate(s0, s1, 8)          # (0, 0), (+-4, 0), (+-8, 0) ... all have S = 0
    assert (e["dx"], e["dy"], e["sad"]) == (0, 0, 0)
    e = ref.estimate(*ref.stripes(64, 48, roll=2), 8)   # (-2, 0) and (2, 0) tie: the smaller dx
    assert (e["dx"], e["dy"], e["sad"]) == (-2, 0, 0)
    c = np.full((40, 96), 77, np.uint8)
    e = ref.estimate(c, c, 10)
    assert (e["dx"], e["dy"], e["sad"], e["sad_zero"]) == (0, 0, 0, 0)


def test_comparison_rule():
    # equal means 2/4 and 3/6: the norm, then dy, then dx decide
    assert ref.better((2, 4, 1, 0), (3, 6, 1, 1)) and not ref.better((3, 6, 1, 1), (2, 4, 1, 0))
    assert ref.better((0, 5, 0, -1), (0, 7, 0, 1)) and ref.better((0, 5, -1, 0), (0, 7, 1, 0))
    assert ref.better((0, 5, 1, -1), (0, 5, -1, 1))       # dy before dx
    assert ref.better((5, 10, 3, 3), (6, 11, 0, 0))       # 55 < 60: the mean comes first
    big = (255 << 26, 1 << 26, 0, 0)
    assert not ref.better(big, big)                       # the products stay below 2^64


@pytest.mark.parametrize("w,h,true,R", [(96, 40, (14, 0), 10), (64, 48, (-9, 11), 8), (130, 70, (0, 9), 5)])
def test_result_stays_within_R(w, h, true, R):
    """A true shift outside R: some in-range shift comes back, and both sums with it."""
    I0, I1 = ref.window_pair(w, h, *true, rng=40)
    e = ref.estimate(I0, I1, R)
    assert abs(e["dx"]) <= R and abs(e["dy"]) <= R
    assert e["sad"] * e["count_zero"] <= e["sad_zero"] * e["count"]   # (0, 0) was a candidate


def test_half_is_the_stack_half():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (46, 66), dtype=np.uint8)
    assert np.array_equal(ref.half(a), avgflow_ref.half(a))
    odd = rng.integers(0, 256, (47, 67), dtype=np.uint8)
    assert np.array_equal(ref.half(odd), avgflow_ref.half(odd[:46, :66]))


def test_sad_table_layout():
    I0, I1 = ref.window_pair(33, 32, 1, 0, rng=2)
    t = ref.sad_table(I0, I1, 2, -1, 1).reshape(3, 3)
    assert t[0, 2] == ref.sad(I0, I1, 3, -2)[0] and t[2, 0] == ref.sad(I0, I1, 1, 0)[0]   # [dy, dx]
    assert (ref.sad_table(I0, I1, 40, 0, 1) == 0).all()


# ---- the library
def test_library_exports_and_null_ctx(built):
    lib = capi.load_engine()
    for name in ("tvl1_estimate_shift", "tvl1_estimate_shift_batch", "tvl1_sad_shifts_u8"):
        assert hasattr(lib, name)
    assert C.sizeof(capi.TVL1Shift) == 48
    rec = capi.TVL1Shift()
    p = C.c_void_p(4096)   # never dereferenced: a NULL ctx is refused first
    assert lib.tvl1_estimate_shift(None, p, 64, p, 64, 64, 48, 8, C.byref(rec), None) == 1
    assert b"ctx" in lib.tvl1_last_error(None)
    sad = (C.c_uint64 * 9)()
    assert lib.tvl1_sad_shifts_u8(None, p, 64, p, 64, 64, 48, 0, 0, 1, sad, None) == 1


def test_struct_layout_matches_header(built, tmp_path):
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tvl1.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(tvl1_shift), '
                   'offsetof(tvl1_shift, levels), offsetof(tvl1_shift, sad), '
                   'offsetof(tvl1_shift, sad_zero), offsetof(tvl1_shift, count_zero));return 0;}\n')
    subprocess.run(["gcc", "-I", str(capi.REPO_ROOT / "include"), "-o", str(tmp_path / "probe"), str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    S = capi.TVL1Shift
    assert got == [C.sizeof(S), S.levels.offset, S.sad.offset, S.sad_zero.offset, S.count_zero.offset]


# ---- the CLI's key, resolved without a GPU (optflow --plan)
@pytest.fixture
def cfg(tmp_path, built):
    rng = np.random.default_rng(9)
    for n in ("p", "q"):
        Image.fromarray(rng.integers(0, 256, (61, 83), dtype=np.uint8)).save(tmp_path / f"{n}.png")
    return {"output_dir": str(tmp_path), "scale": 1, "output_type": "flow",
            "rois": {"top": 20, "bottom": 20},
            "images": [{"p": str(tmp_path / "p.png"), "q": str(tmp_path / "q.png"),
                        "output_name": "pq"}]}


def _plan(tmp_path, cfg, name):
    p = tmp_path / name
    p.write_text(json.dumps(cfg))
    return subprocess.run([str(OPTFLOW), "--plan", str(p)], capture_output=True, text=True, timeout=120)


def _plans(r):
    assert r.returncode == 0, r.stderr
    out = r.stdout
    return json.loads(out[out.index("\n[") + 1:] if not out.startswith("[") else out)


def test_cli_auto_in_the_plan(tmp_path, cfg):
    base = _plans(_plan(tmp_path, cfg, "a.json"))
    assert base[0]["strip_batch"] is True and "initialFlow" not in base[0]
    # inert without the flag: the plan is the base plan
    assert _plans(_plan(tmp_path, {**cfg, "initialFlow": "auto", "initialFlowMaxShift": 7}, "b.json")) == base
    # any other string stays inert with it
    assert _plans(_plan(tmp_path, {**cfg, "useInitialFlow": True, "initialFlow": "Auto"}, "c.json")) == base
    (pl,) = _plans(_plan(tmp_path, {**cfg, "useInitialFlow": True, "initialFlow": "auto"}, "d.json"))
    assert pl["initialFlow"] == "auto" and pl["initialFlowMaxShift"] == 32 and pl["strip_batch"] is False
    assert {k: v for k, v in pl.items() if k not in ("initialFlow", "initialFlowMaxShift", "strip_batch")} == \
           {k: v for k, v in base[0].items() if k != "strip_batch"}


def test_cli_auto_precedence(tmp_path, cfg):
    c2 = {**cfg, "useInitialFlow": True, "initialFlow": [1, 2], "initialFlowMaxShift": 20}
    c2["images"] = [{**cfg["images"][0], "initialFlow": "auto"}]
    (pl,) = _plans(_plan(tmp_path, c2, "e.json"))
    assert pl["initialFlow"] == "auto" and pl["initialFlowMaxShift"] == 20
    c2["images"] = [{**cfg["images"][0], "initialFlow": "auto", "initialFlowMaxShift": 9}]
    (pl,) = _plans(_plan(tmp_path, c2, "f.json"))
    assert pl["initialFlowMaxShift"] == 9
    # a numeric seed per image over a global "auto"
    c3 = {**cfg, "useInitialFlow": True, "initialFlow": "auto"}
    c3["images"] = [{**cfg["images"][0], "initialFlow": [-3.5, 4.25]}]
    (pl,) = _plans(_plan(tmp_path, c3, "g.json"))
    assert pl["initialFlow"] == [-3.5, 4.25] and "initialFlowMaxShift" not in pl


def test_cli_auto_with_features_fails(tmp_path, cfg):
    r = _plan(tmp_path, {**cfg, "useInitialFlow": True, "initialFlow": "auto", "features": 1}, "h.json")
    assert r.returncode != 0 and "initialFlow cannot be combined with feature alignment" in r.stderr
    assert _plans(_plan(tmp_path, {**cfg, "initialFlow": "auto", "features": 1}, "i.json"))[0]["features"] is True
