"""bench.py --dump-outputs and the plain / --full split: a plain run times its steps and
writes the flow the last timed step computed, bit-identical to a direct solve of the same
synthetic pair and the same from run to run; what is measured beside the headline figure
(roofline, math modes, production strips, CPU baseline) is there only with --full."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
W, H, F = 320, 240, 2


def test_dump_sample_is_seeded_and_within_budget(tmp_path, monkeypatch):
    """Above the budget every array is cut to the same ascending sample of its elements,
    identical from call to call; below it the arrays are written whole."""
    torch = pytest.importorskip("torch")
    import bench
    n = W * H   # array k holds k * n + its own element indices (exact in float32)
    flows = [tuple((torch.arange(n) + (2 * j + c) * n).float().reshape(H, W) for c in range(2))
             for j in range(F)]
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 2 * F * 1000)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, 0, flows, [7, 9])
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert names == ["rank0_iterations.npy"] + [f"rank0_slot{j}_{c}.npy" for j in range(F)
                                                for c in "uv"]
    total = 0
    for name in names[1:]:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_BUDGET
    # one sample for all arrays: distinct elements in ascending order
    idx = np.load(tmp_path / "a" / "rank0_slot0_u.npy").astype(np.int64)
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "rank0_slot1_v.npy"), (idx + 3 * n))
    it = np.load(tmp_path / "a" / "rank0_iterations.npy")
    assert it.dtype == np.float64 and it.tolist() == [7.0, 9.0]
    monkeypatch.setattr(bench, "DUMP_BUDGET", 48 << 20)
    bench.dump_outputs(tmp_path / "c", 0, flows, [7, 9])
    assert np.array_equal(np.load(tmp_path / "c" / "rank0_slot1_u.npy"), flows[1][0].numpy())


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(built, tmp_path):
    from optflow_amd import capi, synth
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--width", str(W), "--height", str(H), "--inflight", str(F),
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "slice-pairs/s" and out["higher_is_better"] and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / (1e3 * F) - 1) < 1e-3   # pairs / s of the steps
    assert out["ranks"][0]["pairs"] == 2 * F    # exactly --steps timed steps
    for k in ("roofline", "pair_breakdown_ms", "single_pair_ms", "math_modes",
              "production_strips", "cpu_baseline"):
        assert out[k] is None, k
    eng = capi.Engine(capi.make_params(nscales=5, warps=30, iterations=300, epsilon=0.01))
    its = np.load(tmp_path / "rank0_iterations.npy")
    for j in range(F):
        I0, I1 = synth.gen_pair(W, H, seed=0x5EED, z=1 + j)
        u, v, st, _ = eng.calc_host(I0, I1)
        for name, want in (("u", u), ("v", v)):
            got = np.load(tmp_path / f"rank0_slot{j}_{name}.npy")
            assert got.dtype == np.float32 and got.shape == (H, W)
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
        assert its[j] == st["iterations_total"]
    assert its[0] == out["config"]["iterations_per_pair"]
    eng.close()
