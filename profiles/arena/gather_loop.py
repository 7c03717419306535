"""Steady-state cost of a call that enters and reserves without growing: tvl1_gather_flow, n = 4096,
1000 calls on one ctx after a warm-up call (no growth inside the loop).  Run from a checkout's root
with its built library; prints one JSON line (microseconds per call: median and spread of 5 rounds
of 1000)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path.cwd()
sys.path.insert(0, str(ROOT / "fibsem-optflow_amd"))
import torch  # noqa: E402
from optflow_amd import capi  # noqa: E402

dev = torch.device("cuda", 0)
n, elems = 4096, 512 * 512
uv = torch.randn((2, elems), dtype=torch.float32, device=dev)
off = np.random.default_rng(1).integers(0, elems, n)
eng = capi.Engine(capi.make_params())
torch.cuda.synchronize()
for _ in range(20):
    eng.gather_flow(uv[0].data_ptr(), uv[1].data_ptr(), elems, off, stream=eng.stream)
rounds = []
for _ in range(5):
    t0 = time.perf_counter()
    for _ in range(1000):
        eng.gather_flow(uv[0].data_ptr(), uv[1].data_ptr(), elems, off, stream=eng.stream)
    rounds.append((time.perf_counter() - t0) * 1e3)   # ms per 1000 calls = us per call
eng.close()
print(json.dumps(dict(tree=str(ROOT.name), n=n, calls=1000, us_per_call_rounds=[round(r, 2) for r in rounds],
                      us_per_call_median=round(float(np.median(rounds)), 2))))
