#!/bin/bash
# How the files of this folder were made: one MI355X, from the repository root.
set -e
python tools/zncc_measure.py profiles/zncc_score                          # measure.json
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`;
# bench_strips_*_N.json: `python bench.py --gpus 1 --workload strips --steps 40 --warmup 5`.
# N = 1..3: one call, three alternations, a checkout of the parent commit with its own build
# first, then this one.  N = 4..6 (full frames only): a second call with this build first, made
# because whichever build ran first in an alternation of the first call was the faster by 0.07 %.
# kernel_resources_vs_parent.diff: `python tools/kernel_resources.py` of the parent against this
# build (no GPU needed): five added kernels, nothing else.
# gpu_zncc_tests.log, cli_tests.log: `python -m pytest -q tests/test_gpu_zncc.py` and
# `tests/test_cli_zncc_gpu.py tests/test_cli_consistency_gpu.py` in earlier calls on the same
# kind of box.
