#!/bin/bash
# How the files of this folder were made: one MI355X, one call, from the repository root.
set -e
python -m pytest -q -m gpu tests/test_gpu_invert.py --durations=8 > profiles/invert/gpu_invert_tests.log
python -m pytest -q -m gpu tests/test_cli_invert_gpu.py --durations=5 > profiles/invert/cli_invert_tests.log
python tools/invert_measure.py profiles/invert                            # measure.json
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`,
# N = 1..3: the same call, three alternations, a checkout of the parent commit with its own
# build first, then this one.
# kernel_resources_vs_parent.diff: `python tools/kernel_resources.py` of the parent against this
# build (no GPU needed): the two instantiations of k_invert_flow added, nothing else.
