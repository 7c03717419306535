#!/bin/bash
# How the files of this folder were made: one MI355X, from the repository root.
set -e
python tools/compose_measure.py profiles/compose                          # measure.json
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`,
# N = 1..3: one call (the same as measure.json's), three alternations, a checkout of the parent
# commit with its own build first, then this one.
# kernel_resources_vs_parent.diff: `python tools/kernel_resources.py` of the parent against this
# build (no GPU needed): one added kernel, nothing else.
# gpu_compose_tests.log, cli_compose_tests.log: `python -m pytest -q -m gpu
# tests/test_gpu_compose.py` and `tests/test_cli_compose_gpu.py` in calls of their own on the
# same kind of box.
