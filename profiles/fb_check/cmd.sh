#!/bin/bash
# How the files of this folder were made: one MI355X, one call, from the repository root.
set -e
python tools/fbcheck_measure.py profiles/fb_check                          # measure.json
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`, in the
# same call, three alternations: a checkout of the parent commit with its own build, then this one.
# kernel_resources_vs_parent.diff: `python tools/kernel_resources.py` of the parent against this
# build (no GPU needed): two added kernels, nothing else.
# gpu_fbcheck_tests.log, cli_tests.log: `python -m pytest -q tests/test_gpu_fbcheck.py` and
# `tests/test_cli_consistency_gpu.py` in earlier calls on the same kind of box.
