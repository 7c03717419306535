#!/bin/bash
# How the files of this folder were made: one MI355X, from the repository root.
set -e
python -m pytest -q tests/test_cli_shift_gpu.py > profiles/shift_estimate/cli_tests.log
python tools/shift_measure.py profiles/shift_estimate                      # measure.json
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/shift_trace -o run -- \
  python tools/shift_measure.py profiles/shift_estimate --trace            # measure_trace.json
cp /tmp/shift_trace/run_kernel_stats.csv profiles/shift_estimate/kernel_stats.csv
python tools/shift_measure.py --per-launch /tmp/shift_trace/run_kernel_trace.csv > profiles/shift_estimate/per_launch.txt
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`, three
# runs in a checkout of the parent commit with its own build and three in this one, alternating.
