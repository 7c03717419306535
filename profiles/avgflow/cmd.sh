#!/bin/bash
# How the files of this folder were made: one MI355X, one call, from the repository root.
# S = a scratch folder for the 16-slice stack (1.6 GB with the outputs).
set -e
S=${1:?scratch folder}
python tools/avgflow_measure.py gen $S
python tools/avgflow_measure.py cli $S profiles/avgflow          # timing.json, stats.json, cli_stdout.txt
python tools/avgflow_measure.py kernels $S profiles/avgflow      # measure.json
# bench_parent_N.json / bench_new_N.json: `python bench.py --gpus 1 --steps 20 --warmup 5`, three
# runs in a checkout of the parent commit with its own build and three in this one, alternating.
