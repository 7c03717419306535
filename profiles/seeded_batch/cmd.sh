#!/bin/bash
# How the files of this folder were made: one MI355X, from the repository root.  PARENT is a
# checkout of the parent commit with its own build.
set -e
O=profiles/seeded_batch
python -m pytest tests/test_gpu_batch_const_seed.py tests/test_cli_seeded_batch_gpu.py -m gpu -q --durations=12 > $O/new_gpu_tests.log
python -m pytest tests -m gpu -q --durations=15 | tail -22 > $O/gpu_suite_tail.txt
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt
# solver unmoved: three alternations per workload in one call
for i in 1 2 3; do
  (cd $PARENT && python bench.py --gpus 1 --steps 20 --warmup 5) > $O/bench_parent_$i.json
  python bench.py --gpus 1 --steps 20 --warmup 5 > $O/bench_new_$i.json
done
for i in 1 2 3; do   # bench.py --full's production_strips workload, as a run of its own
  (cd $PARENT && python bench.py --gpus 1 --workload strips --steps 40 --warmup 5) > $O/strips_parent_$i.json
  python bench.py --gpus 1 --workload strips --steps 40 --warmup 5 > $O/strips_new_$i.json
done
python tools/seeded_batch_measure.py chain $O                          # chain.json
python tools/seeded_batch_measure.py cli $O --slices 385 --reps 3      # cli.jsonl, cli_summary.json
# first_run/: an earlier call on another box with --steps 10 --warmup 3 for the strips and
# --slices 129 --reps 2 for the CLI job (chain.json is from that call).
# no GPU: the code-object notes of this tree, and their diff against the parent's
python tools/kernel_resources.py --out $O/kernel_resources.txt
(cd $PARENT && python tools/kernel_resources.py) | diff - $O/kernel_resources.txt > $O/kernel_resources_vs_parent.diff || true
