#!/bin/bash
# How the files of this folder were made.  PARENT is a second checkout of the parent commit with
# its own build; both trees on one MI355X, nothing else of ours on the card.
#
# kernel_resources_vs_parent.diff (empty: no kernel moved; no GPU needed)
python tools/kernel_resources.py --out new.txt; (cd PARENT && python tools/kernel_resources.py --out parent.txt)
diff PARENT/parent.txt new.txt > profiles/batch_walk/kernel_resources_vs_parent.diff
# set1/: three alternations, the parent first; one call
for i in 1 2 3; do for tree in PARENT .; do (cd $tree
  python bench.py --gpus 1 --steps 20 --warmup 5 --workload strips | tail -1   # bench_strips_{parent,new}_$i.json
  python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1); done; done         # bench_{parent,new}_$i.json
# set2/: the same in a second call (another box), this build first in every alternation
# set3/: the same in a third call, the parent first
# gpu_batch_tests_tail.txt: python -m pytest -v -m gpu --durations=15 tests/test_gpu_batch.py \
#   tests/test_gpu_batch_const_seed.py tests/test_gpu_fast_bitwise.py tests/test_cli_batch_gpu.py
