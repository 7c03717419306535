#!/bin/bash
# How the files of this folder were made.  PARENT is a second checkout of the parent commit with
# its own build; both trees on one MI355X, nothing else of ours on the card.
# kernel_resources_vs_parent.diff (empty: no kernel moved; no GPU needed), exported_symbols_vs_parent.diff
python tools/kernel_resources.py --out new.txt; (cd PARENT && python tools/kernel_resources.py --out parent.txt)
diff PARENT/parent.txt new.txt > profiles/arena/kernel_resources_vs_parent.diff
diff <(nm -D --defined-only PARENT/fibsem-optflow_amd/lib/libtvl1_hip.so | awk '{print $2, $3}' | sort) \
     <(nm -D --defined-only fibsem-optflow_amd/lib/libtvl1_hip.so | awk '{print $2, $3}' | sort) \
  > profiles/arena/exported_symbols_vs_parent.diff
# cpu_tests_tail.txt, gpu_suite_tail.txt, smoke.txt
python -m pytest -q -m "not gpu" tests | tail -1 > profiles/arena/cpu_tests_tail.txt
python -m pytest -q -m gpu --durations=15 tests | tail -25 > profiles/arena/gpu_suite_tail.txt
python -c "import __graft_entry__ as g; g.smoke()" > profiles/arena/smoke.txt
# bench_{parent,new}_{1,2,3}.json: three alternations in one call, the parent first
for i in 1 2 3; do for tree in PARENT .; do (cd $tree
  python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1); done; done
# gather_loop_{parent_a,new,parent_b}.json: the same call, in that order (two runs of the parent give
# the run-to-run difference)
for arm in PARENT . PARENT; do (cd $arm; python ROOT/profiles/arena/gather_loop.py); done
