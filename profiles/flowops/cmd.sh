#!/bin/bash
# How the files of this folder were made.  PARENT is a second checkout of the parent commit with
# its own build; both trees on one MI355X, nothing else of ours on the card.
#
# tests/golden/flowop_errors.json: the parent's library under this change's test code.  The edits
# to the four test_bad_arguments_return_before_a_launch tests and tests/flowop_badargs.py touch no
# engine code, so they were copied into PARENT/tests and run there in recording mode:
(cd PARENT && TVL1_FLOWOP_ERRORS_OUT=$PWD/flowop_errors.json python -m pytest -q -m gpu -k bad_arguments \
  tests/test_gpu_fbcheck.py tests/test_gpu_zncc.py tests/test_gpu_compose.py tests/test_gpu_invert.py)
cp PARENT/flowop_errors.json tests/golden/flowop_errors.json
# kernel_resources_vs_parent.diff (empty: no kernel moved; no GPU needed), exported_symbols.txt
python tools/kernel_resources.py --out new.txt; (cd PARENT && python tools/kernel_resources.py --out parent.txt)
diff PARENT/parent.txt new.txt > profiles/flowops/kernel_resources_vs_parent.diff
diff <(nm -D --defined-only PARENT/fibsem-optflow_amd/lib/libtvl1_hip.so | awk '{print $2, $3}' | sort) \
     <(nm -D --defined-only fibsem-optflow_amd/lib/libtvl1_hip.so | awk '{print $2, $3}' | sort) \
  > profiles/flowops/exported_symbols_vs_parent.diff
# diff_stat.txt, section_lines.txt
git diff --stat HEAD > profiles/flowops/diff_stat.txt
# cpu_tests_tail.txt, gpu_tests_tail.txt
python -m pytest -q -m "not gpu" tests | tail -5 > profiles/flowops/cpu_tests_tail.txt
python -m pytest -q -m gpu --durations=15 tests | tail -25 > profiles/flowops/gpu_tests_tail.txt
# bench_{parent,new}_{1,2,3}.json: three alternations in one call, the parent first
for i in 1 2 3; do for tree in PARENT .; do (cd $tree
  python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1); done; done
# measure_{compose,invert}_{parent_a,new,parent_b}.json: the utility calls' own timings, in the same call,
# in that order (two runs of the parent give the run-to-run difference)
for tool in compose invert; do for arm in PARENT . PARENT; do (cd $arm
  python tools/${tool}_measure.py OUT); done; done
