#!/bin/bash
# How the files of this folder were made.  PARENT is a second checkout of the parent commit
# with its own bin/optflow, linked against the same engine library (csrc/ is unchanged).
#
# equal.txt, plan_equal.txt: equal_jobs.py runs both binaries on every job variant from a
# directory of their own with relative paths and compares exit status, stdout, stderr, every
# output file byte for byte, and stats_json without "seconds" (time-seeded random_points jobs:
# stats_json and the shapes of the records).  With --plan no GPU is needed.
OPTFLOW_PARENT=PARENT/fibsem-optflow_amd/bin/optflow python profiles/cli_split/equal_jobs.py WORK > profiles/cli_split/equal.txt
OPTFLOW_PARENT=PARENT/fibsem-optflow_amd/bin/optflow python profiles/cli_split/equal_jobs.py WORK_PLAN --plan > profiles/cli_split/plan_equal.txt
# kernel_resources.diff (empty: the engine did not move)
python tools/kernel_resources.py --out new.txt; (cd PARENT && python tools/kernel_resources.py --out parent.txt)
diff PARENT/parent.txt new.txt > profiles/cli_split/kernel_resources.diff
# speed.txt: the production strip job, both binaries alternating on one stack, 3 runs per arm
for i in 1 2 3; do for bin in PARENT/fibsem-optflow_amd/bin/optflow fibsem-optflow_amd/bin/optflow; do
  python tools/cli_e2e.py --format tiff --jobs strips --no-single-thread --slices 401 --strides 1-120 \
    --out STACK --bin $bin; done; done > profiles/cli_split/speed.txt
# bench.txt
python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > profiles/cli_split/bench.txt
