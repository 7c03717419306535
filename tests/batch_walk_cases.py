"""The chunks behind tests/golden/batch_walk_sequence.json: small batches whose pairs leave the
warp loops at different iterations, each with a pair that continues past its first check after
a warp of exactly 2 iterations (the re-gather of the store prediction).  The frames are small
pyramids whose middle levels hover around the stopping threshold; the seeds were picked with
the oracle (tests/test_batch_walk_cpu.py checks what they were picked for)."""
import numpy as np

from optflow_amd import synth

# pair seeds; pair b's second frame is slice 1 + seed % 3
CHUNKS = [
    dict(W=97, H=61, params=dict(nscales=5, warps=4), seeds=[1028, 1093, 1098, 1069]),
    dict(W=97, H=61, params=dict(nscales=4, warps=5), seeds=[1242, 1307, 1472]),
    dict(W=130, H=33, params=dict(nscales=4, warps=5), seeds=[1073, 1055, 1013, 1042]),
    dict(W=48, H=30, params=dict(nscales=3, warps=5), seeds=[1123, 1207, 1231, 1126, 1127, 1128]),
    dict(W=260, H=66, params=dict(nscales=5, warps=5), seeds=[1151, 1270, 1323]),
]
KNOBS = ["", "TVL1_BATCH_GROUP=0", "TVL1_BATCH_FUSE=0", "TVL1_BATCH_STORE=1", "TVL1_BATCH_SMALL=0"]
KNOB_NAMES = sorted({k.split("=")[0] for k in KNOBS if k})


def chunk_pairs(ch):
    I0s, I1s = zip(*(synth.gen_pair(ch["W"], ch["H"], seed=s, z=1 + s % 3) for s in ch["seeds"]))
    return np.stack(I0s), np.stack(I1s)


def chunk_id(ch):
    return "%dx%d-%s" % (ch["W"], ch["H"], ",".join(f"{k}{v}" for k, v in ch["params"].items()))
