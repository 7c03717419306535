"""A ctx's scratch blocks across a growth (csrc/tvl1_arena.hpp: enter + reserve).

One ctx, two streams.  Each family of calls runs small on stream A, then large enough to grow its
block on stream B, then small again on A, with no host synchronisation in between beyond what the
call itself does: the second call retires the block the first may still read, zero-fills the new
one on the ctx's own stream and orders B behind both; the third re-lays the grown block in place
behind B's work.  Every result equals, bit for bit, the same call on a fresh ctx.  Then the ctx is
destroyed with its retired blocks and another one solves 64 x 48 bit-identically to the oracle.
Tiny shapes: the lifecycle can go wrong only at a growth, not at size.
"""
import ctypes as C

import numpy as np
import pytest

from optflow_amd import capi, synth
from oracle import checker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SOLVE = dict(nscales=3, warps=2)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _pairs(n, w, h, seed):
    fr = [synth.gen_pair(w, h, seed=seed + b) for b in range(n)]
    return _dev(np.stack([f[0] for f in fr])), _dev(np.stack([f[1] for f in fr]))


def _flows(n, w, h, seed, amp=1.5):
    rng = np.random.default_rng(seed)
    return _dev((amp * rng.standard_normal((2, n, h, w))).astype(np.float32))


# A family: job(big) uploads one call's inputs and returns (launch(eng, stream) -> what the call
# returned on the host, collect() -> its device outputs as numpy arrays, read after the streams
# are synchronised).
def calc(big):
    w, h = (96, 80) if big else (64, 48)
    d0, d1 = _pairs(1, w, h, 400 + big)
    uv = torch.zeros((2, h, w), dtype=torch.float32, device=d0.device)

    def launch(eng, st):
        eng.calc_device(d0.data_ptr(), w, d1.data_ptr(), w, w, h, uv[0].data_ptr(), uv[1].data_ptr(), 4 * w,
                        stream=st, stats=False)
    return launch, lambda: [uv.cpu().numpy()]


def calc_batch(big, w=96, h=24, const=False):
    n = 5 if big else 2
    d0, d1 = _pairs(n, w, h, 410)
    uv = torch.zeros((2, n, h, w), dtype=torch.float32, device=d0.device)
    seeds = np.array([[0.5 * b, -0.25 * b] for b in range(n)], np.float32) if const else None

    def launch(eng, st):
        eng.calc_batch_device(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h, uv[0].data_ptr(),
                              uv[1].data_ptr(), 4 * w, 4 * w * h, stream=st, init_const=seeds)
    return launch, lambda: [uv.cpu().numpy()]


def calc_const_alone(big):
    """gamma != 0: the pairs are solved one by one and take their constant as two planes in the seed
    block, 2 * 128 * 96 * 4 bytes at the large size: above its 64 KiB floor."""
    return calc_batch(False, *((128, 96) if big else (32, 32)), const=True)


def gather_flow(big):
    n = 5000 if big else 1   # 5000 offsets and values: above the block's 64 KiB floor
    uv = _flows(1, 100, 100, 420)
    off = np.random.default_rng(421 + big).integers(0, 100 * 100, n)
    return (lambda eng, st: eng.gather_flow(uv[0].data_ptr(), uv[1].data_ptr(), 100 * 100, off, stream=st),
            lambda: [])


def postprocess_affine(big):
    w = h = 64 if big else 32
    uv = _flows(1, w, h, 430)
    i1 = _dev(np.random.default_rng(431).integers(0, 4, (h, w), dtype=np.uint8))
    aff = (C.c_float * 6)(1.01, 0.02, 0.5, -0.02, 0.99, -0.25)

    def launch(eng, st):
        eng._check(eng.lib.tvl1_postprocess_affine(eng.ctx, uv[0].data_ptr(), uv[1].data_ptr(), 4 * w, i1.data_ptr(),
                                                   w, w, h, 0, aff, C.c_void_p(st)), "tvl1_postprocess_affine")
    return launch, lambda: [uv.cpu().numpy()]


def orb_detect(big):
    w, h = (160, 128) if big else (64, 64)
    f = _dev(np.random.default_rng(440 + big).integers(0, 256, (h, w), dtype=np.uint8))
    return lambda eng, st: eng.orb_detect(f.data_ptr(), w, w, h, stream=st), lambda: []


def estimate_shift_batch(big):
    n, w, h = 3 if big else 1, 64, 64
    d0, d1 = _pairs(n, w, h, 450)

    def launch(eng, st):
        rs = eng.estimate_shift_batch(n, d0.data_ptr(), w, w * h, d1.data_ptr(), w, w * h, w, h, 8, stream=st)
        return [np.array([[v for _, v in sorted(r.items())] for r in rs], np.int64)]
    return launch, lambda: []


def invert_counted(big):
    n, w, h = 3 if big else 1, 48, 40
    f = _flows(n, w, h, 460)
    g = torch.zeros((2, n, h, w), dtype=torch.float32, device=f.device)

    def launch(eng, st):
        return [eng.invert_flow_batch(n, f[0].data_ptr(), f[1].data_ptr(), 4 * w, 4 * w * h, 4, 0.01, g[0].data_ptr(),
                                      g[1].data_ptr(), 4 * w, 4 * w * h, 0, 0, 0, w, h, stream=st)]
    return launch, lambda: [g.cpu().numpy()]


FAMILIES = [(calc, SOLVE), (calc_batch, SOLVE), (gather_flow, SOLVE), (postprocess_affine, SOLVE),
            (orb_detect, SOLVE), (estimate_shift_batch, SOLVE), (calc_const_alone, dict(SOLVE, gamma=0.2)),
            (invert_counted, SOLVE)]


def _arrays(host, collected):
    out = list(collected)
    for x in (host if isinstance(host, (list, tuple)) else [] if host is None else [host]):
        out.append(np.asarray(x))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def shared(built):
    dev = torch.device("cuda", 0)
    eng = capi.Engine(capi.make_params(**SOLVE))
    yield eng, torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    eng.close()


def _grow(eng, sa, sb, family):
    """small on A, large on B, small on A again: every call's arrays, read after both streams are done"""
    jobs = [family(big) for big in (0, 1, 0)]
    torch.cuda.synchronize()   # the uploads, before the first call
    host = [launch(eng, st.cuda_stream) for (launch, _), st in zip(jobs, (sa, sb, sa))]
    sb.synchronize()
    sa.synchronize()
    return [_arrays(h, collect()) for h, (_, collect) in zip(host, jobs)]


@pytest.mark.parametrize("family,params", FAMILIES, ids=[f.__name__ for f, _ in FAMILIES])
def test_results_across_a_growth_equal_a_fresh_ctx(shared, family, params):
    eng, sa, sb = shared
    eng.set_params(capi.make_params(**params))
    got = _grow(eng, sa, sb, family)
    want = []
    for big in (0, 1):
        fresh = capi.Engine(capi.make_params(**params))
        launch, collect = family(big)
        torch.cuda.synchronize()
        h = launch(fresh, sa.cuda_stream)
        sa.synchronize()
        want.append(_arrays(h, collect()))
        fresh.close()
    assert all(len(a) > 0 for a in want) and all(x.size > 0 for x in want[1]), "the call returned nothing to compare"
    for k, big in enumerate((0, 1, 0)):
        assert _same(got[k], want[big]), (family.__name__, "call", k)


def test_destroy_with_retired_blocks_then_a_new_ctx_equals_the_oracle(built):
    dev = torch.device("cuda", 0)
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    p = capi.make_params(**SOLVE)
    eng = capi.Engine(p)
    _grow(eng, sa, sb, calc)
    _grow(eng, sa, sb, gather_flow)
    eng.close()
    I0, I1 = synth.gen_pair(64, 48, seed=470)
    eng = capi.Engine(p)
    u, v, st, wi = eng.calc_host(I0, I1)
    eng.close()
    ur, vr, _, wr = checker.oracle_calc(I0, I1, p)
    np.testing.assert_array_equal(wi, wr)
    assert _same([u, v], [ur, vr])
