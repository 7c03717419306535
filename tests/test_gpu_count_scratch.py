"""The counted utility calls share one count scratch per ctx (csrc/tvl1_engine.hip, run_chunks):
tvl1_zero_above_batch, tvl1_invert_flow_batch, tvl1_compose_flow_batch and tvl1_zero_above_batch
again, on one ctx and one stream with nothing between them, each with its host counts.  A call
that read another's counters, or a chunk that read the previous chunk's, would change a count:
every count and every plane must equal the restatements' (tests/fbcheck_ref.py,
tests/invert_ref.py, tests/compose_ref.py), bit for bit.  n = 2, and n = 257: the smallest batch
with a second chunk."""
import numpy as np
import pytest

import compose_cases as CT
import compose_ref as cref
import fbcheck_ref as fref
import invert_ref as iref
from optflow_amd import capi
from test_gpu_compose import SENTINEL, Planes, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K, TOL, BETA = 2, 0.01, 1.0


@pytest.fixture(scope="module")
def eng0(built):
    e = capi.Engine(capi.make_params())
    yield e
    e.close()


@pytest.mark.parametrize("n, W, H", [(2, 20, 6), (257, 8, 3)], ids=["n2-20x6", "n257-8x3"])
def test_counted_calls_in_a_row_keep_their_own_counts(eng0, n, W, H):
    e = eng0
    # (reversed: the case's last pair zeroes whole, and the pair alone in the second chunk should count)
    ua, va, ub, vb = (a[::-1].copy() for a in CT.planes(CT.Case(f"scratch{n}x{W}x{H}", W, H, "smooth", n=n)))
    # the restatements, chained as the calls are: zero a where !(ub <= BETA); g = inverse of that a;
    # c = a o b; zero g where !(resid <= TOL)
    z1 = [fref.zero_above(ua[b], va[b], ub[b], BETA) for b in range(n)]
    au, av = np.stack([z[0] for z in z1]), np.stack([z[1] for z in z1])
    inv = [iref.invert(au[b], av[b], K, TOL) for b in range(n)]
    com = [cref.compose(au[b], av[b], ub[b], vb[b]) for b in range(n)]
    z2 = [fref.zero_above(inv[b][0], inv[b][1], inv[b][2], TOL) for b in range(n)]

    blank = np.full(ua.shape, SENTINEL, np.float32)
    d = [Planes(a) for a in (ua, va, ub, vb)]
    gu, gv, rs, cu, cv = (Planes(blank) for _ in range(5))
    torch.cuda.synchronize()
    P, S, st = d[0].pitch, d[0].stride, e.stream
    rej1 = e.zero_above_batch(n, d[0].ptr, d[1].ptr, P, S, d[2].ptr, P, S, W, H, BETA, stream=st)
    cinv = e.invert_flow_batch(n, d[0].ptr, d[1].ptr, P, S, K, TOL, gu.ptr, gv.ptr, P, S, rs.ptr, P, S, W, H,
                               stream=st)
    ccom = e.compose_flow_batch(n, d[0].ptr, d[1].ptr, P, S, d[2].ptr, d[3].ptr, P, S, W, H, cu.ptr, cv.ptr,
                                P, S, stream=st)
    rej2 = e.zero_above_batch(n, gu.ptr, gv.ptr, P, S, rs.ptr, P, S, W, H, TOL, stream=st)
    torch.cuda.synchronize()

    assert [int(x) for x in rej1] == [z[2] for z in z1]
    assert [tuple(int(x) for x in c) for c in cinv] == [o[3:5] for o in inv]
    assert [int(x) for x in ccom] == [o[2] for o in com]
    assert [int(x) for x in rej2] == [z[2] for z in z2] == [o[4] for o in inv]
    # the counts are no constants, the last pair's included: a stale or a foreign record would show
    assert len({int(x) for x in rej1}) > 1 and sum(int(x) for x in rej2) > 0
    assert int(cinv[-1][0]) > 0 and int(ccom[-1]) > 0 and int(cinv[-1][0]) != int(ccom[-1])
    for got, want, what in ((d[0], au, "ua"), (d[1], av, "va"), (rs, np.stack([o[2] for o in inv]), "resid"),
                            (cu, np.stack([o[0] for o in com]), "uc"), (cv, np.stack([o[1] for o in com]), "vc"),
                            (gu, np.stack([z[0] for z in z2]), "ug"), (gv, np.stack([z[1] for z in z2]), "vg")):
        g, clean = got.get()
        assert clean and same_bits(g, want), what
