"""The bad-argument rows of the flow-utility calls, shared by the four GPU tests
test_bad_arguments_return_before_a_launch (tests/test_gpu_{fbcheck,zncc,compose,invert}.py: real
device pointers, the engine's status and message) and by tests/test_planes_cpu.py (the same rows on
integer addresses, through csrc/tvl1_planes.hpp on a CPU).

A test's rows are stated on a namespace `A` of plane addresses: every plane of the test is dense,
W x H with n = 2 pairs (pitch P, pair stride S; the u8 frames of the ZNCC test P8, S8), `big` is
one plane of 2 H + 1 rows for overlapping views and `J` one u8 plane.  defaults(test, A) gives each
call's good arguments, rows(test, A) the (call, changed arguments, status) rows: the TVL1_EINVAL
rows first, then the TVL1_ESIZE rows.

The messages the rows raise are recorded in tests/golden/flowop_errors.json from the library of
the commit before the checks moved into tvl1_planes.hpp (profiles/flowops/README.md says how):
assert_recorded compares a test's messages to the record, or with TVL1_FLOWOP_ERRORS_OUT=<file>
writes them there instead.
"""
import json
import os
from pathlib import Path
from types import SimpleNamespace

W, H = 20, 6
P, S = 4 * W, 4 * W * H
P8, S8 = W, W * H + (-(W * H)) % 16        # the ZNCC test's planes start 16-byte aligned per pair
ZS = 4 * S8                                # ... so its f32 pair stride is this
NAN = float("nan")
GOLDEN = Path(__file__).resolve().parent / "golden" / "flowop_errors.json"

PLANES = {"fbcheck": ("d0", "d1", "d2", "d3", "s", "big"),
          "zncc": ("d0", "d1", "d2", "d3", "s", "big", "J"),
          "compose": ("d0", "d1", "d2", "d3", "cu", "cv", "big"),
          "invert": ("d0", "d1", "gu", "gv", "rs", "big")}


def fake_addresses(test, base=0x7F3A00000000, step=0x1000):
    """Integer addresses as an allocator might give them: 16-byte aligned, none overlapping."""
    assert step >= max(2 * S, 2 * ZS, 4 * W * (2 * H + 1))
    return SimpleNamespace(**{name: base + k * step for k, name in enumerate(PLANES[test])})


def defaults(test, A):
    if test == "fbcheck":
        return {"score": dict(n=2, uf=A.d0, vf=A.d1, fp=P, fs=S, ub=A.d2, vb=A.d3, bp=P, bs=S, w=W, h=H,
                              alpha=0.01, sc=A.s, sp=P, ss=S),
                "zero": dict(n=2, u=A.d0, v=A.d1, fp=P, fs=S, sc=A.s, sp=P, ss=S, w=W, h=H, beta=0.5)}
    if test == "zncc":
        return {"score": dict(n=2, i0=A.d0, p0=P8, s0=S8, i1=A.d1, p1=P8, s1=S8, u=A.d2, v=A.d3, fp=P,
                              fs=ZS, w=W, h=H, r=2, sc=A.s, sp=P, ss=ZS),
                "warp": dict(i1=A.d1, p1=P8, u=A.d2, v=A.d3, fp=P, w=W, h=H, dst=A.J, dp=P8, valid=0, vp=0)}
    if test == "compose":
        return {"comp": dict(n=2, ua=A.d0, va=A.d1, ap=P, as_=S, ub=A.d2, vb=A.d3, bp=P, bs=S, w=W, h=H,
                             uc=A.cu, vc=A.cv, cp=P, cs=S)}
    if test == "invert":
        return {"inv": dict(n=2, uf=A.d0, vf=A.d1, fp=P, fs=S, K=2, tol=0.01, ug=A.gu, vg=A.gv, gp=P, gs=S,
                            r=A.rs, rp=P, rs_=S, w=W, h=H)}
    raise KeyError(test)


def _fbcheck(A):
    B24 = (1 << 24) + 1
    einval = [
        ("score", dict(uf=0)), ("score", dict(vf=0)), ("score", dict(ub=0)), ("score", dict(vb=0)),
        ("score", dict(sc=0)), ("score", dict(n=0)), ("score", dict(n=-3)), ("score", dict(w=0)),
        ("score", dict(h=0)), ("score", dict(w=-1)), ("score", dict(fp=P - 4)), ("score", dict(bp=P + 2)),
        ("score", dict(sp=P - 4)), ("score", dict(sp=P + 1)), ("score", dict(fs=S + 2)),
        ("score", dict(bs=S + 1)), ("score", dict(ss=S + 3)), ("score", dict(fs=S - 4)),
        ("score", dict(alpha=NAN)),
        ("score", dict(sc=A.d0)), ("score", dict(sc=A.d3 + 4)),               # score over a flow plane
        ("score", dict(n=1, sc=A.big, uf=A.big + P * H - 4)),                 # ... by one float
        ("score", dict(ub=A.d0)), ("score", dict(vb=A.d1 + S)),               # backward over forward
        ("zero", dict(u=0)), ("zero", dict(v=0)), ("zero", dict(sc=0)), ("zero", dict(n=0)),
        ("zero", dict(w=0)), ("zero", dict(h=-2)), ("zero", dict(fp=P - 4)), ("zero", dict(fp=P + 2)),
        ("zero", dict(sp=P - 4)), ("zero", dict(fs=S + 2)), ("zero", dict(ss=S + 1)),
        ("zero", dict(beta=NAN)), ("zero", dict(sc=A.d0)), ("zero", dict(sc=A.d1 + S)),
    ]
    esize = [("score", dict(w=B24, fp=4 * B24, bp=4 * B24, sp=4 * B24, n=1)),
             ("score", dict(h=B24, n=1)),
             ("zero", dict(h=B24, n=1)),
             ("zero", dict(w=B24, fp=4 * B24, sp=4 * B24, n=1))]
    return einval, esize


def _zncc(A):
    B19 = (1 << 19) + 1
    einval = [
        ("score", dict(i0=0)), ("score", dict(i1=0)), ("score", dict(u=0)), ("score", dict(v=0)),
        ("score", dict(sc=0)), ("score", dict(n=0)), ("score", dict(n=-3)), ("score", dict(w=0)),
        ("score", dict(h=0)), ("score", dict(w=-1)), ("score", dict(r=0)), ("score", dict(r=5)),
        ("score", dict(r=-1)), ("score", dict(p0=W - 1)), ("score", dict(p1=W - 1)),
        ("score", dict(fp=P - 4)), ("score", dict(fp=P + 2)), ("score", dict(sp=P - 4)),
        ("score", dict(sp=P + 1)), ("score", dict(fs=ZS + 2)), ("score", dict(ss=ZS + 3)),
        ("score", dict(fs=P * (H - 1))), ("score", dict(ss=4)), ("score", dict(s0=1)),
        ("score", dict(s1=P8 * (H - 1))),                                 # (a frame stride 0 is a shared frame)
        ("score", dict(sc=A.d2)), ("score", dict(sc=A.d3 + 4)),           # score over a flow plane
        ("score", dict(n=1, sc=A.big, u=A.big + P * H - 4)),              # ... by one float
        ("score", dict(n=1, sc=A.big, sp=P, i0=A.big + P * H - 1)),       # score over frame0, by one byte
        ("score", dict(n=1, sc=A.big, i1=A.big + 3)),                     # score over frame1
        ("warp", dict(i1=0)), ("warp", dict(u=0)), ("warp", dict(v=0)), ("warp", dict(dst=0)),
        ("warp", dict(w=0)), ("warp", dict(h=-2)), ("warp", dict(p1=W - 1)), ("warp", dict(dp=W - 1)),
        ("warp", dict(fp=P - 4)), ("warp", dict(fp=P + 2)), ("warp", dict(valid=A.J + 8, vp=W - 1)),
        ("warp", dict(dst=A.d1)), ("warp", dict(dst=A.d2 + 5)), ("warp", dict(valid=A.d3, vp=W)),
        ("warp", dict(valid=A.J + W * H - 1, vp=W)),                      # valid over dst by one byte
    ]
    esize = [("score", dict(w=B19, p0=B19, p1=B19, fp=4 * B19, sp=4 * B19, n=1)),
             ("score", dict(h=B19, n=1)), ("warp", dict(h=B19)),
             ("warp", dict(w=B19, p1=B19, dp=B19, fp=4 * B19))]
    return einval, esize


def _compose(A):
    B24 = (1 << 24) + 1
    einval = [
        dict(ua=0), dict(va=0), dict(ub=0), dict(vb=0), dict(uc=0), dict(vc=0),
        dict(n=0), dict(n=-3), dict(w=0), dict(h=0), dict(w=-1), dict(h=-2),
        dict(ap=P - 4), dict(bp=P - 4), dict(cp=P - 4), dict(ap=P + 2), dict(bp=P + 1), dict(cp=P + 3),
        dict(as_=S + 2), dict(bs=S + 1), dict(cs=S + 3),            # strides that are no multiple of 4
        dict(as_=S - 4), dict(bs=S - 4), dict(cs=S - 4), dict(cs=0),   # ... that do not cover a plane
        dict(uc=A.d2), dict(vc=A.d3), dict(uc=A.d3 + 4), dict(vc=A.d2 + S),   # c over b
        dict(n=1, uc=A.big, ub=A.big + P * H - 4),                     # ... by one float
        # c over a other than a exactly: one plane only, swapped, shifted, another pitch or stride
        dict(uc=A.d0), dict(vc=A.d1), dict(uc=A.d1, vc=A.d0),
        dict(uc=A.d0 + 4, vc=A.d1), dict(n=1, uc=A.d0, vc=A.d1, cs=S + 4),
        dict(n=1, ua=A.big, va=A.d1, ap=2 * P, uc=A.big, vc=A.d1, cp=P),
        dict(n=1, ua=A.big, uc=A.big + P * H - 4),
    ]
    esize = [dict(w=B24, ap=4 * B24, bp=4 * B24, cp=4 * B24, n=1), dict(h=B24, n=1)]
    return [("comp", kw) for kw in einval], [("comp", kw) for kw in esize]


def _invert(A):
    B24 = (1 << 24) + 1
    einval = [
        dict(uf=0), dict(vf=0), dict(ug=0), dict(vg=0),
        dict(n=0), dict(n=-3), dict(w=0), dict(h=0), dict(w=-1), dict(h=-2),
        dict(K=0), dict(K=-1), dict(K=33), dict(tol=NAN),
        dict(fp=P - 4), dict(gp=P - 4), dict(rp=P - 4), dict(fp=P + 2), dict(gp=P + 1), dict(rp=P + 3),
        dict(fs=S + 2), dict(gs=S + 1), dict(rs_=S + 3),            # strides that are no multiple of 4
        dict(fs=S - 4), dict(gs=S - 4), dict(rs_=S - 4), dict(gs=0),   # ... that do not cover a plane
        # g over f: exactly (nothing runs in place), swapped, shifted, by one float
        dict(ug=A.d0), dict(vg=A.d1), dict(ug=A.d0, vg=A.d1), dict(ug=A.d1, vg=A.d0),
        dict(ug=A.d0 + 4), dict(vg=A.d1 + S), dict(n=1, uf=A.big, ug=A.big + P * H - 4),
        dict(n=1, ug=A.big, uf=A.big + P * H - 4),
        # resid over f or g, and ug over vg
        dict(r=A.d0), dict(r=A.d1 + 4), dict(r=A.gu), dict(r=A.gv + S), dict(ug=A.gv),
        dict(n=1, ug=A.big, r=A.big + P * H - 4), dict(n=1, vg=A.big, ug=A.big + P * H - 4),
    ]
    esize = [dict(w=B24, fp=4 * B24, gp=4 * B24, rp=4 * B24, n=1), dict(h=B24, n=1)]
    return [("inv", kw) for kw in einval], [("inv", kw) for kw in esize]


_ROWS = {"fbcheck": _fbcheck, "zncc": _zncc, "compose": _compose, "invert": _invert}


def rows(test, A):
    einval, esize = _ROWS[test](A)
    return [(c, kw, "TVL1_EINVAL") for c, kw in einval] + [(c, kw, "TVL1_ESIZE") for c, kw in esize]


def recorded(test):
    return json.loads(GOLDEN.read_text())[test]


def assert_recorded(test, messages):
    """The rows' messages (str of the TVL1Error), in row order, against the record."""
    out = os.environ.get("TVL1_FLOWOP_ERRORS_OUT")
    if out:
        path = Path(out)
        rec = json.loads(path.read_text()) if path.exists() else {}
        rec[test] = messages
        path.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
        return
    want = recorded(test)
    assert len(messages) == len(want)
    for k, (got, w) in enumerate(zip(messages, want)):
        assert got == w, (test, k, got, w)
