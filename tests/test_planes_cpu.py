"""The argument rules of the flow-utility calls (csrc/tvl1_planes.hpp) on a CPU.

tests/planes_check.cpp, a stand-alone program built with g++ and the host sanitizers (ASan +
UBSan), runs check_planes and check_overlaps on case lines of integer addresses; nothing is
dereferenced.  `rule` below is the same rule written from the contract in include/tvl1.h, in
Python's unbounded integers, with each call's plane and overlap tables (CALLS).  The program must
agree with it, status and message, on

  * every row of the four GPU bad-argument tables (tests/flowop_badargs.py), which with the calls'
    scalar checks must also give the messages recorded on the GPU (tests/golden/flowop_errors.json);
  * both sides of every inequality, the size limits, overlaps by one byte and none, across the pair
    stride, compose in place and not quite;
  * spans that do not fit the address space, which the expression the engine had before this
    header (parent_accepts) let through by wrapping;
  * two faults at once: the earlier one is reported.
"""
import math
import subprocess

import pytest

import flowop_badargs as B
from test_plan_cpu import CSRC, ROOT

OK, EINVAL, ESIZE = 0, 1, 2
STATUS = {OK: "TVL1_OK", EINVAL: "TVL1_EINVAL", ESIZE: "TVL1_ESIZE"}
WHY = {24: "float(x) is no longer exact", 19: "the 1/32 px map is no longer exact"}
ADDRESS_SPACE = 1 << 64


def plane_bytes(q, w, h):
    _, _, pitch, _, elem, _ = q
    return pitch * (h - 1) + w * elem


def span(q, n, w, h):
    return q[1], q[1] + (n - 1) * q[3] + plane_bytes(q, w, h)


def rule(c):
    """(status, message) of a case: include/tvl1.h's TVL1_EINVAL / TVL1_ESIZE lists, in the order
    the calls have always tested them.  A plane is (name, address, pitch, pair stride, bytes per
    px, "a pair stride 0 is one shared plane")."""
    n, w, h, pl, skip = c["n"], c["w"], c["h"], c["planes"], c.get("skip", -1)
    live = [(i, q) for i, q in enumerate(pl) if i != skip]
    for _, q in live:
        if q[1] == 0:
            return EINVAL, f"{q[0]} is NULL"
    if n < 1:
        return EINVAL, f"n must be >= 1 (got {n})"
    if w < 1 or h < 1:
        return EINVAL, f"bad size {w}x{h}"
    if w > 1 << c["limit"] or h > 1 << c["limit"]:
        return ESIZE, f"size {w}x{h} above 2^{c['limit']} ({WHY[c['limit']]})"
    for _, q in live:
        name, _, pitch, stride, elem, shared = q
        if elem == 1:
            if pitch < w:
                return EINVAL, f"{name}: pitch must be >= w"
        else:
            if pitch % 4 or pitch < 4 * w:
                return EINVAL, f"{name}: pitch must be a multiple of 4 and >= 4 * w"
            if stride % 4:
                return EINVAL, f"{name}: pair stride must be a multiple of 4"
        if span(q, n, w, h)[1] >= ADDRESS_SPACE:
            return EINVAL, f"{name}: plane span overflows the address space"
        if n > 1 and not (shared and stride == 0) and stride < plane_bytes(q, w, h):
            return EINVAL, f"{name}: pair stride must cover one plane"
    if c.get("scalar"):
        return EINVAL, c["scalar"]
    for a, b, unless_in_place in c.get("ov", []):
        if a == skip or b == skip or (unless_in_place and c.get("in_place")):
            continue
        (a0, a1), (b0, b1) = span(pl[a], n, w, h), span(pl[b], n, w, h)
        if a0 < b1 and b0 < a1:
            tail = " without being flow a itself" if unless_in_place else ""
            return EINVAL, f"{pl[a][0]} overlaps {pl[b][0]}{tail}"
    return OK, ""


def parent_accepts(c):
    """What the engine evaluated before tvl1_planes.hpp, for f32 planes, in size_t:
         hi = lo + (size_t)(n - 1) * stride + pitch * (size_t)(h - 1) + (size_t)w * sizeof(float)
       (overlap iff a.lo < b.hi && b.lo < a.hi), and
         n > 1 && stride < pitch * (size_t)(h - 1) + (size_t)w * sizeof(float)
       for "pair stride must cover one plane": every product and sum modulo 2^64."""
    n, w, h, pl = c["n"], c["w"], c["h"], c["planes"]
    m = ADDRESS_SPACE
    hi = lambda q: (q[1] + ((n - 1) * q[3]) % m + (q[2] * (h - 1)) % m + 4 * w) % m
    for q in pl:
        assert q[4] == 4 and q[1] and 1 <= w <= 1 << 24 and 1 <= h <= 1 << 24 and n >= 1
        if q[2] % 4 or q[2] < 4 * w or q[3] % 4:
            return False
        if n > 1 and q[3] < ((q[2] * (h - 1)) % m + 4 * w) % m:
            return False
    return not any(pl[a][1] < hi(pl[b]) and pl[b][1] < hi(pl[a]) for a, b, _ in c.get("ov", []))


def line(c):
    out = [c["n"], c["w"], c["h"], c["limit"], c.get("skip", -1), int(bool(c.get("in_place"))), len(c["planes"])]
    for name, p, pitch, stride, elem, shared in c["planes"]:
        out += [name, p, pitch, stride, elem, int(shared)]
    out.append(len(c.get("ov", [])))
    for a, b, flag in c.get("ov", []):
        out += [a, b, int(flag)]
    return " ".join(str(x) for x in out)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("planes")
    exe = d / "planes_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "planes_check.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        """[(status, message)] of the cases, planes and overlaps only (no scalar check)."""
        path = d / "cases.txt"
        path.write_text("\n".join(line(c) for c in cases) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # a sanitizer report
        out = [ln.split("\t", 1) for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return [(int(s), m) for s, m in out]

    return run


# ---- the calls' tables, from include/tvl1.h: (name, pointer, pitch, pair stride) argument names of
# tests/flowop_badargs.py, bytes per px, shared; then the overlap pairs ----
def _f32(name, p, pitch, stride):
    return (name, p, pitch, stride, 4, False)


CALLS = {
    ("fbcheck", "score"): dict(
        cname="tvl1_fb_score_batch", limit=24,
        planes=[_f32("uf", "uf", "fp", "fs"), _f32("vf", "vf", "fp", "fs"), _f32("ub", "ub", "bp", "bs"),
                _f32("vb", "vb", "bp", "bs"), _f32("score", "sc", "sp", "ss")],
        ov=[(4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 3, 0), (2, 0, 0), (3, 0, 0), (2, 1, 0), (3, 1, 0)],
        scalar=lambda a: "alpha is NaN" if math.isnan(a["alpha"]) else None),
    ("fbcheck", "zero"): dict(
        cname="tvl1_zero_above_batch", limit=24,
        planes=[_f32("u", "u", "fp", "fs"), _f32("v", "v", "fp", "fs"), _f32("score", "sc", "sp", "ss")],
        ov=[(2, 0, 0), (2, 1, 0)],
        scalar=lambda a: "beta is NaN" if math.isnan(a["beta"]) else None),
    ("zncc", "score"): dict(
        cname="tvl1_zncc_score_batch", limit=19,
        planes=[("I0", "i0", "p0", "s0", 1, True), ("I1", "i1", "p1", "s1", 1, True), _f32("u", "u", "fp", "fs"),
                _f32("v", "v", "fp", "fs"), _f32("score", "sc", "sp", "ss")],
        ov=[(4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 3, 0)],
        scalar=lambda a: None if 1 <= a["r"] <= 4 else f"radius must be 1..4 (got {a['r']})"),
    ("zncc", "warp"): dict(
        cname="tvl1_warp_by_flow_u8", limit=19,
        planes=[("I1", "i1", "p1", None, 1, False), ("dst", "dst", "dp", None, 1, False),
                ("valid", "valid", "vp", None, 1, False), _f32("u", "u", "fp", None), _f32("v", "v", "fp", None)],
        ov=[(1, 0, 0), (1, 3, 0), (1, 4, 0), (2, 0, 0), (2, 3, 0), (2, 4, 0), (2, 1, 0)],
        skip=lambda a: -1 if a["valid"] else 2),
    ("compose", "comp"): dict(
        cname="tvl1_compose_flow_batch", limit=24,
        planes=[_f32("ua", "ua", "ap", "as_"), _f32("va", "va", "ap", "as_"), _f32("ub", "ub", "bp", "bs"),
                _f32("vb", "vb", "bp", "bs"), _f32("uc", "uc", "cp", "cs"), _f32("vc", "vc", "cp", "cs")],
        ov=[(4, 2, 0), (4, 3, 0), (5, 2, 0), (5, 3, 0), (4, 0, 1), (4, 1, 1), (5, 0, 1), (5, 1, 1)],
        in_place=lambda a: (a["uc"], a["vc"], a["cp"], a["cs"]) == (a["ua"], a["va"], a["ap"], a["as_"])),
    ("invert", "inv"): dict(
        cname="tvl1_invert_flow_batch", limit=24,
        planes=[_f32("uf", "uf", "fp", "fs"), _f32("vf", "vf", "fp", "fs"), _f32("ug", "ug", "gp", "gs"),
                _f32("vg", "vg", "gp", "gs"), _f32("resid", "r", "rp", "rs_")],
        ov=[(2, 0, 0), (2, 1, 0), (3, 0, 0), (3, 1, 0), (3, 2, 0), (4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 3, 0)],
        skip=lambda a: -1 if a["r"] else 4,
        scalar=lambda a: (f"iterations must be 1..32 (got {a['K']})" if not 1 <= a["K"] <= 32 else
                          "tol is NaN" if math.isnan(a["tol"]) else None)),
}


def restate(test, call, args):
    """A GPU row (the call's arguments) as a case of planes."""
    t = CALLS[test, call]
    planes = [(name, args[p], args[pitch], args[stride] if stride else 0, elem, shared)
              for name, p, pitch, stride, elem, shared in t["planes"]]
    return dict(n=args.get("n", 1), w=args["w"], h=args["h"], limit=t["limit"], planes=planes, ov=t["ov"],
                skip=t.get("skip", lambda a: -1)(args), in_place=t.get("in_place", lambda a: False)(args),
                scalar=t.get("scalar", lambda a: None)(args))


@pytest.mark.parametrize("test", list(B.PLANES))
def test_the_gpu_tables_rows_on_integer_addresses(program, test):
    A = B.fake_addresses(test)
    good = B.defaults(test, A)
    rows = B.rows(test, A)
    cases = [restate(test, call, {**good[call], **kw}) for call, kw, _ in rows]
    got = program(cases)
    recorded = B.recorded(test)
    assert len(recorded) == len(rows)
    for (call, kw, status), c, g, rec in zip(rows, cases, got, recorded):
        assert g == rule(dict(c, scalar=None)), (call, kw)      # the header alone: no scalar check
        st, msg = rule(c)                                       # the call: its scalar checks in their place
        assert STATUS[st] == status, (call, kw, msg)
        assert f"{CALLS[test, call]['cname']}: {status}: {msg}" == rec, (call, kw)
        if not c["scalar"]:
            assert g == (st, msg), (call, kw)
    # and the good arguments pass
    assert program([restate(test, call, a) for call, a in good.items()]) == [(OK, "")] * len(good)


BASE = 0x7F3A00000000
W, H = 20, 6
ROW, ONE = 4 * W, 4 * W * (H - 1) + 4 * W   # a dense f32 plane's row and its bytes


def f32(name, p, pitch=ROW, stride=ONE, shared=False):
    return (name, p, pitch, stride, 4, shared)


def u8(name, p, pitch=W, stride=W * H, shared=False):
    return (name, p, pitch, stride, 1, shared)


def case(planes, n=2, w=W, h=H, limit=24, **kw):
    return dict(n=n, w=w, h=h, limit=limit, planes=planes, **kw)


def test_both_sides_of_each_inequality(program):
    A, C = BASE, BASE + 0x10000
    ov = [(1, 0, 0)]
    cover = "pair stride must cover one plane"
    table = [
        # pitch = row, row - 1; f32 pitch = 2 (mod 4)
        (case([f32("a", A, pitch=ROW, stride=ONE)]), OK, ""),
        (case([f32("a", A, pitch=ROW - 1, stride=ONE)]), EINVAL, "a: pitch must be a multiple of 4 and >= 4 * w"),
        (case([f32("a", A, pitch=ROW - 4, stride=ONE)]), EINVAL, "a: pitch must be a multiple of 4 and >= 4 * w"),
        (case([f32("a", A, pitch=ROW + 2, stride=2 * ONE)]), EINVAL, "a: pitch must be a multiple of 4 and >= 4 * w"),
        (case([u8("I", A, pitch=W)]), OK, ""),
        (case([u8("I", A, pitch=W - 1)]), EINVAL, "I: pitch must be >= w"),
        # stride = pitch (h - 1) + row, and one element less
        (case([f32("a", A, pitch=ROW + 8, stride=(ROW + 8) * (H - 1) + ROW)]), OK, ""),
        (case([f32("a", A, pitch=ROW + 8, stride=(ROW + 8) * (H - 1) + ROW - 4)]), EINVAL, "a: " + cover),
        (case([u8("I", A, pitch=W + 3, stride=(W + 3) * (H - 1) + W)]), OK, ""),
        (case([u8("I", A, pitch=W + 3, stride=(W + 3) * (H - 1) + W - 1)]), EINVAL, "I: " + cover),
        (case([f32("a", A, stride=ONE + 2)]), EINVAL, "a: pair stride must be a multiple of 4"),
        (case([u8("I", A, stride=W * H + 1)]), OK, ""),          # a u8 stride need not be
        # n = 1 with stride 0; a shared u8 plane with stride 0 at n = 3 (ZNCC's frames); a plane no call
        # flags as shareable, every f32 plane among them, is refused with stride 0 at n = 3
        (case([f32("a", A, stride=0), u8("I", C, stride=0)], n=1), OK, ""),
        (case([u8("I0", A, stride=0, shared=True), f32("u", C)], n=3, limit=19), OK, ""),
        (case([u8("I0", A, stride=0, shared=False), f32("u", C)], n=3, limit=19), EINVAL, "I0: " + cover),
        (case([f32("a", A, stride=0, shared=False)], n=3), EINVAL, "a: " + cover),
        # ... and a shared plane's span is one plane: touching it is no overlap, one byte in is
        (case([u8("I0", A, stride=0, shared=True), u8("J", A + W * H)], n=3, ov=ov), OK, ""),
        (case([u8("I0", A, stride=0, shared=True), u8("J", A + W * H - 1)], n=3, ov=ov), EINVAL, "J overlaps I0"),
    ]
    _agree(program, table)


def _agree(program, table):
    got = program([c for c, _, _ in table])
    for k, ((c, st, msg), g) in enumerate(zip(table, got)):
        assert g == (st, msg), (k, c)
        assert rule(c) == (st, msg), (k, c)


def test_size_limits(program):
    def at(w, h, limit):   # one f32 and one u8 plane, dense at that size
        pw, ph = max(w, 1), max(h, 1)
        return case([f32("u", BASE, pitch=4 * pw, stride=4 * pw * ph), u8("I", 1 << 40, pitch=pw, stride=pw * ph)],
                    n=1, w=w, h=h, limit=limit)
    table = []
    for lim in (24, 19):
        top = 1 << lim
        table += [(at(top, 3, lim), OK, ""), (at(3, top, lim), OK, ""),
                  (at(top + 1, 3, lim), ESIZE, f"size {top + 1}x3 above 2^{lim} ({WHY[lim]})"),
                  (at(3, top + 1, lim), ESIZE, f"size 3x{top + 1} above 2^{lim} ({WHY[lim]})")]
    # 2^19 + 1 passes the 2^24 limit; a bad size is TVL1_EINVAL, before the limit
    table += [(at((1 << 19) + 1, 2, 24), OK, ""), (at(0, (1 << 24) + 1, 24), EINVAL, f"bad size 0x{(1 << 24) + 1}"),
              (at(3, -1, 19), EINVAL, "bad size 3x-1")]
    _agree(program, table)


def test_overlaps(program):
    A = BASE
    ov = [(1, 0, 0)]
    comp = [(2, 0, 1), (2, 1, 1), (3, 0, 1), (3, 1, 1)]
    a2 = lambda **kw: [f32("ua", A, **kw), f32("va", A + 0x10000, **kw)]
    c2 = lambda **kw: [f32("uc", A, **kw), f32("vc", A + 0x10000, **kw)]
    table = [
        # by exactly one byte, and touching, in both orders (n = 1: ONE bytes each)
        (case([f32("a", A), f32("b", A + ONE)], n=1, ov=ov), OK, ""),
        (case([f32("a", A), f32("b", A + ONE - 1)], n=1, ov=ov), EINVAL, "b overlaps a"),
        (case([f32("a", A + ONE), f32("b", A)], n=1, ov=ov), OK, ""),
        (case([f32("a", A + ONE - 1), f32("b", A)], n=1, ov=ov), EINVAL, "b overlaps a"),
        (case([u8("I", A), u8("J", A + W * H)], n=1, ov=ov), OK, ""),
        (case([u8("I", A), u8("J", A + W * H - 1)], n=1, ov=ov), EINVAL, "J overlaps I"),
        # across the pair stride: pair 1 of a lies over pair 0 of b, its pair 0 does not
        (case([f32("a", A, stride=3 * ONE), f32("b", A + 3 * ONE + 8, stride=ONE)], n=2, ov=ov), EINVAL, "b overlaps a"),
        (case([f32("a", A, stride=3 * ONE), f32("b", A + 3 * ONE + 8, stride=ONE)], n=1, ov=ov), OK, ""),
        # compose in place, exact; in place with another pitch is no exemption
        (case(a2() + c2(), ov=comp, in_place=True), OK, ""),
        (case(a2() + c2(), ov=comp, in_place=False), EINVAL, "uc overlaps ua without being flow a itself"),
        (case(a2() + c2(pitch=2 * ROW, stride=2 * ONE), ov=comp, in_place=False), EINVAL,
         "uc overlaps ua without being flow a itself"),
        # an optional plane left out is neither checked nor compared
        (case([f32("a", A), f32("r", 0, pitch=3, stride=1)], skip=1, ov=ov), OK, ""),
        (case([f32("a", A), f32("r", A + 4)], skip=-1, ov=ov), EINVAL, "r overlaps a"),
    ]
    _agree(program, table)


def test_spans_that_do_not_fit_the_address_space_are_refused(program):
    A = BASE
    ov = [(1, 0, 0)]
    over = "plane span overflows the address space"
    table = [
        # stride = 2^63 with n = 3: (n - 1) stride is 2^64
        (case([f32("a", A, stride=1 << 63), f32("b", A + ONE)], n=3, ov=ov), EINVAL, "a: " + over),
        # pitch = 2^62 with h = 5: pitch (h - 1) is 2^64
        (case([f32("a", A, pitch=1 << 62, stride=0), f32("b", A + 4 * W)], n=1, h=5, ov=ov), EINVAL, "a: " + over),
        # base 2^64 - 16 with a 32-byte plane
        (case([f32("a", (1 << 64) - 16, pitch=32, stride=32), f32("b", 16, pitch=32, stride=32)], n=1, w=8, h=1,
              ov=ov), EINVAL, "a: " + over),
    ]
    _agree(program, table)
    wrapped = [parent_accepts(c) for c, _, _ in table]
    assert sum(wrapped) >= 2, wrapped
    # the largest spans that fit are accepted as before: ending on the last byte, not one past it
    top = 1 << 64
    fits = [
        (case([f32("a", top - 33, pitch=32, stride=32)], n=1, w=8, h=1), OK, ""),
        (case([f32("a", top - 32, pitch=32, stride=32)], n=1, w=8, h=1), EINVAL, "a: " + over),
        (case([f32("a", 16, pitch=32, stride=(1 << 62))], n=4, w=8, h=1), OK, ""),
        (case([f32("a", 16, pitch=32, stride=(1 << 62))], n=5, w=8, h=1), EINVAL, "a: " + over),
    ]
    _agree(program, fits)
    assert parent_accepts(fits[0][0])


def test_the_earlier_of_two_faults_is_reported(program):
    A, C = BASE, BASE + 0x10000
    ov = [(1, 0, 0)]
    table = [
        # a NULL plane before n, n before the size, the size's sign before its limit
        (case([f32("a", A), f32("b", 0)], n=0), EINVAL, "b is NULL"),
        (case([f32("a", A)], n=0, w=0), EINVAL, "n must be >= 1 (got 0)"),
        (case([f32("a", A)], w=(1 << 24) + 1, h=0), EINVAL, f"bad size {(1 << 24) + 1}x0"),
        # the limit before a pitch; plane 0's stride before plane 1's pitch; pitch before stride
        (case([f32("a", A, pitch=2)], w=(1 << 24) + 1, n=1), ESIZE, f"size {(1 << 24) + 1}x{H} above 2^24 ({WHY[24]})"),
        (case([f32("a", A, stride=ONE - 4), f32("b", C, pitch=ROW - 4)]), EINVAL, "a: pair stride must cover one plane"),
        (case([f32("a", A, pitch=ROW + 1, stride=ONE + 1)]), EINVAL, "a: pitch must be a multiple of 4 and >= 4 * w"),
        (case([f32("a", A, stride=ONE - 2)]), EINVAL, "a: pair stride must be a multiple of 4"),
        # a plane's own fault before any overlap, and the overlap table in its order
        (case([f32("a", A), f32("b", A, pitch=ROW - 4)], ov=ov), EINVAL, "b: pitch must be a multiple of 4 and >= 4 * w"),
        (case([f32("a", A), f32("b", A), f32("c", A)], ov=[(2, 1, 0), (1, 0, 0)]), EINVAL, "c overlaps b"),
        (case([f32("a", A), f32("b", A), f32("c", A)], ov=[(1, 0, 1), (2, 0, 0)], in_place=True), EINVAL, "c overlaps a"),
    ]
    _agree(program, table)
