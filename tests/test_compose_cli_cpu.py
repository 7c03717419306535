"""The CLI side of an "initialFlow" chain without a GPU: `--plan` on a chained config, and the
flow-file reader behind the chain's links (ofio::read_tiff_f32, reached through the hidden
`optflow --decode-flow in.tiff out.tiff`): a file written by write_tiff_f32 round-trips byte for
byte, in one strip or many, and everything else -- truncated, compressed, 8-bit or integer
samples, two samples, big-endian, strips out of range, huge dimensions -- gives exit status 1
and a message, never a crash or an unbounded allocation.  Runs on the release binary and on the
stand-alone ASan + UBSan build of the CLI (`make -C fibsem-optflow_amd asan`), in the manner of
tests/test_host_hardening_cpu.py."""
import fcntl
import json
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from optflow_amd import capi

BINS = {"release": capi.PKG_ROOT / "bin" / "optflow",
        "asan": capi.PKG_ROOT / "bin" / "optflow_asan"}   # make -C fibsem-optflow_amd asan
_bin = [str(BINS["release"])]


@pytest.fixture(autouse=True, params=["release", "asan"])
def optflow_bin(request, built):
    path = BINS[request.param]
    if request.param == "asan":
        # one build at a time (pytest-xdist workers): a worker must not run the binary
        # while another is still linking it
        with open(capi.PKG_ROOT / "bin" / ".asan.lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if not path.exists():
                r = subprocess.run(["make", "-C", str(capi.PKG_ROOT), "asan"], capture_output=True,
                                   text=True)
                if r.returncode != 0:
                    pytest.skip("ASan/UBSan build unavailable: " + r.stderr[-300:])
    _bin[0] = os.environ.get("OPTFLOW_BIN", str(path))
    yield


def run(*args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([_bin[0], *map(str, args)], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode not in (98, 99), r.stderr
    assert r.returncode >= 0, f"optflow killed by signal {-r.returncode}: {r.stderr}"
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r


def ftiff(w, h, rows_per_strip, strips, bps=32, fmt=3, comp=1, spp=1, order="<", count_override=None,
          offsets=None, counts=None):
    """A baseline TIFF as write_tiff_f32 lays it out: one IFD of ten entries, the strips' data
    after it (and, with several strips, their offset and count arrays after that)."""
    entries = []
    data = b"".join(strips)
    ns = len(strips)
    data_off = 8 + 2 + 12 * 10 + 4
    offs_arr = data_off + len(data)
    cnts_arr = offs_arr + 4 * ns
    if offsets is None:
        offsets, o = [], data_off
        for s in strips:
            offsets.append(o)
            o += len(s)
    if counts is None:
        counts = [len(s) for s in strips]

    def ent(tag, typ, cnt, val):
        if typ == 3 and cnt == 1:
            entries.append(struct.pack(order + "HHIHH", tag, typ, cnt, val, 0))
        else:
            entries.append(struct.pack(order + "HHII", tag, typ, cnt, val))

    ent(256, 4, 1, w)
    ent(257, 4, 1, h)
    ent(258, 3, 1, bps)
    ent(259, 3, 1, comp)
    ent(262, 3, 1, 1)
    ent(273, 4, count_override or ns, offsets[0] if ns == 1 else offs_arr)
    ent(277, 3, 1, spp)
    ent(278, 4, 1, rows_per_strip)
    ent(279, 4, ns, counts[0] if ns == 1 else cnts_arr)
    ent(339, 3, 1, fmt)
    magic = b"II*\0" if order == "<" else b"MM\0*"
    out = magic + struct.pack(order + "I", 8) + struct.pack(order + "H", 10) + b"".join(entries)
    out += b"\0\0\0\0" + data
    if ns > 1:
        out += struct.pack(f"{order}{ns}I", *offsets) + struct.pack(f"{order}{ns}I", *counts)
    return out


def flow_plane(w, h, seed=4):
    a = np.random.default_rng(seed).normal(0.0, 3.0, (h, w)).astype(np.float32)
    a.flat[:6] = [np.nan, np.inf, -np.inf, -0.0, 1e30, 2.0 ** -140][:min(6, a.size)]
    return a


def decode_fails(tmp_path, data, expect=None):
    src = tmp_path / "bad.tiff"
    src.write_bytes(data)
    out = tmp_path / "out.tiff"
    r = run("--decode-flow", src, out)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.strip() and str(src) in r.stderr, r.stderr
    if expect:
        assert expect in r.stderr, r.stderr
    assert not out.exists()
    return r


def test_a_written_flow_file_round_trips_byte_for_byte(tmp_path):
    a = flow_plane(37, 23)
    first = tmp_path / "a.tiff"
    first.write_bytes(ftiff(37, 23, 23, [a.tobytes()]))
    # the reader's output through the writer, and that file through both again
    r = run("--decode-flow", first, tmp_path / "b.tiff")
    assert r.returncode == 0, r.stderr
    r = run("--decode-flow", tmp_path / "b.tiff", tmp_path / "c.tiff")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "b.tiff").read_bytes() == (tmp_path / "c.tiff").read_bytes()
    # the layout above is write_tiff_f32's own: the first hop changes nothing either
    assert (tmp_path / "b.tiff").read_bytes() == first.read_bytes()
    back = np.array(Image.open(tmp_path / "c.tiff"))
    assert back.dtype == np.float32 and back.tobytes() == a.tobytes()


def test_many_strips_read_as_one(tmp_path):
    a = flow_plane(10, 12)
    one = tmp_path / "one.tiff"
    one.write_bytes(ftiff(10, 12, 12, [a.tobytes()]))
    for rps in (1, 4, 5):   # the last strip of 5-row strips holds 2 rows
        src = tmp_path / f"s{rps}.tiff"
        src.write_bytes(ftiff(10, 12, rps, [a[i:i + rps].tobytes() for i in range(0, 12, rps)]))
        out = tmp_path / f"o{rps}.tiff"
        r = run("--decode-flow", src, out)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == one.read_bytes()


def test_truncated_files(tmp_path):
    good = ftiff(8, 6, 6, [flow_plane(8, 6).tobytes()])
    for cut in (len(good) - 1, len(good) - 100, 8 + 2 + 60, 9, 7, 3, 0):
        decode_fails(tmp_path, good[:cut])
    decode_fails(tmp_path, b"II*\0" + struct.pack("<I", 0x7FFFFFF0) + b"\0" * 8, "IFD")


def test_missing_file(tmp_path):
    r = run("--decode-flow", tmp_path / "nothing.tiff", tmp_path / "o.tiff")
    assert r.returncode == 1 and "nothing.tiff" in r.stderr


@pytest.mark.parametrize("kw,what", [
    (dict(comp=5), "compression"), (dict(comp=8), "compression"), (dict(comp=32773), "compression"),
    (dict(bps=8, fmt=1), "32-bit IEEE float"), (dict(bps=16, fmt=1), "32-bit IEEE float"),
    (dict(bps=32, fmt=1), "32-bit IEEE float"), (dict(bps=32, fmt=2), "32-bit IEEE float"),
    (dict(bps=64, fmt=3), "32-bit IEEE float"),
    (dict(spp=2), "one sample"), (dict(spp=3), "one sample"),
    (dict(order=">"), "little-endian"),
], ids=["lzw", "deflate", "packbits", "u8", "u16", "u32", "i32", "f64", "two-samples", "rgb", "big-endian"])
def test_other_formats_are_refused(tmp_path, kw, what):
    a = flow_plane(8, 6)
    decode_fails(tmp_path, ftiff(8, 6, 6, [a.tobytes()], **kw), what)


def test_an_8_bit_slice_is_no_flow_file(tmp_path):
    p = tmp_path / "slice.tif"
    Image.fromarray(np.zeros((6, 8), np.uint8)).save(p)
    r = run("--decode-flow", p, tmp_path / "o.tiff")
    assert r.returncode == 1 and str(p) in r.stderr


def test_strips_out_of_range(tmp_path):
    a = flow_plane(8, 6)
    raw = a.tobytes()
    n = len(ftiff(8, 6, 6, [raw]))
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw], offsets=[n - 4]), "out of range")
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw], offsets=[0xFFFFFFF0]), "out of range")
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw], counts=[len(raw) - 4]), "wrong size")
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw], counts=[0xFFFFFFFF]), "wrong size")
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw], count_override=0xFFFFFFFF), "out of range")
    # fewer strips than the rows need, and more
    decode_fails(tmp_path, ftiff(8, 6, 2, [a[:2].tobytes(), a[2:4].tobytes()]), "strips")
    decode_fails(tmp_path, ftiff(8, 6, 6, [raw, raw]), "strips")
    # a strip of the second chunk past the end of the file
    s = [a[i:i + 2].tobytes() for i in range(0, 6, 2)]
    good = ftiff(8, 6, 2, s)
    decode_fails(tmp_path, ftiff(8, 6, 2, s, offsets=[134, 134 + 64, len(good) - 8]), "out of range")


@pytest.mark.parametrize("w,h", [(1 << 20, 1 << 20), (0xFFFFFFFF, 1), (0x7FFFFFFF, 0x7FFFFFFF),
                                 (1 << 25, 2), (4096, 4096), (0, 6), (8, 0)])
def test_huge_and_empty_dimensions(tmp_path, w, h):
    """Nothing is allocated before the file is known to hold w x h floats."""
    decode_fails(tmp_path, ftiff(w, h, max(h, 1), [b"\0" * 192]))


# ---- --plan on a chained config

def _slices(tmp_path, n=3, w=48, h=40):
    rng = np.random.default_rng(8)
    out = []
    for k in range(n):
        p = tmp_path / f"s{k}.tif"
        Image.fromarray(rng.integers(2, 255, (h, w), dtype=np.uint8)).save(p)
        out.append(str(p))
    return out


def _plan(tmp_path, cfg):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return run("--plan", p)


def _entries(r):
    """The plan: the JSON list after the pair lines the pair loop prints."""
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    return json.loads("\n".join(lines[lines.index("["):]))


def test_plan_reports_the_chain_and_no_strip_batch(tmp_path):
    s = _slices(tmp_path)
    links = [str(tmp_path / "z0_1.00"), str(tmp_path / "z1_1.00")]
    cfg = {"output_dir": str(tmp_path), "scale": 1, "output_type": "flow", "rois": {"top": 16, "bottom": 16},
           "images": [
               {"p": s[0], "q": s[1], "output_name": "z0"},
               {"p": s[1], "q": s[2], "output_name": "z1"},
               {"p": s[0], "q": s[2], "output_name": "far", "useInitialFlow": True,
                "initialFlow": {"chain": links}}]}
    plan = _entries(_plan(tmp_path, cfg))
    assert [p["strip_batch"] for p in plan] == [True, True, False]
    assert plan[2]["initialFlow"] == {"chain": links, "links": 2}
    assert "initialFlow" not in plan[0]
    # a global chain keeps every pair out of the strip batch, "seededStripBatch" or not
    cfg2 = dict(cfg, useInitialFlow=True, initialFlow={"chain": links[:1]}, seededStripBatch=True)
    plan = _entries(_plan(tmp_path, cfg2))
    assert [p["strip_batch"] for p in plan] == [False, False, False]
    assert plan[0]["initialFlow"] == {"chain": links[:1], "links": 1}
    # without "useInitialFlow" the key stays inert
    cfg["images"][2].pop("useInitialFlow")
    plan = _entries(_plan(tmp_path, cfg))
    assert "initialFlow" not in plan[2]


@pytest.mark.parametrize("chain", [[], ["x"] * 65, "x", [1, 2], ["ok", ""]],
                         ids=["empty", "65", "string", "numbers", "empty-name"])
def test_a_malformed_chain_ends_the_job(tmp_path, chain):
    s = _slices(tmp_path, 2)
    cfg = {"output_dir": str(tmp_path), "scale": 1, "rois": {"top": 16},
           "images": [{"p": s[0], "q": s[1], "output_name": "a", "useInitialFlow": True,
                       "initialFlow": {"chain": chain}}]}
    r = _plan(tmp_path, cfg)
    assert r.returncode == 2 and "chain" in r.stderr and "1 to 64" in r.stderr, (r.returncode, r.stderr)
    cfg["images"][0]["initialFlow"] = {"chain": ["x"] * 64}
    assert _plan(tmp_path, cfg).returncode == 0


def test_a_chain_with_features_is_the_seed_error(tmp_path):
    s = _slices(tmp_path, 2)
    cfg = {"output_dir": str(tmp_path), "scale": 1, "rois": {"top": 16}, "features": 1,
           "images": [{"p": s[0], "q": s[1], "output_name": "a", "useInitialFlow": True,
                       "initialFlow": {"chain": ["x"]}}]}
    r = _plan(tmp_path, cfg)
    assert r.returncode == 2 and "initialFlow cannot be combined with feature alignment" in r.stderr
