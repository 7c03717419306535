"""Known answers of the CLI's HIP-free parts: cli/config.hpp (ROIs, the seed and check parsers,
the resolved per-pair config, the stats_json solve record) and cli/points.hpp (the private glibc
generator, the sampled draw, the keep-first-consistent selection).

tests/cli_units.cpp includes only those two headers and json.hpp -- no hip_runtime.h is on its
include path -- and is built with g++ and the host sanitizers (ASan + UBSan) and run directly,
as tests/walk_model.cpp is.  The debug outputs of the CLI rest on GlibcRand reproducing rand().
"""
from __future__ import annotations

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "fibsem-optflow_amd" / "cli"


def test_cli_units(tmp_path):
    exe = tmp_path / "cli_units"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CLI), "-o", str(exe), str(ROOT / "tests" / "cli_units.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])   # a check or a sanitizer report
    lines = r.stdout.splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), lines
    # every group of checks ran
    for group in ("GlibcRand", "sample_points", "keep", "get_rois", "check", "solve_record"):
        assert any(ln.startswith(f"ok {group}") for ln in lines), group
