"""The memory lifecycle of a ctx (csrc/tvl1_arena.hpp) on a CPU.

tests/arena_model.cpp, a stand-alone program built with g++ and the host sanitizers (ASan + UBSan),
is a second backend for the header: a device of per-stream operation queues in which an event
completes when the script says so, a free drains every queue as hipFree does, and the next malloc,
event create or record on a chosen stream can be made to fail.  Around every enter + reserve the
driver checks what the header promises:

  * no block is freed twice, and none is freed without waiting before every one of its events is done;
  * at most kRetiredMax blocks are retired when a reserve returns;
  * release_all leaves no allocation and no event, with retired blocks and failed allocations behind it;
  * the first kernel on `use` after a growth is behind the zero fill;
  * a call on another stream waits for the previous stream's last operation, and a ctx that stays
    on one stream enqueues no wait;
  * ENOMEM with retired blocks frees all of them, retries once and succeeds; without, it is
    TVL1_ENOMEM with today's text, the block empty, and a later smaller reserve succeeds;
  * a destroyed stream's record fails and is skipped, and the block is reaped once the others are done;
  * the ninth stream evicts the oldest, re-noting moves a stream to the end;
  * a reserve that fits enqueues, allocates and frees nothing;

in one hand-written script each (SCRIPTS), and in 300 seeded random sequences of enter + reserve,
complete event, destroy stream and injected failures over 3 blocks and 10 streams.

Sensitivity, tried on scratch copies of the header (each one line changed; the script that caught it):
reap() that does not query a block's last event -- "reap_frees_once_every_event_is_done: block freed
before its event 5 was done"; no wait for the oldest above kRetiredMax -- "3 blocks retired after a
reserve"; no stream wait behind the zero fill -- "a kernel on stream 1 may run before the block's zero
fill"; no wait at a switch of streams -- "stream 2 does not wait for stream 1's last operation"; no
second malloc -- "enomem_with_retired_blocks: the retry did not succeed"; drop() that keeps the
events -- "2 events leaked"; a window of 9 -- "stream_window: the ninth evicts the oldest"; `need <
bytes` for `need <= bytes` -- "a reserve that fits changed the block".
"""
import subprocess

import pytest

from test_plan_cpu import CSRC, ROOT

SCRIPTS = ["noop_reserve", "floor_applies_to_growth_only", "one_stream_enqueues_no_wait",
           "stream_switch_waits_for_the_previous_stream", "zero_fill_orders_the_first_use",
           "retired_bound_under_alternating_growth", "reap_frees_once_every_event_is_done",
           "enomem_with_retired_blocks", "enomem_without_retired_blocks", "destroyed_stream",
           "failed_event_create_and_record", "stream_window", "release_all_with_history", "random_sequences"]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("arena") / "arena_model"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "arena_model.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])   # a FAIL line or a sanitizer report
    return r.stdout.splitlines()


@pytest.mark.parametrize("script", SCRIPTS)
def test_the_header_keeps_its_promises_on_the_model(output, script):
    assert f"ok {script}" in output, output


def test_every_script_of_the_program_is_listed(output):
    assert sorted(ln[3:] for ln in output if ln.startswith("ok ")) == sorted(SCRIPTS)
    assert not [ln for ln in output if ln.startswith("FAIL")]


def test_the_header_takes_no_hip_header():
    text = (CSRC / "tvl1_arena.hpp").read_text()
    assert "hip_runtime" not in text and "#include <hip" not in text
