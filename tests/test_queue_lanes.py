"""The hand-out of the work queue (margin_amd/csrc/mrp_queue_lanes.cpp: run_lanes and its LaneHooks) without the library, Python or a
device: tests/queue_lanes_check.cpp, a stand-alone program compiled together with that one file, built and run once with the thread
sanitizer and once with the address and undefined-behaviour sanitizers.  Fake hooks record every call; the record is held to the
contract above LaneHooks.  Without a failure, on devices x lanes in {1x1, 2x1, 2x4, 3x4}, with 0, 1, n_devices, n_devices * lanes - 1,
n_devices * lanes and 23 batches and 1, 2 or all lanes active: every batch is prefetched, phased and retired once, in that order and on
one lane, nothing is discarded, a lane's first batch is (w % lanes) * n_devices + w / lanes, a lane without work calls no hook, begin
and end bracket every other lane, and a lane's prefetch has returned before the batch phased beside it is retired.  With one failure
injected on 2x4 lanes and 23 batches -- in begin, in a lane's first prefetch, in a later prefetch, in the phase of a lane's first, of a
middle and of the last batch -- and with two failures on two lanes: run_lanes returns an injected code, every batch whose prefetch was
called ends in exactly one of retire and discard, no batch is phased twice, end is called if and only if begin returned MRP_OK, and no
hook is called after run_lanes has returned.  Every case runs with lane 0 on the caller's thread and on a thread of its own, with an
on_thread_start that must be each worker's first call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_hand_out_keeps_its_contract(tmp_path, sanitize):
    exe = str(tmp_path / "queue_lanes_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "queue_lanes_check.cpp"), os.path.join(ROOT, "margin_amd", "csrc", "mrp_queue_lanes.cpp")])
    out = subprocess.check_output([exe], text=True)
    assert out.strip() == "queue lanes ok", out
