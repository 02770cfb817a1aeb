"""The persistent host thread pool (margin_amd/csrc/mrp_host_pool.cpp) without the library, Python or a device:
tests/host_pool_check.cpp, a stand-alone program compiled together with the pool, built and run once with the thread sanitizer and
once with the address and undefined-behaviour sanitizers.  It asserts that every index of every loop runs exactly once: n in
{0, 1, 15, 16, 17, 4 097} with grains {1, 3, n, n + 1}; n = 16 * grain - 1, 16 * grain, 16 * grain + 1 (the split into ranges); one
host thread (every loop inline) and eight; four posting threads with priorities 0..3 and 50 loops each at once; a loop posted from
inside a loop body; mrp_pool_set_weight(1) (a short loop runs on the caller) and (1000) with n = 4 097 (capped wake-ups); a private
pool of three threads adopted by two threads at once, given back and destroyed while the process pool lives on; and
mrp_set_host_threads(0) and (257) are refused."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_every_index_runs_once(tmp_path, sanitize):
    exe = str(tmp_path / "host_pool_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "host_pool_check.cpp"), os.path.join(ROOT, "margin_amd", "csrc", "mrp_host_pool.cpp")])
    out = subprocess.check_output([exe], text=True)
    assert out.strip() == "host pool ok", out
