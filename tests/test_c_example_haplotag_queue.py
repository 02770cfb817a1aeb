"""examples/haplotag_from_alignments_queue.c: mrp_haplotag_aligned_chunks_on_devices from plain C.  On a GPU each of the three blocks it
prints (the same chunk three times, one chunk per batch) must be, character for character, what examples/haplotag_from_alignments.c prints
for the one call over that chunk.  (That it compiles with -Wall -Werror and refuses to run without a device is in
tests/test_haplotag_queue_args.py.)"""
import os
import subprocess

import pytest

from margin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT_LINES = ("hap", "h1", "h2")
INPUT_LINES = ("variant", "read", "model_f", "model_r")


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", name + ".c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def _lines(text, first_words):
    return [ln for ln in text.splitlines() if ln.split() and ln.split()[0] in first_words]


@pytest.mark.gpu
def test_c_example_prints_the_single_call_three_times(tmp_path, gpu_ctx):
    one = subprocess.run([_build(tmp_path, "haplotag_from_alignments")], capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stdout + one.stderr
    r = subprocess.run([_build(tmp_path, "haplotag_from_alignments_queue")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _lines(r.stdout, INPUT_LINES) == _lines(one.stdout, INPUT_LINES)  # the same input and state machines
    want = _lines(one.stdout, RESULT_LINES)
    assert [ln.split()[0] for ln in want] == list(RESULT_LINES)
    blocks = r.stdout.split("\ncopy ")[1:]
    assert [b.split()[0] for b in blocks] == ["0", "1", "2"]
    for b in blocks:
        assert _lines(b.split("\n", 1)[1], RESULT_LINES) == want
    assert "3 chunks of " in r.stdout and "in 3 batches on 1 device, 0 on the per-chunk path" in r.stdout
