"""examples/haplotag_from_alignments.c: mrp_haplotag_aligned_chunks from plain C.  It must compile against include/ and link
against the in-tree library; on a GPU the tags and totals it prints must be those of the Python call over the same input,
which the example writes out, and agree with tools/tagFromPhasedVcf.c's chunk loop restated in Python."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import extract_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "haplotag_from_alignments")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "haplotag_from_alignments.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(text):
    variants, gt, reads, out = [], [], [], {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "variant":
            variants.append((int(w[1]), w[4:], 0))
            gt.append((int(w[2]), int(w[3])))
        elif w[0] == "read":
            reads.append((int(w[1]), w[2], int(w[3]), int(w[4])))
        elif w[0] == "hap":
            out["hap"] = np.array(w[1:], dtype=np.int8)
        elif w[0] in ("model_f", "model_r", "h1", "h2"):
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    return ec.make(variants, reads), np.array(gt, np.int32), out


@pytest.mark.gpu
def test_c_example_equals_the_python_call(tmp_path, gpu_ctx):
    from oracle import pairhmm as ph
    from tests import haplotag_aligned_oracle as hao
    from tests import haptag_oracle as ho
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reads tagged" in r.stdout
    chunk, gt, out = _parse(r.stdout)
    assert len(chunk.read_pos) == 12 and len(chunk.alleles) == 3
    f, rv = (capi.PairHmm.from_buffer_copy(out[k].tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    got, st = capi.haplotag_aligned_chunks(gpu_ctx, [chunk], [gt], f, rv, ec.OPTS)  # the example's options
    assert np.array_equal(out["hap"], got[0]["hap"])
    for k in ("h1", "h2"):
        assert np.array_equal(out[k].view(np.uint64), got[0][k].view(np.uint64)), k
    want = hao.haplotag([chunk], [gt], ec.OPTS, ph.Model.from_buffer_copy(bytes(f)), ph.Model.from_buffer_copy(bytes(rv)))[0]
    ho.assert_margins_decisive(want["h1"], want["h2"], "example")
    assert np.array_equal(out["hap"], want["hap"]) and (out["hap"] > 0).sum() >= 6 and (out["hap"] == -1).sum() >= 2
