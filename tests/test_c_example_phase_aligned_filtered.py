"""examples/phase_from_alignments_filtered.c: mrp_phase_aligned_chunks_with_filtered from plain C.  It must compile against include/
and link against the in-tree library; on a GPU everything it prints must be what the Python call gives over the same input, which the
example writes out."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "phase_from_alignments_filtered")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "phase_from_alignments_filtered.c"), "-L" + libdir, "-lmargin_rphmm", "-lm",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(text):
    variants, fvariants, gt, reads, keep, out = [], [], [], [], [], {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "variant":
            variants.append((int(w[1]), w[2:], 0))
        elif w[0] == "fvariant":
            fvariants.append((int(w[1]), w[4:], 0))
            gt.append((int(w[2]), int(w[3])))
        elif w[0] == "read":
            reads.append((int(w[1]), w[2], int(w[3]), int(w[4])))
            keep.append(int(w[5]))
        elif w[0] in ("hap", "bubble_variant", "filtered_read", "read_hap", "variant_state"):
            out[w[0]] = np.array(w[1:], dtype=np.int64)
        elif w[0] in ("model_f", "model_r", "phred", "h1", "h2", "cis", "trans"):
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    return ec.make(variants, reads), ec.make(fvariants, reads), np.array(gt, np.int32), np.array(keep, np.uint8), out


@pytest.mark.gpu
def test_c_example_equals_the_python_call(tmp_path, gpu_ctx):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resident=1" in r.stdout and "filtered variants phased" in r.stdout
    chunk, filtered, gt, keep, out = _parse(r.stdout)
    assert len(chunk.read_pos) == 12 and len(chunk.alleles) == 2 and len(filtered.alleles) == 2 and (keep == 0).sum() == 1
    f, rv = (capi.PairHmm.from_buffer_copy(out[k].tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    got, st = capi.phase_aligned_chunks_with_filtered(gpu_ctx, [chunk], [(filtered, gt)], f, rv, p, options=ec.OPTS, keeps=[keep], min_phred=30)
    g = got[0]
    assert np.array_equal(out["hap"], g["hap"]) and np.array_equal(out["bubble_variant"], g["bubble_variant"])
    assert np.array_equal(out["filtered_read"], g["filtered_read"]) and 7 in g["filtered_read"] and 6 in g["filtered_read"]  # masked, low mapq
    assert np.array_equal(out["read_hap"], g["filtered"]["read_hap"]) and np.array_equal(out["variant_state"], g["filtered"]["variant_state"])
    assert np.array_equal(out["phred"].view(np.uint64), g["phred"].view(np.uint64))
    for k in ("h1", "h2", "cis", "trans"):
        assert np.array_equal(out[k].view(np.uint64), g["filtered"][k].view(np.uint64)), k
    assert (out["variant_state"] != capi.VARIANT_NOT_VISITED).any() and (out["read_hap"][12:] > 0).any()
