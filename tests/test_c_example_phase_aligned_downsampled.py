"""examples/phase_from_alignments_downsampled.c: mrp_context_set_downsampling and mrp_phase_aligned_chunks_with_filtered from plain C,
beside the chain mrp_extract_read_substrings -> mrp_aln_read_lengths -> mrp_downsample_keep_from_extracted.  It must compile against
include/ and link against the in-tree library; on a GPU the mask it prints must be the Python restatement's, and everything else it
prints what the Python call gives over the same input with that mask passed as keep on a context without the setting."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import downsample_oracle as do
from tests import extract_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "phase_from_alignments_downsampled")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "phase_from_alignments_downsampled.c"), "-L" + libdir, "-lmargin_rphmm", "-lm",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(text):
    variants, fvariants, gt, reads, out = [], [], [], [], {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "variant":
            variants.append((int(w[1]), w[2:], 0))
        elif w[0] == "fvariant":
            fvariants.append((int(w[1]), w[4:], 0))
            gt.append((int(w[2]), int(w[3])))
        elif w[0] == "read":
            reads.append((int(w[1]), w[2], int(w[3]), int(w[4])))
        elif w[0] in ("hap", "bubble_variant", "filtered_read", "read_hap", "variant_state", "downsampling", "status", "n_substrings", "aln_len", "keep"):
            out[w[0]] = np.array(w[1:], dtype=np.int64)
        elif w[0] == "discarded":
            out["stats"] = dict(zip(w[0::2], (int(v) for v in w[1::2])))
        elif w[0] in ("model_f", "model_r", "phred", "h1", "h2", "cis", "trans", "prob"):
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    return ec.make(variants, reads), ec.make(fvariants, reads), np.array(gt, np.int32), out


@pytest.mark.gpu
def test_c_example_equals_the_python_call(tmp_path, gpu_ctx):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resident=1" in r.stdout and "the downsampling kernel took" in r.stdout
    chunk, filtered, gt, out = _parse(r.stdout)
    assert len(chunk.read_pos) == 12 and len(chunk.alleles) == 2 and len(filtered.alleles) == 2
    depth, seed, did = (int(v) for v in out["downsampling"])
    # the mask of the long way round is the Python restatement's
    assert np.array_equal(out["aln_len"], capi.aln_read_lengths(chunk))
    keep, prob, wdid, _ = do.downsample(out["status"], out["n_substrings"], out["aln_len"], 2, depth, seed, chunk.overlap_start, chunk.overlap_end)
    assert did == wdid == 1 and np.array_equal(out["keep"], keep) and np.array_equal(out["prob"].view(np.uint64), prob.view(np.uint64))
    discarded = np.flatnonzero((out["status"] == capi.READ_KEPT) & (keep == 0))
    assert len(discarded) == 3 and out["stats"] == dict(discarded=3, of_chunks=1, downsampled=1, mask_bytes=12 + 4)
    # the one call with the setting on equals the call with that mask on a context that never had it
    f, rv = (capi.PairHmm.from_buffer_copy(out[k].tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    got, st = capi.phase_aligned_chunks_with_filtered(gpu_ctx, [chunk], [(filtered, gt)], f, rv, p, options=ec.OPTS, keeps=[keep], min_phred=30)
    g = got[0]
    assert np.array_equal(out["hap"], g["hap"]) and np.array_equal(out["bubble_variant"], g["bubble_variant"])
    assert np.array_equal(out["filtered_read"], g["filtered_read"]) and set(discarded.tolist()) <= set(g["filtered_read"].tolist()) and 6 in g["filtered_read"]
    assert np.array_equal(out["read_hap"], g["filtered"]["read_hap"]) and np.array_equal(out["variant_state"], g["filtered"]["variant_state"])
    assert np.array_equal(out["phred"].view(np.uint64), g["phred"].view(np.uint64))
    for k in ("h1", "h2", "cis", "trans"):
        assert np.array_equal(out[k].view(np.uint64), g["filtered"][k].view(np.uint64)), k
    assert (out["hap"][discarded] == -1).all() and (out["read_hap"][12:] > 0).any()
