"""examples/phase_from_alignments_records.c: from alignments through mrp_phase_aligned_chunks_with_records, mrp_stitch_chunk and
mrp_variants_from_records to mrp_phase_sets, from plain C.  It must compile against include/ with plain gcc and link against the
in-tree library; on a GPU it exits 0 and everything it prints is what the Python calls give over the same input, which the example
writes out."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "phase_from_alignments_records")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "phase_from_alignments_records.c"), "-L" + libdir, "-lmargin_rphmm", "-lm",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(text):
    variants, fvariants, gt, reads, keep, records, phased, out = [], [], [], [], [], [], [], {}
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
        elif w[0] == "record":
            records.append(dict(chunk=int(w[1]), site=int(w[2]), state=int(w[3]), gt=(int(w[4]), int(w[5])), logs=[float.fromhex(x) for x in w[6:9]],
                                n_hap1=int(w[9]), n_hap2=int(w[10]), reads=[int(x) for x in w[11:]]))
        elif w[0] == "phased":
            a, b = w[2].split("|")
            phased.append((int(w[1]), int(a), int(b), int(w[4]), int(w[6]), int(w[8]), int(w[10])))
        elif w[0] == "switched":
            out["switched"] = [int(x) for x in w[1:]]
        elif w[0] in ("model_f", "model_r"):
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    return variants, fvariants, np.array(gt, np.int32), reads, np.array(keep, np.uint8), records, phased, out


@pytest.mark.gpu
def test_c_example_equals_the_python_calls(tmp_path, gpu_ctx):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bytes of records downloaded" in r.stdout
    variants, fvariants, gt, reads, keep, records, phased, out = _parse(r.stdout)
    chunks = [ec.make(variants, reads, chunk_start=100, chunk_end=120), ec.make(variants, reads, chunk_start=120, chunk_end=140)]
    rests = [(ec.make(fvariants, reads, chunk_start=c.chunk_start, chunk_end=c.chunk_end), gt) for c in chunks]
    f, rv = (capi.PairHmm.from_buffer_copy(out[k].tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    got, st = capi.phase_aligned_chunks_with_records(gpu_ctx, chunks, rests, f, rv, p, options=ec.OPTS, keeps=[keep, keep], min_phred=0)
    assert len(records) == sum(len(g["records"]["state"]) for g in got) == 8
    for rec in records:
        R, s = got[rec["chunk"]]["records"], rec["site"]
        assert (rec["state"], rec["gt"], rec["n_hap1"], rec["n_hap2"]) == (R["state"][s], tuple(R["gt"][s]), R["n_hap1"][s], R["n_hap2"][s])
        assert rec["reads"] == R["reads"][R["read_first"][s]:R["read_first"][s + 1]].tolist()
        for k, v in zip(("genotype_log_prob", "hap1_log_prob", "hap2_log_prob"), rec["logs"]):
            assert np.float32(v).view(np.uint32) == R[k][s].view(np.uint32)
    assert any(rec["state"] == capi.RECORD_UPDATED and rec["reads"] for rec in records)
    # the stitching, the variants and the phase sets, through the binding
    stitch = capi.Stitch()
    switched = []
    for c, g in enumerate(got):
        tags = g["filtered"]["read_hap"][:len(reads)]
        sw, _ = stitch.chunk({f"hand{q}": 1.0 for q in np.flatnonzero(tags == 1)}, {f"hand{q}": 1.0 for q in np.flatnonzero(tags == 2)}, do_not_switch=c == 0)
        switched.append(int(sw))
    stitch.close()
    assert switched == out["switched"]
    na = [np.array([len(v[1]) for v in variants], np.int32)] * 2
    fna = [np.array([len(v[1]) for v in fvariants], np.int32)] * 2
    vs = capi.variants_from_records([g["records"] for g in got], [c.variant_pos for c in chunks], na, [fl.variant_pos for fl, _ in rests], fna, switched,
                                    [np.arange(len(reads), dtype=np.int32)] * 2)
    ps = capi.phase_sets(vs, 2, 0.05, 0.5)
    assert phased == [(v["pos"], v["gt1"], v["gt2"], v["chunk"], v["site"], s, why) for v, (s, why) in zip(vs, ps)] and len(phased) > 0
