"""examples/phase_contig_queue.c: three adjacent chunks of one contig through mrp_queue_phase_aligned_chunks_with_records and
mrp_close_contig, from plain C.  It must compile against include/ with plain gcc and link against the in-tree library; on a GPU it exits
0 and everything it prints is what the Python calls give over the same input, which the example writes out."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "phase_contig_queue")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "phase_contig_queue.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(text):
    out = dict(variants=[], fvariants=[], gt=[], reads=[], keep=[], cores=[], stitched=[], phased=[], tags=[])
    for line in text.splitlines():
        w = line.split()
        if w[0] == "variant":
            out["variants"].append((int(w[1]), w[2:], 0))
        elif w[0] == "fvariant":
            out["fvariants"].append((int(w[1]), w[4:], 0))
            out["gt"].append((int(w[2]), int(w[3])))
        elif w[0] == "read":
            out["reads"].append((int(w[1]), w[2], int(w[3]), int(w[4])))
            out["keep"].append(int(w[5]))
        elif w[0] == "chunk":
            out["cores"].append((int(w[1]), int(w[2])))
        elif w[0] == "stitched":
            out["stitched"].append((int(w[3]), tuple(int(x) for x in w[5:9])))
        elif w[0] == "phased":
            a, b = w[2].split("|")
            out["phased"].append((int(w[1]), int(a), int(b), int(w[4]), int(w[6]), int(w[8]), int(w[10])))
        elif w[0] == "tags":
            out["tags"].append([int(x) for x in w[2:]])
        elif w[0] in ("model_f", "model_r"):
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    return out


@pytest.mark.gpu
def test_c_example_equals_the_python_calls(tmp_path, gpu_ctx):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 batches" in r.stdout and "bytes of records downloaded" in r.stdout
    o = _parse(r.stdout)
    variants, fvariants, reads = o["variants"], o["fvariants"], o["reads"]
    gt, keep = np.array(o["gt"], np.int32), np.array(o["keep"], np.uint8)
    assert len(o["cores"]) == 3
    chunks = [ec.make(variants, reads, chunk_start=lo, chunk_end=hi) for lo, hi in o["cores"]]
    rests = [(ec.make(fvariants, reads, chunk_start=c.chunk_start, chunk_end=c.chunk_end), gt) for c in chunks]
    f, rv = (capi.PairHmm.from_buffer_copy(o[k].tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    # the one call over the three chunks (what the queue returns at every chunk's position), then the closing through the binding
    got, _ = capi.phase_aligned_chunks_with_records(gpu_ctx, chunks, rests, f, rv, p, options=ec.OPTS, keeps=[keep] * 3, min_phred=0)
    na = np.array([len(v[1]) for v in variants], np.int32)
    fna = np.array([len(v[1]) for v in fvariants], np.int32)
    names = [f"hand{q}" for q in range(len(reads))]
    closed = capi.close_contig([dict(read_names=names, read_id=np.arange(len(reads), dtype=np.int32), hap=g["hap"], phred=g["phred"], filtered=g["filtered"],
                                     filtered_read=g["filtered_read"], records=g["records"], variant_pos=c.variant_pos, n_alleles=na,
                                     fvariant_pos=fl.variant_pos, fn_alleles=fna) for g, c, (fl, _) in zip(got, chunks, rests)], rules=(2, 0.05, 0.5))
    assert o["stitched"] == list(zip(closed["switched"], closed["counts"]))
    assert o["phased"] == [(v["pos"], v["gt1"], v["gt2"], v["chunk"], v["site"], s, why) for v, (s, why) in zip(closed["variants"], closed["phase_sets"])]
    assert len(o["phased"]) > 0 and len(o["stitched"]) == 3
    assert o["tags"] == [t.tolist() for t in closed["final_hap"]] and {1, 2} & set(o["tags"][0])
    assert o["tags"][0] == o["tags"][1] == o["tags"][2]  # the same name, the same tag
