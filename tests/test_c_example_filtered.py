"""examples/phase_from_strings_filtered.c: mrp_phase_string_chunks_with_filtered from plain C.  It must compile against include/
and link against the in-tree library; on a GPU its results must be those of the chain of single calls over the same inputs
(tests/string_filtered_cases.py), which the example writes out."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "phase_from_strings_filtered")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "phase_from_strings_filtered.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr


def _parse(path):
    sym = lambda s: synth_symbols(s)
    bubbles, fsubs, variants, out = [], [], [], {}
    strand_p = strand_f = None
    where = None
    for line in open(path):
        w = line.split()
        if w[0] == "reads":
            n_primary, n_filtered = int(w[1]), int(w[2])
        elif w[0] == "strand_p":
            strand_p = np.array(w[1:], dtype=np.uint8)
        elif w[0] == "strand_f":
            strand_f = np.array(w[1:], dtype=np.uint8)
        elif w[0] == "bubble":
            bubbles.append(([], [], []))
            fsubs.append([])
            where = "bubble"
        elif w[0] == "variant":
            variants.append(([], (int(w[1]), int(w[2])), []))
            where = "variant"
        elif w[0] == "a":
            (bubbles[-1][0] if where == "bubble" else variants[-1][0]).append(sym(w[1]))
        elif w[0] == "p":
            bubbles[-1][1].append(int(w[1]))
            bubbles[-1][2].append(sym(w[2]) if len(w) > 2 else np.zeros(0, np.uint8))
        elif w[0] == "f":
            fsubs[-1].append((int(w[1]), sym(w[2]) if len(w) > 2 else np.zeros(0, np.uint8)))
        elif w[0] == "e":
            variants[-1][2].append((int(w[1]), sym(w[2]) if len(w) > 2 else np.zeros(0, np.uint8)))
        elif w[0] in ("read_hap", "variant_state"):
            out[w[0]] = np.array(w[1:], dtype=np.int32)
        else:
            out[w[0]] = np.array([float.fromhex(x) for x in w[1:]], dtype=np.float64)
    assert len(strand_p) == n_primary and len(strand_f) == n_filtered
    chunk = synth.StringChunk(bubbles=bubbles, read_names=[f"read{r:04d}" for r in range(n_primary)], read_forward_strand=strand_p, hap=np.zeros(n_primary, int),
                              truth=[0] * len(bubbles))
    return chunk, dict(forward_strand=strand_f, fsubs=fsubs, variants=variants), out


def synth_symbols(s):
    return np.frombuffer(s.encode().translate(bytes.maketrans(b"ACGT", bytes([0, 1, 2, 3]))), dtype=np.uint8).copy()


@pytest.mark.gpu
def test_c_example_equals_the_python_chain(tmp_path, gpu_ctx):
    from tests import haptag_oracle as ho
    from tests import string_filtered_cases as sf
    from tests.test_gpu_string_chunks import params
    dump = str(tmp_path / "example.txt")
    r = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resident=1" in r.stdout and "filtered variants phased" in r.stdout
    chunk, rest, out = _parse(dump)
    f, rv = (capi.PairHmm.from_buffer_copy(out.pop(k).tobytes()) for k in ("model_f", "model_r"))  # the example's state machines
    _front, back = sf.chain(gpu_ctx, [chunk], [rest], f, rv, params(), min_phred=30)  # the example's min_phred
    b = back[0]
    ho.assert_margins_decisive(b["h1"], b["h2"], "partition")
    ho.assert_margins_decisive(b["cis"], b["trans"], "phasing")
    assert (b["tagged"][:len(chunk.read_names)] == 0).any() and (out["read_hap"][len(chunk.read_names):] != 0).mean() > 0.8
    for k in ("read_hap", "variant_state"):
        assert (out[k] == b[k]).all(), k
    for k in ("h1", "h2", "cis", "trans"):
        assert (sf.bits(out[k]) == sf.bits(b[k])).all(), k
