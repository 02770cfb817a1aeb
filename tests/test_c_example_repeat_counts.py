"""examples/ml_repeat_counts.c: mrp_rle_compress, mrp_posterior_aligned_pairs_rle, mrp_ml_repeat_counts and mrp_rle_expand from plain C.
It must compile against include/ and link against the in-tree library; on a GPU the counts, log probabilities and the polished sequence
it prints must be the sequential restatements' (tests/rle_pairhmm_oracle.py, then tests/repeat_count_oracle.py), exactly."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import repeat_count_cases as cases
from tests import repeat_count_oracle as rco
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 8
DRAFT = "ACCGTTTTTGCAATGGC"
READS = ("ACCCGTTTTTTGCAATGGGC", "ACCCGTTTTTTGCAATGGC", "ACCCGTTTTTGCAATGGGC", "ACCGTTTTTTGCAATGGGC", "ACCCGTTTTTTGCAAATGGGC")
STRANDS = (1, 0, 1, 0, 1)
KW = dict(expansion=20, min_diags=1000, traceback_diagonals=40)


def _build(tmp_path):
    exe = str(tmp_path / "ml_repeat_counts")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ml_repeat_counts.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def _table():
    t = np.zeros((4, R, R))
    for b in range(4):
        for u in range(R):
            for o in range(R):
                t[b, u, o] = -0.05 if u == o else -(0.6 + 0.05 * (b in (1, 2))) * abs(u - o)
    return t


def _draft_line():
    sym, cnt = ro.rle_compress(DRAFT, 256)
    return f"draft {len(sym)}:" + "".join(f" {'ACGTN'[b]}{c}" for b, c in zip(sym, cnt))


def test_c_example_builds_compresses_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "mrp_context_create" in r.stderr
    assert r.stdout.splitlines() == [_draft_line()]  # the compression needs no device


@pytest.mark.gpu
def test_c_example_prints_the_restatements_sequence(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == _draft_line()
    m = capi.PairHmm.default_nucleotide()
    models = {1: m, 0: m.reverse_complement()}
    sx, cx = (np.array(a, np.uint8) for a in ro.rle_compress(DRAFT, R))
    matches, lengths = [], []
    for read, strand in zip(READS, STRANDS):
        sy, cy = (np.array(a, np.uint8) for a in ro.rle_compress(read, R))
        lists, _ = rc.want_posterior(models[strand], _table(), strand, (sx, cx, sy, cy, []), KW, 0.01)
        matches.append([(x, y, w) for w, x, y, _ in lists[0]])
        lengths.append(np.array(ro.rle_compress(read, 256)[1], np.uint8))
    w = cases.want(_table(), [cases.consensus(sx, lengths, STRANDS, matches)], walk_backwards=True)
    want = [f"node {i} {'ACGTN'[b]} {c} {float(v).hex()}" for i, (b, c, v) in enumerate(zip(sx, w["count"], w["log_prob"]))]
    got = [ln for ln in lines if ln.startswith("node ")]
    norm = lambda ln: " ".join(ln.split()[:4] + [float.fromhex(ln.split()[4]).hex()])
    assert [norm(ln) for ln in got] == [norm(ln) for ln in want]
    polished = rco.rle_expand(sx, w["count"])
    assert lines[-2] == "polished " + polished and polished == "ACCCGTTTTTTGCAATGGGC" != DRAFT
    assert lines[-1] == f"{w['observations']} observations of {w['nodes_observed']} nodes, {w['candidates']} candidates"
