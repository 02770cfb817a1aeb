"""examples/poa_consensus.c: mrp_rle_compress, mrp_posterior_aligned_pairs_rle(with_gaps = 1), mrp_poa_augment, mrp_poa_consensus and
mrp_rle_expand from plain C.  It must compile against include/ and link against the in-tree library; on a GPU every node, the totals, the
map and the sequence it prints must be the sequential restatements' (tests/rle_pairhmm_oracle.py, then tests/poa_oracle.py), exactly."""
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import poa_cases as cases
from tests import poa_oracle as po
from tests import repeat_count_oracle as rco
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro
from tests.test_c_example_repeat_counts import KW, R, READS, STRANDS, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAFT = "ACCGTTTTTCAATTGGC"


def _build(tmp_path):
    exe = str(tmp_path / "poa_consensus")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "poa_consensus.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def _draft_line():
    sym, cnt = ro.rle_compress(DRAFT, 256)
    return f"draft {len(sym)}:" + "".join(f" {'ACGTN'[b]}{c}" for b, c in zip(sym, cnt))


def expected_lines():
    """the oracle chain: the three lists of every read, the graph, the consensus"""
    m = capi.PairHmm.default_nucleotide()
    models = {1: m, 0: m.reverse_complement()}
    sx, cx = (np.array(a, np.uint8) for a in ro.rle_compress(DRAFT, R))
    reads = []
    flip = lambda l: [(x, y, w) for w, x, y, _ in l]
    for read, strand in zip(READS, STRANDS):
        sy, cy = (np.array(a, np.uint8) for a in ro.rle_compress(read, R))
        lists, _ = rc.want_posterior(models[strand], _table(), strand, (sx, cx, sy, cy, []), KW, 0.01)
        reads.append(cases.read(sy, ro.rle_compress(read, 256)[1], strand, flip(lists[0]), flip(lists[1]), flip(lists[2])))
    call = [cases.consensus(sx, cx, reads)]
    w, (poa,), st = cases.want(call, R)
    lines = []
    for k, node in enumerate(poa["nodes"]):
        ln = f"node {k} {'ACGTN'[node['base']]} pick {'ACGTN'[node['base_pick']]} {node['repeat_count_pick']} weights" + "".join(f" {v:.0f}" for v in node["base_weights"])
        for e in node["inserts"]:
            ln += " +" + "".join(f"{'ACGTN'[b]}{c}" for b, c in zip(e["symbols"], e["counts"])) + f":{e['forward']:.0f}/{e['reverse']:.0f}"
        for e in node["deletes"]:
            ln += f" -{e['length']}:{e['forward']:.0f}/{e['reverse']:.0f}"
        lines.append(ln)
    lines.append("totals " + " ".join(f"{v:.0f}" for v in w["totals"][0]))
    s, c, cmap = po.consensus(poa, True)
    lines.append("map" + "".join(f" {v}" for v in cmap))
    sequence = rco.rle_expand(s, c)
    lines.append("consensus " + sequence)
    n = [sum(len(rd[k]) for rd in reads) for k in ("matches", "deletes", "inserts")]
    lines.append(f"{n[0]} matches, {n[1]} deletes, {n[2]} inserts: {st['complete_inserts']} complete inserts ({len(w['insert_str_len'])} distinct), "
                 f"{st['complete_deletes']} complete deletes ({len(w['delete_length'])} distinct)")
    return lines, sequence


def test_c_example_builds_compresses_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "mrp_context_create" in r.stderr
    assert r.stdout.splitlines() == [_draft_line()]  # the compression needs no device


def test_the_oracle_chain_repairs_the_draft():
    """no device: what the example is expected to print ends in the reads' sequence, not the draft's"""
    lines, sequence = expected_lines()
    assert sequence != DRAFT and sequence == "ACCCGTTTTTTGCAATGGGC"
    assert any(" +G1:" in ln for ln in lines) and lines[-1].split()[0].isdigit()


@pytest.mark.gpu
def test_c_example_prints_the_oracle_chains_sequence(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    want, sequence = expected_lines()
    assert lines[0] == _draft_line()
    assert lines[1:] == want
    assert lines[-2] == "consensus " + sequence
