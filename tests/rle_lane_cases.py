"""What the tests of the run-length lane kernel and of mrp_allele_read_supports_rle share (tests/test_rle_supports_host.py,
tests/test_gpu_rle_lane.py): the C example's inputs and build, the restatement of the polish loop, and the pair list that stands on
every edge of the pair-per-lane kernel's launch classes."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from margin_amd import capi
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the C example (examples/allele_read_supports_rle.c) ---------------------------------------------------------------------------

EXAMPLE_R = 8
EXAMPLE_ALLELES = ["ACCCGTTTTTGCAATGGC", "ACCCGTTTGCAATGGC"]
EXAMPLE_READS = ["ACCCGTTTTGCAATGGC", "ACCGTTTTTGCATGGC", "ACCCGTTTTGCAATGGC", ""]
EXAMPLE_STRANDS = [1, 0, 0, 1]
EXAMPLE_EXPANSION = 20


def build_example(tmp_path):
    exe = str(tmp_path / "allele_read_supports_rle")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "allele_read_supports_rle.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def example_table():
    t = np.zeros((4, EXAMPLE_R, EXAMPLE_R))
    for b in range(4):
        for u in range(EXAMPLE_R):
            for o in range(EXAMPLE_R):
                t[b, u, o] = -0.05 if u == o else -(0.6 + 0.05 * (b in (1, 2))) * abs(u - o)
    return t


def example_compressed_lines():
    out = []
    for name, strings in (("allele", EXAMPLE_ALLELES), ("read", EXAMPLE_READS)):
        for k, s in enumerate(strings):
            sym, cnt = ro.rle_compress(s, EXAMPLE_R)
            out.append(f"{name} {k} {len(sym)}:" + "".join(f" {'ACGTN'[b]}{c}" for b, c in zip(sym, cnt)))
    return out


def example_bubble():
    comp = lambda strings: [tuple(np.array(v, np.uint8) for v in ro.rle_compress(s, EXAMPLE_R)) for s in strings]
    a, r = comp(EXAMPLE_ALLELES), comp(EXAMPLE_READS)
    return ([s for s, _ in a], [c for _, c in a], [s for s, _ in r], [c for _, c in r], EXAMPLE_STRANDS)


# ---- the restatement of the loop (bubbleGraph.c:1045-1073) --------------------------------------------------------------------------

def oracle_forward(model, table, strand, sx, cx, sy, cy, expansion):
    """computeForwardProbability with run-length emissions for one unanchored pair; a symbol byte beyond 4 is an N, as the kernels read it"""
    R = table.shape[1]
    sym = lambda s, c: ro.symbols(np.minimum(np.asarray(s, np.uint8), 4), c, R)
    return ro.forward_probability(model, sym(sx, cx), sym(sy, cy), [], expansion=expansion, rsm=ro.RepeatSubMatrix(table, strand))


def want_supports(forward_model, reverse_model, forward_table, reverse_table, bubbles, expansion):
    """-> ([float32 [n_alleles, n_reads] per bubble], number of owner pairs).  forward_table / reverse_table: (table, strand).  The first
    read of a bubble with a given substring (symbols and counts) owns the scores, whatever the strand of the later equal ones."""
    out, owners = [], 0
    for alleles, allele_counts, reads, read_counts, fwd in bubbles:
        sup = np.zeros((len(alleles), len(reads)), np.float32)
        cached = {}
        for k, (r, c) in enumerate(zip(reads, read_counts)):
            key = (np.asarray(r, np.uint8).tobytes(), np.asarray(c, np.uint8).tobytes())
            if key in cached:
                sup[:, k] = sup[:, cached[key]]
                continue
            cached[key] = k
            model, (table, strand) = (forward_model, forward_table) if fwd[k] else (reverse_model, reverse_table)
            for j, (a, ac) in enumerate(zip(alleles, allele_counts)):
                sup[j, k] = np.float32(oracle_forward(model, table, strand, a, ac, r, c, expansion))
                owners += 1
        out.append(sup)
    return out, owners


# ---- the pair list of the kernel's edges ----------------------------------------------------------------------------------------------

def lane_class(lx, caps):
    """the launch class phm_classify gives an eligible pair: the first whose cap holds its x string"""
    return next(c for c in range(4) if lx <= caps[c])


def edge_pairs(caps, bound, R, seed=101):
    """-> [(sx, cx, sy, cy, model index, eligible)]: every case the lane kernel's issue lists.  eligible is the test's own count: no
    anchors anywhere, x within the last cap, every count below the bound."""
    rng = np.random.default_rng(seed)
    pairs = []

    def string(n, lo=0, hi=4):
        return rng.integers(lo, hi, size=n).astype(np.uint8)

    def small_counts(n):
        c = rng.integers(0, bound, size=n).astype(np.uint8)
        if n >= 2:
            i, j = rng.choice(n, size=2, replace=False)
            c[i], c[j] = 0, bound - 1
        return c

    def add(lx, ly, model=None, sx=None, sy=None, cx=None, cy=None):
        sx = string(lx) if sx is None else np.asarray(sx, np.uint8)
        sy = string(ly) if sy is None else np.asarray(sy, np.uint8)
        cx = small_counts(len(sx)) if cx is None else np.asarray(cx, np.uint8)
        cy = small_counts(len(sy)) if cy is None else np.asarray(cy, np.uint8)
        model = len(pairs) % 2 if model is None else model
        eligible = len(sx) <= caps[3] and (len(cx) == 0 or cx.max() < bound) and (len(cy) == 0 or cy.max() < bound)
        pairs.append((sx, cx, sy, cy, model, bool(eligible)))

    for lx in (0, 1, 2, 3):  # the first rows and columns; two rows at a time: ly odd and even
        for ly in (0, 1, 2, 3, 7, 8):
            add(lx, ly)
    for c in range(4):  # on and beyond every class edge; cap[3] + 1 is a wave pair
        add(caps[c], caps[c] - 1 - c % 2)
        add(caps[c] + 1, caps[c] + c % 2)
    add(5, 6, sx=[4] * 5, sy=[4] * 6)  # a pair of N symbols
    add(6, 5, sx=[0, 7, 2, 255, 3, 1], sy=[9, 1, 2, 5, 0])  # symbol bytes beyond 4
    add(2, 30); add(30, 2); add(2, 20); add(20, 2)  # widely unequal shapes in one wave
    cx = small_counts(12); cx[5] = bound
    add(12, 11, cx=cx)  # a single count equal to the bound: a wave pair
    cy = small_counts(13); cy[0] = R - 1
    add(9, 13, cy=cy)  # a count of R - 1: a wave pair
    for k in range(65):  # 64 + 1 pairs of one class: its second wave is partly empty
        add(caps[1] + 3, caps[1] + 1 + k % 4, model=k % 2)
    return pairs


def pack_edge_pairs(pairs):
    pool, counts, xo, xl, yo, yl, _, _ = rc.pack([(sx, cx, sy, cy, []) for sx, cx, sy, cy, _, _ in pairs])
    return pool, counts, xo, xl, yo, yl, np.array([p[4] for p in pairs], np.uint8)
