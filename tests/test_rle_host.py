"""The run-length emissions without a device: the restatement (tests/rle_pairhmm_oracle.py) against the nucleotide one on an all-zero
table, mrp_rle_compress against rleString_construct's restatement, every new MRP_ERR_ARG of the two entries with a NULL context (raised
before the context is looked at, nothing written), and the C example's build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import posterior_oracle as po
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["1_12x9", "3_30x29", "6_160_e4"])
def test_zero_table_is_the_nucleotide_restatement(name):
    sx, sy, anchors, kw = pc.CASES[name]
    rng = np.random.default_rng(5)
    R = 9
    cx, cy = rc.random_counts(rng, len(sx), R), rc.random_counts(rng, len(sy), R)
    want, want_info = pc.expected(name, 0.01)
    for strand in (0, 1):
        got, info = rc.want_posterior(pc.model(), np.zeros((4, R, R)), strand, (sx, cx, sy, cy, anchors), kw, 0.01)
        for k in range(3):
            assert len(want[k]) > 0
            assert [(w, x, y, float(v).hex()) for w, x, y, v in got[k]] == [(w, x, y, float(v).hex()) for w, x, y, v in want[k]]
        assert [(d, float(t).hex()) for *_, rec in info for d, t in rec] == [(d, float(t).hex()) for *_, rec in want_info for d, t in rec]
    # the forward probability: the total of the last traceback, with and without counts
    fkw = dict(expansion=kw["expansion"], ragged_left=kw.get("ragged_left", False), ragged_right=kw.get("ragged_right", False))
    plain = ro.forward_probability(pc.model(), sx, sy, anchors, **fkw)
    assert plain.hex() == float(rc.total_of(want_info, len(sx) + len(sy))).hex()
    rsm = ro.RepeatSubMatrix(np.zeros((4, R, R)), 1)
    assert ro.forward_probability(pc.model(), ro.symbols(sx, cx, R), ro.symbols(sy, cy, R), anchors, rsm=rsm, **fkw).hex() == plain.hex()


def test_the_table_changes_the_restatement_and_the_strand_shows():
    sx, sy, anchors, kw = pc.CASES["3_30x29"]
    rng = np.random.default_rng(6)
    R = 5
    table = rc.random_table(rng, R)
    pair = (sx, rc.random_counts(rng, len(sx), R), sy, rc.random_counts(rng, len(sy), R), anchors)
    a, _ = rc.want_posterior(pc.model(), table, 1, pair, kw, 0.01)
    b, _ = rc.want_posterior(pc.model(), table, 0, pair, kw, 0.01)
    assert a[0] != b[0] and a[0] != pc.expected("3_30x29", 0.01)[0][0]


def test_index_and_symbols():
    rsm = ro.RepeatSubMatrix(np.arange(4 * 3 * 3, dtype=np.float64).reshape(4, 3, 3), 1)
    assert rsm.index(2, True, 1, 2) == 2 * 9 + 2 * 3 + 1 and rsm.index(2, False, 1, 2) == 1 * 9 + 2 * 3 + 1
    assert rsm.index(4, True, 0, 0) == 0 and rsm.index(4, False, 0, 0) == 3 * 9  # N -> A, then the strand (repeatSubMatrix.c:16-29)
    s = ro.symbol_add_repeat_count(3, 9, 8)
    assert (ro.symbol_strip_repeat_count(s), ro.symbol_get_repeat_length(s)) == (3, 7)
    assert ro.symbol_get_repeat_length(4) == 0  # the symbol before the first: N with count 0


# ---- mrp_rle_compress -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s, R", [("", 51), ("A", 51), ("G" * 9 + "T", 4), ("C" * 3 + "A" * 4 + "C" * 50, 4), ("acgtnNNxACGT", 51), ("aaAAccCgG", 51),
                                  ("T" * 300, 256), ("ACGT" * 20, 2)])
def test_rle_compress(s, R):
    sym, cnt = capi.rle_compress(s, R)
    want_sym, want_cnt = ro.rle_compress(s, R)
    assert sym.tolist() == want_sym and cnt.tolist() == want_cnt
    assert len(sym) == len(ro.rle_string(s)[0]) and all(c <= R - 1 for c in cnt.tolist())
    assert sum(ro.rle_string(s)[1]) == len(s)


def test_rle_compress_refuses():
    L = capi.load()
    out = np.zeros(4, np.uint8)
    assert L.mrp_rle_compress(b"AC", 2, 1, out.ctypes.data, out.ctypes.data) == -1
    assert L.mrp_rle_compress(b"AC", 2, 257, out.ctypes.data, out.ctypes.data) == -1
    assert L.mrp_rle_compress(b"AC", -1, 51, out.ctypes.data, out.ctypes.data) == -1
    assert L.mrp_rle_compress(b"AC", 2, 51, None, out.ctypes.data) == -1
    assert L.mrp_rle_compress(None, 0, 51, None, None) == 0


# ---- the argument errors ------------------------------------------------------------------------------------------------------------

SX, SY = np.array([0, 1, 2, 3], np.uint8), np.array([0, 1, 3, 3, 2], np.uint8)
CX, CY = np.array([1, 2, 0, 3], np.uint8), np.array([1, 1, 3, 0, 2], np.uint8)


def entries():
    """both entries as f(models, repeat, pairs, counts=..., model_index=...) with a NULL context"""
    def posterior(models, repeat, pairs, model_index=None, counts="packed", options=None):
        pool, cnt, xo, xl, yo, yl, ao, an = rc.pack(pairs)
        return capi.posterior_aligned_pairs_rle(None, models, repeat, pool, cnt if isinstance(counts, str) else counts, xo, xl, yo, yl, model_index, ao, an,
                                                options or capi.PosteriorOptions())

    def forward(models, repeat, pairs, model_index=None, counts="packed", options=None):
        pool, cnt, xo, xl, yo, yl, ao, an = rc.pack(pairs)
        return capi.forward_probabilities_rle(None, models, repeat, pool, cnt if isinstance(counts, str) else counts, xo, xl, yo, yl, model_index, ao, an)

    return [("mrp_posterior_aligned_pairs_rle", posterior), ("mrp_forward_probabilities_rle", forward)]


@pytest.mark.parametrize("who, entry", entries(), ids=[e[0] for e in entries()])
def test_arg_errors_come_before_the_context(who, entry):
    m = pc.model()
    ok = capi.RepeatModel(np.zeros((4, 4, 4)), strand=1)
    small = [(SX, CX, SY, CY, [])]

    def expect(code, text, *a, **kw):
        with pytest.raises(capi.MrpError) as e:
            entry(*a, **kw)
        assert e.value.code == code, str(e.value)
        assert text in str(e.value) and who in str(e.value), str(e.value)

    expect(capi.MRP_ERR_ARG, "repeat is NULL", [m], None, small)
    expect(capi.MRP_ERR_ARG, "counts is NULL", [m], [ok], small, counts=None)
    expect(capi.MRP_ERR_ARG, "no log_prob", [m], [capi.RepeatModel(None, 1, max_repeat=4)], small)
    expect(capi.MRP_ERR_ARG, "repeat model 1 has no log_prob", [m, m], [ok, capi.RepeatModel(None, 1, max_repeat=4)], small)
    for R in (1, 0, -3, 257):
        expect(capi.MRP_ERR_ARG, f"max_repeat {R} outside [2, 256]", [m], [capi.RepeatModel(np.zeros((4, 4, 4)), 1, max_repeat=R)], small)
    for strand in (2, -1):
        expect(capi.MRP_ERR_ARG, "strand must be 0 or 1", [m], [capi.RepeatModel(np.zeros((4, 4, 4)), strand)], small)
    # a count that is not below the R of its pair's model; the message names the pair
    bad = [(SX, CX, SY, CY, []), (SX, CX, SY, np.array([1, 1, 4, 0, 2], np.uint8), [])]
    expect(capi.MRP_ERR_ARG, "pair 1: the count 4 of y symbol 2", [m], [ok], bad)
    expect(capi.MRP_ERR_ARG, "pair 0: the count 3 of x symbol 3", [m, m], [ok, capi.RepeatModel(np.zeros((4, 3, 3)), 0)], small,
           model_index=np.array([1], np.uint8))
    # counts up to R - 1 pass on to the next class of errors: the context
    expect(capi.MRP_ERR_NO_DEVICE, "no context", [m], [ok], small)
    expect(capi.MRP_ERR_NO_DEVICE, "no context", [m], [capi.RepeatModel(np.zeros((4, 256, 256)), 0)], [(SX, CX + 252, SY, CY, [])])
    # the entries' other argument errors keep their place in front of the context
    expect(capi.MRP_ERR_ARG, "model", [m], [ok], small, model_index=np.array([1], np.uint8))


def test_posterior_rle_errors_write_nothing_and_keep_their_order():
    L = capi.load()
    pool, cnt, xo, xl, yo, yl, ao, an = rc.pack([(SX, CX, SY, CY + 9, [])])  # a count beyond R
    m, o = pc.model(), capi.PosteriorOptions()
    rep = capi.RepeatModel(np.zeros((4, 4, 4)), 1)
    rs = rep.struct()
    match = capi.PosteriorPairs()
    total = np.full(1, 7.0)
    p = lambda a: a.ctypes.data
    rc_ = L.mrp_posterior_aligned_pairs_rle(None, C.addressof(m), C.addressof(rs), 1, 1, p(pool), p(cnt), pool.size, p(xo), p(xl), p(yo), p(yl), None, None, None,
                                            None, C.byref(o), C.byref(match), None, None, p(total), None)
    assert rc_ == capi.MRP_ERR_ARG and not match.first and total[0] == 7.0
    out = np.full(1, 7.0)
    rc_ = L.mrp_forward_probabilities_rle(None, C.addressof(m), C.addressof(rs), 1, 1, p(pool), p(cnt), pool.size, p(xo), p(xl), p(yo), p(yl), None, None, None, 4,
                                          0, 0, p(out), None)
    assert rc_ == capi.MRP_ERR_ARG and out[0] == 7.0
    # the options' errors and the run-length ones are argument errors alike, both in front of MRP_ERR_UNSUPPORTED
    wide = [(np.zeros(2048, np.uint8), np.zeros(2048, np.uint8), np.zeros(2048, np.uint8), np.zeros(2048, np.uint8), [])]
    pool, cnt, xo, xl, yo, yl, ao, an = rc.pack(wide + [(SX, CX, SY, CY + 9, [])])
    with pytest.raises(capi.MrpError) as e:
        capi.posterior_aligned_pairs_rle(None, [m], [rep], pool, cnt, xo, xl, yo, yl, None, ao, an, o)
    assert e.value.code == capi.MRP_ERR_ARG and "pair 1" in str(e.value)
    pool, cnt, xo, xl, yo, yl, ao, an = rc.pack(wide)
    with pytest.raises(capi.MrpError) as e:
        capi.posterior_aligned_pairs_rle(None, [m], [rep], pool, cnt, xo, xl, yo, yl, None, ao, an, o)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "2049 cells (limit 2048" in str(e.value)


def test_exports_and_abi():
    L = capi.load()
    assert capi.ABI_VERSION == L.mrp_abi_version() == 6  # additions only
    for name in ("mrp_rle_compress", "mrp_forward_probabilities_rle", "mrp_posterior_aligned_pairs_rle"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.RepeatModelStruct) == 16


# ---- the C example ----------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    exe = str(tmp_path / "posterior_aligned_pairs_rle")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "posterior_aligned_pairs_rle.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


EXAMPLE_X, EXAMPLE_Y, EXAMPLE_R = "ACCCGTTTTTTTTTTGCAATGGC", "ACCGTTTTTTTTGCAATGGC", 8


def example_table():
    t = np.zeros((4, EXAMPLE_R, EXAMPLE_R))
    for b in range(4):
        for u in range(EXAMPLE_R):
            for o in range(EXAMPLE_R):
                t[b, u, o] = -0.05 if u == o else -(0.6 + 0.05 * (b in (1, 2))) * abs(u - o)
    return t


def example_compressed_lines():
    out = []
    for name, s in (("x", EXAMPLE_X), ("y", EXAMPLE_Y)):
        sym, cnt = ro.rle_compress(s, EXAMPLE_R)
        out.append(f"{name} {len(sym)}:" + "".join(f" {'ACGTN'[b]}{c}" for b, c in zip(sym, cnt)))
    return out


def test_c_example_builds_and_compresses_without_a_device(tmp_path):
    exe = build_example(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is tests/test_gpu_rle_pairhmm.py's)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "mrp_context_create" in r.stderr
    assert r.stdout.splitlines() == example_compressed_lines()  # the compression needs no device
