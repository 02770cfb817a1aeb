"""mrp_forward_probabilities_rle and mrp_posterior_aligned_pairs_rle on the device against the sequential restatement
(tests/rle_pairhmm_oracle.py): every list exactly (first, x, y, weight, and log_posterior as bit patterns), the totals as bit patterns,
and the posterior total equal to the forward entry's on the same pair (tests/rle_cases.py's run checks that on every call with the
constant band)."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import rle_cases as rc
from tests import rle_pairhmm_oracle as ro
from tests import test_rle_host as host

pytestmark = pytest.mark.gpu

HOOK_WIDE = 128  # bit 7 of mrp_context_set_test_hooks: every pair of a posterior call on the pair-per-workgroup kernels, 128 threads, one workgroup
DEFAULTS = dict(expansion=20, min_diags=1000, traceback_diagonals=40)  # the reference's: one traceback over every diagonal


@contextlib.contextmanager
def hooked(ctx, on=True):
    ctx.set_test_hooks(HOOK_WIDE if on else 0)
    try:
        yield
    finally:
        ctx.set_test_hooks(0)


def same(a, b):
    for k in range(3):
        pc.assert_lists_equal(a[k], b[k])
    assert np.array_equal(a[3].view(np.int64), b[3].view(np.int64))


def totals_of(pairs, wants):
    return np.array([rc.total_of(info, len(p[0]) + len(p[2])) for p, (_, info) in zip(pairs, wants)], np.float64)


# ---- 1. an all-zero table: the plumbing, independently of the restatement ------------------------------------------------------------

def test_zero_table_equals_the_nucleotide_entries(gpu_ctx):
    rng = np.random.default_rng(11)
    R = 7
    names = ["1_12x9", "3_30x29", "4_70x65", "6_160_e4", "5_100"]
    plain = [pc.CASES[n][:3] for n in names]
    pairs = [(sx, rc.random_counts(rng, len(sx), R), sy, rc.random_counts(rng, len(sy), R), a) for sx, sy, a in plain]
    models = [pc.model(), pc.model().reverse_complement()]
    repeat = [capi.RepeatModel(np.zeros((4, R, R)), 1), capi.RepeatModel(np.zeros((4, R, R)), 0)]
    mi = np.array([0, 1, 0, 1, 1], np.uint8)
    pool, counts, xo, xl, yo, yl, ao, an = rc.pack(pairs)
    assert counts.max() == R - 1 and counts.min() == 0
    fwd, _ = capi.forward_probabilities(gpu_ctx, models, pool, xo, xl, yo, yl, mi, ao, an, expansion=10)
    got, st = capi.forward_probabilities_rle(gpu_ctx, models, repeat, pool, counts, xo, xl, yo, yl, mi, ao, an, expansion=10)
    assert np.array_equal(got.view(np.int64), fwd.view(np.int64)) and st.pairs_lane == 0 and st.pairs_wave == len(pairs)
    opt = capi.PosteriorOptions(threshold=0.01, expansion=10, min_diags_between_traceback=30, traceback_diagonals=8, with_gaps=True)
    exps = np.array([2 * int(v) for v in rng.integers(0, 8, size=len(an) // 2)], np.int64)
    assert len(set(exps.tolist())) > 2
    for ae in (None, exps):
        want = capi.posterior_aligned_pairs(gpu_ctx, models, pool, xo, xl, yo, yl, mi, ao, an, opt, anchor_expansion=ae, dynamic=ae is not None)
        assert all(len(want[k]["x"]) > 0 for k in range(3))
        for hook in (False, True):
            with hooked(gpu_ctx, hook):
                same(capi.posterior_aligned_pairs_rle(gpu_ctx, models, repeat, pool, counts, xo, xl, yo, yl, mi, ao, an, opt, anchor_expansion=ae), want)


# ---- 2. the table's index and the strand --------------------------------------------------------------------------------------------

def index_pair():
    """30 x 29 with N in both strings, counts over the whole range"""
    sx, sy = (np.array(s, np.uint8).copy() for s in pc.CASES["3_30x29"][:2])
    sx[[4, 17]] = 4
    sy[[9, 17, 28]] = 4
    rng = np.random.default_rng(21)
    R = 6
    return (sx, rc.random_counts(rng, len(sx), R), sy, rc.random_counts(rng, len(sy), R), []), rc.random_table(rng, R)


# one traceback of 59 diagonals: the total is recomputed five times beyond the first; and six tracebacks of ten posterior diagonals
INDEX_KW = {"one_long": DEFAULTS, "several": dict(expansion=20, min_diags=14, traceback_diagonals=3)}


@functools.lru_cache(maxsize=None)
def index_expected(kw_name, strand):
    pair, table = index_pair()
    return rc.want_posterior(pc.model(), table, strand, pair, INDEX_KW[kw_name], 0.01)


@pytest.mark.parametrize("with_gaps", [False, True])
@pytest.mark.parametrize("kw_name", sorted(INDEX_KW))
def test_index_and_strand(gpu_ctx, kw_name, with_gaps):
    pair, table = index_pair()
    assert len(pair[0]) == 30 and len(pair[2]) == 29 and (pair[0] == 4).any() and (pair[2] == 4).any()
    assert len({table[b].tobytes() for b in range(4)}) == 4  # a different table for every base: 3 - b shows
    got = {}
    for strand in (1, 0):
        want, info = index_expected(kw_name, strand)
        if kw_name == "one_long":
            assert len(info) == 1 and info[0][3] > 10 and len(info[0][4]) >= 2  # more than 10 diagonals: the total is taken again
        else:
            assert len(info) >= 3
        opt = pc.options(INDEX_KW[kw_name], 0.01, with_gaps)
        got[strand] = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(table, strand)], [pair], opt)
        rc.check(got[strand], [want], with_gaps)
        assert np.array_equal(got[strand][3].view(np.int64), totals_of([pair], [(want, info)]).view(np.int64))
    # a test that ignored the strand, or the counts, could not pass
    assert not np.array_equal(got[0][0]["log_posterior"], got[1][0]["log_posterior"]) and got[0][3][0] != got[1][3][0]
    pool, _, xo, xl, yo, yl, ao, an = rc.pack([pair])
    plain = capi.posterior_aligned_pairs(gpu_ctx, [pc.model()], pool, xo, xl, yo, yl, None, ao, an, pc.options(INDEX_KW[kw_name], 0.01, with_gaps))
    assert plain[3][0] != got[1][3][0] and plain[3][0] != got[0][3][0]


# ---- 3. two models in one call ---------------------------------------------------------------------------------------------------------

def test_two_models_with_different_tables(gpu_ctx):
    rng = np.random.default_rng(31)
    models = [pc.model(), pc.model().reverse_complement()]
    tables = [rc.random_table(rng, 51), rc.random_table(rng, 4)]
    strands = [1, 0]
    mi = [1, 0, 1]
    kw = dict(expansion=10, min_diags=12, traceback_diagonals=3)
    pairs, wants = [], []
    for k, m in enumerate(mi):
        R = tables[m].shape[1]
        sx, cx, sy, cy = rc.rle_pair(310 + k, 25 + 6 * k, R)
        pairs.append((sx, cx, sy, cy, []))
        wants.append(rc.want_posterior(models[m], tables[m], strands[m], pairs[-1], kw, 0.01))
    assert max(int(p[1].max()) for p in pairs) == 50 and max(int(pairs[0][1].max()), int(pairs[2][1].max())) == 3
    repeat = [capi.RepeatModel(t, s) for t, s in zip(tables, strands)]
    for hook in (False, True):
        with hooked(gpu_ctx, hook):
            got = rc.run(gpu_ctx, models, repeat, pairs, pc.options(kw, 0.01, True), model_index=np.array(mi, np.uint8))
        rc.check(got, [w[0] for w in wants])
        assert np.array_equal(got[3].view(np.int64), totals_of(pairs, wants).view(np.int64))


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------------

def test_edges(gpu_ctx):
    e = np.zeros(0, np.uint8)
    u8 = lambda *v: np.array(v, np.uint8)
    pairs = [(e, e, e, e, []), (e, e, u8(0, 1, 2, 3, 0), u8(1, 0, 4, 2, 1), []), (u8(2), u8(3), u8(2), u8(4), []), (u8(1), u8(0), e, e, []),
             (u8(0, 4, 2, 7, 3, 1), u8(4, 1, 0, 2, 3, 1), u8(0, 4, 2, 9, 1), u8(2, 2, 1, 0, 4), [])]
    table = rc.random_table(np.random.default_rng(41), 5)
    kw = dict(expansion=4, min_diags=4, traceback_diagonals=1)
    wants = [rc.want_posterior(pc.model(), table, 1, (np.minimum(p[0], 4), p[1], np.minimum(p[2], 4), p[3], p[4]), kw, 0.01) for p in pairs]
    for hook in (False, True):
        with hooked(gpu_ctx, hook):
            got = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(table, 1)], pairs, pc.options(kw, 0.01, True))
        rc.check(got, [w[0] for w in wants])
        assert got[3][0] == 0.0 and all(got[k]["first"][1] == 0 for k in range(3))
        assert np.array_equal(got[3].view(np.int64), totals_of(pairs, wants).view(np.int64))


# ---- 5. every launch class ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(rc.GOLDEN, "posterior", "rle_classes.npz"))


def golden_pair(g, name):
    want = []
    for tag in ("match", "gapx", "gapy"):
        w = {f: g[f"{name}_{tag}_{f}"] for f in ("x", "y", "weight", "log_posterior")}
        w["first"] = np.array([0, len(w["x"])], np.int64)
        assert len(w["x"]) > 0
        want.append(w)
    return (g[name + "_x"], g[name + "_cx"], g[name + "_y"], g[name + "_cy"], []), want, g[name + "_total"]


@pytest.mark.parametrize("lx, ly, cls", [(40, 44, 64), (70, 70, 256)])
def test_small_launch_classes_live(gpu_ctx, lx, ly, cls):
    sx, cx, sy, cy = rc.rle_pair(500 + lx, lx, rc.R_SHIPPED, ly)
    width = capi.pair_diagonal_width([], lx, ly, 20)[0]
    assert width <= cls and (cls == 64 or width > 64)
    pair = (sx, cx, sy, cy, [])
    kw = dict(expansion=20, min_diags=24, traceback_diagonals=5)
    want, info = rc.want_posterior(pc.model(), rc.shipped_matrix(), 1, pair, kw, 0.01)
    got = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(rc.shipped_matrix(), 1)], [pair], pc.options(kw, 0.01, True))
    rc.check(got, [want])
    assert np.array_equal(got[3].view(np.int64), totals_of([pair], [(want, info)]).view(np.int64))


@pytest.mark.parametrize("name, cls, strand, kw", [("w257", 1024, 0, dict(expansion=20, min_diags=30, traceback_diagonals=4)), ("w1101", 2048, 1, DEFAULTS)])
def test_large_launch_classes_from_the_fixture(gpu_ctx, golden, name, cls, strand, kw):
    pair, want, total = golden_pair(golden, name)
    width = capi.pair_diagonal_width([], len(pair[0]), len(pair[2]), 20)[0]
    assert cls // 2 < width <= cls if cls == 2048 else 256 < width <= cls
    got = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(rc.shipped_matrix(), strand)], [pair], pc.options(kw, 0.01, True))
    for k in range(3):
        pc.assert_lists_equal(got[k], want[k])
    assert np.array_equal(got[3].view(np.int64), total.view(np.int64))


# ---- 6. the pair-per-workgroup kernels ------------------------------------------------------------------------------------------------

AROUND = {127: (126, 138), 128: (127, 139), 129: (128, 140), 257: (256, 268)}  # widest diagonal -> lx, ly
AROUND_KW = dict(expansion=20, min_diags=30, traceback_diagonals=4)
AROUND_THRESHOLD = 1e-4


def around_pair(width):
    lx, ly = AROUND[width]
    return (*rc.rle_pair(1000 + width, lx, rc.R_SHIPPED, ly), [])


@functools.lru_cache(maxsize=None)
def around_expected(width):
    return rc.want_posterior(pc.model(), rc.shipped_matrix(), 1, around_pair(width), AROUND_KW, AROUND_THRESHOLD)


@pytest.mark.parametrize("width", sorted(AROUND))
def test_around_the_hook_workgroup(gpu_ctx, width):
    pair = around_pair(width)
    assert capi.pair_diagonal_width([], len(pair[0]), len(pair[2]), 20)[0] == width
    want, info = around_expected(width)
    assert len(info) >= 3
    before = gpu_ctx.posterior_wide_count()
    with hooked(gpu_ctx):
        got = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(rc.shipped_matrix(), 1)], [pair], pc.options(AROUND_KW, AROUND_THRESHOLD, True))
    assert gpu_ctx.posterior_wide_count()[0] == before[0] + 1  # the pair-per-workgroup kernels took it
    rc.check(got, [want])
    assert np.array_equal(got[3].view(np.int64), totals_of([pair], [(want, info)]).view(np.int64))


def test_three_pairs_share_one_workgroup(gpu_ctx):
    """a grid of one workgroup: the second and third pair (and their tracebacks) start over in the slice the one before left behind"""
    pairs = [around_pair(257), (*rc.rle_pair(61, 70, rc.R_SHIPPED, 65), []), around_pair(129)]
    wants = [around_expected(257), rc.want_posterior(pc.model(), rc.shipped_matrix(), 1, pairs[1], AROUND_KW, AROUND_THRESHOLD), around_expected(129)]
    repeat = [capi.RepeatModel(rc.shipped_matrix(), 1)]
    opt = pc.options(AROUND_KW, AROUND_THRESHOLD, True)
    with hooked(gpu_ctx):
        got = rc.run(gpu_ctx, [pc.model()], repeat, pairs, opt)
    rc.check(got, [w[0] for w in wants])
    same(got, rc.run(gpu_ctx, [pc.model()], repeat, pairs, opt))  # the pair-per-wave kernels


def test_forward_beyond_2048_cells(gpu_ctx, golden):
    name = "w2060"
    pair = (golden[name + "_x"], golden[name + "_cx"], golden[name + "_y"], golden[name + "_cy"], [])
    pool, counts, xo, xl, yo, yl, ao, an = rc.pack([pair])
    assert capi.pair_diagonal_width([], int(xl[0]), int(yl[0]), 20)[0] > 2048
    repeat = [capi.RepeatModel(rc.shipped_matrix(), 1)]
    with pytest.raises(capi.MrpError) as e:
        capi.forward_probabilities_rle(gpu_ctx, [pc.model()], repeat, pool, counts, xo, xl, yo, yl, expansion=20)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    gpu_ctx.set_wide_pairs(True)
    try:
        before = gpu_ctx.wide_pair_count()
        got, st = capi.forward_probabilities_rle(gpu_ctx, [pc.model()], repeat, pool, counts, xo, xl, yo, yl, expansion=20)
        assert gpu_ctx.wide_pair_count()[0] == before[0] + 1
    finally:
        gpu_ctx.set_wide_pairs(False)
    assert np.array_equal(got.view(np.int64), golden[name + "_total"].view(np.int64))


# ---- 7. the two bands ---------------------------------------------------------------------------------------------------------------------

def test_dynamic_and_constant_band(gpu_ctx):
    kw = pc.CASES["6_160_e10"][3]  # expansion 10, eight tracebacks, ragged at both ends
    sx, cx, sy, cy = rc.rle_pair(71, 160, rc.R_SHIPPED)
    anchors = [(i, min(i, len(sy) - 1)) for i in range(20, min(len(sx), len(sy)) - 5, 25)]
    pair = (sx, cx, sy, cy, anchors)
    exps = [2 * (k % 4) + 2 * (k == 2) * 5 for k in range(len(anchors))]
    assert len(set(exps)) > 2
    repeat = [capi.RepeatModel(rc.shipped_matrix(), 0)]
    opt = pc.options(kw, 0.01, True)
    want_dyn = rc.want_posterior(pc.model(), rc.shipped_matrix(), 0, pair, kw, 0.01, expansions=exps)
    want_const = rc.want_posterior(pc.model(), rc.shipped_matrix(), 0, pair, kw, 0.01)
    assert want_dyn[0] != want_const[0]
    for hook in (False, True):
        with hooked(gpu_ctx, hook):
            dyn = rc.run(gpu_ctx, [pc.model()], repeat, [pair], opt, anchor_expansion=np.array(exps, np.int64))
            const = rc.run(gpu_ctx, [pc.model()], repeat, [pair], opt)  # anchor_expansion = NULL: band_construct with opt->expansion
        rc.check(dyn, [want_dyn[0]])
        rc.check(const, [want_const[0]])
        assert np.array_equal(dyn[3].view(np.int64), totals_of([pair], [want_dyn]).view(np.int64))
        assert np.array_equal(const[3].view(np.int64), totals_of([pair], [want_const]).view(np.int64))


# ---- 8. a shipped matrix ------------------------------------------------------------------------------------------------------------------

def test_shipped_matrix_and_geometric_counts(gpu_ctx):
    table = rc.shipped_matrix()
    assert table.shape == (4, 51, 51) and len({table[b].tobytes() for b in range(4)}) == 4
    sx, cx, sy, cy = rc.rle_pair(81, 100, rc.R_SHIPPED)
    assert 90 <= len(sy) <= 104
    pair = (sx, cx, sy, cy, [])
    for strand in (1, 0):
        want, info = rc.want_posterior(pc.model(), table, strand, pair, DEFAULTS, 0.01)
        got = rc.run(gpu_ctx, [pc.model()], [capi.RepeatModel(table, strand)], [pair], pc.options(DEFAULTS, 0.01, True))
        rc.check(got, [want])
        assert np.array_equal(got[3].view(np.int64), totals_of([pair], [(want, info)]).view(np.int64))
        sym = lambda s, c: ro.symbols(s, c, rc.R_SHIPPED)
        fwd = ro.forward_probability(pc.model(), sym(sx, cx), sym(sy, cy), [], expansion=20, rsm=ro.RepeatSubMatrix(table, strand))
        assert float(got[3][0]).hex() == fwd.hex()


# ---- the C example ------------------------------------------------------------------------------------------------------------------------

def test_c_example_equals_the_restatement(tmp_path):
    r = subprocess.run([host.build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:2] == host.example_compressed_lines()
    R = host.EXAMPLE_R
    (sx, cx), (sy, cy) = ro.rle_compress(host.EXAMPLE_X, R), ro.rle_compress(host.EXAMPLE_Y, R)
    lists, info = rc.want_posterior(capi.PairHmm.default_nucleotide(), host.example_table(), 1, (sx, cx, sy, cy, []), DEFAULTS, 0.01)
    total = float(rc.total_of(info, len(sx) + len(sy)))
    assert float.fromhex(lines[2].split()[1]) == total and float.fromhex(lines[3].split()[1]) == total
    want = [f"{name} {px} {py} {w} {float(v).hex()}" for name, l in zip(("match", "gap_x", "gap_y"), lists) for w, px, py, v in l]
    got = [ln for ln in lines if ln.split()[0] in ("match", "gap_x", "gap_y")]
    norm = lambda ln: " ".join(ln.split()[:4] + [float.fromhex(ln.split()[4]).hex()])
    assert len(lists[0]) > 0 and [norm(ln) for ln in got] == [norm(ln) for ln in want]
