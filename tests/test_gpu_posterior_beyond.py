"""The posterior entries beyond what tests/test_gpu_posterior.py covers: the pair-per-workgroup kernels (pairs past a diagonal of 2 048
cells, mrp_context_set_posterior_wide_pairs; every pair with test hook bit 7, at 128 threads and a grid of one workgroup) and the dynamic
anchor band (mrp_posterior_aligned_pairs_dynamic), against the sequential restatement: every list exactly, the log posteriors as bit
patterns, and total_out bit for bit the forward value."""
import contextlib
import functools
import os

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import posterior_cases as pc
from tests import posterior_dynamic_oracle as pdo
from tests import posterior_oracle as po

pytestmark = pytest.mark.gpu

HOOK_WIDE = 128  # bit 7 of mrp_context_set_test_hooks


@contextlib.contextmanager
def hooked(ctx, on=True):
    ctx.set_test_hooks(HOOK_WIDE if on else 0)
    try:
        yield
    finally:
        ctx.set_test_hooks(0)


def run(ctx, pairs, opt, check_total=True):
    """the constant band; total_out against mrp_forward_probabilities for the same band"""
    pool, xo, xl, yo, yl, ao, an = pc.pack(pairs)
    got = capi.posterior_aligned_pairs(ctx, [pc.model()], pool, xo, xl, yo, yl, None, ao, an, opt)
    if check_total:
        fwd, _ = capi.forward_probabilities(ctx, [pc.model()], pool, xo, xl, yo, yl, None, ao, an, expansion=opt.expansion,
                                            ragged_left=bool(opt.ragged_left), ragged_right=bool(opt.ragged_right))
        assert np.array_equal(got[3].view(np.int64), fwd.view(np.int64))
    return got


def check(got, want_lists, with_gaps=True, non_empty=True):
    for k in range(3 if with_gaps else 1):
        want = pc.as_arrays([w[k] for w in want_lists])
        if non_empty:
            assert len(want["x"]) > 0
        pc.assert_lists_equal(got[k], want)


def same(a, b, with_gaps=True):
    for k in range(3 if with_gaps else 1):
        pc.assert_lists_equal(a[k], b[k])
    assert np.array_equal(a[3].view(np.int64), b[3].view(np.int64))


# ---- 1. the new kernels against the restatement, at the sizes the restatement can afford ------------------------------------------

@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("with_gaps", [False, True])
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_cases_on_the_workgroup_kernels(gpu_ctx, name, with_gaps, threshold):
    sx, sy, anchors, kw = pc.CASES[name]
    want, _ = pc.expected(name, threshold)
    opt = pc.options(kw, threshold, with_gaps)
    before = gpu_ctx.posterior_wide_count()
    with hooked(gpu_ctx):
        got = run(gpu_ctx, [(sx, sy, anchors)], opt)
    check(got, [want], with_gaps)
    after = gpu_ctx.posterior_wide_count()
    assert after[0] == before[0] + 1 and after[1] == before[1] + got[4].cells  # the new kernels took it
    plain = run(gpu_ctx, [(sx, sy, anchors)], opt)
    assert gpu_ctx.posterior_wide_count() == after
    same(got, plain, with_gaps)


def edge_pairs():
    e = np.zeros(0, np.uint8)
    return [(e, e, []), (e, np.array([0, 1, 2, 3, 0], np.uint8), []), (np.array([2], np.uint8), np.array([2], np.uint8), []), (np.array([1], np.uint8), e, []),
            (np.array([0, 4, 2, 7, 3, 1], np.uint8), np.array([0, 4, 2, 9, 1], np.uint8), [])]


def test_edges_on_the_workgroup_kernels(gpu_ctx):
    pairs = edge_pairs()
    opt = capi.PosteriorOptions(threshold=0.01, expansion=4, min_diags_between_traceback=4, traceback_diagonals=1, with_gaps=True)
    want = [po.posterior(pc.model(), sx, sy, a, expansion=4, threshold=0.01, min_diags=4, traceback_diagonals=1, with_gaps=True)[0] for sx, sy, a in pairs]
    with hooked(gpu_ctx):
        got = run(gpu_ctx, pairs, opt)
    check(got, want)
    assert got[3][0] == 0.0 and all(got[k]["first"][1] == 0 for k in range(3))
    same(got, run(gpu_ctx, pairs, opt))


@functools.lru_cache(maxsize=None)
def forty(dynamic):
    """drawn as tests/pairwiseAlignerTest.c:423-438 draws them; dynamic: an even expansion 0 .. 20 per anchor beside them"""
    rng = np.random.default_rng(423 if not dynamic else 463)
    tb = int(rng.integers(1, 11))
    kw = dict(traceback_diagonals=tb, min_diags=tb + int(rng.integers(2, 11)), expansion=2 * int(rng.integers(0, 11)))
    pairs, exps = [], []
    for _ in range(40):
        sx = synth.random_sequence(rng, int(rng.integers(0, 101)))
        sy = synth.evolve_sequence(rng, sx)
        pairs.append((sx, sy, pc.random_anchors(rng, len(sx), len(sy))))
        exps.append(pdo.random_expansions(rng, len(pairs[-1][2])) if dynamic else None)
    m = pc.model()
    if dynamic:
        res = [pdo.posterior_dynamic(m, sx, sy, a, e, threshold=0.01, with_gaps=True, **kw) for (sx, sy, a), e in zip(pairs, exps)]
    else:
        res = [po.posterior(m, sx, sy, a, threshold=0.01, with_gaps=True, **kw) for sx, sy, a in pairs]
    # the total the reference takes at diagonal lx + ly, the first of the last traceback (0.0 for two empty strings, :721-723)
    totals = np.array([dict(info[-1][4])[len(p[0]) + len(p[1])] if info else 0.0 for p, (_, info) in zip(pairs, res)], np.float64)
    return kw, pairs, exps, [r[0] for r in res], totals


def test_forty_random_pairs_on_the_workgroup_kernels(gpu_ctx):
    kw, pairs, _, want, totals = forty(False)
    opt = pc.options(kw, 0.01, True)
    with hooked(gpu_ctx):
        got = run(gpu_ctx, pairs, opt)
    check(got, want)
    assert np.array_equal(got[3].view(np.int64), totals.view(np.int64))
    same(got, run(gpu_ctx, pairs, opt))


# ---- 2. around the 128-thread workgroup of the hook -----------------------------------------------------------------------------

AROUND = {127: (126, 138), 128: (127, 139), 129: (128, 140), 257: (256, 268)}  # widest diagonal -> lx, ly
AROUND_KW = dict(expansion=20, min_diags=30, traceback_diagonals=4)
# at the reference's 0.01 a diagonal keeps one or two neighbouring cells, which seldom lie on both sides of cell 63 | 64 or 127 | 128; at 1e-4 the
# lists of these pairs do (asserted below), so a wave's and a chunk's offset into a list is not always 0
AROUND_THRESHOLD = 1e-4


def around_pair(width):
    lx, ly = AROUND[width]
    rng = np.random.default_rng(1000 + width)
    sx = synth.random_sequence(rng, lx)
    sy = pc._fit(rng, synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05), ly)
    return sx, sy


@functools.lru_cache(maxsize=None)
def around_expected(width, ragged):
    sx, sy = around_pair(width)
    return po.posterior(pc.model(), sx, sy, [], threshold=AROUND_THRESHOLD, with_gaps=True, ragged_left=ragged, ragged_right=ragged, **AROUND_KW)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("width", sorted(AROUND))
def test_around_the_hook_workgroup(gpu_ctx, width, ragged):
    sx, sy = around_pair(width)
    assert capi.pair_diagonal_width([], len(sx), len(sy), 20)[0] == width
    want, info = around_expected(width, ragged)
    assert len(info) >= 3                                   # several tracebacks
    assert max(len(rec) for *_, rec in info) >= 3           # one of them takes more than 20 diagonals: three totals
    kw = dict(AROUND_KW, ragged_left=ragged, ragged_right=ragged)
    with hooked(gpu_ctx):
        got = run(gpu_ctx, [(sx, sy, [])], pc.options(kw, AROUND_THRESHOLD, True))
    check(got, [want])
    # a list's entries of one diagonal come from both sides of a wave's last cell (cell 63 | 64) and, at 257, of a chunk's (127 | 128)
    for boundary in [b for b in (64, 128) if b < width - 1]:
        assert any(straddles(got[k], len(sx), len(sy), boundary) for k in range(3)), boundary


def straddles(lst, lx, ly, boundary):
    """some diagonal has list entries in cells below `boundary` and in cells from it on (cells count from the diagonal's least x - y)"""
    lo, _ = capi.band_diagonals([], lx, ly, 20)
    side = {}
    for x, y in zip(lst["x"].tolist(), lst["y"].tolist()):
        d = x + y + 2
        side.setdefault(d, set()).add(((x - y) - int(lo[d])) // 2 >= boundary)
    return any(len(s) == 2 for s in side.values())


# ---- 3. slice reuse and mixing ------------------------------------------------------------------------------------------------

def test_three_pairs_share_one_workgroup(gpu_ctx):
    """a grid of one workgroup: the second and third pair (and their tracebacks) start over in the slice the one before left behind"""
    a, b = around_pair(257), around_pair(129)
    c = pc.CASES["4_70x65"][:2]
    pairs = [(a[0], a[1], []), (c[0], c[1], []), (b[0], b[1], [])]
    opt = pc.options(AROUND_KW, AROUND_THRESHOLD, True)
    alone = [run(gpu_ctx, [p], opt) for p in pairs]  # the ordinary kernels
    with hooked(gpu_ctx):
        got = run(gpu_ctx, pairs, opt)
        alone_hooked = [run(gpu_ctx, [p], opt) for p in pairs]
    check(got, [around_expected(257, False)[0], po.posterior(pc.model(), c[0], c[1], [], threshold=AROUND_THRESHOLD, with_gaps=True, **AROUND_KW)[0],
                around_expected(129, False)[0]])
    for k in range(3):
        for src in (alone, alone_hooked):
            for f in ("x", "y", "weight"):
                assert np.array_equal(got[k][f], np.concatenate([r[k][f] for r in src]))
            assert np.array_equal(got[k]["log_posterior"].view(np.int64), np.concatenate([r[k]["log_posterior"] for r in src]).view(np.int64))
            assert np.array_equal(np.diff(got[k]["first"]), [len(r[k]["x"]) for r in src])
    assert np.array_equal(got[3].view(np.int64), np.concatenate([r[3] for r in alone]).view(np.int64))


# ---- 4. a really wide pair ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "posterior", "beyond_2048.npz"))
    want = []
    for tag in ("match", "gapx", "gapy"):
        w = {f: g[f"w2060_{tag}_{f}"] for f in ("x", "y", "weight", "log_posterior")}
        w["first"] = np.array([0, len(w["x"])], np.int64)
        assert len(w["x"]) > 0
        want.append(w)
    return g["w2060_x"], g["w2060_y"], want, g["w2060_total"]


@pytest.fixture
def wide_ctx(gpu_ctx):
    """the posterior wide switch on, and the forward-only one for the yardstick; both off again afterwards"""
    gpu_ctx.set_posterior_wide_pairs(True)
    gpu_ctx.set_wide_pairs(True)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_posterior_wide_pairs(False)
        gpu_ctx.set_wide_pairs(False)
        gpu_ctx.set_posterior_workspace(0)
        gpu_ctx.set_test_hooks(0)


def test_wide_pair_equals_the_fixture(wide_ctx, golden):
    sx, sy, want, total = golden
    width, cells = capi.pair_diagonal_width([], len(sx), len(sy), 20)
    assert width > 2048 and cells == (len(sx) + 1) * (len(sy) + 1)
    opt = capi.PosteriorOptions(with_gaps=True)  # the reference's defaults
    before = wide_ctx.posterior_wide_count()
    got = run(wide_ctx, [(sx, sy, [])], opt)  # (the total against mrp_forward_probabilities with wide pairs on)
    for k in range(3):
        pc.assert_lists_equal(got[k], want[k])
    assert np.array_equal(got[3].view(np.int64), total.view(np.int64))
    assert wide_ctx.posterior_wide_count() == (before[0] + 1, before[1] + cells)
    with hooked(wide_ctx):  # 128 threads, one workgroup
        same(got, run(wide_ctx, [(sx, sy, [])], opt, check_total=False))


def test_wide_pair_between_small_ones(wide_ctx, golden):
    sx, sy, want, _ = golden
    small = [pc.CASES["5_100"][:3], pc.CASES["3_30x29"][:3]]
    opt = capi.PosteriorOptions(with_gaps=True)
    alone = [run(wide_ctx, [p], opt) for p in small]
    before = wide_ctx.posterior_wide_count()
    got = run(wide_ctx, [small[0], (sx, sy, []), small[1]], opt)
    after = wide_ctx.posterior_wide_count()
    assert after == (before[0] + 1, before[1] + (len(sx) + 1) * (len(sy) + 1))  # the small pairs kept their kernels
    assert wide_ctx.last_posterior().groups == 1
    for k in range(3):
        f = got[k]["first"]
        parts = [alone[0][k], want[k], alone[1][k]]
        assert np.array_equal(np.diff(f), [len(p["x"]) for p in parts])
        for name in ("x", "y", "weight"):
            assert np.array_equal(got[k][name], np.concatenate([p[name] for p in parts]))
        assert np.array_equal(got[k]["log_posterior"].view(np.int64), np.concatenate([p["log_posterior"] for p in parts]).view(np.int64))


def test_wide_pair_and_the_workspace(wide_ctx, golden):
    sx, sy, want, _ = golden
    small = pc.CASES["3_30x29"][:3]
    cells = (len(sx) + 1) * (len(sy) + 1)
    opt = capi.PosteriorOptions(with_gaps=True)
    wide_ctx.set_posterior_workspace(24 * cells)  # the wide pair fits exactly: a group of its own
    got = run(wide_ctx, [small, (sx, sy, []), small], opt)
    assert wide_ctx.last_posterior().groups == 3
    for k in range(3):
        a, b = got[k]["first"][1], got[k]["first"][2]
        assert np.array_equal(got[k]["x"][a:b], want[k]["x"]) and np.array_equal(got[k]["log_posterior"][a:b].view(np.int64), want[k]["log_posterior"].view(np.int64))
    wide_ctx.set_posterior_workspace(24 * cells - 1)
    with pytest.raises(capi.MrpError) as e:
        run(wide_ctx, [(sx, sy, [])], opt, check_total=False)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED and f"limit {24 * cells - 1} bytes" in str(e.value)


def test_wide_pair_with_the_switch_off(gpu_ctx, golden):
    sx, sy, _, _ = golden
    before = gpu_ctx.posterior_wide_count()
    cells_before = gpu_ctx.last_posterior().cells
    for hook in (False, True):  # the hook picks kernels, it does not lift the refusal
        with hooked(gpu_ctx, hook):
            with pytest.raises(capi.MrpError) as e:
                run(gpu_ctx, [(sx, sy, [])], capi.PosteriorOptions(with_gaps=True), check_total=False)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and f"{min(len(sx), len(sy)) + 1} cells (limit 2048" in str(e.value)
    assert gpu_ctx.posterior_wide_count() == before and gpu_ctx.last_posterior().cells == cells_before  # nothing ran


# ---- 5. the dynamic band on the device ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("hook", [False, True])
def test_forty_random_pairs_with_per_anchor_expansions(gpu_ctx, hook):
    kw, pairs, exps, want, totals = forty(True)
    assert sum(len(set(e)) > 1 for e in exps) > 10  # bands no single expansion gives
    pool, xo, xl, yo, yl, ao, an = pc.pack(pairs)
    flat = np.array([v for e in exps for v in e], np.int64)
    with hooked(gpu_ctx, hook):
        got = capi.posterior_aligned_pairs(gpu_ctx, [pc.model()], pool, xo, xl, yo, yl, None, ao, an, pc.options(kw, 0.01, True), anchor_expansion=flat)
    check(got, want)
    assert np.array_equal(got[3].view(np.int64), totals.view(np.int64))
    for i, (sx, sy, _) in enumerate(pairs):
        for k, (xg, yg) in enumerate(((False, False), (True, False), (False, True))):
            a, b = got[k]["first"][i], got[k]["first"][i + 1]
            po.check_aligned_pairs(list(zip(got[k]["weight"][a:b], got[k]["x"][a:b], got[k]["y"][a:b])), len(sx), len(sy), xg, yg)
