"""mrp_posterior_aligned_pairs on the device against the sequential restatement (tests/posterior_oracle.py): every list exactly --
first, x, y, weight, and the log posteriors as bit patterns -- and the totals exactly those of mrp_forward_probabilities."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests import posterior_cases as pc
from tests import posterior_oracle as po

pytestmark = pytest.mark.gpu


def run(ctx, pairs, opt, models=None, model_index=None):
    pool, xo, xl, yo, yl, ao, an = pc.pack(pairs)
    models = models or [pc.model()]
    got = capi.posterior_aligned_pairs(ctx, models, pool, xo, xl, yo, yl, model_index, ao, an, opt)
    fwd, _ = capi.forward_probabilities(ctx, models, pool, xo, xl, yo, yl, model_index, ao, an, expansion=opt.expansion,
                                        ragged_left=bool(opt.ragged_left), ragged_right=bool(opt.ragged_right))
    assert np.array_equal(got[3].view(np.int64), fwd.view(np.int64))  # the total at the last diagonal, bit for bit
    return got


def check(got, want_lists, with_gaps, non_empty=True):
    """want_lists: per pair (match, gap_x, gap_y) of the restatement"""
    for k in range(3 if with_gaps else 1):
        want = pc.as_arrays([w[k] for w in want_lists])
        if non_empty:
            assert len(want["x"]) > 0
        pc.assert_lists_equal(got[k], want)
    if not with_gaps:
        assert got[1] is None and got[2] is None


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("with_gaps", [False, True])
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_cases(gpu_ctx, name, with_gaps, threshold):
    sx, sy, anchors, kw = pc.CASES[name]
    want, info = pc.expected(name, threshold)
    got = run(gpu_ctx, [(sx, sy, anchors)], pc.options(kw, threshold, with_gaps))
    check(got, [want], with_gaps)
    st = gpu_ctx.last_posterior()
    assert st.groups == 1 and st.cells == got[4].cells and got[4].pairs_wave == 1
    assert st.downloaded_bytes == 16 * st.candidates + 12 * len(info) + 8


def test_edges(gpu_ctx):
    m = pc.model()
    e = np.zeros(0, np.uint8)
    pairs = [(e, e, []),                                             # two empty strings
             (e, np.array([0, 1, 2, 3, 0], np.uint8), []),           # lx = 0: no match pairs, gap-y only
             (np.array([2], np.uint8), np.array([2], np.uint8), []),  # one symbol each
             (np.array([1], np.uint8), e, []),                       # one symbol in all
             (np.array([0, 4, 2, 7, 3, 1], np.uint8), np.array([0, 4, 2, 9, 1], np.uint8), [])]  # symbols >= 4 are N
    opt = capi.PosteriorOptions(threshold=0.01, expansion=4, min_diags_between_traceback=4, traceback_diagonals=1, with_gaps=True)
    want = [po.posterior(m, sx, sy, a, expansion=4, threshold=0.01, min_diags=4, traceback_diagonals=1, with_gaps=True)[0] for sx, sy, a in pairs]
    got = run(gpu_ctx, pairs, opt)
    check(got, want, True)
    assert got[3][0] == 0.0
    for k in range(3):
        assert got[k]["first"][1] == 0  # the empty pair's lists
    assert got[0]["first"][2] == got[0]["first"][1] and got[1]["first"][2] == got[1]["first"][1] and got[2]["first"][2] - got[2]["first"][1] == 5
    assert got[0]["first"][3] - got[0]["first"][2] == 1  # the one-symbol pair aligns its symbols
    # the empty pair alone, and no pair at all
    got = run(gpu_ctx, pairs[:1], opt)
    assert got[3].tolist() == [0.0] and all(got[k]["first"].tolist() == [0, 0] for k in range(3))
    got = capi.posterior_aligned_pairs(gpu_ctx, [m], e, [], [], [], [], options=opt)
    assert all(got[k]["first"].tolist() == [0] for k in range(3))


def test_two_models(gpu_ctx):
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    models = [pc.model(), f.reverse_complement()]
    sx, sy, _, _ = pc.CASES["3_30x29"]
    opt = capi.PosteriorOptions(threshold=0.05, expansion=20, min_diags_between_traceback=14, traceback_diagonals=3)
    want = [po.posterior(models[i], sx, sy, [], expansion=20, threshold=0.05, min_diags=14, traceback_diagonals=3)[0] for i in (1, 0, 1)]
    assert want[0][0] != want[1][0]
    got = run(gpu_ctx, [(sx, sy, [])] * 3, opt, models=models, model_index=np.array([1, 0, 1], np.uint8))
    check(got, want, False)


def test_forty_random_pairs(gpu_ctx):
    """drawn as tests/pairwiseAlignerTest.c:423-438 draws them (one draw of the parameters for the call, no dynamic band)"""
    rng = np.random.default_rng(423)
    tb = int(rng.integers(1, 11))
    kw = dict(traceback_diagonals=tb, min_diags=tb + int(rng.integers(2, 11)), expansion=2 * int(rng.integers(0, 11)))
    pairs = []
    for _ in range(40):
        sx = synth.random_sequence(rng, int(rng.integers(0, 101)))
        sy = synth.evolve_sequence(rng, sx)
        pairs.append((sx, sy, pc.random_anchors(rng, len(sx), len(sy))))
    m = pc.model()
    want = [po.posterior(m, sx, sy, a, threshold=0.01, with_gaps=True, **kw)[0] for sx, sy, a in pairs]
    got = run(gpu_ctx, pairs, pc.options(kw, 0.01, True))
    check(got, want, True)
    for i, (sx, sy, _) in enumerate(pairs):
        for k, (xg, yg) in enumerate(((False, False), (True, False), (False, True))):
            a, b = got[k]["first"][i], got[k]["first"][i + 1]
            po.check_aligned_pairs(list(zip(got[k]["weight"][a:b], got[k]["x"][a:b], got[k]["y"][a:b])), len(sx), len(sy), xg, yg)


def test_groups_and_workspace(gpu_ctx):
    """the same three pairs as three groups: identical to the one-group call; a pair just over the budget is refused"""
    names = ["3_30x29", "4_70x65", "1_12x9"]
    pairs = [pc.CASES[n][:3] for n in names]
    opt = capi.PosteriorOptions(threshold=0.01, expansion=20, min_diags_between_traceback=14, traceback_diagonals=3, with_gaps=True)
    cells = [capi.pair_diagonal_width(a, len(sx), len(sy), 20)[1] for sx, sy, a in pairs]
    try:
        one = run(gpu_ctx, pairs, opt)
        assert gpu_ctx.last_posterior().groups == 1
        assert cells[1] == 71 * 66 and cells[0] < cells[1] and cells[2] < cells[1]
        gpu_ctx.set_posterior_workspace(24 * cells[1])  # the largest pair, in the middle, fits exactly: no two neighbours do
        three = run(gpu_ctx, pairs, opt)
        assert gpu_ctx.last_posterior().groups == 3
        for k in range(3):
            assert len(one[k]["x"]) > 0
            pc.assert_lists_equal(three[k], one[k])
        assert np.array_equal(one[3].view(np.int64), three[3].view(np.int64))
        gpu_ctx.set_posterior_workspace(24 * cells[1] - 1)
        with pytest.raises(capi.MrpError) as e:
            run(gpu_ctx, pairs, opt)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and f"limit {24 * cells[1] - 1} bytes" in str(e.value)
    finally:
        gpu_ctx.set_posterior_workspace(0)


def test_wide_diagonal_is_refused(gpu_ctx):
    z = np.zeros(2048, np.uint8)
    pool, xo, xl, yo, yl, ao, an = pc.pack([(z, z, [])])
    for wide in (False, True):  # wide pairs are not extended to this entry
        gpu_ctx.set_wide_pairs(wide)
        try:
            with pytest.raises(capi.MrpError) as e:
                capi.posterior_aligned_pairs(gpu_ctx, [pc.model()], pool, xo, xl, yo, yl, None, ao, an, capi.PosteriorOptions())
        finally:
            gpu_ctx.set_wide_pairs(False)
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "2049 cells" in str(e.value)
    assert gpu_ctx.last_posterior().cells != 2049 * 2049  # nothing ran


@pytest.mark.parametrize("name", ["w256", "w1024", "w2048"])
def test_wide_launch_classes(gpu_ctx, name):
    """diagonals of up to 256, 1 024 and 2 048 cells: the three larger launch classes of both kernels.  The restatement needs up to a
    minute for these, so its lists are a fixture (tests/make_posterior_golden.py wrote it); the reference's defaults, with gaps"""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "posterior", "wide_classes.npz"))
    sx, sy = g[name + "_x"], g[name + "_y"]
    width = min(len(sx), len(sy)) + 1
    assert {"w256": 64 < width <= 256, "w1024": 256 < width <= 1024, "w2048": 1024 < width <= 2048}[name]
    got = run(gpu_ctx, [(sx, sy, [])], capi.PosteriorOptions(with_gaps=True))
    for k, tag in enumerate(("match", "gapx", "gapy")):
        want = {f: g[f"{name}_{tag}_{f}"] for f in ("x", "y", "weight", "log_posterior")}
        want["first"] = np.array([0, len(want["x"])], np.int64)
        assert len(want["x"]) > 0
        pc.assert_lists_equal(got[k], want)
