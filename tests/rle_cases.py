"""What the run-length tests share (tests/test_rle_host.py, tests/test_gpu_rle_pairhmm.py, tests/make_rle_posterior_golden.py): tables,
counts, the packing of pairs with counts, and the calls with their standing checks."""
from __future__ import annotations

import functools
import os

import numpy as np

from margin_amd import capi, synth
from tests import posterior_cases as pc
from tests import rle_pairhmm_oracle as ro

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
R_SHIPPED = 51  # MAXIMUM_REPEAT_LENGTH


def random_table(rng, R):
    """log probabilities [4, R, R], different for every base, underlying and observed count"""
    return -rng.uniform(0.01, 1.0, size=(4, R, R))


def random_counts(rng, n, R):
    """n counts in 0 .. R - 1 with both ends present (from two symbols on)"""
    c = rng.integers(0, R, size=n).astype(np.uint8)
    if n >= 2:
        i, j = rng.choice(n, size=2, replace=False)
        c[i], c[j] = 0, R - 1
    return c


def geometric_counts(rng, n, R, p=0.5):
    """run lengths as a run-length encoded read has them: 1 + geometric, clamped as symbol_addRepeatCount clamps"""
    return np.minimum(rng.geometric(p, size=n), R - 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shipped_matrix():
    """the four repeatCountLogProbabilities_*_F arrays of the shipped r9.4 g507 polish parameters, [4, 51, 51]"""
    return np.load(os.path.join(GOLDEN, "repeat_matrix_r94_g507.npz"))["log_prob_F"]


def pack(pairs):
    """[(sx, cx, sy, cy, anchors)] -> pool, counts, x_off, x_len, y_off, y_len, anchor_off, anchors"""
    pool, xo, xl, yo, yl, ao, an = pc.pack([(sx, sy, a) for sx, _, sy, _, a in pairs])
    counts = [np.asarray(c, np.uint8) for _, cx, _, cy, _ in pairs for c in (cx, cy)]
    return pool, (np.concatenate(counts) if counts else np.zeros(0, np.uint8)), xo, xl, yo, yl, ao, an


def want_posterior(model, table, strand, pair, kw, threshold, expansions=None):
    """the restatement for one pair -> ((match, gap_x, gap_y), info)"""
    sx, cx, sy, cy, anchors = pair
    R = table.shape[1]
    rsm = ro.RepeatSubMatrix(table, strand)
    a, b = ro.symbols(sx, cx, R), ro.symbols(sy, cy, R)
    if expansions is not None:
        return ro.posterior_dynamic(model, rsm, a, b, anchors, expansions, threshold=threshold, with_gaps=True, **kw)
    return ro.posterior(model, rsm, a, b, anchors, threshold=threshold, with_gaps=True, **kw)


def run(ctx, models, repeat, pairs, opt, model_index=None, anchor_expansion=None, check_total=True):
    """mrp_posterior_aligned_pairs_rle; the totals equal mrp_forward_probabilities_rle on the same pairs (the constant band only: the
    forward entry has no dynamic band)"""
    pool, counts, xo, xl, yo, yl, ao, an = pack(pairs)
    got = capi.posterior_aligned_pairs_rle(ctx, models, repeat, pool, counts, xo, xl, yo, yl, model_index, ao, an, opt, anchor_expansion=anchor_expansion)
    if check_total and anchor_expansion is None:
        fwd, st = capi.forward_probabilities_rle(ctx, models, repeat, pool, counts, xo, xl, yo, yl, model_index, ao, an, expansion=opt.expansion,
                                                 ragged_left=bool(opt.ragged_left), ragged_right=bool(opt.ragged_right))
        assert st.pairs_lane == 0  # no run-length pair takes the pair-per-lane kernel
        assert np.array_equal(got[3].view(np.int64), fwd.view(np.int64))
    return got


def check(got, want_lists, with_gaps=True, non_empty=True):
    for k in range(3 if with_gaps else 1):
        want = pc.as_arrays([w[k] for w in want_lists])
        if non_empty:
            assert len(want["x"]) > 0
        pc.assert_lists_equal(got[k], want)


def total_of(info, n):
    """the total the reference takes at diagonal n = lx + ly, the first of the last traceback"""
    return dict(info[-1][4])[n] if info else 0.0


def rle_pair(seed, lx, R, ly=None, p=0.05):
    """x random with run lengths 1 + geometric (clamped); y = x with about 5 % substitutions, insertions and deletions each, a kept
    symbol's count kept at 80 % and one more or less otherwise, counts 0 and R - 1 planted in both; ly given: y cut or padded to it"""
    rng = np.random.default_rng(seed)
    sx = synth.random_sequence(rng, lx)
    cx = geometric_counts(rng, lx, R)
    sy, cy = [], []
    for b, c in zip(sx.tolist(), cx.tolist()):
        u = rng.random()
        if u < p:
            continue
        if u < 2 * p:
            sy.append(int(rng.integers(0, 4))); cy.append(int(geometric_counts(rng, 1, R)[0]))
        sy.append(int(rng.integers(0, 4)) if u >= 1 - p else b)
        cy.append(c if rng.random() < 0.8 else min(R - 1, max(0, c + int(rng.choice((-1, 1))))))
    if ly is not None:
        sy, cy = sy[:ly], cy[:ly]
        while len(sy) < ly:
            sy.append(int(rng.integers(0, 4))); cy.append(int(geometric_counts(rng, 1, R)[0]))
    cy = np.array(cy, np.uint8)
    for c in (cx, cy):
        if len(c) >= 2:
            i, j = rng.choice(len(c), size=2, replace=False)
            c[i], c[j] = 0, R - 1
    return sx, cx, np.array(sy, np.uint8), cy
