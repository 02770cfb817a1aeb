"""The run-length instantiation of the pair-per-lane kernel (mrp_context_set_rle_lane_pairs) and mrp_allele_read_supports_rle on the
device: the switch on against the switch off (the pair-per-wave kernel), against the sequential restatement
(tests/rle_pairhmm_oracle.py), and the loop against its restatement (tests/rle_lane_cases.py) -- always as bit patterns.  The counts of
lane pairs the tests assert are what keeps them from passing with everything on the pair-per-wave kernel."""
import contextlib
import functools
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import posterior_cases as pc
from tests import rle_cases as rc
from tests import rle_lane_cases as lc

pytestmark = pytest.mark.gpu

R = rc.R_SHIPPED
EXPANSION = 20


@contextlib.contextmanager
def lane_pairs(ctx, on=True):
    ctx.set_rle_lane_pairs(on)
    try:
        yield
    finally:
        ctx.set_rle_lane_pairs(False)


@functools.lru_cache(maxsize=None)
def shipped_models():
    """the shipped margin phase hmm: gap_switch_to_x / _y = log(0), so the kernels' HAS_SWITCH = false instantiations run; the reverse
    strand's model differs"""
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    fwd = capi.PairHmm.from_margin_hmm(t, tr, em)
    assert fwd.gap_switch_to_x == -np.inf and fwd.gap_switch_to_y == -np.inf
    rev = fwd.reverse_complement()
    assert bytes(rev) != bytes(fwd)
    return [fwd, rev]


@functools.lru_cache(maxsize=None)
def switch_models():
    """finite gap_switch_to_x / _y (stateMachine3_constructNucleotide's): the HAS_SWITCH = true instantiations; two models that differ"""
    a = pc.model()
    b = a.copy()
    b.gap_switch_to_x, b.gap_switch_to_y, b.match_from_gap_x = -3.5, -4.25, -1.5
    b.e_match[1], b.e_match[6], b.e_gap_x[2], b.e_gap_y[0] = -4.0, -3.9, -1.5, -1.25
    assert np.isfinite([a.gap_switch_to_x, a.gap_switch_to_y]).all() and bytes(a) != bytes(b)
    return [a, b]


@functools.lru_cache(maxsize=None)
def tables():
    rng = np.random.default_rng(17)
    return [(rc.random_table(rng, R), 1), (rc.random_table(rng, R), 0)]


def repeat_models():
    return [capi.RepeatModel(t, s) for t, s in tables()]


@functools.lru_cache(maxsize=None)
def edges():
    caps, bound = capi.rle_lane_caps(2)
    pairs = lc.edge_pairs(caps, bound, R)
    return caps, bound, pairs


def forward(ctx, models, pairs, on):
    pool, counts, xo, xl, yo, yl, mi = lc.pack_edge_pairs(pairs)
    with lane_pairs(ctx, on):
        return capi.forward_probabilities_rle(ctx, models, repeat_models(), pool, counts, xo, xl, yo, yl, mi, expansion=EXPANSION)


def want(models, pair):
    sx, cx, sy, cy, m, _ = pair
    table, strand = tables()[m]
    return lc.oracle_forward(models[m], table, strand, sx, cx, sy, cy, EXPANSION)


def find(pairs, pred):
    return next(i for i, p in enumerate(pairs) if pred(p))


# ---- 1. switch on equals switch off -------------------------------------------------------------------------------------------------

def test_the_list_holds_every_edge():
    caps, bound, pairs = edges()
    assert caps[3] <= 100 and len(pairs) < 300 and max(max(len(p[0]), len(p[2])) for p in pairs) <= 101
    shapes = {(len(p[0]), len(p[2])) for p in pairs}
    assert all((lx, ly) in shapes for lx in (0, 1, 2, 3) for ly in (0, 1, 2, 3))
    lxs = {s[0] for s in shapes}
    assert all(caps[c] in lxs and caps[c] + 1 in lxs for c in range(4))
    assert any(len(p[0]) and (p[0] == 4).all() and (p[2] == 4).all() for p in pairs) and any((p[0] > 4).any() and (p[2] > 4).any() for p in pairs)
    assert any(p[5] and len(p[1]) and len(p[3]) and p[1].min() == 0 and p[1].max() == bound - 1 and p[3].min() == 0 and p[3].max() == bound - 1 for p in pairs)
    assert sum(1 for p in pairs if not p[5] and len(p[0]) <= caps[3] and max(p[1].max(), p[3].max()) == bound) == 1
    assert sum(1 for p in pairs if not p[5] and len(p[0]) <= caps[3] and max(p[1].max(), p[3].max()) == R - 1) == 1
    assert {p[4] for p in pairs if p[5]} == {0, 1} and {(2, 30), (30, 2)} <= shapes
    per_class = np.bincount([lc.lane_class(len(p[0]), caps) for p in pairs if p[5]], minlength=4)
    assert (per_class > 0).all() and any(n > 64 and n % 64 != 0 for n in per_class)  # a second wave that is partly empty
    assert sum(1 for p in pairs if len(p[0]) == caps[3] + 1) == 1 and not pairs[find(pairs, lambda p: len(p[0]) == caps[3] + 1)][5]


def test_switch_on_equals_switch_off(gpu_ctx):
    _, _, pairs = edges()
    off, st_off = forward(gpu_ctx, shipped_models(), pairs, False)
    on, st_on = forward(gpu_ctx, shipped_models(), pairs, True)
    eligible = sum(1 for p in pairs if p[5])
    assert st_off.pairs_lane == 0 and st_off.pairs_wave == len(pairs)
    assert 0 < eligible < len(pairs) and st_on.pairs_lane == eligible and st_on.pairs_wave == len(pairs) - eligible
    assert np.array_equal(on.view(np.int64), off.view(np.int64))
    assert np.isfinite(on).all() and on[find(pairs, lambda p: len(p[0]) == 0 and len(p[2]) == 0)] == 0.0
    again, st = forward(gpu_ctx, shipped_models(), pairs, False)  # the switch went off again: the parent's path
    assert st.pairs_lane == 0 and np.array_equal(again.view(np.int64), off.view(np.int64))


# ---- 2. against the restatement ------------------------------------------------------------------------------------------------------

def twelve(caps, bound, pairs):
    shape = lambda lx, ly: (lambda p: len(p[0]) == lx and len(p[2]) == ly)
    picks = [find(pairs, shape(0, 3)), find(pairs, shape(3, 0)), find(pairs, shape(1, 1)), find(pairs, shape(2, 3)),
             find(pairs, lambda p: len(p[0]) and (p[0] == 4).all()), find(pairs, lambda p: (p[0] > 4).any()), find(pairs, shape(2, 30)),
             find(pairs, shape(30, 2)), find(pairs, lambda p: len(p[0]) == caps[0]), find(pairs, lambda p: len(p[0]) == caps[0] + 1),
             find(pairs, lambda p: len(p[0]) == caps[3]), find(pairs, lambda p: len(p[0]) == caps[1] + 3 and p[4] == 1)]
    assert len(set(picks)) == 12 and all(pairs[i][5] for i in picks)
    assert any(len(pairs[i][1]) and pairs[i][1].min() == 0 and pairs[i][1].max() == bound - 1 for i in picks)
    return picks


def test_lane_pairs_equal_the_restatement(gpu_ctx):
    caps, bound, pairs = edges()
    picks = twelve(caps, bound, pairs)
    some = [pairs[i] for i in picks]
    got, st = forward(gpu_ctx, shipped_models(), some, True)
    assert st.pairs_lane == 12 and st.pairs_wave == 0
    for k, p in enumerate(some):
        assert float(got[k]).hex() == float(want(shipped_models(), p)).hex(), (k, len(p[0]), len(p[2]))


# ---- 3. models with a gap switch -----------------------------------------------------------------------------------------------------

def test_models_with_a_gap_switch(gpu_ctx):
    caps, bound, pairs = edges()
    off, st_off = forward(gpu_ctx, switch_models(), pairs, False)
    on, st_on = forward(gpu_ctx, switch_models(), pairs, True)
    assert st_off.pairs_lane == 0 and st_on.pairs_lane == sum(1 for p in pairs if p[5]) > 0
    assert np.array_equal(on.view(np.int64), off.view(np.int64))
    plain, _ = forward(gpu_ctx, shipped_models(), pairs, True)
    assert not np.array_equal(on, plain)  # other models, another instantiation
    for i in (find(pairs, lambda p: len(p[0]) == 3 and len(p[2]) == 8), find(pairs, lambda p: len(p[0]) == caps[1] + 3 and p[4] == 1),
              find(pairs, lambda p: len(p[0]) == caps[0] and p[5])):
        assert float(on[i]).hex() == float(want(switch_models(), pairs[i])).hex(), i


# ---- 4. all-zero tables: the new instantiation against the nucleotide lane kernel -----------------------------------------------------

def random_bubbles(rng, shapes, bound, max_len=24):
    """[(n_alleles, n_reads)] -> bubbles as allele_read_supports_rle takes them, counts below the bound; six symbols or more, so that no
    two reads of a bubble are equal"""
    out = []
    for na, nr in shapes:
        lens = rng.integers(6, max_len + 1, size=na + nr)
        strings = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lens]
        counts = [rng.integers(0, bound, size=n).astype(np.uint8) for n in lens]
        out.append((strings[:na], counts[:na], strings[na:], counts[na:], [int(v) for v in rng.integers(0, 2, size=nr)]))
    return out


def test_zero_tables_equal_the_nucleotide_supports(gpu_ctx):
    _, bound = capi.rle_lane_caps(2)
    bubbles = random_bubbles(np.random.default_rng(41), [(3, 40), (2, 30), (1, 1), (4, 25)], bound)
    zero = [capi.RepeatModel(np.zeros((4, R, R)), 1), capi.RepeatModel(np.zeros((4, R, R)), 0)]
    fwd, rev = shipped_models()
    plain, pst = capi.allele_read_supports(gpu_ctx, fwd, rev, [(a, r, s) for a, _, r, _, s in bubbles], expansion=EXPANSION, sv_threshold=10 ** 6)
    got, st = capi.allele_read_supports_rle(gpu_ctx, fwd, rev, zero[0], zero[1], bubbles, expansion=EXPANSION)
    # no two reads of a bubble have equal symbols, so both calls score every pair, a pair a lane
    assert all(len({r.tobytes() for r in b[2]}) == len(b[2]) for b in bubbles)
    assert pst.pairs_lane == st.pairs_lane == sum(len(b[0]) * len(b[2]) for b in bubbles) and st.pairs_wave == 0
    for g, p in zip(got, plain):
        assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), p.view(np.int32))


# ---- 5. the loop ---------------------------------------------------------------------------------------------------------------------

def u8(*v):
    return np.array(v, np.uint8)


def loop_bubbles():
    a = [u8(0, 1, 2, 3, 0, 2, 1), u8(0, 1, 3, 0, 2, 1), u8(0, 1, 2, 3, 3, 0, 2, 1, 4)]
    ac = [u8(1, 2, 1, 3, 1, 1, 2), u8(1, 2, 4, 1, 1, 2), u8(1, 2, 1, 1, 2, 1, 1, 2, 0)]
    r = [u8(0, 1, 2, 3, 0, 2, 1), u8(0, 1, 2, 0, 2, 1), u8(0, 1, 2, 3, 0, 2, 1), u8(0, 1, 2, 0, 2, 1), u8(), u8(0, 1, 2, 3, 0, 2, 1)]
    rcnt = [u8(1, 2, 1, 3, 1, 1, 2), u8(1, 2, 5, 1, 1, 2), u8(1, 2, 1, 3, 1, 1, 2), u8(1, 2, 6, 1, 1, 2), u8(), u8(1, 2, 1, 3, 1, 1, 15)]
    # reads 0 and 2: equal symbols and counts on different strands (2 copies 0, whose strand decides); 1 and 3: equal symbols, different
    # counts (both computed); 4: empty; 5: a third set of counts on the strand of read 2
    first = (a, ac, r, rcnt, [1, 0, 0, 0, 1, 0])
    second = ([u8(2, 2, 1)], [u8(3, 0, 1)], [u8(2, 1)], [u8(3, 1)], [0])
    third = ([u8(1, 2), u8(3)], [u8(1, 1), u8(2)], [], [], [])
    return [first, second, third]


def test_the_loop(gpu_ctx):
    bubbles = loop_bubbles()
    fwd, rev = shipped_models()
    want_sup, owners = lc.want_supports(fwd, rev, tables()[0], tables()[1], bubbles, EXPANSION)
    assert owners == 3 * 5 + 1
    got, st = capi.allele_read_supports_rle(gpu_ctx, fwd, rev, *repeat_models(), bubbles, expansion=EXPANSION)
    assert st.pairs_lane + st.pairs_wave == owners and st.pairs_lane == owners
    assert [g.shape for g in got] == [(3, 6), (1, 1), (2, 0)]
    for g, w in zip(got, want_sup):
        assert np.array_equal(g.view(np.int32), w.view(np.int32))
    first = got[0]
    assert np.array_equal(first[:, 2], first[:, 0]) and not np.array_equal(first[:, 1], first[:, 3]) and not np.array_equal(first[:, 5], first[:, 0])
    # the earlier read's strand decided: read 2 on its own strand would have scored otherwise
    alone = [(bubbles[0][0], bubbles[0][1], [bubbles[0][2][2]], [bubbles[0][3][2]], [0])]
    other, _ = capi.allele_read_supports_rle(gpu_ctx, fwd, rev, *repeat_models(), alone, expansion=EXPANSION)
    assert not np.array_equal(other[0][:, 0], first[:, 2])


# ---- 6. a mixed call -----------------------------------------------------------------------------------------------------------------

def test_a_mixed_call(gpu_ctx):
    caps, bound = capi.rle_lane_caps(2)
    rng = np.random.default_rng(61)
    (b,) = random_bubbles(rng, [(3, 4)], bound, max_len=12)
    n = caps[3] + 5
    b[0][1], b[1][1] = rng.integers(0, 4, size=n).astype(np.uint8), rng.integers(0, bound, size=n).astype(np.uint8)  # the pair-per-wave kernel's
    fwd, rev = shipped_models()
    want_sup, owners = lc.want_supports(fwd, rev, tables()[0], tables()[1], [b], EXPANSION)
    got, st = capi.allele_read_supports_rle(gpu_ctx, fwd, rev, *repeat_models(), [b], expansion=EXPANSION)
    assert st.pairs_lane == 8 and st.pairs_wave == 4 and owners == 12
    assert np.array_equal(got[0].view(np.int32), want_sup[0].view(np.int32))


# ---- 7. the shipped matrix ------------------------------------------------------------------------------------------------------------

def test_shipped_matrix_and_geometric_counts(gpu_ctx):
    rng = np.random.default_rng(71)
    caps, bound = capi.rle_lane_caps(2)
    table = rc.shipped_matrix()
    pairs = []
    for k in range(2000):
        lx, ly = (int(v) for v in rng.integers(15, 26, size=2))
        sx, sy = synth.random_sequence(rng, lx), synth.random_sequence(rng, ly)
        pairs.append((sx, rc.geometric_counts(rng, lx, R), sy, rc.geometric_counts(rng, ly, R), k % 2, True))
    eligible = sum(1 for p in pairs if max(p[1].max(), p[3].max()) < bound)
    pool, counts, xo, xl, yo, yl, mi = lc.pack_edge_pairs(pairs)
    repeat = [capi.RepeatModel(table, 1), capi.RepeatModel(table, 0)]
    off, st_off = capi.forward_probabilities_rle(gpu_ctx, shipped_models(), repeat, pool, counts, xo, xl, yo, yl, mi, expansion=EXPANSION)
    with lane_pairs(gpu_ctx):
        on, st_on = capi.forward_probabilities_rle(gpu_ctx, shipped_models(), repeat, pool, counts, xo, xl, yo, yl, mi, expansion=EXPANSION)
    assert st_off.pairs_lane == 0 and st_on.pairs_lane == eligible and st_on.pairs_lane >= 0.95 * len(pairs)
    assert np.array_equal(on.view(np.int64), off.view(np.int64))


# ---- the C example --------------------------------------------------------------------------------------------------------------------

def test_c_example_equals_the_python_call(gpu_ctx, tmp_path):
    r = subprocess.run([lc.build_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    n = len(lc.example_compressed_lines())
    assert lines[:n] == lc.example_compressed_lines()
    m = capi.PairHmm.default_nucleotide()
    (sup,), st = capi.allele_read_supports_rle(gpu_ctx, m, m, capi.RepeatModel(lc.example_table(), 1), capi.RepeatModel(lc.example_table(), 0),
                                               [lc.example_bubble()], expansion=lc.EXAMPLE_EXPANSION)
    got = {(int(ln.split()[1]), int(ln.split()[2])): np.float32(float.fromhex(ln.split()[3])) for ln in lines if ln.startswith("support ")}
    assert len(got) == sup.size == 8
    for (j, k), v in got.items():
        assert v.view(np.int32) == sup[j, k].view(np.int32), (j, k)
    assert np.array_equal(sup[:, 2], sup[:, 0]) and lines[-1].startswith(f"{st.pairs_lane} pairs a lane, 0 pairs a wave")
