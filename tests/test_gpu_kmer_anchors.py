"""mrp_kmer_alignment_anchors_many on the device against the host function (mrp_kmer_alignment_anchors, the transcription of
getKmerAlignmentAnchors, pairwiseAligner.c:1519-1627), pair by pair, counts and values equal -- one call holds every case.

The cases are chosen for the places the kernel can go wrong: fewer and more y positions than a wave has lanes, lengths around the
k-mer size, repeats inside x (many y k-mers map to the same first x, so the chain must skip records and the rule where the walk
back stops decides), a block of x transposed in y, Ns and other symbol bytes inside k-mers, and a chain whose walk back passes more
than 64 records, the number the kernel keeps in registers."""
import numpy as np
import pytest

from margin_amd import capi, synth

pytestmark = pytest.mark.gpu

K = 20


def cases():
    rng = np.random.default_rng(11)
    rs = lambda n: synth.random_sequence(rng, n)
    out = []
    a = rs(300)
    out.append(("evolved", a, synth.evolve_sequence(rng, a)))
    out.append(("lightly evolved", a, synth.evolve_sequence(rng, a, 0.01, 0.005, 0.005)))
    out.append(("identical", a, a.copy()))
    out.append(("unrelated", rs(200), rs(200)))
    base = rs(100)
    for n in (0, 19, 20, 21):
        out.append((f"lx {n}", base[:n], base))
        out.append((f"ly {n}", base, base[:n]))
    out.append(("both 20", base[:20], base[:20].copy()))
    short = rs(50)
    out.append(("31 y k-mers", short, np.concatenate([short[5:], rs(5)])))
    # repeats inside x: a tandem repeat (period 7, 70 symbols) and a homopolymer run of 40, flanked by unique sequence
    unit = rs(7)
    rep = np.concatenate([rs(60), np.tile(unit, 10), rs(50), np.full(40, 2, np.uint8), rs(60)])
    out.append(("repeats, same", rep, rep.copy()))
    out.append(("repeats, evolved", rep, synth.evolve_sequence(rng, rep, 0.01, 0.005, 0.005)))
    longer = np.concatenate([rep[:60], np.tile(unit, 14), rep[130:180], np.full(55, 2, np.uint8), rep[220:]])
    out.append(("repeats, longer in y", rep, longer))
    # a block of x transposed in y: the chain takes one of the two and skips the other's matches
    p, q, t, u = rs(80), rs(90), rs(70), rs(60)
    out.append(("transposed", np.concatenate([p, q, t, u]), np.concatenate([p, t, q, u])))
    # Ns and other bytes inside k-mers (byte equality, whatever the symbol)
    n1 = synth.random_sequence(rng, 260, n_rate=0.08)
    n2 = n1.copy()
    n2[100] = 7 if n2[100] != 7 else 9
    n2[180:183] = 4
    out.append(("Ns", n1, n2))
    # a walk back over more than 64 records: blocks of x in y as block 0, then blocks 79 .. 10 (descending x: a record chains to the
    # very first one and to little else, so the walk goes all the way), then block 5
    blocks = [rs(K) for _ in range(80)]
    out.append(("long walk back", np.concatenate(blocks), np.concatenate([blocks[0]] + blocks[79:9:-1] + [blocks[5]])))
    return out + [(name + ", swapped", y, x) for name, x, y in out]


def n_matches(x, y):
    first = {}
    for i in range(len(x) - K + 1):
        first.setdefault(x[i:i + K].tobytes(), i)
    return sum(y[j:j + K].tobytes() in first for j in range(len(y) - K + 1)) if len(x) >= K else 0


def longest_walk_back(x, y):
    """the most records the reference's walk back (:1583-1594) passes for one match of the pair"""
    first = {}
    for i in range(len(x) - K + 1):
        first.setdefault(x[i:i + K].tobytes(), i)
    recs, top, longest = [], 0, 0
    for j in range(len(y) - K + 1):
        xi = first.get(y[j:j + K].tobytes())
        if xi is None:
            continue
        score, steps = 1, 0
        for rx, rscore, rhigh in reversed(recs):
            steps += 1
            if rx < xi:
                score = max(score, rscore + 1)
                if rhigh:
                    break
        longest = max(longest, steps)
        recs.append((xi, score, score >= top))
        top = max(top, score)
    return longest


def layout(strings):
    pool, off, at = [], [], 0
    for s in strings:
        off.append(at)
        pool.append(np.ascontiguousarray(s, np.uint8))
        at += len(s)
    return (np.concatenate(pool) if at else np.zeros(0, np.uint8)), off


def test_every_case_in_one_call(gpu_ctx):
    cs = cases()
    pool, off = layout([s for _, x, y in cs for s in (x, y)])
    x_off, y_off = off[0::2], off[1::2]
    x_len, y_len = [len(c[1]) for c in cs], [len(c[2]) for c in cs]
    want = [capi.kmer_alignment_anchors(x, y) for _, x, y in cs]
    # what the case list exercises
    assert any(len(w) == 0 for w in want) and any(0 < len(w) < n_matches(x, y) for w, (_, x, y) in zip(want, cs))
    assert any(len(y) - K + 1 > 64 for _, _, y in cs) and any(0 < len(y) - K + 1 < 64 for _, _, y in cs)
    assert longest_walk_back(*[c[1:] for c in cs if c[0] == "long walk back"][0]) > 64
    aoff, anchors, st = capi.kmer_alignment_anchors_many(gpu_ctx, pool, x_off, x_len, y_off, y_len)
    assert aoff[0] == 0 and aoff[-1] == len(anchors) == sum(len(w) for w in want)
    for i, (c, w) in enumerate(zip(cs, want)):
        got = anchors[aoff[i]:aoff[i + 1]]
        assert len(got) == len(w), (c[0], len(got), len(w))
        assert np.array_equal(got, w), c[0]
    assert st.kernel_ms > 0 and st.total_ms > 0
    # the same list again gives the same bytes
    aoff2, anchors2, _ = capi.kmer_alignment_anchors_many(gpu_ctx, pool, x_off, x_len, y_off, y_len)
    assert aoff2.tobytes() == aoff.tobytes() and anchors2.tobytes() == anchors.tobytes()


def test_empty_lists(gpu_ctx):
    aoff, anchors, _ = capi.kmer_alignment_anchors_many(gpu_ctx, np.zeros(0, np.uint8), [], [], [], [])
    assert aoff.tolist() == [0] and anchors.shape == (0, 2)
    # pairs, but none long enough for a k-mer: no anchors, and nothing but the counts comes back
    pool = synth.random_sequence(np.random.default_rng(3), 40)
    aoff, anchors, _ = capi.kmer_alignment_anchors_many(gpu_ctx, pool, [0, 0], [19, 40], [20, 30], [20, 10])
    assert aoff.tolist() == [0, 0, 0] and anchors.shape == (0, 2)
