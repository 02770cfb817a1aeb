"""CPU checks of tests/haptag_oracle.py (the restatement of bubbleGraph.c:1749-2351 the GPU tests compare against) on small
hand-built cases that pin its quirks, and the loud failure of the two C-ABI entries without a device."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import haptag_oracle as ho


def models():
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    return ph.Model.from_buffer_copy(bytes(f)), ph.Model.from_buffer_copy(bytes(f.reverse_complement()))


def sym(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


REF, ALT = sym("GATTACAGGCTACGATCGATCGGTA"), sym("GATTACAGGCTAGGATCGATCGGTA")
READ = sym("GATTACAGCTACGGATCGTCGGTA")  # a noisy copy, neither allele exactly


def test_log_add_exact():
    assert ho.log_add_exact(-np.inf, -2.0) == -2.0 and ho.log_add_exact(-2.0, -np.inf) == -2.0
    assert ho.log_add_exact(-1.0, -3.0) == ho.log_add_exact(-3.0, -1.0)
    assert abs(ho.log_add_exact(np.log(0.25), np.log(0.5)) - np.log(0.75)) < 1e-15


def test_duplicate_substring_on_opposite_strands():
    """Partition (b->reads popped, bubbleGraph.c:1818) scores a duplicated substring with the LAST-listed read's strand;
    phasing (:2238) with the FIRST tagged read's.  The two strands give different supports, so the case discriminates."""
    fwd, rev = models()
    f_sup = [ph.forward_probability(fwd, a, READ) for a in (REF, ALT)]
    r_sup = [ph.forward_probability(rev, a, READ) for a in (REF, ALT)]
    assert f_sup != r_sup
    strand = [True, False]  # read 0 forward, read 1 reverse; both carry the same substring
    site = ([REF, ALT], (0, 1), [(0, READ), (1, READ.copy())])
    _, h1, h2 = ho.partition_filtered_reads(fwd, rev, [site], 2, strand)
    s1, s2 = (float(np.float32(v)) for v in r_sup)  # the last-listed read (1, reverse strand) owns the scores
    assert h1[0] == h1[1] == s1 - ho.log_add_exact(s1, s2)
    assert h2[0] == h2[1] == s2 - ho.log_add_exact(s2, s1)
    f1, f2 = (float(np.float32(v)) for v in f_sup)
    assert h1[0] != f1 - ho.log_add_exact(f1, f2)
    # phasing: read 0 untagged, so the first TAGGED entry (read 1, reverse) owns; with read 0 tagged, read 0 (forward) owns
    _, c_rev, _ = ho.phase_filtered_variants(fwd, rev, [site], 2, strand, [0, 1])
    _, c_fwd, _ = ho.phase_filtered_variants(fwd, rev, [site], 2, strand, [1, 1])
    a, b = r_sup
    assert c_rev[0] == a - ho.log_add_exact(a, b)
    a, b = f_sup
    assert c_fwd[0] == 2 * (a - ho.log_add_exact(a, b))


def test_supports_are_rounded_to_float_in_partition_only():
    fwd, rev = models()
    site = ([REF, ALT], (0, 1), [(0, READ)])
    _, h1, _ = ho.partition_filtered_reads(fwd, rev, [site], 1, [True])
    _, cis, _ = ho.phase_filtered_variants(fwd, rev, [site], 1, [True], [1])
    a, b = (ph.forward_probability(fwd, x, READ) for x in (REF, ALT))
    assert cis[0] == a - ho.log_add_exact(a, b)
    fa, fb = float(np.float32(a)), float(np.float32(b))
    assert h1[0] == fa - ho.log_add_exact(fa, fb) and h1[0] != cis[0]


def test_homozygous_sites_are_skipped():
    fwd, rev = models()
    hom = ([REF, ALT], (1, 1), [(0, READ)])
    hap, h1, h2 = ho.partition_filtered_reads(fwd, rev, [hom], 2, [True, True])
    assert (hap == 0).all() and (h1 == 0).all() and (h2 == 0).all()
    state, cis, trans = ho.phase_filtered_variants(fwd, rev, [hom], 2, [True, True], [1, 2])
    assert state[0] == ho.NOT_VISITED and cis[0] == trans[0] == 0
    # two different indices whose strings are equal are NOT skipped (the reference compares allele pointers)
    same = ([REF, REF.copy()], (0, 1), [(0, READ)])
    hap, h1, h2 = ho.partition_filtered_reads(fwd, rev, [same], 1, [True])
    assert hap[0] == 0 and h1[0] == h2[0] != 0


def test_variant_states():
    fwd, rev = models()
    ref_read, alt_read = REF.copy(), ALT.copy()
    variants = [([REF, ALT], (0, 1), [(0, ref_read)]),            # read 0 is hap 1 and carries gt1: cis
                ([REF, ALT], (0, 1), [(1, ref_read)]),            # read 1 is hap 2 and carries gt1: trans
                ([REF, ALT], (0, 1), [(2, alt_read)]),            # untagged only: tie
                ([REF, ALT], (0, 1), []),                         # no entries: not visited
                ([REF, ALT, sym("GATTACA")], (2, 1), [(0, READ), (1, READ)])]  # equal supports on both haplotypes: exact tie
    state, cis, trans = ho.phase_filtered_variants(fwd, rev, variants, 3, [True, True, True], [1, 2, 0])
    assert state.tolist() == [ho.CIS, ho.TRANS, ho.TIE, ho.NOT_VISITED, ho.TIE]
    assert cis[2] == trans[2] == 0 and cis[3] == trans[3] == 0
    assert cis[4] == trans[4] != 0


def test_partition_never_anchors_phasing_anchors_past_sv_threshold():
    rng = np.random.default_rng(3)
    fwd, rev = models()
    flank = synth.random_sequence(rng, 300)
    alt = np.concatenate([flank[:150], synth.random_sequence(rng, 120), flank[150:]])
    read = synth.evolve_sequence(rng, alt, 0.03, 0.01, 0.01)
    site = ([flank, alt], (0, 1), [(0, read)])
    assert len(ph.kmer_anchors(alt, read)) > 0
    _, cis, trans = ho.phase_filtered_variants(fwd, rev, [site], 1, [True], [1], sv_threshold=200)
    full = [ph.forward_probability(fwd, a, read) for a in (flank, alt)]
    banded = [ph.forward_probability(fwd, a, read, ph.kmer_anchors(a, read)) for a in (flank, alt)]
    assert full != banded
    a, b = banded
    assert cis[0] == a - ho.log_add_exact(a, b) and trans[0] == b - ho.log_add_exact(a, b)
    _, h1, _ = ho.partition_filtered_reads(fwd, rev, [site], 1, [True])
    fa, fb = (float(np.float32(v)) for v in full)
    assert h1[0] == fa - ho.log_add_exact(fa, fb)


def test_assert_margins_decisive():
    ho.assert_margins_decisive([0.0, -5.0], [0.0, -4.0])
    with pytest.raises(AssertionError):
        ho.assert_margins_decisive([-5.0], [-5.0 + 1e-9])


@pytest.mark.parametrize("entry", ["mrp_partition_reads_by_haplotype", "mrp_phase_variants_from_tagged_reads"])
def test_entries_fail_loudly_without_a_context(entry):
    lib = capi.load()
    fn = getattr(lib, entry)
    m = capi.PairHmm.default_nucleotide()
    S = capi.HaptagSites()
    if entry == "mrp_partition_reads_by_haplotype":
        rc = fn(None, C.byref(m), C.byref(m), C.byref(S), 0, None, 4, None, None, None, None)
    else:
        rc = fn(None, C.byref(m), C.byref(m), C.byref(S), 0, None, None, 4, 512, None, None, None, None)
    assert rc == capi.MRP_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.mrp_last_error()
