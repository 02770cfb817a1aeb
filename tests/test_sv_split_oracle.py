"""The SV split of the extraction (mrp_context_set_sv_split), CPU side: the three symbols are exported under
the unchanged ABI, mrp_mark_structural_variants against the rule of vcf.c:173-185, the setters and the refusal without a context, and
the oracle wrapper tests/extract_sv_oracle.py on a hand-made case whose expected values are written out."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests import extract_sv_oracle as so
from tests import sv_split_cases as sc

SYMBOLS = ["mrp_context_set_sv_split", "mrp_queue_set_sv_split", "mrp_mark_structural_variants"]


def test_symbols_are_exported_and_the_abi_is_unchanged():
    lib = capi.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED_SYMBOLS, s
    assert capi.ABI_VERSION == 6 and lib.mrp_abi_version() == 6
    assert callable(capi.Context.set_sv_split) and callable(capi.Queue.set_sv_split) and callable(capi.mark_structural_variants)
    # no public struct changed size (the figures of tests/test_extract_oracle.py::test_symbols_and_layout)
    assert C.sizeof(capi.AlignedChunk) == 23 * 8 and C.sizeof(capi.ExtractOptions) == 5 * 8 and C.sizeof(capi.ExtractedChunk) == 15 * 8


def test_the_setters_refuse_a_null_handle():
    lib = capi.load()
    assert lib.mrp_context_set_sv_split(None, 1) == lib.mrp_context_set_wide_pairs(None, 1) == capi.MRP_ERR_ARG
    assert lib.mrp_queue_set_sv_split(None, 1) == lib.mrp_queue_set_wide_pairs(None, 1) == capi.MRP_ERR_ARG


def chunk_with_allele_lengths(lengths):
    """a chunk over ec.REF whose variant v has alleles of the given lengths (only allele_first and allele_len are read)"""
    return ec.make([(100 + v, ["A" * n for n in ls], 0) for v, ls in enumerate(lengths)], [])


def test_mark_structural_variants_is_the_rule_of_the_vcf_loader():
    rng = np.random.default_rng(173)
    lengths = [[int(n) for n in rng.integers(1, 120, size=int(rng.integers(1, 5)))] for _ in range(39)]
    chunk = chunk_with_allele_lengths(lengths)
    for size in (-3, 0, 1, 20, 50, 119, 120):
        want = [int(size > 0 and any(n > size for n in ls)) for ls in lengths]  # vcf.c:182
        got = capi.mark_structural_variants(chunk, size)
        assert got.dtype == np.uint8 and got.tolist() == want, size
    assert any(capi.mark_structural_variants(chunk, 50)) and not all(capi.mark_structural_variants(chunk, 50))
    # the boundary: an allele as long as the threshold is small, one longer structural; a threshold <= 0 marks none
    edge = chunk_with_allele_lengths([[1, 50], [1, 51], [51, 1], [50, 50, 50], [1]])
    assert capi.mark_structural_variants(edge, 50).tolist() == [0, 1, 1, 0, 0]
    assert capi.mark_structural_variants(edge, 0).tolist() == [0] * 5 and capi.mark_structural_variants(edge, -1).tolist() == [0] * 5
    assert capi.mark_structural_variants(ec.make([], []), 50).size == 0
    lib = capi.load()
    assert lib.mrp_mark_structural_variants(None, 50, None) == capi.MRP_ERR_ARG
    S, keep = capi.aligned_chunk_struct(edge)
    assert lib.mrp_mark_structural_variants(C.byref(S), 50, None) == capi.MRP_ERR_ARG
    # only allele_first and allele_len are read
    for field in ("variant_pos", "allele_off", "allele_chars", "is_sv", "reference"):
        setattr(S, field, None)
    assert capi.mark_structural_variants(edge, 50, struct=(S, keep)).tolist() == [0, 1, 1, 0, 0]


def _rc(call):
    with pytest.raises(capi.MrpError) as e:
        call()
    return e.value.code, str(e.value)


def test_without_a_context_the_mode_is_refused_after_the_argument_errors():
    """a NULL context counts as off: ARG, then UNSUPPORTED, then NO_DEVICE, with the message of before"""
    base = sc.delayed_start()
    code, msg = _rc(lambda: capi.extract_read_substrings(None, [base], sc.OPTS))
    assert code == capi.MRP_ERR_UNSUPPORTED and "indelSizeForSVHandling > 0 (htsIntegration.c:1724-1755) is not supported" in msg
    assert _rc(lambda: capi.extract_read_substrings(None, [base], dict(sc.OPTS, indel_size_for_sv_handling=-1)))[0] == capi.MRP_ERR_UNSUPPORTED
    assert _rc(lambda: capi.extract_read_substrings(None, [base], sc.UNSPLIT))[0] == capi.MRP_ERR_NO_DEVICE
    assert _rc(lambda: capi.extract_read_substrings(None, [base], dict(sc.OPTS, expansion_small=-1)))[0] == capi.MRP_ERR_ARG
    # (the chunks' own argument errors are looked for after the mode, as before: tests/test_extract_oracle.py::test_argument_errors)
    f = capi.PairHmm.default_nucleotide()
    r = f.reverse_complement()
    gts = [np.array([[0, 1], [0, 1]], np.int32)]
    unsorted = sc.make(sc.REF, [sc.ins(sc.REF, 620), sc.snp(sc.REF, 600)], [(100, "1000M", 60, 0)])
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    for chunks, want in (([base], capi.MRP_ERR_UNSUPPORTED), ([unsorted], capi.MRP_ERR_ARG)):
        assert _rc(lambda: capi.haplotag_aligned_chunks(None, chunks, gts, f, r, sc.OPTS))[0] == want
        assert _rc(lambda: capi.phase_aligned_chunks(None, chunks, f, r, p, options=sc.OPTS))[0] == want
        assert _rc(lambda: capi.haplotag_aligned_chunks_on_devices([0], chunks, gts, f, r, sc.OPTS))[0] == want
        assert _rc(lambda: capi.phase_aligned_chunks_on_devices([0], chunks, f, r, p, options=sc.OPTS))[0] == want


def test_hand_made_delayed_start():
    """expansion_small 12, expansion_sv 64, overlap from 0, a small variant at 600 and one read 1000M from 100 (read base = position - 100).

    With the structural variant at 700 its window [636, 765] begins after the small one's [588, 613]: the two walks agree.  (The positions
    first proposed for this case; they do not interact, since 700 - 64 > 600 - 12.)  With it at 620 its window [556, 685]
    begins BEFORE the small variant's, which is listed first: in the one-list walk it starts only once that one has, at 588; in its
    own walk it starts at 556."""
    apart = sc.delayed_start(700)
    for x in (eo.extract_chunk(apart, sc.UNSPLIT), so.extract_chunk(apart, sc.OPTS)):
        assert [(w["aln_start"], w["aln_stop"]) for w in x["variants"]] == [(588, 613), (636, 765)]
        assert x["subs"] == [[(0, 488, 513), (1, 536, 665)]] and x["status"].tolist() == [eo.KEPT]
    chunk = sc.delayed_start(620)
    unsplit, split = eo.extract_chunk(chunk, sc.UNSPLIT), so.extract_chunk(chunk, sc.OPTS)
    for x in (unsplit, split):
        assert [(w["aln_start"], w["aln_stop"]) for w in x["variants"]] == [(588, 613), (556, 685)]
        assert x["status"].tolist() == [eo.KEPT]
    assert unsplit["subs"] == [[(0, 488, 513), (1, 488, 585)]]  # the SV's substring starts at the small variant's window start
    assert split["subs"] == [[(0, 488, 513), (1, 456, 585)]]    # ... and at its own
    # the required condition: on this input the split is not a formality
    a, b = eo.as_arrays(eo.extract([chunk], sc.UNSPLIT)[0]), eo.as_arrays(so.extract([chunk], sc.OPTS)[0])
    assert a["entry_len"].tolist() == [25, 97] and b["entry_len"].tolist() == [25, 129]
    assert not np.array_equal(a["pool"], b["pool"])
    for k in ("ref_aln_start", "ref_aln_stop_incl", "allele_first", "allele_off", "allele_len", "read_status", "read_n_substrings", "entry_first", "entry_read"):
        assert np.array_equal(a[k], b[k]), k


def test_the_wrapper_merges_by_read_index():
    """a read only one walk lists is listed; a read neither lists is dropped; counts are summed; a chunk of one class equals the one-list walk"""
    ref = sc.REF
    chunk = sc.make(ref, [sc.ins(ref, 300), sc.snp(ref, 500)],
                    [(100, "600M", 60, 0), (400, "200M", 60, 0), (100, "300M", 60, 0), (520, "100M", 60, 0), (100, "600M", 3, 0)])
    x = so.extract_chunk(chunk, sc.OPTS)
    assert x["status"].tolist() == [eo.KEPT, eo.KEPT, eo.KEPT, eo.DROPPED, eo.FILTERED]
    assert [len(s) for s in x["subs"]] == [2, 1, 1, 0, 2] and [v for v, _, _ in x["subs"][1]] == [1] and [v for v, _, _ in x["subs"][2]] == [0]
    for only in (chunk.is_sv * 0, chunk.is_sv * 0 + 1):
        one = dataclasses.replace(chunk, is_sv=only.astype(np.uint8))
        a, b = eo.as_arrays(eo.extract([one], sc.UNSPLIT)[0]), eo.as_arrays(so.extract([one], sc.OPTS)[0])
        assert all(np.array_equal(a[k], b[k]) for k in a)
