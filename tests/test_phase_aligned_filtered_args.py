"""mrp_phase_aligned_chunks_with_filtered and mrp_equal_substring_classes without a device: the symbols are exported and transcribed,
and each reports its errors in the order the header states -- every MRP_ERR_ARG before the context is looked at, the two refused
extraction modes as MRP_ERR_UNSUPPORTED with a NULL context, and only for well-formed arguments MRP_ERR_NO_DEVICE.  The binding asserts,
on every error, that no output was written and that filtered_out is zeroed."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import rest_cases as rc


@pytest.fixture(scope="module")
def call():
    """-> (chunks of the primary variants, rests (filtered chunk, gt))"""
    chunks, rests = [], []
    for seed in range(2):
        primary, filtered, _ = rc.split_variants(rc.synthetic(seed))
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    return chunks, rests


def models():
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    return f, f.reverse_complement(), capi.Params.from_reference_names(synth.shipped_phase_params())


def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_phase_aligned_chunks_with_filtered", "mrp_equal_substring_classes", "mrp_string_chunk_rest_from_extracted"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.AlignedChunkRest) == 9 * 8
    assert C.sizeof(capi.PhaseAlignedFilteredStats) == C.sizeof(capi.PhaseAlignedStats) + 8 * 8
    assert C.sizeof(capi.PhaseAlignedStats) == C.sizeof(capi.ExtractStats) + C.sizeof(capi.StringChunksStats) + 13 * 8  # as it was


def code_of(chunks, rests, *args, **kw):
    with pytest.raises(capi.MrpError) as e:
        capi.phase_aligned_chunks_with_filtered(None, chunks, rests, *args, **kw)
    return e.value.code, str(e.value)


def test_composite_errors_in_order(call):
    chunks, rests = call
    f, r, p = models()
    # the front's own checks
    assert code_of(chunks, rests, None, r, p)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, rests, f, None, p)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, rests, f, r, None)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, rests, f, r, p, expansion=3)[0] == capi.MRP_ERR_ARG
    for what in ("options", "out", "hap_out", "read_names", "hap_out[0]", "phred_out[0]", "read_names[0]", "read_names[0][0]"):
        code, msg = code_of(chunks, rests, f, r, p, nulls=(what,))
        assert code == capi.MRP_ERR_ARG, (what, msg)
    # a NULL rest / filtered_out / filtered_read_out, NULL genotypes
    for what in ("rest", "filtered_out", "filtered_read_out", "gt[0]"):
        code, msg = code_of(chunks, rests, f, r, p, nulls=(what,))
        assert code == capi.MRP_ERR_ARG, (what, msg)
    # a gt outside the variant's alleles
    fl, gt = rests[1]
    for v, w, bad in ((0, 0, len(fl.alleles[0])), (len(fl.alleles) - 1, 1, -1)):
        g = gt.copy()
        g[v, w] = bad
        code, msg = code_of(chunks, [rests[0], (fl, g)], f, r, p)
        assert code == capi.MRP_ERR_ARG and "chunk 1" in msg and f"filtered variant {v}" in msg, msg
    # the extraction's checks on the rest's variants: not ascending, outside the overlap, a REF allele that disagrees with the reference
    swapped = dataclasses.replace(fl, variant_pos=np.ascontiguousarray(fl.variant_pos[::-1]))
    assert code_of(chunks, [rests[0], (swapped, gt)], f, r, p)[0] == capi.MRP_ERR_ARG
    outside = dataclasses.replace(fl, variant_pos=np.concatenate([fl.variant_pos[:-1], [fl.overlap_end]]))
    code, msg = code_of(chunks, [rests[0], (outside, gt)], f, r, p)
    assert code == capi.MRP_ERR_ARG and "outside the overlap" in msg
    hand = ec.make([ec.SNP110], [(100, "40M", 60, 0)])
    broken = ec.make([(125, ["A" if ec.REF[25] != "A" else "C", "G"], 0)], [(100, "40M", 60, 0)])
    assert code_of([hand], [(broken, [(0, 1)])], f, r, p, options=ec.OPTS)[0] == capi.MRP_ERR_ARG
    # ... and on the chunk's own
    assert code_of([broken], [(hand, [(0, 1)])], f, r, p, options=ec.OPTS)[0] == capi.MRP_ERR_ARG
    # well-formed: only now is the context looked at
    code, msg = code_of(chunks, rests, f, r, p)
    assert code == capi.MRP_ERR_NO_DEVICE and "no CPU fallback" in msg
    assert code_of(chunks, rests, f, r, p, keeps=[None, np.ones(len(chunks[1].read_pos), np.uint8)])[0] == capi.MRP_ERR_NO_DEVICE
    assert code_of([], [], f, r, p)[0] == capi.MRP_ERR_NO_DEVICE
    no_rest = rc.subset(chunks[0], [])  # a rest without variants needs no arrays
    assert code_of(chunks[:1], [(no_rest, [])], f, r, p)[0] == capi.MRP_ERR_NO_DEVICE
    # the two refused extraction modes, as the extraction reports them: without a context
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        opts = dict(capi.shipped_extract_options(), **{mode: 1})
        assert code_of(chunks, rests, f, r, p, options=opts)[0] == capi.MRP_ERR_UNSUPPORTED
        # ... but an argument error of the same call still comes first
        assert code_of(chunks, rests, f, r, None, options=opts)[0] == capi.MRP_ERR_ARG
        g = gt.copy()
        g[0, 0] = 99
        assert code_of(chunks, [rests[0], (fl, g)], f, r, p, options=opts)[0] == capi.MRP_ERR_ARG
        assert code_of(chunks, rests, f, r, p, options=opts, nulls=("filtered_out",))[0] == capi.MRP_ERR_ARG


def classes_code(*args, **kw):
    with pytest.raises(capi.MrpError) as e:
        capi.equal_substring_classes(None, *args, **kw)
    return e.value.code, str(e.value)


def test_classes_errors_in_order():
    pool = np.arange(50, dtype=np.uint8) % 5
    ok = ([0, 2, 2, 3], [0, 10, 40], [10, 10, 10])
    for what in ("entry_first", "pool", "off", "len", "rep_out"):
        assert classes_code(ok[0], pool, ok[1], ok[2], nulls=(what,))[0] == capi.MRP_ERR_ARG, what
    assert classes_code([1, 2, 2, 3], pool, ok[1], ok[2])[0] == capi.MRP_ERR_ARG      # offsets not from 0
    assert classes_code([0, 2, 1, 3], pool, ok[1], ok[2])[0] == capi.MRP_ERR_ARG      # not ascending
    for off, length in (([0, 10, 41], [10, 10, 10]), ([0, -1, 40], [10, 10, 10]), ([0, 10, 40], [10, -1, 10])):
        code, msg = classes_code(ok[0], pool, off, length)
        assert code == capi.MRP_ERR_ARG and "outside the symbol pool" in msg
    code, msg = classes_code(ok[0], pool, ok[1], ok[2])
    assert code == capi.MRP_ERR_NO_DEVICE and "no CPU fallback" in msg
    assert classes_code([0], pool, [], [])[0] == capi.MRP_ERR_NO_DEVICE                # no site
    assert classes_code([0, 0, 0], np.zeros(0, np.uint8), [], [])[0] == capi.MRP_ERR_NO_DEVICE
