"""mrp_haptag_sites_from_extracted and the argument checks of mrp_haplotag_aligned_chunks, without a device: the symbols are
exported and transcribed, the host-only site builder equals its Python restatement (tests/haplotag_aligned_oracle.py) array for
array, and the composite reports every MRP_ERR_ARG before it looks at the context."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests import haplotag_aligned_oracle as hao

SITE_KEYS = ("allele_first", "allele_off", "allele_len", "compare", "entry_first", "entry_read", "entry_off", "entry_len", "pool")


@pytest.fixture(scope="module")
def synthetic():
    chunks = [synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0) for seed in range(6)]
    return chunks, [hao.draw_genotypes(c, seed) for seed, c in enumerate(chunks)]


def models():
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    return f, f.reverse_complement()


def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_haptag_sites_from_extracted", "mrp_haplotag_aligned_chunks"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert C.sizeof(capi.HaplotagAlignedStats) == C.sizeof(capi.ExtractStats) + C.sizeof(capi.PairHmmStats) + 7 * 8


def assert_sites_equal(got, want, got_first, want_first):
    assert got["n_sites"] == want["n_sites"]
    for k in SITE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got_first.dtype == want_first.dtype and np.array_equal(got_first, want_first)


def test_sites_from_extracted_synthetic_in_one_call(synthetic):
    chunks, gts = synthetic
    xs = [eo.as_arrays(x) for x in eo.extract(chunks, capi.shipped_extract_options())]
    got, first = capi.haptag_sites_from_extracted(xs, gts)
    want, want_first = hao.sites_from_extracted(xs, gts)
    assert_sites_equal(got, want, first, want_first)
    assert got["n_sites"] == sum(len(c.alleles) for c in chunks) and first[-1] == sum(len(c.read_pos) for c in chunks)
    # low-mapq reads have entries in the extraction and none in the sites; variants without entries are listed
    n_all = sum(len(x["entry_read"]) for x in xs)
    assert 0 < got["entry_read"].size < n_all and (np.diff(got["entry_first"]) == 0).any()


def test_sites_from_extracted_hand_cases():
    cases = ec.cases()
    chunks = [c[1] for c in cases]
    xs = [eo.as_arrays(x) for x in eo.extract(chunks, ec.OPTS)]
    gts = [np.array([[0, 1]] * len(c.alleles), np.int32).reshape(-1, 2) for c in chunks]
    got, first = capi.haptag_sites_from_extracted(xs, gts)
    want, want_first = hao.sites_from_extracted(xs, gts)
    assert_sites_equal(got, want, first, want_first)
    # "lists": the low-mapq read's substring is not an entry, and reads are numbered over the call
    assert got["entry_read"].size < sum(len(x["entry_read"]) for x in xs) and got["entry_read"].max() >= len(chunks[0].read_pos)
    got, first = capi.haptag_sites_from_extracted([], [])
    assert got["n_sites"] == 0 and first.tolist() == [0]


def test_sites_from_extracted_errors(synthetic):
    chunks, gts = synthetic
    xs = [eo.as_arrays(x) for x in eo.extract(chunks[:2], capi.shipped_extract_options())]
    for bad in (-1, len(chunks[1].alleles[3])):
        g = [gts[0], gts[1].copy()]
        g[1][3, 1] = bad
        with pytest.raises(capi.MrpError) as e:
            capi.haptag_sites_from_extracted(xs, g)
        assert e.value.code == capi.MRP_ERR_ARG and "chunk 1" in str(e.value) and "variant 3" in str(e.value)
        with pytest.raises(ValueError, match="chunk 1, variant 3"):
            hao.sites_from_extracted(xs, g)
    for kw, g in ((dict(null_gt=True), gts[:2]), ({}, [gts[0], None])):
        with pytest.raises(capi.MrpError) as e:
            capi.haptag_sites_from_extracted(xs, g, **kw)
        assert e.value.code == capi.MRP_ERR_ARG
    lib = capi.load()
    assert lib.mrp_haptag_sites_from_extracted(0, None, None, None, None) == capi.MRP_ERR_ARG


def code_of(*args, **kw):
    with pytest.raises(capi.MrpError) as e:
        capi.haplotag_aligned_chunks(None, *args, **kw)
    return e.value.code, str(e.value)


def test_composite_argument_errors_come_before_the_context(synthetic):
    chunks, gts = synthetic
    chunks, gts = chunks[:2], gts[:2]
    f, r = models()
    bad = [gts[0], gts[1].copy()]
    bad[1][5, 0] = len(chunks[1].alleles[5])
    code, msg = code_of(chunks, bad, f, r)
    assert code == capi.MRP_ERR_ARG and "chunk 1" in msg and "variant 5" in msg
    bad[1][5, 0] = -1
    assert code_of(chunks, bad, f, r)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, [gts[0], None], f, r)[0] == capi.MRP_ERR_ARG       # a NULL genotype array for a chunk with variants
    assert code_of(chunks, gts, None, r)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, gts, f, None)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, gts, f, r, expansion=3)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, gts, f, r, expansion=-2)[0] == capi.MRP_ERR_ARG
    assert code_of(chunks, gts, f, r, null_options=True)[0] == capi.MRP_ERR_ARG
    # the extraction's own checks: a REF allele that disagrees with the reference
    broken = ec.make([(110, ["A" if ec.REF[10] != "A" else "C", "G"], 0)], [(100, "20M", 60, 0)])
    assert code_of([broken], [np.array([[0, 1]], np.int32)], f, r, options=ec.OPTS)[0] == capi.MRP_ERR_ARG
    # well-formed: only now is the context looked at
    code, msg = code_of(chunks, gts, f, r)
    assert code == capi.MRP_ERR_NO_DEVICE and "no CPU fallback" in msg
    assert code_of([], [], f, r)[0] == capi.MRP_ERR_NO_DEVICE
    # the two refused extraction modes, as the extraction reports them
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        opts = dict(capi.shipped_extract_options(), **{mode: 1})
        assert code_of(chunks, gts, f, r, options=opts)[0] == capi.MRP_ERR_UNSUPPORTED
        # ... but an argument error of the same call still comes first
        assert code_of(chunks, bad, f, r, options=opts)[0] == capi.MRP_ERR_ARG
