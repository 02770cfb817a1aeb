"""mrp_extract_read_substrings on the device against the reference's walk (tests/extract_oracle.py), byte for byte:
synthetic chunks over several seeds and option sets in one call, the real-data fixture, every hand-built rule case in one
call, repeat calls and host-thread counts, empty and degenerate chunks, and extract -> mrp_string_chunk_from_extracted ->
mrp_phase_string_chunks against the same chain on the oracle's output."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests.test_extract_oracle import load_fixture

pytestmark = pytest.mark.gpu

OPTION_SETS = [capi.shipped_extract_options(),
               dict(expansion_small=4, expansion_sv=64, min_mapq=20, include_secondary=1, include_supplementary=1),
               dict(expansion_small=0, expansion_sv=0, min_mapq=0, include_secondary=0, include_supplementary=1)]


def assert_same(got, want, where=""):
    for k, v in want.items():
        g = got[k]
        assert g.dtype == np.asarray(v).dtype and np.array_equal(g, v), f"{where} {k}"


def check(ctx, chunks, opts):
    got, st = capi.extract_read_substrings(ctx, chunks, opts)
    want = eo.extract(chunks, opts)
    assert len(got) == len(chunks)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, eo.as_arrays(w), f"chunk {i}")
    return got, st


@pytest.fixture(scope="module")
def synthetic():
    return [synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0) for seed in range(16)]


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_synthetic_48_chunks(gpu_ctx, synthetic, k):
    # 48 chunks in one call: the 16 seeds three times over, each pass with other option sets
    chunks = synthetic * 3
    _, st = check(gpu_ctx, chunks, OPTION_SETS[k])
    assert st.entries > 0 and st.kernel_ms > 0 and st.bytes_uploaded > 0 and st.cigar_ops == sum(len(c.cigar) for c in chunks)


def test_realdata_fixture(gpu_ctx):
    got, st = check(gpu_ctx, [load_fixture()], capi.shipped_extract_options())
    assert got[0]["entry_read"].size > 100


def test_hand_cases_in_one_call(gpu_ctx):
    cases = ec.cases()
    got, _ = check(gpu_ctx, [c[1] for c in cases], ec.OPTS)
    for (name, _, subs, status), g in zip(cases, got):
        assert g["read_status"].tolist() == status, name
        assert g["read_n_substrings"].tolist() == [len(s) for s in subs], name


def test_repeat_and_host_threads(gpu_ctx, synthetic):
    lib = capi.load()
    first, _ = capi.extract_read_substrings(gpu_ctx, synthetic)
    try:
        for threads in (1, 3, 0):
            lib.mrp_set_host_threads(threads)
            again, _ = capi.extract_read_substrings(gpu_ctx, synthetic)
            for a, b in zip(first, again):
                assert_same(b, a, f"threads {threads}")
    finally:
        lib.mrp_set_host_threads(0)


def test_degenerate_chunks(gpu_ctx):
    empty = ec.make([], [])
    no_variants = ec.make([], [(100, "20M", 60, 0)])
    no_cigar = ec.make([ec.SNP110], [(100, "20M", 60, 0), (100, "20M", 60, 0), (101, "18M", 60, 0)])
    cf = no_cigar.cigar_first.copy()
    no_cigar.cigar = np.delete(no_cigar.cigar, 1)  # read 1 keeps its bases but loses its CIGAR
    no_cigar.cigar_first = np.array([0, 1, 1, 2], np.int64)
    assert cf.tolist() == [0, 1, 2, 3]
    got, _ = check(gpu_ctx, [empty, no_variants, no_cigar], ec.OPTS)
    assert got[0]["read_status"].size == 0 and got[1]["read_status"].tolist() == [0]
    assert got[2]["read_status"].tolist() == [1, 0, 1]
    got, _ = check(gpu_ctx, [], ec.OPTS)
    assert got == []


def _phase(ctx, string_chunks):
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    out, _ = capi.phase_string_chunks(ctx, string_chunks, fwd, fwd.reverse_complement(), params, expansion=4, sv_threshold=512)
    return out


@pytest.mark.parametrize("source", ["synthetic", "fixture"])
def test_end_to_end_phasing(gpu_ctx, synthetic, source):
    chunks = synthetic[:6] if source == "synthetic" else [load_fixture()]
    opts = capi.shipped_extract_options()
    got, _ = capi.extract_read_substrings(gpu_ctx, chunks, opts)
    want = eo.extract(chunks, opts)
    dev_sc, ora_sc = [], []
    for c, g, w in zip(chunks, got, want):
        keep = (np.arange(len(c.read_pos)) % 5 != 2).astype(np.uint8)
        sc, bv, raw = capi.string_chunk_from_extracted(g, c.read_names, c.read_forward_strand, keep=keep)
        sc_o, bv_o, raw_o = capi.string_chunk_from_extracted(eo.as_arrays(w), c.read_names, c.read_forward_strand, keep=keep)
        for k in raw:
            assert np.array_equal(raw[k], raw_o[k]), k
        bub, var = eo.bubbles_from_extracted(w, keep)
        assert bv.tolist() == var and len(sc.bubbles) == len(bub) > 0
        dev_sc.append(sc)
        ora_sc.append(sc_o)
    a, b = _phase(gpu_ctx, dev_sc), _phase(gpu_ctx, ora_sc)
    for x, y in zip(a, b):
        assert np.array_equal(x["hap"], y["hap"]) and np.array_equal(x["phred"], y["phred"])
        for k in ("hap1", "hap2", "reads1", "reads2"):
            assert np.array_equal(np.asarray(x["result"][k]), np.asarray(y["result"][k])), k
