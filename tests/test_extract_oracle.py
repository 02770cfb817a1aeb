"""The extraction of read substrings at variant sites without a device: the reference's walk restated in
tests/extract_oracle.py on one hand-built case per rule, on the real-data fixture, the generator's determinism,
mrp_string_chunk_from_extracted against the oracle's bubble construction, the argument checks and the loud failure
without a context."""
import ctypes as C
import os

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as eo

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "realdata_extract.npz")


@pytest.mark.parametrize("case", ec.cases(), ids=lambda c: c[0])
def test_hand_case(case):
    name, chunk, subs, status = case
    x = eo.extract_chunk(chunk, ec.OPTS)
    assert [sorted(s) for s in x["subs"]] == [sorted(s) for s in subs]
    assert list(x["status"]) == status


def test_hand_case_substring_symbols():
    name, chunk, subs, _ = ec.cases()[0]
    (x,) = eo.extract([chunk], ec.OPTS)
    # read 0: bases cycle A C G T, substring = seq[8:15]
    assert x["entries"][0][0][0] == 0 and x["entries"][0][0][1].tolist() == [0, 1, 2, 3, 0, 1, 2]
    # allele strings: prefix REF[8:10] + allele + suffix REF[11:13]
    assert [a.tolist() for a in x["alleles"][0]] == [eo.symbols(ec.REF[8:13]).tolist(), eo.symbols(ec.REF[8:10] + ec.SNP110[1][1] + ec.REF[11:13]).tolist()]


def load_fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    alleles = [str(a).split(",") for a in z["alleles"]]
    return synth.AlignedChunk(overlap_start=int(z["coords"][0]), overlap_end=int(z["coords"][1]), chunk_start=int(z["coords"][2]),
                              chunk_end=int(z["coords"][3]), reference=str(z["reference"]), variant_pos=z["variant_pos"], alleles=alleles,
                              is_sv=z["is_sv"], read_pos=z["read_pos"], flag=z["flag"], mapq=z["mapq"], l_qseq=z["l_qseq"],
                              cigar_first=z["cigar_first"], cigar=z["cigar"], seq_first=z["seq_first"], seq=z["seq"],
                              read_names=[str(n) for n in z["read_names"]])


def test_fixture_oracle_counts():
    ch = load_fixture()
    opts = capi.shipped_extract_options()
    (x,) = eo.extract([ch], opts)
    # statuses from the fields directly: flags, mapq, span, a variant at or after the start
    ref_span = []
    for r in range(len(ch.read_pos)):
        w = ch.cigar[ch.cigar_first[r]:ch.cigar_first[r + 1]]
        ref_span.append(int(sum(int(c) >> 4 for c in w if int(c) & 15 in (0, 2, 3, 7, 8))))
    for r in range(len(ch.read_pos)):
        ok = ch.l_qseq[r] > 0 and not ch.flag[r] & 0x904 and ch.read_pos[r] < ch.chunk_end and ch.read_pos[r] + ref_span[r] > ch.chunk_start
        ok = ok and (ch.variant_pos >= ch.read_pos[r]).any()
        want = (eo.FILTERED if ch.mapq[r] < opts["min_mapq"] else eo.KEPT) if ok else eo.DROPPED
        assert x["read_status"][r] == want, r
    # a SNP window lies inside a listed read's span: the read gives it a substring unless the window is deleted whole
    for v, ents in enumerate(x["entries"]):
        g0, g1 = ch.overlap_start + x["ref_aln_start"][v], ch.overlap_start + x["ref_aln_stop_incl"][v]
        cover = {r for r in range(len(ch.read_pos)) if x["read_status"][r] != eo.DROPPED and ch.read_pos[r] < g0 and ch.read_pos[r] + ref_span[r] > g1}
        got = {r for r, _ in ents}
        assert got <= {r for r in range(len(ch.read_pos)) if x["read_status"][r] != eo.DROPPED}
        assert len(cover - got) <= max(1, len(cover) // 10), v
        for r, s in ents:
            assert 1 <= len(s) <= 60
    assert sum(len(e) for e in x["entries"]) == int(x["read_n_substrings"].sum()) > 100


def test_generator_deterministic():
    a, b, c = synth.make_aligned_chunk(3), synth.make_aligned_chunk(3), synth.make_aligned_chunk(4)
    for f in ("variant_pos", "is_sv", "read_pos", "flag", "mapq", "l_qseq", "cigar_first", "cigar", "seq_first", "seq"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.reference == b.reference and a.alleles == b.alleles
    assert a.reference != c.reference
    ops = a.cigar & 15
    assert {0, 1, 2, 3, 4, 5}.issubset(set(ops.tolist())) or {7, 8}.issubset(set(ops.tolist()))
    assert a.is_sv.any() and (a.flag & 0x900).any() and (a.mapq < 5).any()


def test_string_chunk_from_extracted_matches_oracle():
    chunk = synth.make_aligned_chunk(5)
    opts = capi.shipped_extract_options()
    (x,) = eo.extract([chunk], opts)
    arrays = eo.as_arrays(x)
    keep = (np.arange(len(chunk.read_pos)) % 3 != 0).astype(np.uint8)
    for k in (None, keep):
        sc, bv, raw = capi.string_chunk_from_extracted(arrays, chunk.read_names, chunk.read_forward_strand, keep=k)
        want, want_v = eo.bubbles_from_extracted(x, k)
        assert bv.tolist() == want_v
        assert len(sc.bubbles) == len(want)
        for (ga, gr, gs), (wa, wr, ws) in zip(sc.bubbles, want):
            assert [a.tolist() for a in ga] == [a.tolist() for a in wa]
            assert gr == wr
            assert [s.tolist() for s in gs] == [s.tolist() for s in ws]


def test_null_context_fails_loudly():
    with pytest.raises(capi.MrpError) as e:
        capi.extract_read_substrings(None, [synth.make_aligned_chunk(1)])
    assert e.value.code == capi.MRP_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def _rc(chunks, opts=None, mutate=None):
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    if mutate:
        mutate(built)
    with pytest.raises(capi.MrpError) as e:
        capi.extract_read_substrings(None, chunks, opts, structs=built)
    return e.value.code


def test_argument_errors():
    base = ec.make([ec.SNP110, (120, [ec.REF[20], "A"], 0)], [(100, "20M", 60, 0)])
    assert _rc([base]) == capi.MRP_ERR_NO_DEVICE
    c = ec.make([(120, [ec.REF[20], "A"], 0), ec.SNP110], [(100, "20M", 60, 0)])
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # unsorted
    c = ec.make([ec.SNP110], [(100, "20M", 60, 0)])
    c.cigar = c.cigar.copy(); c.cigar[0] = (20 << 4) | 9
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # op code 9
    c = ec.make([(110, ["T" if ec.REF[10] != "T" else "A", "G"], 0)], [(100, "20M", 60, 0)])
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # REF disagrees
    c = ec.make([ec.SNP110], [(100, "20M", 60, 0)])
    c.reference = c.reference[:-1]
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # slice length
    c = ec.make([(150, ["A", "C"], 0)], [(100, "20M", 60, 0)])
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # outside the overlap
    c = ec.make([ec.SNP110], [(100, "20M", 60, 0)])
    c.l_qseq = c.l_qseq + 1
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # query length
    c = ec.make([ec.SNP110], [(100, "10M0I10M", 60, 0)])
    assert _rc([c]) == capi.MRP_ERR_ARG                                    # zero-length op
    n = ec.make([ec.SNP110], [(100, "10M", 60, 0)])
    assert _rc([base, n]) == capi.MRP_ERR_NO_DEVICE
    assert _rc([base], dict(capi.shipped_extract_options(), indel_size_for_sv_handling=50)) == capi.MRP_ERR_UNSUPPORTED
    assert _rc([base], dict(capi.shipped_extract_options(), use_run_length_encoding=1)) == capi.MRP_ERR_UNSUPPORTED
    assert _rc([base], dict(capi.shipped_extract_options(), expansion_small=-1)) == capi.MRP_ERR_ARG

    def null(field):
        def f(built):
            setattr(built[0][0], field, None)
        return f
    for field in ("variant_pos", "allele_first", "pos", "cigar_first", "seq_first", "reference"):
        assert _rc([base], mutate=null(field)) == capi.MRP_ERR_ARG, field


def test_symbols_and_layout():
    lib = capi.load()
    for s in ("mrp_extract_read_substrings", "mrp_string_chunk_from_extracted"):
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert C.sizeof(capi.AlignedChunk) == 23 * 8 and C.sizeof(capi.ExtractOptions) == 5 * 8 and C.sizeof(capi.ExtractedChunk) == 15 * 8
