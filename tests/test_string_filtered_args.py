"""mrp_phase_string_chunks_with_filtered and its queue twins without a device: the symbols and their transcription, every argument
check of the rest (made before the context is looked at), an all-empty rest, the ABI version."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import string_filtered_cases as sf

ENTRIES = ("mrp_phase_string_chunks_with_filtered", "mrp_queue_phase_string_chunks_with_filtered", "mrp_phase_string_chunks_with_filtered_on_devices")


def case():
    return sf.split_chunk(3, n_sites=8, coverage=8, duplicate_rate=0.2, n_variants=4)


def call(chunk, R, entry=0, rest_null=False, out_null=False):
    """the C entry with a NULL context / queue / an empty device list; R a StringChunkRest"""
    lib = capi.load()
    S, keep = capi.string_chunk_struct(chunk)
    arr, rarr = (capi.StringChunk * 1)(S), (capi.StringChunkRest * 1)(R)
    hap = np.zeros(max(len(chunk.read_names), 1), np.int8)
    hp = (C.c_void_p * 1)(hap.ctypes.data)
    res = (C.POINTER(capi.PhaseResult) * 1)()
    fout = (capi.FilteredOut * 1)()
    fout[0].n_reads = 77
    m = capi.PairHmm.default_nucleotide()
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    ra, fo = (None if rest_null else rarr), (None if out_null else fout)
    if entry == 0:
        rc = lib.mrp_phase_string_chunks_with_filtered(None, 1, arr, ra, C.byref(m), C.byref(m), 4, 512, 0.0, C.byref(p), 0, res, hp, None, None, fo, None)
    elif entry == 1:
        rc = lib.mrp_queue_phase_string_chunks_with_filtered(None, 1, arr, ra, C.byref(m), C.byref(m), 4, 512, 0.0, C.byref(p), 0, 0, res, hp, None, None, fo, None)
    else:
        dev = (C.c_int32 * 1)(0)
        rc = lib.mrp_phase_string_chunks_with_filtered_on_devices(C.cast(dev, C.c_void_p), 0, 1, arr, ra, C.byref(m), C.byref(m), 4, 512, 0.0, C.byref(p), 0, 0,
                                                                  res, hp, None, None, fo, None)
    if not out_null and not rest_null:
        assert fout[0].n_reads == 0 and not fout[0].read_hap  # zeroed whatever the outcome
    return rc


def test_symbols_transcription_and_abi_version():
    lib = capi.load()
    for s in ENTRIES:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert C.sizeof(capi.StringChunkRest) == 17 * 8 and C.sizeof(capi.FilteredOut) == 8 * 8
    assert C.sizeof(capi.StringFilteredStats) == C.sizeof(capi.StringChunksStats) + 4 * 8
    assert C.sizeof(capi.StringChunk) == 13 * 8  # the existing structs are as they were


@pytest.mark.parametrize("entry", [0, 1])
def test_a_well_formed_rest_reaches_the_missing_device(entry):
    c, rest = case()
    assert rest["variants"] and any(rest["fsubs"])
    R, keep = capi.string_chunk_rest_struct(c, rest)
    assert call(c, R, entry) == capi.MRP_ERR_NO_DEVICE
    assert b"no CPU fallback" in capi.load().mrp_last_error()


def test_an_all_empty_rest_is_accepted():
    c, _ = case()
    for entry in (0, 1):
        assert call(c, capi.StringChunkRest(), entry) == capi.MRP_ERR_NO_DEVICE
    assert call(c, capi.StringChunkRest(), 2) == capi.MRP_ERR_ARG  # no devices: the queue cannot be made, the arguments passed


@pytest.mark.parametrize("entry", [0, 1, 2])
def test_null_rest_or_output(entry):
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    assert call(c, R, entry, rest_null=True) == capi.MRP_ERR_ARG
    assert call(c, R, entry, out_null=True) == capi.MRP_ERR_ARG


@pytest.mark.parametrize("entry", [0, 1])
def test_null_arrays(entry):
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    for field in ("forward_strand", "pool", "fsub_first", "fsub_off", "fsub_len", "fsub_read", "valle_first", "valle_off", "valle_len", "gt", "ventry_first",
                  "ventry_read", "ventry_off", "ventry_len"):
        T = capi.StringChunkRest.from_buffer_copy(bytes(R))
        setattr(T, field, None)
        assert call(c, T, entry) == capi.MRP_ERR_ARG, field
        assert b"null argument" in capi.load().mrp_last_error(), field


def patched(keep, R, field, fn):
    a = keep[field].copy()
    fn(a)
    T = capi.StringChunkRest.from_buffer_copy(bytes(R))
    setattr(T, field, a.ctypes.data)
    return T, a


def test_offsets_not_ascending():
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    for field in ("fsub_first", "valle_first", "ventry_first"):
        def bump(a):
            a[1] = a[2] + 1
        T, _a = patched(keep, R, field, bump)
        assert call(c, T) == capi.MRP_ERR_ARG, field
        assert b"not ascending" in capi.load().mrp_last_error(), field

        def start(a):
            a[0] = 1
        T, _a = patched(keep, R, field, start)
        assert call(c, T) == capi.MRP_ERR_ARG, field


def test_read_indices_out_of_range():
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    n_f, n_all = len(rest["forward_strand"]), len(c.read_names) + len(rest["forward_strand"])
    for field, bads in (("fsub_read", (n_f, -1)), ("ventry_read", (n_all, -1))):
        for bad in bads:
            def put(a):
                a[0] = bad
            T, _a = patched(keep, R, field, put)
            assert call(c, T) == capi.MRP_ERR_ARG, (field, bad)
            assert b"names read" in capi.load().mrp_last_error()
    # a variant entry may name a filtered read: the highest index of the chunk is accepted
    def last(a):
        a[0] = n_all - 1
    T, _a = patched(keep, R, "ventry_read", last)
    assert call(c, T) == capi.MRP_ERR_NO_DEVICE


def test_a_filtered_read_twice_in_a_bubble_or_out_of_order():
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    b = int(np.nonzero(np.diff(keep["fsub_first"]) >= 2)[0][0])
    k0 = int(keep["fsub_first"][b])

    def twice(a):
        a[k0 + 1] = a[k0]
    T, _a = patched(keep, R, "fsub_read", twice)
    assert call(c, T) == capi.MRP_ERR_ARG
    assert b"twice" in capi.load().mrp_last_error()

    def swap(a):
        a[k0], a[k0 + 1] = a[k0 + 1], a[k0]
    T, _a = patched(keep, R, "fsub_read", swap)
    assert call(c, T) == capi.MRP_ERR_ARG
    assert b"ascending" in capi.load().mrp_last_error()


def test_gt_names_an_allele_the_variant_lacks():
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    n_alleles = int(keep["valle_first"][1] - keep["valle_first"][0])
    for bad in (n_alleles, -1):
        def put(a):
            a[1] = bad
        T, _a = patched(keep, R, "gt", put)
        assert call(c, T) == capi.MRP_ERR_ARG
        assert b"genotype allele" in capi.load().mrp_last_error()


def test_strings_outside_the_pool_and_bad_sizes():
    c, rest = case()
    R, keep = capi.string_chunk_rest_struct(c, rest)
    for field in ("fsub_off", "valle_off", "ventry_off"):
        def put(a):
            a[-1] = keep["pool"].size
        T, _a = patched(keep, R, field, put)
        assert call(c, T) == capi.MRP_ERR_ARG, field
        assert b"outside the pool" in capi.load().mrp_last_error()
    for field in ("n_filtered", "n_variants", "pool_bytes"):
        T = capi.StringChunkRest.from_buffer_copy(bytes(R))
        setattr(T, field, -1)
        assert call(c, T) == capi.MRP_ERR_ARG, field


def test_the_cases_are_deterministic():
    a, ra = sf.split_chunk(11, n_sites=20, coverage=10)
    b, rb = sf.split_chunk(11, n_sites=20, coverage=10)
    assert a.read_names == b.read_names and all((x[1] == y[1]).all() for fa, fb in zip(ra["fsubs"], rb["fsubs"]) for x, y in zip(fa, fb))
    chunks, rests = sf.filtered_chunks(26)
    assert len(chunks) == 26 and rests[4] is None and rests[9] is None and not chunks[9].bubbles
