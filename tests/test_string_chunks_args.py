"""mrp_phase_string_chunks without a device: the symbol, the ABI version, the argument checks (made before the context is
looked at) and the loud failure without a context; the synthetic string chunks are deterministic."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth


def call(chunks, ctx=None, hap_out=True):
    lib = capi.load()
    built = [capi.string_chunk_struct(c) for c in chunks]
    return call_structs([b[0] for b in built], [len(c.read_names) for c in chunks], ctx, hap_out), built


def call_structs(structs, n_reads, ctx=None, hap_out=True):
    lib = capi.load()
    n = len(structs)
    arr = (capi.StringChunk * max(n, 1))(*structs)
    haps = [np.zeros(max(k, 1), np.int8) for k in n_reads]
    hp = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h in haps]) if hap_out else None
    res = (C.POINTER(capi.PhaseResult) * max(n, 1))()
    m = capi.PairHmm.default_nucleotide()
    p = capi.Params.from_reference_names(synth.shipped_phase_params())
    return lib.mrp_phase_string_chunks(ctx, n, arr, C.byref(m), C.byref(m), 4, 512, 0.0, C.byref(p), 0, res, hp, None, None, None)


def small():
    return synth.make_string_chunk(seed=1, n_sites=6, coverage=4, span=(2, 4))


def test_symbol_and_abi_version():
    lib = capi.load()
    assert "mrp_phase_string_chunks" in capi.EXPORTED_SYMBOLS and hasattr(lib, "mrp_phase_string_chunks")
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert C.sizeof(capi.StringChunk) == 13 * 8 and C.sizeof(capi.ProfileOut) == 8 * 8


def test_null_context_fails_loudly():
    rc, _ = call([small()])
    assert rc == capi.MRP_ERR_NO_DEVICE
    assert b"no CPU fallback" in capi.load().mrp_last_error()


def test_null_arrays():
    c = small()
    S, keep = capi.string_chunk_struct(c)
    for field in ("allele_first", "sub_first", "allele_off", "sub_read", "read_names", "read_forward_strand"):
        T = capi.StringChunk.from_buffer_copy(bytes(S))
        setattr(T, field, None)
        assert call_structs([T], [len(c.read_names)]) == capi.MRP_ERR_ARG, field
    rc, _ = call([c], hap_out=False)
    assert rc == capi.MRP_ERR_ARG


def test_offsets_not_ascending():
    c = small()
    S, keep = capi.string_chunk_struct(c)
    sf = keep["sub_first"].copy()
    sf[2] = sf[3] + 1
    S.sub_first = sf.ctypes.data
    assert call_structs([S], [len(c.read_names)]) == capi.MRP_ERR_ARG
    assert b"not ascending" in capi.load().mrp_last_error()
    S, keep = capi.string_chunk_struct(c)
    af = keep["allele_first"].copy()
    af[1] = af[0]  # a bubble without alleles
    S.allele_first = af.ctypes.data
    assert call_structs([S], [len(c.read_names)]) == capi.MRP_ERR_ARG


def test_read_index_out_of_range_or_twice_in_a_bubble():
    c = small()
    for bad in (len(c.read_names), -1):
        S, keep = capi.string_chunk_struct(c)
        sr = keep["sub_read"].copy()
        sr[0] = bad
        S.sub_read = sr.ctypes.data
        assert call_structs([S], [len(c.read_names)]) == capi.MRP_ERR_ARG
        assert b"names read" in capi.load().mrp_last_error()
    S, keep = capi.string_chunk_struct(c)
    first = int(np.nonzero(np.diff(keep["sub_first"]) >= 2)[0][0])
    sr = keep["sub_read"].copy()
    k0 = int(keep["sub_first"][first])
    sr[k0 + 1] = sr[k0]
    S.sub_read = sr.ctypes.data
    assert call_structs([S], [len(c.read_names)]) == capi.MRP_ERR_ARG
    assert b"twice" in capi.load().mrp_last_error()


def test_substring_outside_the_pool():
    c = small()
    S, keep = capi.string_chunk_struct(c)
    so = keep["sub_off"].copy()
    so[-1] = keep["pool"].size
    S.sub_off = so.ctypes.data
    assert call_structs([S], [len(c.read_names)]) == capi.MRP_ERR_ARG


def _fingerprint(c):
    return (c.read_names, c.read_forward_strand.tolist(), c.hap.tolist(), c.truth,
            [([a.tobytes() for a in al], list(rs), [s.tobytes() for s in sb]) for al, rs, sb in c.bubbles])


@pytest.mark.parametrize("opts", [dict(), dict(multi_allelic=0.5, duplicate_rate=0.3, sv_sites=2, orphan_reads=4, empty_bubbles=3)])
def test_generator_is_deterministic(opts):
    a = synth.make_string_chunk(seed=5, n_sites=40, coverage=10, **opts)
    b = synth.make_string_chunk(seed=5, n_sites=40, coverage=10, **opts)
    d = synth.make_string_chunk(seed=6, n_sites=40, coverage=10, **opts)
    assert _fingerprint(a) == _fingerprint(b) and _fingerprint(a) != _fingerprint(d)


def test_generator_options():
    c = synth.make_string_chunk(seed=2, n_sites=60, coverage=20, multi_allelic=0.5, duplicate_rate=0.3, sv_sites=2, sv_len=600, orphan_reads=4,
                                empty_bubbles=3)
    n_alleles = [len(al) for al, _rs, _sb in c.bubbles]
    assert set(n_alleles) >= {2, 3, 4}
    assert sum(1 for al, _rs, _sb in c.bubbles if max(len(a) for a in al) > 512) == 2
    assert sum(1 for _al, rs, _sb in c.bubbles if not rs) >= 3
    listed = {r for _al, rs, _sb in c.bubbles for r in rs}
    assert len(c.read_names) - len(listed) >= 4
    dups = sum(len(sb) - len({s.tobytes() for s in sb}) for _al, _rs, sb in c.bubbles)
    assert dups > 10
    for _al, rs, _sb in c.bubbles:
        assert len(rs) == len(set(rs))
