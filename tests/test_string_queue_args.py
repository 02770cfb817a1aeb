"""The work queue over string chunks without a device (mrp_queue_phase_string_chunks, mrp_phase_string_chunks_on_devices,
mrp_string_chunk_units): the symbols, the cost of a chunk, the order the queue gives the chunks (phase.c:257-263), and the
argument checks, which reach the caller before a queue or a device is looked at, in the order of mrp_phase_string_chunks."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth

NEW_SYMBOLS = ("mrp_string_chunk_units", "mrp_queue_phase_string_chunks", "mrp_phase_string_chunks_on_devices")


def small(seed=1):
    return synth.make_string_chunk(seed=seed, n_sites=6, coverage=4, span=(2, 4))


def no_bubbles():
    return synth.StringChunk(bubbles=[], read_names=["lonely_a", "lonely_b"], read_forward_strand=np.array([1, 0], np.uint8), hap=np.zeros(2, int), truth=[])


class Call:
    """one call of either entry over ready-made structs, with outputs the test can look at afterwards"""

    SENTINEL = 0x5A5A5A50  # a non-NULL pattern: `untouched` means the library wrote neither NULL nor a result over it

    def __init__(self, structs, n_reads):
        n = len(structs)
        self.n = n
        self.arr = (capi.StringChunk * max(n, 1))(*structs)
        self.haps = [np.full(max(k, 1), 77, np.int8) for k in n_reads]
        self.hp = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h in self.haps])
        self.res = (C.c_void_p * max(n, 1))(*([self.SENTINEL] * max(n, 1)))
        self.prof = (capi.ProfileOut * max(n, 1))()
        for P in self.prof:
            P.n_seqs = 12345
        self.stats = capi.QueueStats()
        self.stats.batches = 99
        self.model = capi.PairHmm.default_nucleotide()
        self.params = capi.Params.from_reference_names(synth.shipped_phase_params())

    def _tail(self):
        return (self.n, self.arr, C.byref(self.model), C.byref(self.model), 4, 512, 0.0, C.byref(self.params), 0, 0,
                C.cast(self.res, C.POINTER(C.POINTER(capi.PhaseResult))), self.hp, None, self.prof, C.byref(self.stats))

    def queue(self, q=None):
        return capi.load().mrp_queue_phase_string_chunks(q, *self._tail())

    def on_devices(self, devices=(0,)):
        dev = (C.c_int32 * len(devices))(*devices)
        return capi.load().mrp_phase_string_chunks_on_devices(C.cast(dev, C.c_void_p), len(devices), *self._tail())

    def untouched(self):
        return (all(self.res[i] == self.SENTINEL for i in range(self.n)) and all(P.n_seqs == 12345 and not P.pool for P in self.prof)
                and all((h == 77).all() for h in self.haps))


def test_symbols_and_abi_version():
    lib = capi.load()
    for s in NEW_SYMBOLS:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert hasattr(capi.Queue, "phase_string_chunks") and callable(capi.phase_string_chunks_on_devices) and callable(capi.string_chunk_units)


@pytest.mark.parametrize("opts", [dict(), dict(empty_bubbles=3), dict(orphan_reads=4), dict(sv_sites=2), dict(multi_allelic=0.5, duplicate_rate=0.3, empty_bubbles=2,
                                                                                                                  orphan_reads=3, sv_sites=1)])
def test_units_are_the_substrings_of_the_chunk(opts):
    c = synth.make_string_chunk(seed=21, n_sites=40, coverage=10, **opts)
    S, keep = capi.string_chunk_struct(c)
    want = int(np.asarray(keep["sub_first"])[-1])
    assert want == sum(len(rs) for _al, rs, _sb in c.bubbles) > 0
    assert capi.string_chunk_units(c) == want
    assert capi.string_chunk_units(c, struct=(S, keep)) == want


def test_units_of_a_chunk_without_bubbles_and_null_arguments():
    lib = capi.load()
    assert capi.string_chunk_units(no_bubbles()) == 0
    S, keep = capi.string_chunk_struct(small())
    u = C.c_int64(-7)
    assert lib.mrp_string_chunk_units(None, C.byref(u)) == capi.MRP_ERR_ARG
    assert lib.mrp_string_chunk_units(C.byref(S), None) == capi.MRP_ERR_ARG
    T = capi.StringChunk.from_buffer_copy(bytes(S))
    T.sub_first = None
    assert lib.mrp_string_chunk_units(C.byref(T), C.byref(u)) == capi.MRP_ERR_ARG
    assert u.value == -7


def test_queue_order_over_units_is_largest_first_and_stable():
    """ties built on purpose: the same chunk three times, and two different chunks trimmed to the same number of substrings"""
    a = synth.make_string_chunk(seed=3, n_sites=30, coverage=10)
    b = synth.make_string_chunk(seed=4, n_sites=60, coverage=12, empty_bubbles=2)
    d = synth.make_string_chunk(seed=5, n_sites=12, coverage=6, orphan_reads=2)
    chunks = [d, a, no_bubbles(), b, a, d, b, a, no_bubbles()]
    units = np.array([capi.string_chunk_units(c) for c in chunks], dtype=np.int64)
    assert units[2] == units[8] == 0 and units[1] == units[4] == units[7] and units[3] == units[6] > units[1] > units[0] == units[5] > 0
    order, batch = capi.queue_plan(units, 2)
    assert order.tolist() == [3, 6, 1, 4, 7, 0, 5, 2, 8]
    assert order.tolist() == sorted(range(len(chunks)), key=lambda i: (-units[i], i))
    assert batch[order].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4]


def malformed_cases():
    """the malformed chunks of tests/test_string_chunks_args.py: (name, edit of a struct and the arrays it points into)"""
    def null(field):
        def f(S, keep):
            setattr(S, field, None)
        return f

    def not_ascending(S, keep):
        sf = keep["sub_first"].copy()
        sf[2] = sf[3] + 1
        keep["bad"] = sf
        S.sub_first = sf.ctypes.data

    def no_allele(S, keep):
        af = keep["allele_first"].copy()
        af[1] = af[0]
        keep["bad"] = af
        S.allele_first = af.ctypes.data

    def read_out_of_range(S, keep):
        sr = keep["sub_read"].copy()
        sr[0] = S.n_reads
        keep["bad"] = sr
        S.sub_read = sr.ctypes.data

    def read_twice(S, keep):
        first = int(np.nonzero(np.diff(keep["sub_first"]) >= 2)[0][0])
        sr = keep["sub_read"].copy()
        k0 = int(keep["sub_first"][first])
        sr[k0 + 1] = sr[k0]
        keep["bad"] = sr
        S.sub_read = sr.ctypes.data

    def outside_pool(S, keep):
        so = keep["sub_off"].copy()
        so[-1] = keep["pool"].size
        keep["bad"] = so
        S.sub_off = so.ctypes.data

    cases = [(f"null_{f}", null(f)) for f in ("allele_first", "sub_first", "allele_off", "sub_read", "read_names", "read_forward_strand")]
    return cases + [("not_ascending", not_ascending), ("no_allele", no_allele), ("read_out_of_range", read_out_of_range), ("read_twice", read_twice),
                    ("outside_pool", outside_pool)]


@pytest.mark.parametrize("name,edit", malformed_cases(), ids=[n for n, _ in malformed_cases()])
def test_malformed_chunk_in_the_middle_is_an_argument_error_without_a_device(name, edit):
    chunks = [small(1), small(2), small(3), small(4), small(5)]
    built = [capi.string_chunk_struct(c) for c in chunks]
    bad = capi.StringChunk.from_buffer_copy(bytes(built[2][0]))
    edit(bad, built[2][1])
    structs = [b[0] for b in built]
    structs[2] = bad
    n_reads = [len(c.read_names) for c in chunks]
    for entry in ("queue", "on_devices"):
        call = Call(structs, n_reads)
        rc = call.queue(None) if entry == "queue" else call.on_devices()
        assert rc == capi.MRP_ERR_ARG, (entry, name)
        assert b"chunk 2" in capi.load().mrp_last_error(), (entry, capi.load().mrp_last_error())
        assert call.untouched() and call.stats.batches == 99, entry


def test_bad_call_arguments_come_before_the_queue():
    c = small()
    S, _keep = capi.string_chunk_struct(c)
    lib = capi.load()
    call = Call([S], [len(c.read_names)])
    tail = list(call._tail())
    for idx in (2, 3, 7, 10, 11):  # forward model, reverse model, params, out, hap_out
        t = list(tail)
        t[idx] = None
        assert lib.mrp_queue_phase_string_chunks(None, *t) == capi.MRP_ERR_ARG, idx
    t = list(tail)
    t[4] = 3  # an odd diagonalExpansion
    assert lib.mrp_queue_phase_string_chunks(None, *t) == capi.MRP_ERR_ARG
    assert call.untouched()


def test_well_formed_chunks_and_no_queue_fail_loudly():
    chunks = [small(1), no_bubbles(), small(2)]
    built = [capi.string_chunk_struct(c) for c in chunks]
    call = Call([b[0] for b in built], [len(c.read_names) for c in chunks])
    assert call.queue(None) == capi.MRP_ERR_NO_DEVICE
    assert b"no CPU fallback" in capi.load().mrp_last_error()
    assert call.untouched() and call.stats.batches == 99
