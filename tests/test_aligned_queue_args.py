"""The work queue over aligned chunks without a device (mrp_queue_phase_aligned_chunks, mrp_queue_phase_aligned_chunks_with_filtered, their
*_on_devices forms, mrp_aligned_chunk_units): the symbols, the cost of a chunk, the order the queue gives the chunks (phase.c:257-263),
and the argument checks, which reach the caller before a queue or a device is looked at, in the order of the one call:
MRP_ERR_ARG, then MRP_ERR_UNSUPPORTED for the refused extraction modes, then MRP_ERR_NO_DEVICE.  Up to there nothing is written."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import rest_cases as rc

NEW_SYMBOLS = ("mrp_aligned_chunk_units", "mrp_queue_phase_aligned_chunks", "mrp_queue_phase_aligned_chunks_with_filtered",
               "mrp_phase_aligned_chunks_on_devices", "mrp_phase_aligned_chunks_with_filtered_on_devices")
INT64_MAX = 2 ** 63 - 1


@pytest.fixture(scope="module")
def synthetic():
    """the six 8 kb / 8x chunks -> (whole chunks, primary chunks, rests (filtered chunk, gt))"""
    whole, chunks, rests = [], [], []
    for seed in range(6):
        w = rc.synthetic(seed)
        primary, filtered, _ = rc.split_variants(w)
        whole.append(w)
        chunks.append(primary)
        rests.append((filtered, rc.genotypes(filtered, seed)))
    return whole, chunks, rests


def no_variants():
    return ec.make([], [(100, "20M", 60, 0)])


def formula(chunk, rest=None) -> int:
    """floor(B * V / L) in Python integers, clamped to INT64_MAX"""
    b = sum(int(x) for x in chunk.l_qseq)
    v = len(chunk.alleles) + (len(rest.alleles) if rest is not None else 0)
    return min(INT64_MAX, b * v // max(1, int(chunk.overlap_end) - int(chunk.overlap_start)))


class Call:
    """one call of any of the four entries over ready-made structs, with outputs the test can look at afterwards"""

    SENTINEL = 0x5A5A5A50  # a non-NULL pattern: `untouched` means the library wrote neither NULL nor a result over it

    def __init__(self, chunks, structs, rest_structs=None, options=None, expansion=4):
        n = self.n = len(structs)
        m = max(n, 1)
        self.structs, self.rest_structs = structs, rest_structs
        self.arr = (capi.AlignedChunk * m)(*[s[0] for s in structs])
        self.rarr = None if rest_structs is None else (capi.AlignedChunkRest * m)(*[r[0] for r in rest_structs])
        nr = [int(s[0].n_reads) for s in structs]
        self.names = [[s.encode() for s in c.read_names] for c in chunks]
        self.name_arrs = [(C.c_char_p * max(len(x), 1))(*x) for x in self.names]
        self.name_ptrs = (C.c_void_p * m)(*[C.cast(a, C.c_void_p) if k else None for a, k in zip(self.name_arrs, nr)])
        self.haps = [np.full(max(k, 1), 77, np.int8) for k in nr]
        self.hp = (C.c_void_p * m)(*[h.ctypes.data for h in self.haps])
        self.res = (C.c_void_p * m)(*([self.SENTINEL] * m))
        self.bv = (C.c_void_p * m)(*([self.SENTINEL] * m))
        self.fr = (C.c_void_p * m)(*([self.SENTINEL] * m))
        self.prof = (capi.ProfileOut * m)()
        for P in self.prof:
            P.n_seqs = 12345
        self.fout = (capi.FilteredOut * m)()
        for O in self.fout:
            O.n_reads = 4242
        self.stats = capi.QueueStats()
        self.stats.batches = 99
        self.model = capi.PairHmm.default_nucleotide()
        self.params = capi.Params.from_reference_names(synth.shipped_phase_params())
        self.opt = capi.ExtractOptions.from_dict(options or capi.shipped_extract_options())
        self.expansion = expansion
        self.sv_threshold = 512
        self.per_batch = 0

    def _tail(self, filtered):
        head = (self.n, self.arr) + ((self.rarr,) if filtered else ())
        outs = (C.cast(self.res, C.POINTER(C.POINTER(capi.PhaseResult))), self.hp, None, self.prof, self.bv) + ((self.fout, self.fr) if filtered else ())
        return head + (self.name_ptrs, None, C.byref(self.opt), C.byref(self.model), C.byref(self.model), self.expansion, self.sv_threshold, 0.0, C.byref(self.params), 0,
                       self.per_batch) + outs + (C.byref(self.stats),)

    def run(self, entry, filtered, q=None, devices=(0,)):
        L = capi.load()
        if entry == "queue":
            fn = L.mrp_queue_phase_aligned_chunks_with_filtered if filtered else L.mrp_queue_phase_aligned_chunks
            return fn(q, *self._tail(filtered))
        dev = (C.c_int32 * len(devices))(*devices)
        fn = L.mrp_phase_aligned_chunks_with_filtered_on_devices if filtered else L.mrp_phase_aligned_chunks_on_devices
        return fn(C.cast(dev, C.c_void_p), len(devices), *self._tail(filtered))

    def untouched(self):
        return (all(self.res[i] == self.bv[i] == self.fr[i] == self.SENTINEL for i in range(self.n)) and all(P.n_seqs == 12345 and not P.pool for P in self.prof)
                and all(O.n_reads == 4242 and not O.read_hap for O in self.fout) and all((h == 77).all() for h in self.haps) and self.stats.batches == 99)


ENTRIES = [(e, f) for e in ("queue", "on_devices") for f in (False, True)]


def built(chunks, rests):
    return [capi.aligned_chunk_struct(c) for c in chunks], [capi.aligned_chunk_rest_struct(f, g) for f, g in rests]


def test_symbols_and_abi_version():
    lib = capi.load()
    for s in NEW_SYMBOLS:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert hasattr(capi.Queue, "phase_aligned_chunks") and hasattr(capi.Queue, "phase_aligned_chunks_with_filtered")
    assert callable(capi.phase_aligned_chunks_on_devices) and callable(capi.phase_aligned_chunks_with_filtered_on_devices) and callable(capi.aligned_chunk_units)


def test_units_are_what_uniform_coverage_gives(synthetic):
    whole, chunks, rests = synthetic
    for w, c, (f, gt) in zip(whole, chunks, rests):
        assert capi.aligned_chunk_units(c) == formula(c) > 0
        assert capi.aligned_chunk_units(c, (f, gt)) == formula(c, f) == formula(w) > formula(c)
    assert capi.aligned_chunk_units(no_variants()) == 0
    assert capi.aligned_chunk_units(ec.make([ec.SNP110], [])) == 0
    assert capi.aligned_chunk_units(ec.make([], [])) == 0
    # a chunk without variants of its own still costs its rest's
    some = ec.make([ec.SNP110], [(100, "20M", 60, 0), (100, "40M", 60, 0)])
    assert capi.aligned_chunk_units(no_variants(), some) == 20 * 1 // 40 == 0 and capi.aligned_chunk_units(some, some) == 60 * 2 // 40 == 3


def test_units_clamp_to_int64_max():
    """the product runs in 128 bits: 2^31 bases x 2^40 variants over one base"""
    S, keep = capi.aligned_chunk_struct(ec.make([ec.SNP110], [(100, "20M", 60, 0)]))
    keep["big"] = np.array([2 ** 31 - 1], np.int32)
    S.l_qseq = keep["big"].ctypes.data
    S.n_variants = 2 ** 40
    S.overlap_end = S.overlap_start + 1
    assert capi.aligned_chunk_units(None, struct=(S, keep)) == INT64_MAX
    S.overlap_end = S.overlap_start  # L = max(1, 0)
    assert capi.aligned_chunk_units(None, struct=(S, keep)) == INT64_MAX
    S.n_variants = 3
    assert capi.aligned_chunk_units(None, struct=(S, keep)) == 3 * (2 ** 31 - 1)


def unit_arg_cases():
    def edit(**fields):
        def f(S, R, keep):
            for k, v in fields.items():
                setattr(S, k, v)
        return f

    def negative_rest(S, R, keep):
        R.n_variants = -1

    def negative_l_qseq(S, R, keep):
        keep["bad"] = keep["l_qseq"].copy()
        keep["bad"][-1] = -1
        S.l_qseq = keep["bad"].ctypes.data

    def ends_before_it_starts(S, R, keep):
        S.overlap_end = S.overlap_start - 1

    return [("negative_n_reads", edit(n_reads=-1)), ("negative_n_variants", edit(n_variants=-1)), ("negative_rest_variants", negative_rest),
            ("overlap_end_before_start", ends_before_it_starts), ("null_l_qseq", edit(l_qseq=None)), ("negative_l_qseq", negative_l_qseq)]


@pytest.mark.parametrize("name,edit", unit_arg_cases(), ids=[n for n, _ in unit_arg_cases()])
def test_units_argument_errors_leave_the_output_alone(name, edit):
    lib = capi.load()
    chunk = ec.make([ec.SNP110], [(100, "20M", 60, 0), (100, "40M", 60, 0)])
    S, keep = capi.aligned_chunk_struct(chunk)
    R, rkeep = capi.aligned_chunk_rest_struct(chunk, [(0, 1)])
    u = C.c_int64(-7)
    assert lib.mrp_aligned_chunk_units(C.byref(S), C.byref(R), C.byref(u)) == capi.MRP_OK and u.value == 3
    u = C.c_int64(-7)
    edit(S, R, keep)
    assert lib.mrp_aligned_chunk_units(C.byref(S), C.byref(R), C.byref(u)) == capi.MRP_ERR_ARG, name
    assert u.value == -7


def test_units_null_arguments():
    lib = capi.load()
    S, keep = capi.aligned_chunk_struct(ec.make([ec.SNP110], [(100, "20M", 60, 0)]))
    u = C.c_int64(-7)
    assert lib.mrp_aligned_chunk_units(None, None, C.byref(u)) == capi.MRP_ERR_ARG and u.value == -7
    assert lib.mrp_aligned_chunk_units(C.byref(S), None, None) == capi.MRP_ERR_ARG


def test_queue_order_over_units_is_largest_first_and_stable(synthetic):
    """ties built on purpose: the same chunk three times, two chunks twice, and a chunk without variants twice"""
    _whole, chunks, _rests = synthetic
    d, a, b = sorted(chunks[:3], key=capi.aligned_chunk_units)
    seq = [d, a, no_variants(), b, a, d, b, a, no_variants()]
    units = np.array([capi.aligned_chunk_units(c) for c in seq], dtype=np.int64)
    assert units[2] == units[8] == 0 and units[1] == units[4] == units[7] and units[3] == units[6] > units[1] > units[0] == units[5] > 0
    order, batch = capi.queue_plan(units, 2)
    assert order.tolist() == [3, 6, 1, 4, 7, 0, 5, 2, 8]
    assert order.tolist() == sorted(range(len(seq)), key=lambda i: (-units[i], i))
    assert batch[order].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4]


def malformed_cases():
    """(name, filtered entries only, edit of chunk 2's struct / its rest's / the call, what the message names)"""
    def not_ascending(call, S, keep, R, rkeep):
        vp = keep["variant_pos"].copy()
        v = int(np.flatnonzero(np.diff(vp) > 0)[0])
        vp[v], vp[v + 1] = vp[v + 1], vp[v]
        keep["bad"] = vp
        S.variant_pos = vp.ctypes.data

    def cigar_query_length(call, S, keep, R, rkeep):
        lq = keep["l_qseq"].copy()
        lq[0] -= 1
        keep["bad"] = lq
        S.l_qseq = lq.ctypes.data

    def null_read_name(call, S, keep, R, rkeep):
        call.name_arrs[2][0] = None

    def gt_outside(call, S, keep, R, rkeep):
        gt = rkeep["gt"].copy()
        gt[1] = 99
        rkeep["bad"] = gt
        R.gt = gt.ctypes.data

    def rest_not_ascending(call, S, keep, R, rkeep):
        vp = rkeep["variant_pos"].copy()
        v = int(np.flatnonzero(np.diff(vp) > 0)[0])
        vp[v], vp[v + 1] = vp[v + 1], vp[v]
        rkeep["bad"] = vp
        R.variant_pos = vp.ctypes.data

    def odd_expansion(call, S, keep, R, rkeep):
        call.expansion = 3

    return [("variants_not_ascending", False, not_ascending, b"chunk 2: variants not ascending"),
            ("cigar_query_length", False, cigar_query_length, b"chunk 2: read 0: CIGAR query length is not l_qseq"),
            ("null_read_name", False, null_read_name, b"chunk 2: read 0 has no name"),
            ("gt_outside_the_alleles", True, gt_outside, b"chunk 2, filtered variant 0: genotype 99"),
            ("rest_variants_not_ascending", True, rest_not_ascending, b"chunk 7: variants not ascending"),  # the one call's "chunk n_chunks + c"
            ("odd_expansion", False, odd_expansion, b"diagonalExpansion must be even")]


@pytest.mark.parametrize("name,filtered_only,edit,message", malformed_cases(), ids=[c[0] for c in malformed_cases()])
@pytest.mark.parametrize("unsupported_too", [False, True])
def test_malformed_chunk_in_the_middle_is_an_argument_error_without_a_device(synthetic, name, filtered_only, edit, message, unsupported_too):
    """... and comes before a refused mode"""
    _whole, chunks, rests = synthetic
    chunks, rests = chunks[:5], rests[:5]
    options = dict(capi.shipped_extract_options(), indel_size_for_sv_handling=1) if unsupported_too else None
    for entry, filtered in ENTRIES:
        if filtered_only and not filtered:
            continue
        structs, rest_structs = built(chunks, rests)
        call = Call(chunks, structs, rest_structs, options=options)
        S = capi.AlignedChunk.from_buffer_copy(bytes(structs[2][0]))
        R = capi.AlignedChunkRest.from_buffer_copy(bytes(rest_structs[2][0]))
        edit(call, S, structs[2][1], R, rest_structs[2][1])
        call.arr[2], call.rarr[2] = S, R
        call.per_batch = 2
        rc_ = call.run(entry, filtered)
        err = capi.load().mrp_last_error()
        assert rc_ == capi.MRP_ERR_ARG, (entry, filtered, name, err)
        assert message in err, (entry, filtered, err)
        assert call.untouched(), (entry, filtered)


def test_bad_call_arguments_come_before_the_queue(synthetic):
    _whole, chunks, rests = synthetic
    structs, rest_structs = built(chunks[:2], rests[:2])
    lib = capi.load()
    call = Call(chunks[:2], structs, rest_structs)
    plain, filtered = list(call._tail(False)), list(call._tail(True))
    for idx in (2, 4, 5, 6, 10, 13, 14):  # read_names, options, forward model, reverse model, params, out, hap_out
        t = list(plain)
        t[idx] = None
        assert lib.mrp_queue_phase_aligned_chunks(None, *t) == capi.MRP_ERR_ARG, idx
    for idx in (2, 3, 5, 6, 7, 11, 14, 15, 19, 20):  # rest, ..., filtered_out, filtered_read_out
        t = list(filtered)
        t[idx] = None
        assert lib.mrp_queue_phase_aligned_chunks_with_filtered(None, *t) == capi.MRP_ERR_ARG, idx
    assert call.untouched()


def test_refused_modes_need_neither_queue_nor_device(synthetic):
    _whole, chunks, rests = synthetic
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        for entry, filtered in ENTRIES:
            structs, rest_structs = built(chunks[:3], rests[:3])
            call = Call(chunks[:3], structs, rest_structs, options=dict(capi.shipped_extract_options(), **{mode: 1}))
            assert call.run(entry, filtered) == capi.MRP_ERR_UNSUPPORTED, (mode, entry, filtered)
            assert call.untouched(), (mode, entry, filtered)


def test_well_formed_chunks_and_no_queue_fail_loudly(synthetic):
    _whole, chunks, rests = synthetic
    seq = [chunks[0], no_variants(), chunks[1]]
    nov = no_variants()
    rs = [rests[0], (nov, np.zeros((0, 2), np.int32)), rests[1]]
    for filtered in (False, True):
        structs, rest_structs = built(seq, rs)
        call = Call(seq, structs, rest_structs)
        assert call.run("queue", filtered, q=None) == capi.MRP_ERR_NO_DEVICE
        assert b"no CPU fallback" in capi.load().mrp_last_error()
        assert call.untouched()


def test_no_chunk_and_no_queue_is_no_device_as_for_strings():
    """mrp_queue_phase_string_chunks checks its (empty) chunk list, then looks for the queue: MRP_ERR_NO_DEVICE.  The aligned twins do
    the same; with a queue, no chunk is MRP_OK with zeroed stats (tests/test_gpu_aligned_queue.py)."""
    from tests.test_string_queue_args import Call as StringCall
    assert StringCall([], []).queue(None) == capi.MRP_ERR_NO_DEVICE
    for filtered in (False, True):
        call = Call([], [], [])
        assert call.run("queue", filtered, q=None) == capi.MRP_ERR_NO_DEVICE
        assert call.stats.batches == 99
