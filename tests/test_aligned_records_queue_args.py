"""mrp_queue_phase_aligned_chunks_with_records and its *_on_devices form without a device: the symbols, and the argument checks, which
reach the caller before a queue or a device is looked at, in the order of mrp_queue_phase_aligned_chunks_with_filtered -- MRP_ERR_ARG (a NULL
records_out among the null arguments), then MRP_ERR_UNSUPPORTED for the refused extraction modes, then MRP_ERR_NO_DEVICE.  Up to there
nothing is written."""
import ctypes as C

import pytest

from margin_amd import capi
from tests.test_aligned_queue_args import Call, built, malformed_cases, no_variants, synthetic  # noqa: F401  (the six 8 kb / 8x chunks)

NEW_SYMBOLS = ("mrp_queue_phase_aligned_chunks_with_records", "mrp_phase_aligned_chunks_with_records_on_devices")
ENTRIES = ("queue", "on_devices")


class RecordsCall(Call):
    """tests/test_aligned_queue_args.Call with records_out and the records' stats behind it"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.recs = (capi.VariantRecords * max(self.n, 1))()
        for R in self.recs:
            R.n_primary = 31337
        self.rstats = capi.QueueRecordsStats()
        self.rstats.records_sites = 77
        self.null_records = False

    def tail(self):
        t = list(self._tail(True))
        return t[:-1] + [None if self.null_records else self.recs, t[-1], C.byref(self.rstats)]

    def run(self, entry, q=None, devices=(0,)):
        L = capi.load()
        if entry == "queue":
            return L.mrp_queue_phase_aligned_chunks_with_records(q, *self.tail())
        dev = (C.c_int32 * len(devices))(*devices)
        return L.mrp_phase_aligned_chunks_with_records_on_devices(C.cast(dev, C.c_void_p), len(devices), *self.tail())

    def untouched(self):
        return super().untouched() and all(R.n_primary == 31337 and not R.state and not R.reads for R in self.recs) and self.rstats.records_sites == 77


def test_symbols_and_abi_version():
    lib = capi.load()
    for s in NEW_SYMBOLS:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.QueueRecordsStats) == 5 * 8
    assert len(lib.mrp_queue_phase_aligned_chunks_with_records.argtypes) == len(lib.mrp_queue_phase_aligned_chunks_with_filtered.argtypes) + 2
    assert len(lib.mrp_phase_aligned_chunks_with_records_on_devices.argtypes) == len(lib.mrp_phase_aligned_chunks_with_filtered_on_devices.argtypes) + 2
    assert hasattr(capi.Queue, "phase_aligned_chunks_with_records") and callable(capi.phase_aligned_chunks_with_records_on_devices)


def test_null_records_out_is_an_argument_error_before_everything_else(synthetic):  # noqa: F811
    _whole, chunks, rests = synthetic
    for entry in ENTRIES:
        for options in (None, dict(capi.shipped_extract_options(), indel_size_for_sv_handling=1)):  # ... before a refused mode too
            structs, rest_structs = built(chunks[:3], rests[:3])
            call = RecordsCall(chunks[:3], structs, rest_structs, options=options)
            call.null_records = True
            assert call.run(entry) == capi.MRP_ERR_ARG, (entry, options)
            assert b"null argument" in capi.load().mrp_last_error() and NEW_SYMBOLS[ENTRIES.index(entry)].encode() in capi.load().mrp_last_error()
            assert call.untouched(), entry


def test_the_other_null_arguments(synthetic):  # noqa: F811
    _whole, chunks, rests = synthetic
    structs, rest_structs = built(chunks[:2], rests[:2])
    lib = capi.load()
    call = RecordsCall(chunks[:2], structs, rest_structs)
    for idx in (2, 3, 5, 6, 7, 11, 14, 15, 19, 20, 21):  # rest, read_names, ..., filtered_out, filtered_read_out, records_out
        t = call.tail()
        t[idx] = None
        assert lib.mrp_queue_phase_aligned_chunks_with_records(None, *t) == capi.MRP_ERR_ARG, idx
    # the two stats are optional: with both NULL the well-formed call gets as far as the queue
    t = call.tail()
    t[22] = t[23] = None
    assert lib.mrp_queue_phase_aligned_chunks_with_records(None, *t) == capi.MRP_ERR_NO_DEVICE
    assert call.untouched()


@pytest.mark.parametrize("name,filtered_only,edit,message", malformed_cases(), ids=[c[0] for c in malformed_cases()])
def test_malformed_chunk_in_the_middle_has_with_filtered_s_message(synthetic, name, filtered_only, edit, message):  # noqa: F811
    _whole, chunks, rests = synthetic
    chunks, rests = chunks[:5], rests[:5]
    for entry in ENTRIES:
        for options in (None, dict(capi.shipped_extract_options(), use_run_length_encoding=1)):
            structs, rest_structs = built(chunks, rests)
            call = RecordsCall(chunks, structs, rest_structs, options=options)
            S = capi.AlignedChunk.from_buffer_copy(bytes(structs[2][0]))
            R = capi.AlignedChunkRest.from_buffer_copy(bytes(rest_structs[2][0]))
            edit(call, S, structs[2][1], R, rest_structs[2][1])
            call.arr[2], call.rarr[2] = S, R
            call.per_batch = 2
            assert call.run(entry) == capi.MRP_ERR_ARG, (entry, name)
            assert message in capi.load().mrp_last_error(), (entry, capi.load().mrp_last_error())
            assert call.untouched(), entry


def test_refused_modes_then_the_queue(synthetic):  # noqa: F811
    _whole, chunks, rests = synthetic
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        for entry in ENTRIES:
            structs, rest_structs = built(chunks[:3], rests[:3])
            call = RecordsCall(chunks[:3], structs, rest_structs, options=dict(capi.shipped_extract_options(), **{mode: 1}))
            assert call.run(entry) == capi.MRP_ERR_UNSUPPORTED, (mode, entry)
            assert call.untouched(), (mode, entry)
    # well-formed chunks (one without variants among them) and no queue
    nov = no_variants()
    seq = [chunks[0], nov, chunks[1]]
    structs, rest_structs = built(seq, [rests[0], (nov, []), rests[1]])
    call = RecordsCall(seq, structs, rest_structs)
    assert call.run("queue", q=None) == capi.MRP_ERR_NO_DEVICE
    assert b"no CPU fallback" in capi.load().mrp_last_error() and b"mrp_queue_phase_aligned_chunks_with_records" in capi.load().mrp_last_error()
    assert call.untouched()
    # no chunk and no queue, as for the twins
    call = RecordsCall([], [], [])
    assert call.run("queue", q=None) == capi.MRP_ERR_NO_DEVICE and call.untouched()
    call.null_records = True  # (no chunk: no array is needed)
    assert call.run("queue", q=None) == capi.MRP_ERR_NO_DEVICE


def test_the_binding_checks_the_same(synthetic):  # noqa: F811
    _whole, chunks, rests = synthetic
    f = capi.PairHmm.default_nucleotide()
    p = call_params()
    with pytest.raises(capi.MrpError) as e:  # (the binding asserts: no output written, filtered_out and records_out zeroed)
        capi._phase_aligned(None, chunks[:2], f, f, p, rests=rests[:2], with_rest=True, with_records=True, queue=None, nulls=("records_out",))
    assert e.value.code == capi.MRP_ERR_ARG
    with pytest.raises(capi.MrpError) as e:
        capi._phase_aligned(None, chunks[:2], f, f, p, rests=rests[:2], with_rest=True, with_records=True, queue=None)
    assert e.value.code == capi.MRP_ERR_NO_DEVICE


def call_params():
    from margin_amd import synth
    return capi.Params.from_reference_names(synth.shipped_phase_params())
