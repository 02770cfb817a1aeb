"""The work queue over haplotagging aligned chunks without a device (mrp_queue_haplotag_aligned_chunks, mrp_haplotag_aligned_chunks_on_devices,
mrp_haplotag_chunk_units): the symbols, the cost of a chunk (bases x het variants / overlap length), and the argument checks, which reach
the caller before a queue or a device is looked at, in the order and with the messages of the one call (mrp_haplotag_aligned_chunks with a
NULL context): MRP_ERR_ARG, then MRP_ERR_UNSUPPORTED for the refused extraction modes, then MRP_ERR_NO_DEVICE.  Up to there nothing is
written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import haplotag_aligned_oracle as hao

NEW_SYMBOLS = ("mrp_haplotag_chunk_units", "mrp_queue_haplotag_aligned_chunks", "mrp_haplotag_aligned_chunks_on_devices")
INT64_MAX = 2 ** 63 - 1
INT32_MAX = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def synthetic():
    chunks = [synth.make_aligned_chunk(seed, overlap_bp=8_000, coverage=8.0) for seed in range(5)]
    return chunks, [hao.draw_genotypes(c, seed) for seed, c in enumerate(chunks)]


def formula(chunk, gt) -> int:
    """floor(B * H / L) in Python integers, clamped to INT64_MAX"""
    b = sum(int(x) for x in chunk.l_qseq)
    g = np.asarray(gt).reshape(-1, 2)
    h = int((g[:, 0] != g[:, 1]).sum())
    return min(INT64_MAX, b * h // max(1, int(chunk.overlap_end) - int(chunk.overlap_start)))


def shaped(l_qseq, n_variants, length):
    """a struct with the fields the units read: the reads' lengths, the variant count, the overlap"""
    S, keep = capi.aligned_chunk_struct(ec.make([ec.SNP110], [(100, "20M", 60, 0)]))
    keep["lens"] = np.ascontiguousarray(l_qseq, np.int32)
    S.n_reads = keep["lens"].size
    S.l_qseq = keep["lens"].ctypes.data if keep["lens"].size else None
    S.n_variants = n_variants
    S.overlap_start, S.overlap_end = 1_000, 1_000 + length
    return S, keep


def units(S, gt):
    g = None if gt is None else np.ascontiguousarray(gt, np.int32).reshape(-1)
    u = C.c_int64(-7)
    rc_ = capi.load().mrp_haplotag_chunk_units(C.byref(S), None if g is None else g.ctypes.data, C.byref(u))
    return rc_, int(u.value)


def test_symbols_and_abi_version():
    lib = capi.load()
    for s in NEW_SYMBOLS:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6
    assert hasattr(capi.Queue, "haplotag_aligned_chunks") and callable(capi.haplotag_aligned_chunks_on_devices) and callable(capi.haplotag_chunk_units)
    with open(os.path.join(ROOT, "include", "margin_rphmm.h")) as f:
        header = f.read()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header, s


def test_units_known_answers():
    het3 = [[0, 1], [1, 1], [1, 0], [0, 0], [2, 1]]
    S, _keep = shaped([400, 600], 5, 100)
    assert units(S, het3) == (capi.MRP_OK, 30)
    assert units(S, [[1, 1]] * 5) == (capi.MRP_OK, 0)                    # all homozygous: nothing is scored
    S.overlap_end = S.overlap_start                                       # L = max(1, 0)
    assert units(S, het3) == (capi.MRP_OK, 3_000)
    S.overlap_end = S.overlap_start + 7                                   # floor
    assert units(S, het3) == (capi.MRP_OK, 3_000 // 7)
    S, _keep = shaped([400, 600], 0, 100)
    assert units(S, None) == (capi.MRP_OK, 0)                             # no variants, NULL gt
    S, _keep = shaped([], 5, 100)
    assert units(S, het3) == (capi.MRP_OK, 0)                             # no reads
    # genotypes are compared, never range-checked
    S, _keep = shaped([100], 2, 10)
    assert units(S, [[-5, 99], [7, 7]]) == (capi.MRP_OK, 10)


def test_units_of_the_synthetic_chunks(synthetic):
    chunks, gts = synthetic
    for c, g in zip(chunks, gts):
        assert capi.haplotag_chunk_units(c, g) == formula(c, g) > 0
        assert formula(c, g) < capi.aligned_chunk_units(c)               # some variants are homozygous
        assert capi.haplotag_chunk_units(c, np.zeros_like(g)) == 0
    assert capi.haplotag_chunk_units(ec.make([], [(100, "20M", 60, 0)]), None) == 0


def test_units_clamp_to_int64_max():
    """the product runs in 128 bits: 4 096 reads of INT32_MAX bases x 2^21 het variants over one base is 2^64 - 2^33"""
    n_var = 2 ** 21
    gt = np.zeros((n_var, 2), np.int32)
    gt[:, 1] = 1
    S, _keep = shaped(np.full(4_096, INT32_MAX, np.int32), n_var, 1)
    assert 4_096 * INT32_MAX * n_var > INT64_MAX
    assert units(S, gt) == (capi.MRP_OK, INT64_MAX)
    S.overlap_end = S.overlap_start
    assert units(S, gt) == (capi.MRP_OK, INT64_MAX)
    gt[4:, 1] = 0                                                         # four het variants left: far below the clamp
    assert units(S, gt) == (capi.MRP_OK, 4 * 4_096 * INT32_MAX)
    S.overlap_end = S.overlap_start + 2 ** 20
    assert units(S, gt) == (capi.MRP_OK, 4 * 4_096 * INT32_MAX // 2 ** 20)


def unit_arg_cases():
    def edit(**fields):
        def f(S, keep):
            for k, v in fields.items():
                setattr(S, k, v)
            return True
        return f

    def negative_l_qseq(S, keep):
        keep["lens"][-1] = -1
        return True

    def ends_before_it_starts(S, keep):
        S.overlap_end = S.overlap_start - 1
        return True

    def null_gt(S, keep):
        return False  # (pass no genotypes)

    return [("negative_n_reads", edit(n_reads=-1)), ("negative_n_variants", edit(n_variants=-1)), ("overlap_end_before_start", ends_before_it_starts),
            ("null_l_qseq", edit(l_qseq=None)), ("negative_l_qseq", negative_l_qseq), ("null_gt_with_variants", null_gt)]


@pytest.mark.parametrize("name,edit", unit_arg_cases(), ids=[n for n, _ in unit_arg_cases()])
def test_units_argument_errors_leave_the_output_alone(name, edit):
    gt = [[0, 1], [1, 0]]
    S, keep = shaped([20, 40], 2, 40)
    assert units(S, gt) == (capi.MRP_OK, 3)
    with_gt = edit(S, keep)
    assert units(S, gt if with_gt else None) == (capi.MRP_ERR_ARG, -7), name


def test_units_null_arguments():
    lib = capi.load()
    S, _keep = shaped([20], 0, 40)
    u = C.c_int64(-7)
    assert lib.mrp_haplotag_chunk_units(None, None, C.byref(u)) == capi.MRP_ERR_ARG and u.value == -7
    assert lib.mrp_haplotag_chunk_units(C.byref(S), None, None) == capi.MRP_ERR_ARG


def test_queue_order_over_het_units_is_largest_first_and_stable(synthetic):
    """ties built on purpose: a chunk twice, and two chunks that cost nothing (all homozygous; no variants)"""
    chunks, gts = synthetic
    nov = ec.make([], [(100, "20M", 60, 0)])
    seq = [(chunks[0], gts[0]), (chunks[1], np.zeros_like(gts[1])), (chunks[2], gts[2]), (chunks[0], gts[0]), (nov, None), (chunks[3], gts[3])]
    u = np.array([capi.haplotag_chunk_units(c, g) for c, g in seq], dtype=np.int64)
    assert u[0] == u[3] > 0 and u[1] == u[4] == 0
    order, batch = capi.queue_plan(u, 2)
    assert order.tolist() == sorted(range(len(seq)), key=lambda i: (-u[i], i))
    assert order.tolist().index(0) + 1 == order.tolist().index(3) and order.tolist()[-2:] == [1, 4]
    assert batch[order].tolist() == [0, 0, 1, 1, 2, 2]


class Call:
    """one call of either new entry, or of the one call with a NULL context, over ready-made structs, with outputs and stats filled with
    sentinel bytes the test can look at afterwards"""

    def __init__(self, structs, gts, options=None, expansion=4):
        n = self.n = len(structs)
        m = max(n, 1)
        self.structs = structs
        self.arr = (capi.AlignedChunk * m)(*[s[0] for s in structs])
        self.garr, self.gkeep = capi._genotype_arrays(gts)
        nr = [int(s[0].n_reads) for s in structs]
        self.haps = [np.full(max(k, 1), 77, np.int8) for k in nr]
        self.h1s = [np.full(max(k, 1), -123.5) for k in nr]
        self.h2s = [np.full(max(k, 1), -321.5) for k in nr]
        ptrs = lambda arrays: (C.c_void_p * m)(*[a.ctypes.data if k else None for a, k in zip(arrays, nr)])
        self.hp, self.p1, self.p2 = ptrs(self.haps), ptrs(self.h1s), ptrs(self.h2s)
        self.stats = capi.QueueStats()
        C.memset(C.byref(self.stats), 0x5A, C.sizeof(self.stats))
        self.stats_before = bytes(self.stats)
        self.fwd = capi.PairHmm.default_nucleotide()
        self.rev = capi.PairHmm.default_nucleotide()
        self.opt = capi.ExtractOptions.from_dict(options or capi.shipped_extract_options())
        self.expansion = expansion
        self.per_batch = 2
        self.n_chunks = n
        self.nulls = set()

    def _args(self, queued):
        z = lambda name, v: None if name in self.nulls else v
        head = (self.n_chunks, z("chunks", self.arr), z("gt", self.garr), z("options", C.byref(self.opt)), z("forward_model", C.byref(self.fwd)),
                z("reverse_model", C.byref(self.rev)), self.expansion)
        outs = (z("hap_out", self.hp), z("h1_out", self.p1), z("h2_out", self.p2))
        return head + ((self.per_batch,) if queued else ()) + outs

    def run(self, entry, q=None, devices=(0,)):
        """-> (status, message)"""
        L = capi.load()
        if entry == "one_call":
            st = capi.HaplotagAlignedStats()
            rc_ = L.mrp_haplotag_aligned_chunks(None, *self._args(False), C.byref(st))
        elif entry == "queue":
            rc_ = L.mrp_queue_haplotag_aligned_chunks(q, *self._args(True), C.byref(self.stats))
        else:
            dev = (C.c_int32 * len(devices))(*devices)
            rc_ = L.mrp_haplotag_aligned_chunks_on_devices(C.cast(dev, C.c_void_p), len(devices), *self._args(True), C.byref(self.stats))
        return rc_, L.mrp_last_error()

    def untouched(self):
        return (all((h == 77).all() for h in self.haps) and all((x == -123.5).all() for x in self.h1s) and all((x == -321.5).all() for x in self.h2s)
                and bytes(self.stats) == self.stats_before)


ENTRIES = ("queue", "on_devices")
NO_SUCH_DEVICE = (99,)


def malformed_cases():
    """(name, edit of the call -- chunk 2 is the one in the middle --, what the message names)"""
    def not_ascending(call):
        S, keep = call.structs[2]
        vp = keep["variant_pos"].copy()
        v = int(np.flatnonzero(np.diff(vp) > 0)[0])
        vp[v], vp[v + 1] = vp[v + 1], vp[v]
        keep["bad"] = vp
        call.arr[2].variant_pos = vp.ctypes.data

    def cigar_query_length(call):
        S, keep = call.structs[2]
        lq = keep["l_qseq"].copy()
        lq[0] -= 1
        keep["bad"] = lq
        call.arr[2].l_qseq = lq.ctypes.data

    def null(name):
        def f(call):
            call.nulls.add(name)
        return f

    def null_entry(array_name):
        def f(call):
            getattr(call, array_name)[2] = None
        return f

    def gt_outside(value):
        def f(call):
            g = call.gkeep[2].copy()
            g[2 * 3 + 1] = value
            call.gkeep.append(g)
            call.garr[2] = g.ctypes.data
        return f

    def expansion(value):
        def f(call):
            call.expansion = value
        return f

    def n_chunks(value):
        def f(call):
            call.n_chunks = value
        return f

    return [("variants_not_ascending", not_ascending, b"chunk 2: variants not ascending"),
            ("cigar_query_length", cigar_query_length, b"chunk 2: read 0: CIGAR query length is not l_qseq"),
            ("null_options", null("options"), b""), ("null_chunks", null("chunks"), b""),
            ("null_forward_model", null("forward_model"), b"null argument"), ("null_reverse_model", null("reverse_model"), b"null argument"),
            ("null_gt", null("gt"), b"null argument"), ("null_hap_out", null("hap_out"), b"null argument"),
            ("null_hap_out_of_a_chunk", null_entry("hp"), b"chunk 2: null output array"),
            ("null_h1_out_of_a_chunk", null_entry("p1"), b"chunk 2: null output array"),
            ("null_h2_out_of_a_chunk", null_entry("p2"), b"chunk 2: null output array"),
            ("null_gt_of_a_chunk", null_entry("garr"), b"chunk 2: null genotypes"),
            ("genotype_beyond_the_alleles", gt_outside(99), b"chunk 2, variant 3: genotype 99"),
            ("negative_genotype", gt_outside(-1), b"chunk 2, variant 3: genotype -1"),
            ("odd_expansion", expansion(3), b"diagonalExpansion must be even"), ("negative_expansion", expansion(-2), b"diagonalExpansion must be even"),
            ("negative_n_chunks", n_chunks(-1), b"")]


def built(chunks):
    return [capi.aligned_chunk_struct(c) for c in chunks]


@pytest.mark.parametrize("name,edit,message", malformed_cases(), ids=[c[0] for c in malformed_cases()])
@pytest.mark.parametrize("unsupported_too", [False, True])
def test_a_malformed_call_is_an_argument_error_without_a_device(synthetic, name, edit, message, unsupported_too):
    """... with the one call's message, and before a refused mode"""
    chunks, gts = synthetic
    options = dict(capi.shipped_extract_options(), indel_size_for_sv_handling=1) if unsupported_too else None
    one = Call(built(chunks), gts, options=options)
    edit(one)
    want_rc, want_msg = one.run("one_call")
    assert want_rc == capi.MRP_ERR_ARG and message in want_msg, (name, want_msg)
    for entry in ENTRIES:
        call = Call(built(chunks), gts, options=options)
        edit(call)
        rc_, msg = call.run(entry, devices=NO_SUCH_DEVICE)
        assert rc_ == capi.MRP_ERR_ARG, (entry, name, msg)
        assert msg == want_msg, (entry, name)
        assert call.untouched(), (entry, name)


def test_refused_modes_need_neither_queue_nor_device(synthetic):
    chunks, gts = synthetic
    for mode in ("indel_size_for_sv_handling", "use_run_length_encoding"):
        options = dict(capi.shipped_extract_options(), **{mode: 1})
        want_rc, want_msg = Call(built(chunks[:3]), gts[:3], options=options).run("one_call")
        assert want_rc == capi.MRP_ERR_UNSUPPORTED
        for entry in ENTRIES:
            call = Call(built(chunks[:3]), gts[:3], options=options)
            rc_, msg = call.run(entry, devices=NO_SUCH_DEVICE)
            assert rc_ == capi.MRP_ERR_UNSUPPORTED and msg == want_msg, (mode, entry, msg)
            assert call.untouched(), (mode, entry)


def well_formed(synthetic):
    chunks, gts = synthetic
    hom = np.zeros_like(gts[1])
    return ([chunks[0], ec.make([], [(100, "20M", 60, 0)]), chunks[1], ec.make([ec.SNP110], []), chunks[2]],
            [gts[0], None, hom, np.array([[0, 1]], np.int32), gts[2]])


def test_only_a_well_formed_call_reaches_the_queue(synthetic):
    cs, gs = well_formed(synthetic)
    for seq, g in ((cs, gs), ([], [])):  # n_chunks == 0 included
        assert Call(built(seq), g).run("one_call")[0] == capi.MRP_ERR_NO_DEVICE
        for totals in (True, False):
            call = Call(built(seq), g)
            if not totals:
                call.nulls |= {"h1_out", "h2_out"}
            rc_, msg = call.run("queue", q=None)
            assert rc_ == capi.MRP_ERR_NO_DEVICE and b"no CPU fallback" in msg, msg
            assert call.untouched()


def test_on_devices_reports_the_queues_own_error_after_the_checks(synthetic):
    """a device that cannot be reached: MRP_ERR_NO_DEVICE where no device is visible, else mrp_queue_create's MRP_ERR_ARG for device 99"""
    cs, gs = well_formed(synthetic)
    visible = capi.load().mrp_device_count()
    for seq, g in ((cs, gs), ([], [])):
        call = Call(built(seq), g)
        rc_, msg = call.run("on_devices", devices=NO_SUCH_DEVICE)
        if visible <= 0:
            assert rc_ == capi.MRP_ERR_NO_DEVICE and b"no CPU fallback" in msg, msg
        else:
            assert rc_ == capi.MRP_ERR_ARG and b"device 99 out of range" in msg, msg
        assert call.untouched()


def test_python_binding_raises_the_same_errors(synthetic):
    chunks, gts = synthetic
    f = capi.PairHmm.default_nucleotide()
    with pytest.raises(capi.MrpError) as e:
        capi._haplotag_aligned(None, chunks[:2], gts[:2], f, f, queue=None)
    assert e.value.code == capi.MRP_ERR_NO_DEVICE
    bad = [gts[0], gts[1].copy()]
    bad[1][5, 0] = len(chunks[1].alleles[5])
    for kw in (dict(queue=None), dict(devices=[99])):
        with pytest.raises(capi.MrpError) as e:
            capi._haplotag_aligned(None, chunks[:2], bad, f, f, chunks_per_batch=1, **kw)
        assert e.value.code == capi.MRP_ERR_ARG and "chunk 1" in str(e.value) and "variant 5" in str(e.value)


def test_c_example_builds_and_refuses_to_run_without_a_device(tmp_path):
    exe = str(tmp_path / "haplotag_from_alignments_queue")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "haplotag_from_alignments_queue.c"), "-L" + libdir, "-lmargin_rphmm", "-lm",
                           "-Wl,-rpath," + libdir, "-o", exe])
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is tests/test_c_example_haplotag_queue.py)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
