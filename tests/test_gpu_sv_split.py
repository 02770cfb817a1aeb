"""The SV split of the extraction on the device (mrp_context_set_sv_split / mrp_queue_set_sv_split): with
indel_size_for_sv_handling > 0 the walk runs over the small variants and over the structural ones separately and the two results are
merged per read.  The output is integers and bytes: it is compared byte for byte with tests/extract_sv_oracle.py, the composites bit
for bit with their chains on the same context, the queues with the one call.  No tolerance anywhere.

Every test makes its own context or queue with the setting on and closes it; the session's gpu_ctx is never switched."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from margin_amd import capi, synth
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests import extract_sv_oracle as so
from tests import haplotag_aligned_oracle as hao
from tests import rest_cases as rc
from tests import sv_split_cases as sc
from tests import test_gpu_haplotag_aligned as ha
from tests import test_gpu_phase_aligned as pa
from tests import test_gpu_phase_aligned_filtered as pf
from tests.test_gpu_extract import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(ec.OPTS, indel_size_for_sv_handling=sc.SV_SIZE)  # windows for extract_cases' 40-base slice: expansion 2 / 6
LONG_ALT = ("GATTACA" * 9)[:60]


@pytest.fixture()
def sv_ctx():
    ctx = capi.Context(0)
    ctx.set_sv_split(1)
    yield ctx
    ctx.close()


@pytest.fixture()
def sv_queue():
    q = capi.Queue([0])
    q.set_sv_split(1)
    yield q
    q.close()


def oracle(chunks, opts):
    split = opts.get("indel_size_for_sv_handling", 0) > 0
    return [eo.as_arrays(x) for x in (so.extract(chunks, opts) if split else eo.extract(chunks, dict(opts, indel_size_for_sv_handling=0)))]


def check(ctx, chunks, opts, want=None):
    got, st = capi.extract_read_substrings(ctx, chunks, opts)
    want = want if want is not None else oracle(chunks, opts)
    assert len(got) == len(chunks) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"chunk {i}")
    return got, st


def small(pos):
    return (pos, [ec.REF[pos - 100], "ACGT"[("ACGT".index(ec.REF[pos - 100]) + 1) % 4]], 0)


def sv(pos):
    return (pos, [ec.REF[pos - 100], ec.REF[pos - 100] + LONG_ALT], 1)


def differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


def test_edges_of_the_classes(sv_ctx):
    K, F, X = capi.READ_KEPT, capi.READ_FILTERED, capi.READ_DROPPED
    # the delayed start: the structural variant listed after a small one whose window starts later
    delayed = [sc.delayed_start(620), sc.delayed_start(700)]
    got, _ = check(sv_ctx, delayed, sc.OPTS)
    assert got[0]["entry_len"].tolist() == [25, 129] and got[1]["entry_len"].tolist() == [25, 129]
    one_list, _ = check(sv_ctx, delayed, sc.UNSPLIT)
    assert one_list[0]["entry_len"].tolist() == [25, 97] and not differs(one_list[1], got[1])
    # reads against the two classes, over extract_cases' 40-base slice: windows sv 105 -> [0, 12], small 120 -> [18, 23], and mirrored
    reads = [(110, "20M", 60, 0),     # 0: starts after the last variant of one class, before one of the other
             (125, "10M", 60, 0),     # 1: past both classes
             (100, "40M", 3, 0),      # 2: low mapq, entries in both classes
             (104, "3S20M", 60, 0),   # 3: a start soft clip
             (95, "40M", 60, 0),      # 4: starts before the overlap
             (100, "40M", 60, 0)]     # 5
    sv_first, small_first = ec.make([sv(105), small(120)], reads), ec.make([small(105), sv(120)], reads)
    for c in (sv_first, small_first):
        assert capi.mark_structural_variants(c, sc.SV_SIZE).tolist() == c.is_sv.tolist()
    got, _ = check(sv_ctx, [sv_first, small_first], SMALL)
    for g in got:
        assert g["read_status"].tolist() == [K, X, F, K, K, K]
        assert g["read_n_substrings"].tolist() == [1, 0, 2, 2, 2, 2]  # read 0: entries of the later class only; read 2: summed
        assert g["entry_read"][g["entry_first"][0]:g["entry_first"][1]].tolist() == [2, 3, 4, 5]
        assert g["entry_read"][g["entry_first"][1]:g["entry_first"][2]].tolist() == [0, 2, 3, 4, 5]
    # a small variant listed after a structural one whose window covers it.  With expansion_sv < expansion_small the structural window
    # [8, 13] starts after the small one's [5, 18]: in the one-list walk the small variant waits for it, in its own walk it does not
    narrow = dict(SMALL, expansion_small=6, expansion_sv=2)
    covered = ec.make([sv(110), small(111)], [(100, "30M", 60, 0), (107, "20M", 60, 0)])
    got, _ = check(sv_ctx, [covered], narrow)
    one_list, _ = check(sv_ctx, [covered], dict(narrow, indel_size_for_sv_handling=0))
    assert got[0]["ref_aln_start"].tolist() == [8, 5]
    assert got[0]["entry_len"].tolist() == [5, 5, 13, 11] and one_list[0]["entry_len"].tolist() == [5, 5, 10, 10]


def test_degenerate_classes(sv_ctx):
    ref = sc.REF
    reads = [(100, "600M", 60, 0), (350, "300M", 60, 0x10), (90, "5S200M", 60, 0), (100, "600M", 3, 0)]
    no_sv = sc.make(ref, [sc.snp(ref, 300), sc.ins(ref, 310, 8), sc.snp(ref, 500)], reads)
    only_sv = sc.make(ref, [sc.ins(ref, 300), sc.ins(ref, 330, 90), sc.ins(ref, 500)], reads)
    no_variants = sc.make(ref, [], reads)
    no_reads = sc.make(ref, [sc.snp(ref, 300), sc.ins(ref, 320)], [])
    chunks = [no_sv, only_sv, no_variants, no_reads]
    assert [int(c.is_sv.sum()) for c in chunks] == [0, 3, 0, 1]
    got, _ = check(sv_ctx, chunks, sc.OPTS)
    assert got[0]["entry_read"].size > 0 and got[1]["entry_read"].size > 0
    assert got[2]["read_status"].tolist() == [0, 0, 0, 0] and got[3]["read_status"].size == 0 and got[3]["entry_first"].tolist() == [0, 0, 0]
    # a chunk of one class: the split walk is the one-list walk
    one_list, _ = capi.extract_read_substrings(sv_ctx, chunks, sc.UNSPLIT)
    for i in (0, 1):
        assert_same(got[i], one_list[i], f"chunk {i} against the one-list walk")
    got, _ = check(sv_ctx, [], sc.OPTS)
    assert got == []


def test_more_than_one_wave_trip_per_class(sv_ctx):
    """one read over 150 small variants interleaved with 70 structural ones: each class spans more than 64 candidates, the running
    maximum is carried across the trips of a class and never across the classes"""
    opts = dict(sc.OPTS, expansion_small=2, expansion_sv=40)
    chunk = sc.interleaved()
    assert len(chunk.alleles) == 220 and int(chunk.is_sv.sum()) == 70 and len(chunk.read_pos) == 1
    got, st = check(sv_ctx, [chunk], opts)
    assert got[0]["read_n_substrings"].tolist() == [220] and st.entries == 220
    one_list, _ = check(sv_ctx, [chunk], dict(opts, indel_size_for_sv_handling=0))
    # in the one-list walk the later starts of the small variants cut the structural windows, in the split walk they do not
    sv_at = np.flatnonzero(chunk.is_sv)
    assert (got[0]["entry_len"][sv_at] > one_list[0]["entry_len"][sv_at]).sum() > 64
    assert np.array_equal(got[0]["entry_len"][chunk.is_sv == 0], one_list[0]["entry_len"][chunk.is_sv == 0])
    # two reads, the second starting in the middle of each class (past the first trip of the small one)
    two = dataclasses.replace(sc.interleaved(), read_pos=np.array([200, 2600], np.int64), flag=np.zeros(2, np.uint16), mapq=np.full(2, 60, np.uint8),
                              l_qseq=np.array([4000, 1500], np.int32), cigar_first=np.array([0, 1, 2], np.int64),
                              cigar=np.array([4000 << 4, 1500 << 4], np.uint32), seq_first=np.array([0, 2000, 2750], np.int64),
                              seq=np.concatenate([chunk.seq, chunk.seq[:750]]), read_names=["a", "b"])
    got, _ = check(sv_ctx, [two, chunk], opts)
    assert 0 < got[0]["read_n_substrings"][1] < 220


@pytest.fixture(scope="module")
def mixed():
    """eight 20 kb chunks at about 8x, about 40 variants each, a share of them structural -> (chunks, split oracle, one-list oracle)"""
    chunks = [sc.synthetic(seed) for seed in range(8)]
    return chunks, oracle(chunks, sc.OPTS), oracle(chunks, sc.UNSPLIT)


def test_many_chunks_mixed_classes(sv_ctx, mixed):
    chunks, want, want_one_list = mixed
    n_var, n_sv = sum(len(c.alleles) for c in chunks), sum(int(c.is_sv.sum()) for c in chunks)
    assert 250 < n_var < 450 and n_var // 8 < n_sv < n_var // 2 and all(0 < c.is_sv.sum() < len(c.is_sv) for c in chunks)
    _, st = check(sv_ctx, chunks, sc.OPTS, want)
    assert st.entries == sum(int(w["entry_read"].size) for w in want) > 0 and st.kernel_ms > 0
    # the input makes the split matter
    assert sum(differs(a, b) for a, b in zip(want, want_one_list)) >= 3
    # the one-list walk on the same context with option 0: the path of before, untouched
    check(sv_ctx, chunks, sc.UNSPLIT, want_one_list)
    check(sv_ctx, chunks, sc.OPTS, want)


@pytest.fixture(scope="module")
def three():
    """three 6 kb chunks at about 6x with their genotypes and, for the filtered call, their variants divided into primary and filtered"""
    chunks = [dataclasses.replace(c, is_sv=capi.mark_structural_variants(c, sc.SV_SIZE))
              for c in (synth.make_aligned_chunk(seed, overlap_bp=6_000, coverage=6.0, variant_every=250, sv_share=0.25) for seed in (21, 22, 23))]
    gts = [hao.draw_genotypes(c, seed) for seed, c in enumerate(chunks)]
    primary, rests = [], []
    for seed, c in enumerate(chunks):
        p, fl, _ = rc.split_variants(c, every=3)
        primary.append(p)
        rests.append((fl, rc.genotypes(fl, seed)))
    return chunks, gts, primary, rests


def test_composites_equal_their_chains(sv_ctx, three):
    chunks, gts, primary, rests = three
    assert all(0 < c.is_sv.sum() < len(c.is_sv) for c in chunks)
    assert all(p.is_sv.any() for p in primary) and all(fl.is_sv.any() and not fl.is_sv.all() for fl, _ in rests)  # the filtered set holds an SV too
    split, _ = capi.extract_read_substrings(sv_ctx, chunks, sc.OPTS)
    one_list, _ = capi.extract_read_substrings(sv_ctx, chunks, sc.UNSPLIT)
    assert any(differs(a, b) for a, b in zip(split, one_list))  # (the chains below start from an extraction the split changes)
    f, r, _, _ = ha.models()
    tags, hst = capi.haplotag_aligned_chunks(sv_ctx, chunks, gts, f, r, sc.OPTS)
    ha.assert_identical(tags, ha.chain(sv_ctx, chunks, gts, sc.OPTS, f, r), "haplotag")
    assert hst.extract.entries == sum(int(g["entry_read"].size) for g in split) and any((t["hap"] > 0).any() for t in tags)
    p = pa.params()
    got, st = pa.composite(sv_ctx, chunks, None, sc.OPTS, p, min_phred=3)
    want, _, _ = pa.chain(sv_ctx, chunks, None, sc.OPTS, p, min_phred=3)
    pa.assert_identical(got, want, "phase aligned")
    assert st.extract.entries == hst.extract.entries and st.bubbles > 0
    got, fst = pf.composite(sv_ctx, primary, rests, None, sc.OPTS, p, min_phred=pf.MIN_PHRED)
    want, _, _, _ = pf.chain(sv_ctx, primary, rests, None, sc.OPTS, p, min_phred=pf.MIN_PHRED)
    pf.assert_identical(got, want, "phase aligned with filtered")
    assert fst.filtered_variants == sum(len(fl.alleles) for fl, _ in rests) and fst.filtered_entries > 0


def refused(call):
    with pytest.raises(capi.MrpError) as e:
        call()
    return e.value.code == capi.MRP_ERR_UNSUPPORTED and "indelSizeForSVHandling" in str(e.value)


def test_queues_equal_the_one_call(sv_ctx, sv_queue, three):
    chunks, gts, primary, rests = three
    f, r = pa.models()
    p = pa.params()
    ref, _ = pa.composite(sv_ctx, chunks, None, sc.OPTS, p, min_phred=3)
    got, st = sv_queue.phase_aligned_chunks(chunks, f, r, p, options=sc.OPTS, profiles=True, min_phred=3, chunks_per_batch=1)
    pa.assert_identical(got, ref, "aligned queue")
    assert st.batches == 3
    ref, _ = pf.composite(sv_ctx, primary, rests, None, sc.OPTS, p, min_phred=pf.MIN_PHRED)
    got, st = sv_queue.phase_aligned_chunks_with_filtered(primary, rests, f, r, p, options=sc.OPTS, profiles=True, min_phred=pf.MIN_PHRED, chunks_per_batch=2)
    pf.assert_identical(got, ref, "aligned queue with filtered")
    assert st.batches == 2
    href, _ = capi.haplotag_aligned_chunks(sv_ctx, chunks, gts, f, r, sc.OPTS)
    hgot, hst = sv_queue.haplotag_aligned_chunks(chunks, gts, f, r, sc.OPTS, chunks_per_batch=1)
    ha.assert_identical(hgot, href, "haplotag queue")
    assert hst.batches == 3
    # a queue with the switch off stops up front, and so does this one once it is switched off
    plain = capi.Queue([0])
    try:
        for q in (plain, sv_queue):
            if q is sv_queue:
                q.set_sv_split(0)
            assert refused(lambda: q.phase_aligned_chunks(chunks, f, r, p, options=sc.OPTS, chunks_per_batch=1))
            assert refused(lambda: q.phase_aligned_chunks_with_filtered(primary, rests, f, r, p, options=sc.OPTS, chunks_per_batch=1))
            assert refused(lambda: q.haplotag_aligned_chunks(chunks, gts, f, r, sc.OPTS, chunks_per_batch=1))
    finally:
        plain.close()
    # the *_on_devices forms make a queue of their own with the switch off
    assert refused(lambda: capi.haplotag_aligned_chunks_on_devices([0], chunks, gts, f, r, sc.OPTS))


def test_the_switch(three):
    chunks, gts, _, _ = three
    f, r = pa.models()
    case = [sc.delayed_start()]
    want = oracle(case, sc.OPTS)
    ctx = capi.Context(0)
    try:
        assert refused(lambda: capi.extract_read_substrings(ctx, case, sc.OPTS))  # off by default
        ctx.set_sv_split(1)
        check(ctx, case, sc.OPTS, want)
        assert refused(lambda: capi.extract_read_substrings(ctx, case, dict(sc.OPTS, indel_size_for_sv_handling=-1)))  # a negative value stays refused
        with pytest.raises(capi.MrpError) as e:
            capi.extract_read_substrings(ctx, case, dict(sc.OPTS, use_run_length_encoding=1))
        assert e.value.code == capi.MRP_ERR_UNSUPPORTED and "run-length" in str(e.value)
        ctx.set_sv_split(0)
        assert refused(lambda: capi.extract_read_substrings(ctx, case, sc.OPTS))  # off again: the refusal of before, on the same context
        assert refused(lambda: capi.haplotag_aligned_chunks(ctx, chunks, gts, f, r, sc.OPTS))
        assert refused(lambda: capi.phase_aligned_chunks(ctx, chunks, f, r, pa.params(), options=sc.OPTS))
        check(ctx, case, sc.UNSPLIT)  # the context then extracts as before
        ctx.set_sv_split(1)
        check(ctx, case, sc.OPTS, want)
    finally:
        ctx.close()


def test_c_example_prints_the_oracles_lengths(tmp_path):
    exe = str(tmp_path / "phase_from_alignments_sv")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "phase_from_alignments_sv.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    variants, reads, status, entries, windows = [], [], None, {}, {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "variant":
            variants.append((int(w[1]), w[3:], int(w[2])))
        elif w[0] == "read":
            reads.append((int(w[1]), w[2], int(w[3]), int(w[4])))
        elif w[0] == "status":
            status = [int(x) for x in w[1:]]
        elif w[0] == "entries":
            windows[int(w[1])] = (int(w[3]), int(w[4].rstrip(":")))
            entries[int(w[1])] = [tuple(int(x) for x in e.split(":")) for e in w[5:]]
    chunk = ec.make(variants, reads)
    assert len(reads) == 12 and chunk.is_sv.tolist() == [0, 1] == capi.mark_structural_variants(chunk, sc.SV_SIZE).tolist()
    want, one_list = oracle([chunk], SMALL)[0], oracle([chunk], dict(SMALL, indel_size_for_sv_handling=0))[0]  # the example's options
    assert status == want["read_status"].tolist()
    for v in range(2):
        a, b = int(want["entry_first"][v]), int(want["entry_first"][v + 1])
        assert entries[v] == list(zip(want["entry_read"][a:b].tolist(), want["entry_len"][a:b].tolist())), v
        assert windows[v] == (int(want["ref_aln_start"][v]), int(want["ref_aln_stop_incl"][v]))
    assert windows == {0: (16, 21), 1: (14, 27)} and not np.array_equal(want["entry_len"], one_list["entry_len"])  # the windows interact
