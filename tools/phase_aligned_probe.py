"""mrp_phase_aligned_chunks at margin phase's shape, beside the chain of calls it joins: the 96 chunks of tools/extract_probe.py and
tools/haplotag_probe.py (100 kb with 10 kb overlaps, 30x, reads of median ~15 kb, a het variant every ~1 kb; a few distinct synthetic
chunks, repeated).  The chain is mrp_extract_read_substrings -> mrp_string_chunk_from_extracted per chunk -> mrp_phase_string_chunks,
called through ctypes on the C structs themselves (no numpy copies in between), in the same process and on the same context.  Reports
the wall time of both (median of --reps, with min and max), their kernel times (HIP events), what the composite downloads before the
pair-HMM launch against the symbols the chain downloads and uploads again, the owners and anchors kernels -- the latter against the host
wall time of mrp_kmer_alignment_anchors over the same anchored pairs, which is what the chain's front spends on them -- and whether
both gave the same results bit for bit.  Prints one JSON line and writes it to --out.

    python tools/phase_aligned_probe.py [--chunks 96] [--distinct 4] [--reps 5] [--cache FILE] [--out profiles/phase_aligned/probe.json]

--filtered: the same shape with one variant in five moved to the filtered set (every fifth, from the third on; gt 0 | 1, every fourth of
them homozygous), mrp_phase_aligned_chunks_with_filtered beside ITS chain: both extractions in one mrp_extract_read_substrings call,
mrp_string_chunk_from_extracted and mrp_string_chunk_rest_from_extracted per chunk, mrp_phase_string_chunks_with_filtered.  Both legs in
one process on one context, a warm-up, the median of --reps; the legs' outputs are compared through a digest.  Writes
profiles/phase_aligned/filtered.json (or --out).

--queue (with or without --filtered): the work queue over the same chunks beside the ONE call.  Leg (a) is mrp_phase_aligned_chunks
(_with_filtered) on one context; leg (b) is mrp_queue_phase_aligned_chunks(_with_filtered) on a queue over device 0, with
--per-batch chunks per batch (12) and with 0, the library's cut.  One process, a warm-up of every leg, the median of --reps with min and
max, the wall time of the C call alone; one digest over every output per leg.  Writes (or, when the file holds the other variant's
record, adds to) profiles/phase_aligned/queue.json (or --out).

--queue --filtered --records: the queue with the phased variant records (mrp_queue_phase_aligned_chunks_with_records) beside the queue
without (mrp_queue_phase_aligned_chunks_with_filtered), the same chunks and --per-batch on one queue over device 0, a warm-up of both,
the median of --reps with min and max; then the wall time of mrp_close_contigs over the result, cut into contigs of --contig-chunks (8)
chunks, with the library's default number of host threads and with one.  Adds its record ("with_records") to the same file.
"""
import argparse
import ctypes as C
import dataclasses
import hashlib
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from margin_amd import capi, synth  # noqa: E402

SV_THRESHOLD = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=96)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--filtered", action="store_true")
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--per-batch", type=int, default=12)
    ap.add_argument("--records", action="store_true")
    ap.add_argument("--contig-chunks", type=int, default=8)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "phase_aligned", "queue.json" if a.queue else ("filtered.json" if a.filtered else "probe.json"))
    opts = capi.shipped_extract_options()
    if a.cache and os.path.exists(a.cache):
        with open(a.cache, "rb") as f:
            distinct = pickle.load(f)
        assert len(distinct) == a.distinct
    else:
        t = time.perf_counter()
        distinct = [synth.make_aligned_chunk(seed, overlap_bp=120_000, margin_bp=10_000, coverage=30.0, read_len=(5_000, 25_000),
                                             variant_every=1_000, sv_share=0.02, oddities=False) for seed in range(a.distinct)]
        print(f"generated {a.distinct} chunks in {time.perf_counter() - t:.0f} s", file=sys.stderr)
        if a.cache:
            with open(a.cache, "wb") as f:
                pickle.dump(distinct, f)
    if a.queue and a.records:
        if not a.filtered:
            ap.error("--records needs --queue --filtered")
        return records_legs(a, distinct, opts)
    if a.queue:
        return queue_legs(a, distinct, opts)
    if a.filtered:
        return filtered_legs(a, distinct, opts)
    chunks = [distinct[i % a.distinct] for i in range(a.chunks)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    n = len(chunks)
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    L = capi.load()
    arr = (capi.AlignedChunk * n)(*[b[0] for b in built])
    opt = capi.ExtractOptions.from_dict(opts)
    names = [[s.encode() for s in c.read_names] for c in chunks]
    name_arrs = [(C.c_char_p * max(len(x), 1))(*x) for x in names]
    strands = [np.ascontiguousarray(c.read_forward_strand, np.uint8) for c in chunks]

    def chain(ctx, anchors_too=False):
        """the calls on the C structs -> (per chunk (hap, phred, hap1, hap2), stats, counts, wall ms[, host anchors ms, pairs, anchors])"""
        out = C.POINTER(capi.ExtractedChunk)()
        est, sst = capi.ExtractStats(), capi.StringChunksStats()
        t0 = time.perf_counter()
        capi._check(L.mrp_extract_read_substrings(ctx.h, n, arr, C.byref(opt), C.byref(out), C.byref(est)))
        sc = (capi.StringChunk * n)()
        bvs = []
        for i in range(n):
            bv = C.POINTER(C.c_int64)()
            capi._check(L.mrp_string_chunk_from_extracted(C.byref(out[i]), None, C.cast(name_arrs[i], C.c_void_p), strands[i].ctypes.data, C.byref(sc[i]), C.byref(bv)))
            bvs.append(bv)
        haps = [np.zeros(len(c.read_pos), np.int8) for c in chunks]
        phreds = [np.zeros(len(c.read_pos)) for c in chunks]
        hp = (C.c_void_p * n)(*[h.ctypes.data for h in haps])
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in phreds])
        res = (C.POINTER(capi.PhaseResult) * n)()
        capi._check(L.mrp_phase_string_chunks(ctx.h, n, sc, C.byref(fwd), C.byref(rev), 4, SV_THRESHOLD, 0.0, C.byref(params), 0, res, hp, pp, None, C.byref(sst)))
        wall = (time.perf_counter() - t0) * 1e3
        results = []
        for i in range(n):
            g = res[i].contents
            results.append((haps[i], phreds[i], capi._as_np(g.haplotype_string1, int(g.length), np.uint64), capi._as_np(g.haplotype_string2, int(g.length), np.uint64)))
            L.mrp_phase_result_destroy(res[i])
        n_sym = n_ent = 0
        host = None
        if anchors_too:
            host_ms, n_anchored, n_anchors = 0.0, 0, 0
            scratch = np.zeros((1 << 16, 2), np.int64)
        for i in range(n):
            S = sc[i]
            nb = int(S.n_bubbles)
            ne = int(capi._as_np(out[i].entry_first, int(out[i].n_variants) + 1, np.int64)[-1])
            n_ent += ne
            n_sym += int(capi._as_np(out[i].entry_len, ne, np.int32).sum())
            if anchors_too and i < a.distinct:  # the distinct chunks repeat: time each once, count it as often as it occurs
                times = len(range(i, n, a.distinct))
                a_first, s_first = capi._as_np(S.allele_first, nb + 1, np.int64), capi._as_np(S.sub_first, nb + 1, np.int64)
                a_off, a_len = capi._as_np(S.allele_off, int(a_first[nb]), np.int64), capi._as_np(S.allele_len, int(a_first[nb]), np.int32)
                s_off, s_len = capi._as_np(S.sub_off, int(s_first[nb]), np.int64), capi._as_np(S.sub_len, int(s_first[nb]), np.int32)
                pool = capi._as_np(S.pool, int(S.pool_bytes), np.uint8)
                base = pool.ctypes.data
                for b in range(nb):
                    seen = set()
                    for k in range(int(s_first[b]), int(s_first[b + 1])):
                        key = pool[s_off[k]:s_off[k] + s_len[k]].tobytes()
                        if key in seen:
                            continue
                        seen.add(key)
                        for j in range(int(a_first[b]), int(a_first[b + 1])):
                            if s_len[k] <= SV_THRESHOLD and a_len[j] <= SV_THRESHOLD:
                                continue
                            t1 = time.perf_counter()
                            got = L.mrp_kmer_alignment_anchors(base + int(a_off[j]), int(a_len[j]), base + int(s_off[k]), int(s_len[k]), scratch.ctypes.data)
                            host_ms += (time.perf_counter() - t1) * 1e3 * times
                            n_anchored += times
                            n_anchors += int(got) * times
                host = (host_ms, n_anchored, n_anchors)
            L.mrp_free(C.cast(S.allele_first, C.c_void_p))
            for f_, _, _ in capi._EXTRACTED_ARRAYS:
                L.mrp_free(C.cast(getattr(out[i], f_), C.c_void_p))
        L.mrp_free(C.cast(out, C.c_void_p))
        return results, est, sst, (n_ent, n_sym), wall, host

    def joint(ctx, count=None):
        """-> results, stats, wall ms of the C call (its own clock: the binding's conversions around it are not the library's)"""
        got, st = capi.phase_aligned_chunks(ctx, chunks[:count], fwd, rev, params, options=opts, structs=built[:count], sv_threshold=SV_THRESHOLD)
        return got, st, st.total_ms

    with capi.Context(0) as ctx:
        joint(ctx, 2)  # warm-up: module load, pools
        ref = chain(ctx, anchors_too=True)
        host_ms, host_pairs, host_anchors = ref[5]
        joint(ctx)
        walls_c, walls_j, stats_c, stats_j = [], [], [], []
        for _ in range(a.reps):
            got, st, w = joint(ctx)
            walls_j.append(w)
            stats_j.append(st)
            ref = chain(ctx)
            walls_c.append(ref[4])
            stats_c.append(ref)
    same = all(np.array_equal(g["hap"], r[0]) and g["phred"].tobytes() == r[1].tobytes() and np.array_equal(g["result"]["hap1"], r[2]) and
               np.array_equal(g["result"]["hap2"], r[3]) for g, r in zip(got, ref[0]))
    kj, kc = int(np.argsort(walls_j)[len(walls_j) // 2]), int(np.argsort(walls_c)[len(walls_c) // 2])
    st = stats_j[kj]
    _, est, sst, (n_ent, n_sym), _, _ = stats_c[kc]
    assert host_pairs == st.pairs_anchored and host_anchors == st.anchors, (host_pairs, st.pairs_anchored, host_anchors, st.anchors)
    comp_kernel = st.extract.kernel_ms + st.owners_ms + st.anchors_ms + st.chunks.pairhmm.kernel_ms + st.chunks.profile_ms + st.chunks.assign_ms
    chain_kernel = est.kernel_ms + sst.pairhmm.kernel_ms + sst.profile_ms + sst.assign_ms
    res = dict(chunks=a.chunks, distinct=a.distinct, reads=int(st.extract.reads), variants=int(st.variants), bubbles=int(st.bubbles),
               substrings=int(st.entries), substrings_used=int(st.entries_used), owners=int(st.owners), pairs=int(st.pairs),
               pairs_wave=int(st.chunks.pairhmm.pairs_wave), pairs_anchored=int(st.pairs_anchored), anchors=int(st.anchors), anchor_runs=int(st.anchor_runs),
               composite_wall_ms=round(walls_j[kj], 2), composite_walls_ms=[round(x, 2) for x in sorted(walls_j)],
               chain_wall_ms=round(walls_c[kc], 2), chain_walls_ms=[round(x, 2) for x in sorted(walls_c)],
               chain_extract_total_ms=round(est.total_ms, 2), chain_string_call_total_ms=round(sst.total_ms, 2),
               composite_kernel_ms=round(comp_kernel, 3), chain_kernel_ms=round(chain_kernel, 3),
               extract_kernel_ms=round(st.extract.kernel_ms, 3), owners_kernel_ms=round(st.owners_ms, 3), anchors_kernel_ms=round(st.anchors_ms, 3),
               host_anchors_ms_single_thread=round(host_ms, 3), pairhmm_kernel_ms=round(st.chunks.pairhmm.kernel_ms, 3),
               chain_pairhmm_kernel_ms=round(sst.pairhmm.kernel_ms, 3), phase_device_ms=round(st.chunks.phase.device_ms, 2), composite_host_ms=round(st.chunks.host_ms, 2), chain_string_call_host_ms=round(sst.host_ms, 2),
               composite_front_bytes_downloaded=int(st.front_bytes_downloaded), substring_symbols=int(n_sym),
               chain_symbol_bytes_down_and_up=int(2 * n_sym), bytes_uploaded=int(st.extract.bytes_uploaded), identical_to_chain=bool(same))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


def split(chunk):
    """-> (the chunk with four variants in five, the chunk with the fifth ones, their gt)"""
    n = len(chunk.variant_pos)
    pick = np.zeros(n, bool)
    pick[2::5] = True
    part = lambda m: dataclasses.replace(chunk, variant_pos=np.ascontiguousarray(chunk.variant_pos[m]), alleles=[al for al, k in zip(chunk.alleles, m) if k],
                                         is_sv=np.ascontiguousarray(chunk.is_sv[m]))
    filtered = part(pick)
    gt = np.array([(0, 0) if v % 4 == 3 else (0, 1) for v in range(len(filtered.alleles))], np.int32).reshape(-1, 2)
    return part(~pick), filtered, gt


def filtered_legs(a, distinct, opts):
    parts = [split(c) for c in distinct]
    n = a.chunks
    chunks = [parts[i % a.distinct][0] for i in range(n)]
    fchunks = [parts[i % a.distinct][1] for i in range(n)]
    gts = [parts[i % a.distinct][2] for i in range(n)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    fbuilt = [capi.aligned_chunk_struct(c) for c in fchunks]   # the same reads over the filtered variants: the chain's second n records
    rbuilt = [capi.aligned_chunk_rest_struct(c, g) for c, g in zip(fchunks, gts)]
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    L = capi.load()
    arr2 = (capi.AlignedChunk * (2 * n))(*([b[0] for b in built] + [b[0] for b in fbuilt]))
    opt = capi.ExtractOptions.from_dict(opts)
    names = [[s.encode() for s in c.read_names] for c in chunks]
    name_arrs = [(C.c_char_p * max(len(x), 1))(*x) for x in names]
    strands = [np.ascontiguousarray(c.read_forward_strand, np.uint8) for c in chunks]
    fpos = [np.ascontiguousarray(c.variant_pos, np.int64) for c in fchunks]
    gflat = [np.ascontiguousarray(g, np.int32).reshape(-1) for g in gts]
    ptr = lambda v: v.ctypes.data if v.size else None

    def digest(items):
        h = hashlib.sha256()
        for x in items:
            h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()

    def chain(ctx):
        out = C.POINTER(capi.ExtractedChunk)()
        est, sst = capi.ExtractStats(), capi.StringFilteredStats()
        t0 = time.perf_counter()
        capi._check(L.mrp_extract_read_substrings(ctx.h, 2 * n, arr2, C.byref(opt), C.byref(out), C.byref(est)))
        sc, rs = (capi.StringChunk * n)(), (capi.StringChunkRest * n)()
        blocks, frs = [], []
        for i in range(n):
            bv, fr, blk = C.POINTER(C.c_int64)(), C.c_void_p(), C.c_void_p()
            capi._check(L.mrp_string_chunk_from_extracted(C.byref(out[i]), None, C.cast(name_arrs[i], C.c_void_p), strands[i].ctypes.data, C.byref(sc[i]), C.byref(bv)))
            capi._check(L.mrp_string_chunk_rest_from_extracted(C.byref(out[i]), None, strands[i].ctypes.data, C.cast(bv, C.c_void_p), sc[i].n_bubbles,
                                                               C.byref(out[n + i]), ptr(fpos[i]), ptr(gflat[i]), int(chunks[i].chunk_start),
                                                               int(chunks[i].chunk_end), C.byref(rs[i]), C.byref(fr), C.byref(blk)))
            blocks.append(blk)
            frs.append(fr)
        haps = [np.zeros(len(c.read_pos), np.int8) for c in chunks]
        phreds = [np.zeros(len(c.read_pos)) for c in chunks]
        hp = (C.c_void_p * n)(*[h.ctypes.data for h in haps])
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in phreds])
        res = (C.POINTER(capi.PhaseResult) * n)()
        fout = (capi.FilteredOut * n)()
        capi._check(L.mrp_phase_string_chunks_with_filtered(ctx.h, n, sc, rs, C.byref(fwd), C.byref(rev), 4, SV_THRESHOLD, 0.0, C.byref(params), 0, res, hp, pp,
                                                            None, fout, C.byref(sst)))
        wall = (time.perf_counter() - t0) * 1e3
        items, n_sym = [], 0
        for i in range(n):
            g, O = res[i].contents, fout[i]
            nr, nv = int(O.n_reads), int(O.n_variants)
            items += [haps[i], phreds[i], capi._as_np(g.haplotype_string1, int(g.length), np.uint64), capi._as_np(g.haplotype_string2, int(g.length), np.uint64),
                      capi._as_np(O.read_hap, nr, np.int32), capi._as_np(O.h1, nr, np.float64), capi._as_np(O.h2, nr, np.float64),
                      capi._as_np(O.variant_state, nv, np.int32), capi._as_np(O.cis, nv, np.float64), capi._as_np(O.trans, nv, np.float64),
                      capi._as_np(frs[i], int(rs[i].n_filtered), np.int32)]
            L.mrp_phase_result_destroy(res[i])
            for f_ in ("read_hap", "h1", "h2", "variant_state", "cis", "trans"):
                L.mrp_free(C.cast(getattr(O, f_), C.c_void_p))
            L.mrp_free(C.cast(sc[i].allele_first, C.c_void_p))
            L.mrp_free(blocks[i])
        for i in range(2 * n):
            ne = int(capi._as_np(out[i].entry_first, int(out[i].n_variants) + 1, np.int64)[-1])
            n_sym += int(capi._as_np(out[i].entry_len, ne, np.int32).sum())
            for f_, _, _ in capi._EXTRACTED_ARRAYS:
                L.mrp_free(C.cast(getattr(out[i], f_), C.c_void_p))
        L.mrp_free(C.cast(out, C.c_void_p))
        return digest(items), est, sst, n_sym, wall

    def joint(ctx, count=None):
        got, st = capi.phase_aligned_chunks_with_filtered(ctx, chunks[:count], None, fwd, rev, params, options=opts, structs=built[:count],
                                                          rest_structs=rbuilt[:count], sv_threshold=SV_THRESHOLD)
        items = []
        for g in got:
            o = g["filtered"]
            items += [g["hap"], g["phred"], g["result"]["hap1"], g["result"]["hap2"], o["read_hap"], o["h1"], o["h2"], o["variant_state"], o["cis"], o["trans"],
                      g["filtered_read"]]
        return digest(items), st, st.aligned.total_ms

    with capi.Context(0) as ctx:
        joint(ctx, 2)  # warm-up: module load, pools
        chain(ctx)
        joint(ctx)
        walls_c, walls_j, stats_c, stats_j = [], [], [], []
        for _ in range(a.reps):
            dj, st, w = joint(ctx)
            walls_j.append(w)
            stats_j.append(st)
            ref = chain(ctx)
            walls_c.append(ref[4])
            stats_c.append(ref)
    kj, kc = int(np.argsort(walls_j)[len(walls_j) // 2]), int(np.argsort(walls_c)[len(walls_c) // 2])
    st = stats_j[kj]
    dc, est, sst, n_sym, _ = stats_c[kc]
    A = st.aligned
    med_c, med_j, spread_c = walls_c[kc], walls_j[kj], max(walls_c) - min(walls_c)
    res = dict(chunks=n, distinct=a.distinct, reads=int(A.extract.reads) // 2, variants=int(A.variants - st.filtered_variants), filtered_variants=int(st.filtered_variants),
               filtered_reads=int(st.filtered_reads), substrings=int(A.entries - st.filtered_entries), filtered_substrings=int(st.filtered_entries),
               pairs_scored=int(st.pairs_scored), pairs_speculative=int(st.pairs_speculative), pairs_read_by_results=int(st.pairs_read_by_results),
               chain_pairs_scored=int(sst.pairs_scored), pairs_anchored=int(A.pairs_anchored), anchors=int(A.anchors),
               composite_wall_ms=round(med_j, 2), composite_walls_ms=[round(x, 2) for x in sorted(walls_j)],
               chain_wall_ms=round(med_c, 2), chain_walls_ms=[round(x, 2) for x in sorted(walls_c)],
               condition_composite_not_above_chain_plus_spread=bool(med_j <= med_c + spread_c),
               chain_extract_total_ms=round(est.total_ms, 2), chain_string_call_total_ms=round(sst.chunks.total_ms, 2),
               composite_kernel_ms=dict(extract=round(A.extract.kernel_ms, 3), owners=round(A.owners_ms, 3), classes=round(st.classes_ms, 3),
                                        anchors=round(A.anchors_ms, 3), pairhmm=round(A.chunks.pairhmm.kernel_ms, 3), profile=round(A.chunks.profile_ms, 3),
                                        assign=round(A.chunks.assign_ms, 3), filtered=round(st.filtered_ms, 3)),
               chain_kernel_ms=dict(extract=round(est.kernel_ms, 3), pairhmm=round(sst.chunks.pairhmm.kernel_ms, 3), profile=round(sst.chunks.profile_ms, 3),
                                    assign=round(sst.chunks.assign_ms, 3), filtered=round(sst.filtered_ms, 3)),
               phase_device_ms=round(A.chunks.phase.device_ms, 2), composite_host_ms=round(A.chunks.host_ms, 2), chain_string_call_host_ms=round(sst.chunks.host_ms, 2),
               composite_front_bytes_downloaded=int(A.front_bytes_downloaded), substring_symbols_both_extractions=int(n_sym),
               chain_symbol_bytes_down_and_up=int(2 * n_sym), bytes_uploaded=int(A.extract.bytes_uploaded), chain_bytes_uploaded=int(est.bytes_uploaded),
               digest=dj, identical_to_chain=bool(dj == dc))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


def queue_legs(a, distinct, opts):
    n = a.chunks
    parts = [split(c) for c in distinct] if a.filtered else [(c, None, None) for c in distinct]
    chunks = [parts[i % a.distinct][0] for i in range(n)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    rbuilt = [capi.aligned_chunk_rest_struct(parts[i % a.distinct][1], parts[i % a.distinct][2]) for i in range(n)] if a.filtered else None
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    units = [capi.aligned_chunk_units(None, struct=built[i], rest_struct=rbuilt[i] if a.filtered else None) for i in range(n)]
    kw = dict(options=opts, structs=built, sv_threshold=SV_THRESHOLD)
    if a.filtered:
        kw.update(rest_structs=rbuilt)

    def digest(got):
        h = hashlib.sha256()
        for g in got:
            items = [g["hap"], g["phred"], g["result"]["hap1"], g["result"]["hap2"], g["bubble_variant"]]
            if a.filtered:
                o = g["filtered"]
                items += [o["read_hap"], o["h1"], o["h2"], o["variant_state"], o["cis"], o["trans"], g["filtered_read"]]
            for x in items:
                h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()

    def one_call(ctx):
        if a.filtered:
            got, st = capi.phase_aligned_chunks_with_filtered(ctx, chunks, None, fwd, rev, params, **kw)
            return digest(got), capi.LAST_ALIGNED_CALL_MS, st.aligned
        got, st = capi.phase_aligned_chunks(ctx, chunks, fwd, rev, params, **kw)
        return digest(got), capi.LAST_ALIGNED_CALL_MS, st

    def queued(q, per_batch):
        if a.filtered:
            got, st = q.phase_aligned_chunks_with_filtered(chunks, None, fwd, rev, params, chunks_per_batch=per_batch, **kw)
        else:
            got, st = q.phase_aligned_chunks(chunks, fwd, rev, params, chunks_per_batch=per_batch, **kw)
        return digest(got), capi.LAST_ALIGNED_CALL_MS, st

    legs = {"one_call": [], f"queue_{a.per_batch}": [], "queue_0": []}
    digests, qstats = {}, {}
    q = capi.Queue([0])
    try:
        with capi.Context(0) as ctx:
            one_call(ctx)  # warm-up of every leg: module load, the contexts' pools, the lanes' contexts
            queued(q, a.per_batch)
            queued(q, 0)
            for _ in range(a.reps):
                d, w, st_a = one_call(ctx)
                legs["one_call"].append(w)
                digests.setdefault("one_call", set()).add(d)
                for per_batch in (a.per_batch, 0):
                    d, w, st = queued(q, per_batch)
                    legs[f"queue_{per_batch}"].append(w)
                    digests.setdefault(f"queue_{per_batch}", set()).add(d)
                    qstats[f"queue_{per_batch}"] = dict(batches=int(st.batches), busy_ms=round(float(st.busy_ms_per_device[0]), 2),
                                                        fallback_chunks=int(st.fallback_chunks), units=int(st.units_per_device[0]))
    finally:
        q.close()
    med = {k: float(np.median(v)) for k, v in legs.items()}
    spread = max(legs["one_call"]) - min(legs["one_call"])
    best = min(med[f"queue_{a.per_batch}"], med["queue_0"])
    same = all(len(v) == 1 for v in digests.values()) and len(set.union(*digests.values())) == 1
    res = dict(filtered=bool(a.filtered), chunks=n, distinct=a.distinct, reps=a.reps, lanes=int(os.environ.get("MRP_QUEUE_LANES", 4)), units_total=int(sum(units)),
               prefetch_uploads_on_second_context=False,
               walls_ms={k: dict(median=round(med[k], 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in legs.items()},
               one_call_host_ms=round(st_a.chunks.host_ms, 2), one_call_extract_host_ms=round(st_a.extract.host_ms, 2), queue=qstats,
               condition_best_queue_not_above_one_call_plus_spread=bool(best <= med["one_call"] + spread),
               digest=sorted(digests["one_call"])[0], identical=bool(same))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    record = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            record = json.load(f)
    record["with_filtered" if a.filtered else "plain"] = res
    with open(a.out, "w") as f:
        f.write(json.dumps(record, indent=1) + "\n")


def records_legs(a, distinct, opts):
    """--queue --filtered --records: the queue with the records beside the queue without, then the closing of the result"""
    n = a.chunks
    parts = [split(c) for c in distinct]
    chunks = [parts[i % a.distinct][0] for i in range(n)]
    fchunks = [parts[i % a.distinct][1] for i in range(n)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    rbuilt = [capi.aligned_chunk_rest_struct(parts[i % a.distinct][1], parts[i % a.distinct][2]) for i in range(n)]
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    kw = dict(options=opts, structs=built, rest_structs=rbuilt, sv_threshold=SV_THRESHOLD, chunks_per_batch=a.per_batch)

    def digest(got):
        h = hashlib.sha256()
        for g in got:
            o = g["filtered"]
            for x in (g["hap"], g["phred"], g["result"]["hap1"], g["result"]["hap2"], g["bubble_variant"], o["read_hap"], o["h1"], o["h2"], o["variant_state"],
                      o["cis"], o["trans"], g["filtered_read"]):
                h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()

    legs = {"queue_with_filtered": [], "queue_with_records": []}
    digests = set()
    q = capi.Queue([0])
    try:
        q.phase_aligned_chunks_with_filtered(chunks, None, fwd, rev, params, **kw)  # warm-up of both legs: module load, the lanes' contexts and pools
        q.phase_aligned_chunks_with_records(chunks, None, fwd, rev, params, **kw)
        for _ in range(a.reps):
            got, _ = q.phase_aligned_chunks_with_filtered(chunks, None, fwd, rev, params, **kw)
            legs["queue_with_filtered"].append(capi.LAST_ALIGNED_CALL_MS)
            digests.add(digest(got))
            got, st = q.phase_aligned_chunks_with_records(chunks, None, fwd, rev, params, **kw)
            legs["queue_with_records"].append(capi.LAST_ALIGNED_CALL_MS)
            digests.add(digest(got))
    finally:
        q.close()
    rs = st.records
    # ---- the closing: the chunks in contigs of --contig-chunks, read ids = a read's index among the distinct chunk's reads
    na = lambda c: np.array([len(al) for al in c.alleles], np.int32)
    dicts = [dict(read_names=list(c.read_names), read_id=np.arange(len(c.read_names), dtype=np.int32), hap=g["hap"], phred=g["phred"], filtered=g["filtered"],
                  filtered_read=g["filtered_read"], records=g["records"], variant_pos=c.variant_pos, n_alleles=na(c), fvariant_pos=f.variant_pos, fn_alleles=na(f))
             for g, c, f in zip(got, chunks, fchunks)]
    cbuilt = [capi.contig_chunk_struct(d) for d in dicts]
    arr = (capi.ContigChunk * n)(*[b[0] for b in cbuilt])
    first = np.ascontiguousarray(list(range(0, n, a.contig_chunks)) + [n], np.int64)
    n_contigs = len(first) - 1
    rules = capi.ContigRules(0, 0, 2, 0.05, 0.5)
    L = capi.load()

    def close_ms():
        walls, seen = [], None
        for _ in range(a.reps + 1):  # (the first is a warm-up: the pool's threads)
            outs = (capi.ContigOut * n_contigs)()
            t0 = time.perf_counter()
            capi._check(L.mrp_close_contigs(n_contigs, first.ctypes.data, arr, C.byref(rules), outs))
            walls.append((time.perf_counter() - t0) * 1e3)
            seen = dict(variants=sum(int(O.variants.n_variants) for O in outs), switched=sum(int(x) for O in outs for x in capi._as_np(O.switched, int(O.n_chunks), np.int32)))
            for O in outs:
                L.mrp_contig_out_clear(C.byref(O))
        walls = walls[1:]
        return dict(median=round(float(np.median(walls)), 3), min=round(min(walls), 3), max=round(max(walls), 3)), seen
    close_default, seen = close_ms()  # the library's own number of host threads: never set in this process
    capi._check(L.mrp_set_host_threads(1))
    close_one, seen_one = close_ms()
    assert seen == seen_one
    med = {k: float(np.median(v)) for k, v in legs.items()}
    res = dict(chunks=n, distinct=a.distinct, reps=a.reps, per_batch=a.per_batch, lanes=int(os.environ.get("MRP_QUEUE_LANES", 4)), batches=int(st.batches),
               walls_ms={k: dict(median=round(med[k], 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in legs.items()},
               records=dict(sites=int(rs.records_sites), updated=int(rs.records_updated), reads_listed=int(rs.reads_listed),
                            bytes_downloaded=int(rs.records_bytes_downloaded), kernel_ms_summed_over_batches=round(float(rs.records_ms), 3)),
               close_contigs=dict(contigs=n_contigs, chunks_per_contig=a.contig_chunks, reads=sum(len(d["read_names"]) for d in dicts), kept_variants=seen["variants"],
                                  chunks_switched=seen["switched"], wall_ms_default_threads=close_default, wall_ms_one_thread=close_one),
               identical_outputs_with_and_without_records=bool(len(digests) == 1))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    record = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            record = json.load(f)
    record["with_records"] = res
    with open(a.out, "w") as f:
        f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
