"""mrp_haplotag_aligned_chunks at margin phase's shape, beside the chain of single calls it joins: the 96 chunks of
tools/extract_probe.py (100 kb with 10 kb overlaps, 30x, reads of median ~15 kb, a het variant every ~1 kb; a few distinct
synthetic chunks, repeated) with phased genotypes drawn per variant (15 % homozygous).  The chain is
mrp_extract_read_substrings -> mrp_haptag_sites_from_extracted -> mrp_partition_reads_by_haplotype, called through ctypes on
the C structs themselves (no numpy copies in between), in the same process and on the same context.  Reports the wall time of
both (median of --reps), their kernel times (HIP events), the bytes each downloads, the owners kernel's share, and whether
both gave the same tags and totals bit for bit.  Prints one JSON line and writes it to --out.

    python tools/haplotag_probe.py [--chunks 96] [--distinct 4] [--reps 5] [--cache FILE] [--out profiles/haplotag/probe.json]

--cache keeps the generated chunks (pickle) so that a later run skips their generation.

--queue N: the work queue over the same chunks beside the ONE call.  Leg (a) is mrp_haplotag_aligned_chunks on one context; leg (b) is
mrp_queue_haplotag_aligned_chunks on a queue over device 0 with N chunks per batch.  One process, a warm-up of both legs, the median of
--reps with min and max, the wall time of the C call alone; one digest over every output per leg, which must be equal.  Writes
profiles/haplotag/queue.json (or --out).  MRP_TIMING=1 prints the lanes' lines.
"""
import argparse
import ctypes as C
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
from tests.haplotag_aligned_oracle import draw_genotypes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=96)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--queue", type=int, default=None, metavar="N")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "haplotag", "probe.json" if a.queue is None else "queue.json")
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
    dgt = [draw_genotypes(c, seed) for seed, c in enumerate(distinct)]
    chunks = [distinct[i % a.distinct] for i in range(a.chunks)]
    gts = [dgt[i % a.distinct] for i in range(a.chunks)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    if a.queue is not None:
        return queue_legs(a, chunks, gts, built, opts)
    n = len(chunks)
    n_reads = sum(len(c.read_pos) for c in chunks)
    strand = np.ascontiguousarray(np.concatenate([c.read_forward_strand for c in chunks]), np.uint8)
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    L = capi.load()
    arr = (capi.AlignedChunk * n)(*[b[0] for b in built])
    garr, gkeep = capi._genotype_arrays(gts)
    opt = capi.ExtractOptions.from_dict(opts)

    def chain(ctx):
        """the three calls on the C structs -> (hap int8 with -1, h1, h2 over the call's reads, stats of the two device calls, the counts
        the bytes they copy back follow from, wall ms of the three calls)"""
        out = C.POINTER(capi.ExtractedChunk)()
        est, pst = capi.ExtractStats(), capi.PairHmmStats()
        t0 = time.perf_counter()
        capi._check(L.mrp_extract_read_substrings(ctx.h, n, arr, C.byref(opt), C.byref(out), C.byref(est)))
        S = capi.HaptagSites()
        first = np.zeros(n + 1, np.int64)
        capi._check(L.mrp_haptag_sites_from_extracted(n, out, garr, C.byref(S), first.ctypes.data))
        hap, h1, h2 = np.zeros(n_reads, np.int32), np.zeros(n_reads), np.zeros(n_reads)
        capi._check(L.mrp_partition_reads_by_haplotype(ctx.h, C.byref(fwd), C.byref(rev), C.byref(S), n_reads, strand.ctypes.data, 4, hap.ctypes.data,
                                                       h1.ctypes.data, h2.ctypes.data, C.byref(pst)))
        wall = (time.perf_counter() - t0) * 1e3
        status = np.concatenate([capi._as_np(out[i].read_status, int(out[i].n_reads), np.uint8) for i in range(n)])
        n_var = sum(int(out[i].n_variants) for i in range(n))
        ents = [int(capi._as_np(out[i].entry_first, int(out[i].n_variants) + 1, np.int64)[-1]) for i in range(n)]
        n_ent = sum(ents)
        n_sym = sum(int(capi._as_np(out[i].entry_len, ents[i], np.int32).sum()) for i in range(n))
        L.mrp_free(S.allele_first)
        for i in range(n):
            for f_, _, _ in capi._EXTRACTED_ARRAYS:
                L.mrp_free(C.cast(getattr(out[i], f_), C.c_void_p))
        L.mrp_free(C.cast(out, C.c_void_p))
        return np.where(status == capi.READ_KEPT, hap, -1).astype(np.int8), h1, h2, est, pst, (n_var, n_ent, n_sym), wall

    with capi.Context(0) as ctx:
        capi.haplotag_aligned_chunks(ctx, chunks[:2], gts[:2], fwd, rev, opts, structs=built[:2])  # warm-up: module load, pools
        chain(ctx)
        capi.haplotag_aligned_chunks(ctx, chunks, gts, fwd, rev, opts, structs=built)
        walls_c, walls_j, stats_c, stats_j = [], [], [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            got, st = capi.haplotag_aligned_chunks(ctx, chunks, gts, fwd, rev, opts, structs=built)
            walls_j.append((time.perf_counter() - t) * 1e3)
            stats_j.append(st)
            ref = chain(ctx)
            walls_c.append(ref[6])
            stats_c.append(ref)
    same = (np.array_equal(np.concatenate([g["hap"] for g in got]), ref[0]) and
            np.array_equal(np.concatenate([g["h1"] for g in got]).view(np.uint64), ref[1].view(np.uint64)) and
            np.array_equal(np.concatenate([g["h2"] for g in got]).view(np.uint64), ref[2].view(np.uint64)))
    kj, kc = int(np.argsort(walls_j)[len(walls_j) // 2]), int(np.argsort(walls_c)[len(walls_c) // 2])
    st = stats_j[kj]
    _, _, _, est, pst, (n_var, n_ent, n_sym), _ = stats_c[kc]
    # what the chain's two device calls copy back (mrp_extract.hip, mrp_aligned.hip): the extraction's total, the status, the scan of the
    # reads' counts, the entry CSR, per entry offset, length and read, every substring's symbols; then hap, h1, h2 per read
    chain_bytes = 16 + (n_reads + 7) // 8 * 8 + 8 * (n_reads + 1) + 8 * (n_var + 1) + 8 * (n_ent + 1) + 12 * n_ent + n_sym + 20 * n_reads
    chain_kernel = est.kernel_ms + pst.kernel_ms
    comp_kernel = st.extract.kernel_ms + st.owners_ms + st.pairhmm.kernel_ms
    res = dict(chunks=a.chunks, distinct=a.distinct, reads=int(st.extract.reads), variants=int(st.sites), active_sites=int(st.active_sites),
               substrings=int(st.extract.entries), entries_scored_or_copied=int(st.entries), owners=int(st.owners),
               pairs=int(st.pairhmm.pairs_lane + st.pairhmm.pairs_wave), pairs_wave=int(st.pairhmm.pairs_wave),
               composite_wall_ms=round(walls_j[kj], 2), composite_walls_ms=[round(x, 2) for x in walls_j], composite_total_ms=round(st.total_ms, 2),
               chain_wall_ms=round(walls_c[kc], 2), chain_walls_ms=[round(x, 2) for x in walls_c],
               chain_extract_total_ms=round(est.total_ms, 2), chain_partition_total_ms=round(pst.total_ms, 2),
               composite_kernel_ms=round(comp_kernel, 3), chain_kernel_ms=round(chain_kernel, 3),
               extract_kernel_ms=round(st.extract.kernel_ms, 3), owners_kernel_ms=round(st.owners_ms, 3), pairhmm_kernel_ms=round(st.pairhmm.kernel_ms, 3),
               owners_share_of_kernel=round(st.owners_ms / comp_kernel, 4), owners_share_of_wall=round(st.owners_ms / walls_j[kj], 5),
               composite_bytes_downloaded=int(st.bytes_downloaded), chain_bytes_downloaded=int(chain_bytes), substring_symbols=int(n_sym),
               bytes_uploaded=int(st.extract.bytes_uploaded), identical_to_chain=bool(same))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


def queue_legs(a, chunks, gts, built, opts):
    fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    rev = fwd.reverse_complement()
    units = [capi.haplotag_chunk_units(c, g, struct=b) for c, g, b in zip(chunks, gts, built)]

    def digest(got):
        h = hashlib.sha256()
        for g in got:
            for k in ("hap", "h1", "h2"):
                h.update(np.ascontiguousarray(g[k]).tobytes())
        return h.hexdigest()

    def one_call(ctx):
        got, _ = capi.haplotag_aligned_chunks(ctx, chunks, gts, fwd, rev, opts, structs=built)
        return digest(got), capi.LAST_HAPLOTAG_CALL_MS

    def queued(q):
        got, st = q.haplotag_aligned_chunks(chunks, gts, fwd, rev, opts, chunks_per_batch=a.queue, structs=built)
        return digest(got), capi.LAST_HAPLOTAG_CALL_MS, st

    legs, digests = {"one_call": [], f"queue_{a.queue}": []}, {"one_call": set(), f"queue_{a.queue}": set()}
    q = capi.Queue([0])
    try:
        with capi.Context(0) as ctx:
            one_call(ctx)  # warm-up of both legs: module load, the contexts' pools, the lanes' contexts
            queued(q)
            for _ in range(a.reps):
                d, w = one_call(ctx)
                legs["one_call"].append(w)
                digests["one_call"].add(d)
                d, w, st = queued(q)
                legs[f"queue_{a.queue}"].append(w)
                digests[f"queue_{a.queue}"].add(d)
    finally:
        q.close()
    same = all(len(v) == 1 for v in digests.values()) and len(set.union(*digests.values())) == 1
    res = dict(chunks=a.chunks, distinct=a.distinct, reps=a.reps, chunks_per_batch=a.queue, lanes=int(os.environ.get("MRP_QUEUE_LANES", 4)),
               units_total=int(sum(units)), walls_ms={k: dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in legs.items()},
               queue=dict(batches=int(st.batches), busy_ms=round(float(st.busy_ms_per_device[0]), 2), fallback_chunks=int(st.fallback_chunks),
                          units=int(st.units_per_device[0])),
               digest=sorted(digests["one_call"])[0], identical=bool(same))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
