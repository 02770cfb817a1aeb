#!/usr/bin/env python3
"""Timing probe of mrp_partition_reads_by_haplotype and mrp_phase_variants_from_tagged_reads on N chunks of config-2 shape
(2 000 het SNP sites x ~30x coverage, 25-symbol alleles and read substrings) in one call each: a chosen fraction of the reads
is filtered (partitioned against the fragment's alleles), the rest is tagged and phases every site as a filtered variant.
Prints pairs/s and call time per entry (kernel_ms covers the pair-HMM and the scoring kernels), the oracle's CPU rate on all
cores, and optionally a parity sample against tests/haptag_oracle.py.  The scoring kernels' share of the device time comes
from a kernel trace of this probe: `rocprofv3 --kernel-trace -d <dir> -o probe -- python tools/haptag_probe.py ...` writes
<dir>/probe_results.db, which --kernel-trace-db reads back."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from margin_amd import capi, synth  # noqa: E402

L_ALLELE = 25


def make_chunk(rng, n_sites, coverage, span, filtered_fraction):
    """per site: ref / alt allele; reads cover `span` consecutive sites and carry their haplotype's allele with 5 % substitutions"""
    ref = rng.integers(0, 4, size=(n_sites, L_ALLELE)).astype(np.uint8)
    alt = ref.copy()
    alt[:, L_ALLELE // 2] = (alt[:, L_ALLELE // 2] + 1 + rng.integers(0, 3, size=n_sites)) % 4
    phase = rng.integers(0, 2, size=n_sites)  # which allele hap 1 carries
    n_reads = max(1, n_sites * coverage // span)
    start = rng.integers(0, n_sites - span + 1, size=n_reads)
    hap = rng.integers(0, 2, size=n_reads)
    strand = (rng.random(n_reads) < 0.5).astype(np.uint8)
    filtered = rng.random(n_reads) < filtered_fraction
    read = np.repeat(np.arange(n_reads), span)
    site = (start[:, None] + np.arange(span)[None, :]).reshape(-1)
    order = np.lexsort((read, site))  # by site, then in read order (buildVcfEntryToReadSubstringsMap)
    read, site = read[order], site[order]
    carries_alt = (phase[site] ^ hap[read]).astype(bool)
    sub = np.where(carries_alt[:, None], alt[site], ref[site])
    noise = rng.random(sub.shape) < 0.05
    sub[noise] = rng.integers(0, 4, size=int(noise.sum()))
    return dict(ref=ref, alt=alt, phase=phase, n_reads=n_reads, hap=hap, strand=strand, filtered=filtered, read=read, site=site, sub=sub)


def build(chunks, which):
    """mrp_haptag_sites of all chunks: which = 'partition' (filtered reads' entries, compare = fragment alleles) or 'phase'
    (every entry, compare = (0, 1))"""
    pools, a_first, e_first, e_read, cmp_, n_a, n_e, read_base, pos = [], [], [], [], [], 0, 0, 0, 0
    a_off, e_off = [], []
    for ch in chunks:
        ns = len(ch["ref"])
        keep = ch["filtered"][ch["read"]] if which == "partition" else np.ones(len(ch["read"]), bool)
        site, read, sub = ch["site"][keep], ch["read"][keep], ch["sub"][keep]
        alleles = np.stack([ch["ref"], ch["alt"]], axis=1).reshape(-1, L_ALLELE)
        pools += [alleles.reshape(-1), sub.reshape(-1)]
        a_off.append(pos + L_ALLELE * np.arange(2 * ns, dtype=np.int64))
        pos += alleles.size
        e_off.append(pos + L_ALLELE * np.arange(len(sub), dtype=np.int64))
        pos += sub.size
        a_first.append(n_a + 2 * np.arange(ns, dtype=np.int64))
        cnt = np.bincount(site, minlength=ns)
        e_first.append(n_e + np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64))
        e_read.append(read_base + read.astype(np.int64))
        c = np.stack([ch["phase"], 1 - ch["phase"]], axis=1) if which == "partition" else np.tile([0, 1], (ns, 1))
        cmp_.append(c.astype(np.int32).reshape(-1))
        n_a += 2 * ns
        n_e += len(sub)
        read_base += ch["n_reads"]
    keep = [np.concatenate(pools).astype(np.uint8), np.concatenate(a_first + [np.array([n_a])]).astype(np.int64), np.concatenate(a_off),
            np.full(n_a, L_ALLELE, np.int32), np.concatenate(cmp_), np.concatenate(e_first + [np.array([n_e])]).astype(np.int64),
            np.concatenate(e_read), np.concatenate(e_off), np.full(n_e, L_ALLELE, np.int32)]
    S = capi.HaptagSites(len(keep[1]) - 1, keep[0].ctypes.data, keep[0].size, *[a.ctypes.data for a in keep[1:]])
    return S, keep, n_e


def read_kernel_trace(path):
    import sqlite3
    db = sqlite3.connect(path)
    tot = {name: float(ns) for name, ns in db.execute("SELECT name, SUM(duration) FROM kernels GROUP BY name")}
    db.close()
    score = sum(v for k, v in tot.items() if "ht_partition_kernel" in k or "ht_phase_kernel" in k)
    hmm = sum(v for k, v in tot.items() if "phm_" in k)
    print(f"kernel trace: scoring kernels {score / 1e6:.3f} ms, pair-HMM kernels {hmm / 1e6:.3f} ms -> scoring share {score / max(score + hmm, 1):.2%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--span", type=int, default=100, help="het sites a read covers")
    ap.add_argument("--filtered", type=float, default=0.25, help="fraction of the reads filtered (downsampled / unphased)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parity", type=int, default=16, help="reads and variants compared with tests/haptag_oracle.py (0: none)")
    ap.add_argument("--cpu-pairs", type=int, default=40000, help="pairs the oracle scores on all cores (0: skip)")
    ap.add_argument("--kernel-trace-db", default=None, help="the rocprofv3 kernel trace of a run of this probe (rocpd database)")
    args = ap.parse_args()
    if args.kernel_trace_db:
        read_kernel_trace(args.kernel_trace_db)
        return
    rng = np.random.default_rng(1)
    t0 = time.time()
    chunks = [make_chunk(rng, args.sites, args.coverage, args.span, args.filtered) for _ in range(args.chunks)]
    n_reads = sum(c["n_reads"] for c in chunks)
    strand = np.concatenate([c["strand"] for c in chunks])
    read_hap = np.concatenate([np.where(c["filtered"], 0, c["hap"] + 1) for c in chunks]).astype(np.int32)
    Sp, keep_p, ne_p = build(chunks, "partition")
    Sv, keep_v, ne_v = build(chunks, "phase")
    print(f"synth {time.time() - t0:.1f}s: {args.chunks} chunks, {n_reads} reads, partition {ne_p} entries, phasing {ne_v} entries", flush=True)
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    L = capi.load()
    ctx = capi.Context(0)
    hap, h1, h2 = np.zeros(n_reads, np.int32), np.zeros(n_reads), np.zeros(n_reads)
    state, cis, trans = (np.zeros(len(keep_v[1]) - 1, np.int32), np.zeros(len(keep_v[1]) - 1), np.zeros(len(keep_v[1]) - 1))
    for rep in range(args.repeat):
        st = capi.PairHmmStats()
        capi._check(L.mrp_partition_reads_by_haplotype(ctx.h, C.byref(f), C.byref(r), C.byref(Sp), n_reads, strand.ctypes.data, 4,
                                                        hap.ctypes.data, h1.ctypes.data, h2.ctypes.data, C.byref(st)))
        n = st.pairs_lane + st.pairs_wave
        print(f"partition run {rep}: {n} pairs, kernel {st.kernel_ms:.3f} ms, call {st.total_ms:.2f} ms, {n / st.kernel_ms * 1e3:.3e} pairs/s (kernel), "
              f"{n / st.total_ms * 1e3:.3e} pairs/s (call); tagged {int(((hap == 1) | (hap == 2)).sum())} of {int(read_hap.size - (read_hap > 0).sum())} filtered",
              flush=True)
        st = capi.PairHmmStats()
        capi._check(L.mrp_phase_variants_from_tagged_reads(ctx.h, C.byref(f), C.byref(r), C.byref(Sv), n_reads, strand.ctypes.data,
                                                            read_hap.ctypes.data, 4, 512, state.ctypes.data, cis.ctypes.data, trans.ctypes.data, C.byref(st)))
        n = st.pairs_lane + st.pairs_wave
        print(f"phasing run {rep}: {n} pairs, kernel {st.kernel_ms:.3f} ms, call {st.total_ms:.2f} ms, {n / st.kernel_ms * 1e3:.3e} pairs/s (kernel), "
              f"{n / st.total_ms * 1e3:.3e} pairs/s (call); states {np.bincount(state, minlength=4).tolist()}", flush=True)
    ctx.close()
    from oracle import pairhmm as ph
    om = [ph.Model.from_buffer_copy(bytes(m)) for m in (f, r)]
    if args.cpu_pairs:
        pool, ns = keep_v[0], min(args.cpu_pairs, ne_v)
        xo = np.repeat(keep_v[2][:1], ns)
        yo, xl, yl = keep_v[7][:ns], np.full(ns, L_ALLELE, np.int32), np.full(ns, L_ALLELE, np.int32)
        mi = (1 - strand[keep_v[6][:ns]]).astype(np.uint8)
        cores = os.cpu_count() or 1
        parts = np.array_split(np.arange(ns), cores)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(cores) as ex:  # the oracle's ctypes calls release the GIL
            list(ex.map(lambda p: ph.forward_batch(om, pool, xo[p], xl[p], yo[p], yl[p], mi[p]), parts))
        dt = time.perf_counter() - t0
        print(f"oracle: {ns / dt:.3e} pairs/s on {cores} cores", flush=True)
    if args.parity:
        from tests import haptag_oracle as ho
        sym = lambda keep, j, off_i, len_i: keep[0][keep[off_i][j]:keep[off_i][j] + keep[len_i][j]]

        def site_tuple(keep, s):
            a0, e0, e1 = keep[1][s], keep[5][s], keep[5][s + 1]
            return ([sym(keep, a0, 2, 3), sym(keep, a0 + 1, 2, 3)], (int(keep[4][2 * s]), int(keep[4][2 * s + 1])),
                    [(int(keep[6][k]), sym(keep, k, 7, 8)) for k in range(e0, e1)])
        ok_r = ok_v = 0
        filt = np.flatnonzero(read_hap == 0)
        prng = np.random.default_rng(7)
        for q in prng.choice(filt, size=min(args.parity, len(filt)), replace=False):
            ss = np.unique(np.searchsorted(keep_p[5], np.flatnonzero(keep_p[6] == q), side="right") - 1).tolist()
            rh, r1, r2 = ho.partition_filtered_reads(om[0], om[1], [site_tuple(keep_p, s) for s in ss], n_reads, strand)
            ok_r += int(rh[q] == hap[q] and abs(r1[q] - h1[q]) <= 1e-9 * max(1, abs(r1[q])) and abs(r2[q] - h2[q]) <= 1e-9 * max(1, abs(r2[q])))
        for v in prng.choice(len(state), size=min(args.parity, len(state)), replace=False):
            s_, c_, t_ = ho.phase_filtered_variants(om[0], om[1], [site_tuple(keep_v, v)], n_reads, strand, read_hap)
            ok_v += int(s_[0] == state[v] and abs(c_[0] - cis[v]) <= 1e-9 * max(1, abs(c_[0])) and abs(t_[0] - trans[v]) <= 1e-9 * max(1, abs(t_[0])))
        print(f"parity: partition {ok_r}/{min(args.parity, len(filt))} reads, phasing {ok_v}/{min(args.parity, len(state))} variants", flush=True)


if __name__ == "__main__":
    main()
