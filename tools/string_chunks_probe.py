"""mrp_phase_string_chunks against the four-call chain it replaces, on two chunk shapes: config 2's (~130 het SNP sites, 30x,
25-symbol alleles) and a 2 000-site chunk.  Every timing is host wall time around the C calls alone (the Python that builds
arguments or converts results is outside); the chain's steps are timed one by one.  Prints one JSON line per shape and
writes them all to --out.

    python tools/string_chunks_probe.py [--small 96] [--large 12] [--reps 3] [--out profiles/string_chunks/probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from margin_amd import capi, synth  # noqa: E402


def chain(ctx, chunks, built, f, r, params, min_phred=0):
    """the four calls, as examples/phase_from_strings.c makes them -> (ms per step, kernel ms, results)"""
    L = capi.load()
    ms = dict(supports=0.0, profile=0.0, phase=0.0, assign=0.0)
    kern = 0.0
    n = len(chunks)
    prep = []
    for c, (S, keep) in zip(chunks, built):
        nb = len(c.bubbles)
        an = np.diff(keep["allele_first"]).astype(np.uint32)
        nr = np.diff(keep["sub_first"])
        sup_off = np.zeros(nb + 1, dtype=np.int64)
        np.cumsum(an.astype(np.int64) * nr, out=sup_off[1:])
        sup = np.zeros(max(int(sup_off[-1]), 1), dtype=np.float32)
        sos = np.ascontiguousarray(keep["strand"][keep["sub_read"]], dtype=np.uint8)
        prep.append((an, sup_off, sup, sos, keep["strand"].astype(np.int32)))
    pst = capi.PairHmmStats()
    for (S, keep), (an, sup_off, sup, sos, fs) in zip(built, prep):
        t0 = time.perf_counter()
        capi._check(L.mrp_allele_read_supports(ctx.h, C.byref(f), C.byref(r), S.n_bubbles, keep["allele_first"].ctypes.data, keep["sub_first"].ctypes.data,
                                               keep["pool"].ctypes.data, keep["pool"].size, keep["allele_off"].ctypes.data, keep["allele_len"].ctypes.data,
                                               keep["sub_off"].ctypes.data, keep["sub_len"].ctypes.data, sos.ctypes.data, 4, 512, sup.ctypes.data, C.byref(pst)))
        ms["supports"] += 1e3 * (time.perf_counter() - t0)
        kern += pst.kernel_ms
    outs = []
    for (S, keep), (an, sup_off, sup, sos, fs) in zip(built, prep):
        b = capi.Bubbles(S.n_bubbles, an.ctypes.data, keep["sub_first"].ctypes.data, keep["sub_read"].ctypes.data, sup_off.ctypes.data, sup.ctypes.data)
        seqs, read_of, pool = C.POINTER(capi.ReadRec)(), C.c_void_p(), C.c_void_p()
        n_seqs, pool_bytes = C.c_int64(0), C.c_int64(0)
        pa, ps, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        t0 = time.perf_counter()
        capi._check(L.mrp_profile_seqs_from_bubbles(C.byref(b), S.n_reads, C.cast(keep["names"], C.c_void_p), fs.ctypes.data, C.byref(seqs), C.byref(read_of),
                                                    C.byref(n_seqs), C.byref(pool), C.byref(pool_bytes)))
        capi._check(L.mrp_reference_from_bubbles(C.byref(b), 0.0, C.byref(pa), C.byref(ps), C.byref(pp)))
        ms["profile"] += 1e3 * (time.perf_counter() - t0)
        outs.append((S.n_bubbles, seqs, read_of, n_seqs.value, pool, pool_bytes.value, pa, ps, pp))
    t0 = time.perf_counter()
    handles = []
    for nb, seqs, read_of, ns, pool, pb, pa, ps, pp in outs:
        h = C.c_void_p()
        capi._check(L.mrp_chunk_create(ctx.h, nb, pa, ps, pp, pool, pb, C.byref(h)))
        handles.append(h)
    ch = (C.c_void_p * n)(*[h.value for h in handles])
    rd = (C.POINTER(capi.ReadRec) * n)(*[o[1] for o in outs])
    nrs = (C.c_int64 * n)(*[o[3] for o in outs])
    res = (C.POINTER(capi.PhaseResult) * n)()
    st = capi.PhaseManyStats()
    capi._check(L.mrp_phase_reads_many(ctx.h, n, ch, rd, nrs, C.byref(params), res, C.byref(st)))
    ms["phase"] += 1e3 * (time.perf_counter() - t0)
    kern += st.device_ms
    units = 0
    haps = []
    for i, (nb, seqs, read_of, ns, pool, pb, pa, ps, pp) in enumerate(outs):
        hap = np.zeros(max(ns, 1), np.int8)
        phred = np.zeros(max(ns, 1))
        t0 = time.perf_counter()
        capi._check(L.mrp_assign_reads_to_haplotypes(nb, pa, pool, seqs, ns, res[i], min_phred, hap.ctypes.data, phred.ctypes.data))
        ms["assign"] += 1e3 * (time.perf_counter() - t0)
        units += sum(seqs[q].length for q in range(ns))
        haps.append(hap[:ns].copy())
    for i in range(n):
        L.mrp_phase_result_destroy(res[i])
    for h in handles:
        L.mrp_chunk_destroy(h)
    for o in outs:
        for p in (o[1], o[2], o[4], o[6], o[7], o[8]):
            L.mrp_free(C.cast(p, C.c_void_p))
    return ms, kern, units, haps


def one_call(ctx, chunks, built, f, r, params):
    out, st = capi.phase_string_chunks(ctx, chunks, f, r, params, structs=built)
    kern = st.pairhmm.kernel_ms + st.profile_ms + st.phase.device_ms + st.assign_ms
    return st, kern, out


def run_shape(ctx, name, chunks, reps, f, r, params):
    built = [capi.string_chunk_struct(c) for c in chunks]
    chain(ctx, chunks, built, f, r, params)  # warm-up: allocator caches, code objects
    one_call(ctx, chunks, built, f, r, params)
    rows_c, rows_n = [], []
    units = 0
    parity = True
    for _ in range(reps):
        ms, kern, units, haps = chain(ctx, chunks, built, f, r, params)
        rows_c.append((sum(ms.values()), kern, ms))
        st, kern_n, out = one_call(ctx, chunks, built, f, r, params)
        rows_n.append((st.total_ms, kern_n, st))
        parity = parity and all(int((o["hap"] >= 0).sum()) == len(h) for o, h in zip(out, haps))
    med = lambda rows: sorted(rows, key=lambda x: x[0])[len(rows) // 2]
    wc, kc, msc = med(rows_c)
    wn, kn, st = med(rows_n)
    return dict(shape=name, chunks=len(chunks), sites=sum(len(c.bubbles) for c in chunks), substrings=sum(len(b[1]) for c in chunks for b in c.bubbles),
                units=units, reps=reps,
                chain=dict(wall_ms=round(wc, 2), kernel_ms=round(kc, 2), host_ms=round(wc - kc, 2), units_per_s=round(units / wc * 1e3),
                           steps_ms={k: round(v, 2) for k, v in msc.items()}),
                one_call=dict(wall_ms=round(wn, 2), kernel_ms=round(kn, 2), host_ms=round(st.host_ms, 2), units_per_s=round(units / wn * 1e3),
                              pairhmm_kernel_ms=round(st.pairhmm.kernel_ms, 2), profile_kernel_ms=round(st.profile_ms, 3), assign_kernel_ms=round(st.assign_ms, 3),
                              phase_ms=round(st.total_ms - st.host_ms, 2), phase_device_ms=round(st.phase.device_ms, 2), resident=int(st.phase.resident)),
                speedup=round(wc / wn, 3), hp_coverage_matches=bool(parity))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=96, help="chunks of the config-2 shape")
    ap.add_argument("--large", type=int, default=12, help="chunks of 2 000 sites")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_chunks", "probe.json"))
    a = ap.parse_args()
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    shapes = [("config2_130_sites", [synth.make_string_chunk(seed=1000 + i, n_sites=130, coverage=30, allele_len=25) for i in range(a.small)]),
              ("2000_sites", [synth.make_string_chunk(seed=2000 + i, n_sites=2000, coverage=30, allele_len=25, span=(10, 60)) for i in range(a.large)])]
    rows = []
    with capi.Context(0) as ctx:
        for name, chunks in shapes:
            row = run_shape(ctx, name, chunks, a.reps, f, r, params)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
