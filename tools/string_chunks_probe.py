"""mrp_phase_string_chunks against the four-call chain it replaces, on two chunk shapes: config 2's (~130 het SNP sites, 30x,
25-symbol alleles) and a 2 000-site chunk.  Every timing is host wall time around the C calls alone (the Python that builds
arguments or converts results is outside); the chain's steps are timed one by one.  Prints one JSON line per shape and
writes them all to --out.

    python tools/string_chunks_probe.py [--small 96] [--large 12] [--reps 3] [--out profiles/string_chunks/probe.json]

--queue measures the work queue over string chunks instead (mrp_queue_phase_string_chunks) on the same two shapes and on a long
queue (the first shape repeated to --long chunks), three ways on device 0: (a) ONE mrp_phase_string_chunks call over all chunks,
the yardstick -- of the library given with --yardstick-lib (a libmargin_rphmm.so built from the commit before the queue took
strings), else of this build; (b) the queue with MRP_QUEUE_LANES=1; (c) the queue with its default lanes -- both with the
library's own batches (chunks_per_batch = 0), which for queues of these sizes are ONE batch, so that no second lane starts; and
therefore (d) the default lanes with batches of --lane-batch chunks, where the lanes and the front made ahead do run.  Each leg is a process
of its own, one after the other (the lane count is read when a queue is made, a second library needs its own process): a
warm-up call, then --reps timed calls, host wall time around the C call alone; the legs are run --rounds times in turn and a
leg's figure is the median over the timed calls of all its processes, its spread (max - min) / median over the same calls; the
legs' outputs are compared through a digest taken outside the timed region.  Prints one JSON line and writes it to --out (default profiles/string_chunks/queue.json).

    python tools/string_chunks_probe.py --queue [--yardstick-lib PATH] [--long 1536] [--lane-batch 192] [--reps 3]

--filtered measures the back half inside the string-chunk call (mrp_phase_string_chunks_with_filtered) on the same two
shapes at 60x with half of each chunk's reads filtered and 10 % as many filtered variants as bubbles, two ways on device 0:
(a) the chain of the existing calls -- ONE mrp_phase_string_chunks over the primary reads, then the sites of every chunk in ONE
mrp_phase_variants_from_tagged_reads and ONE mrp_partition_reads_by_haplotype -- of the library given with --yardstick-lib (built
from the commit before the new call), else of this build; (b) the new call.  Timed is the host wall time around the C calls alone:
the chain's two host assemblies of mrp_haptag_sites are made once, outside the timed region (a caller in C pays for them; here
they are Python), so leg (a) is shown at its best.  Processes of their own, in turn a b a b a b (--rounds 3): a warm-up call, then
--reps timed calls; median and min-max over all timed calls of a leg.  The legs' outputs are compared.  Writes
profiles/string_chunks/filtered.json.

    python tools/string_chunks_probe.py --filtered [--yardstick-lib PATH] [--small 96] [--large 12] [--reps 3] [--rounds 3]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
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


def probe_shapes(small, large, long_n=0):
    shapes = [("config2_130_sites", [synth.make_string_chunk(seed=1000 + i, n_sites=130, coverage=30, allele_len=25) for i in range(small)]),
              ("2000_sites", [synth.make_string_chunk(seed=2000 + i, n_sites=2000, coverage=30, allele_len=25, span=(10, 60)) for i in range(large)])]
    if long_n:
        shapes.append(("config2_130_sites_long", [shapes[0][1][i % small] for i in range(long_n)]))
    return shapes


def digest(rows):
    """every output of every chunk, in input order"""
    h = hashlib.sha256()
    for d in rows:
        g = d["result"]
        for k in sorted(g):
            v = g[k]
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
        h.update(d["hap"].tobytes())
        h.update(d["phred"].tobytes())
    return h.hexdigest()


def queue_leg(a):
    """one leg in this process: per shape a warm-up and a.reps timed C calls -> JSON file a.leg_out"""
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    L = capi.load()
    if a.host_threads:
        capi._check(L.mrp_set_host_threads(a.host_threads))
    ctx = q = None
    if a.queue_leg == "a":
        Y = L
        if a.yardstick_lib:  # the yardstick's own library beside this build's (which serves the host-only helpers above)
            Y = C.CDLL(a.yardstick_lib)
            Y.mrp_runtime_init()
            Y.mrp_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            Y.mrp_context_destroy.argtypes = [C.c_void_p]
            Y.mrp_context_destroy.restype = None
            Y.mrp_phase_string_chunks.argtypes = L.mrp_phase_string_chunks.argtypes
            Y.mrp_phase_result_destroy.argtypes = L.mrp_phase_result_destroy.argtypes
            Y.mrp_phase_result_destroy.restype = None
            Y.mrp_last_error.restype = C.c_char_p
        ctx = C.c_void_p()
        if Y.mrp_context_create(0, C.byref(ctx)) != capi.MRP_OK:
            raise RuntimeError(Y.mrp_last_error().decode())
    else:
        q = capi.Queue([0])
    rows = []
    per_batch = a.lane_batch if a.queue_leg == "d" else 0
    for name, chunks in probe_shapes(a.small, a.large, a.long):
        built = {id(c): capi.string_chunk_struct(c) for c in chunks}
        structs = [built[id(c)] for c in chunks]
        units = sum(capi.string_chunk_units(c, struct=built[id(c)]) for c in chunks)
        times, extra, dig = [], {}, None
        for rep in range(a.reps + 1):
            args = capi.StringChunkArgs(chunks, False, structs)
            if ctx is not None:
                st = capi.StringChunksStats()
                t0 = time.perf_counter()
                rc = Y.mrp_phase_string_chunks(ctx, args.n, args.arr, C.byref(f), C.byref(r), 4, 512, 0.0, C.byref(params), 0, args.res, args.hp, args.pp, None,
                                               C.byref(st))
                ms = 1e3 * (time.perf_counter() - t0)
                if rc != capi.MRP_OK:
                    raise RuntimeError(Y.mrp_last_error().decode())
                info = dict(host_ms=round(st.host_ms, 2), phase_ms=round(st.total_ms - st.host_ms, 2), pairhmm_kernel_ms=round(st.pairhmm.kernel_ms, 2))
            else:
                st = capi.QueueStats()
                t0 = time.perf_counter()
                rc = L.mrp_queue_phase_string_chunks(q.h, args.n, args.arr, C.byref(f), C.byref(r), 4, 512, 0.0, C.byref(params), 0, per_batch, args.res, args.hp, args.pp,
                                                     None, C.byref(st))
                ms = 1e3 * (time.perf_counter() - t0)
                capi._check(rc)
                info = dict(batches=int(st.batches), busy_ms_device0=round(st.busy_ms_per_device[0], 2), fallback_chunks=int(st.fallback_chunks))
            if rep == 0:  # the warm-up call: its outputs are the ones compared (read through this build's binding either way)
                dig = digest(args.results())
            else:
                for i in range(args.n):
                    (Y if ctx is not None else L).mrp_phase_result_destroy(args.res[i])
                times.append(ms)
                extra[ms] = info
        med = sorted(times)[len(times) // 2]
        rows.append(dict(shape=name, chunks=len(chunks), units=int(units), reps_ms=[round(x, 2) for x in times], median_ms=round(med, 2),
                         spread_pct=round(100.0 * (max(times) - min(times)) / med, 1), digest=dig, **extra[med]))
        print(f"leg {a.queue_leg} {name}: {rows[-1]['reps_ms']} ms", file=sys.stderr, flush=True)
    if ctx is not None:
        Y.mrp_context_destroy(ctx)
    else:
        q.close()
    with open(a.leg_out, "w") as fh:
        json.dump(rows, fh)


def filtered_shapes(small, large):
    out = []
    for name, chunks in (("config2_130_sites_60x", [synth.make_string_chunk(seed=3000 + i, n_sites=130, coverage=60, allele_len=25) for i in range(small)]),
                         ("2000_sites_60x", [synth.make_string_chunk(seed=4000 + i, n_sites=2000, coverage=60, allele_len=25, span=(10, 60)) for i in range(large)])):
        pairs = [synth.split_filtered(c, seed=7000 + i) for i, c in enumerate(chunks)]
        out.append((name, [p[0] for p in pairs], [p[1] for p in pairs]))
    return out


def chain_sites(chunks, rests, front):
    """the chain's two host assemblies over every chunk of the call, read indices global to the call: (variants, partition sites,
    strands, primary tags) as capi._haptag_sites takes them (tests/string_filtered_cases.py states the rules)"""
    variants, psites, strands, tags_all, base = [], [], [], [], 0
    for c, rest, g in zip(chunks, rests, front):
        n_primary, n_f = len(c.read_names), len(rest["forward_strand"])
        tags = np.where((g["hap"] == 1) | (g["hap"] == 2), g["hap"], 0).astype(np.int32)
        strands += [c.read_forward_strand, rest["forward_strand"]]
        tags_all += [tags, np.zeros(n_f, np.int32)]
        for alleles, gt, entries in rest["variants"]:
            variants.append((alleles, gt, [(base + q, sub) for q, sub in entries]))
        res = g["result"]
        for j in range(int(res["length"])):
            b = int(res["ref_start"]) + j
            alleles, reads, subs = c.bubbles[b]
            entries = [(base + n_primary + fr, sub) for fr, sub in rest["fsubs"][b]]
            entries += [(base + q, sub) for q, sub in sorted(zip(reads, subs), key=lambda x: x[0]) if tags[q] == 0]
            psites.append((alleles, (int(res["hap1"][j]), int(res["hap2"][j])), entries))
        base += n_primary + n_f
    return variants, psites, np.concatenate(strands).astype(np.uint8), np.concatenate(tags_all), base


def filtered_leg(a):
    """one leg in this process: per shape a warm-up and a.reps timed calls -> JSON file a.leg_out"""
    import pickle
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    L = capi.load()
    with open(a.inputs, "rb") as fh:
        shapes = pickle.load(fh)
    Y, ctx = L, None
    if a.filtered_leg == "a":
        if a.yardstick_lib:
            Y = C.CDLL(a.yardstick_lib)
            Y.mrp_runtime_init()
            for fn in ("mrp_context_create", "mrp_context_destroy", "mrp_phase_string_chunks", "mrp_phase_result_destroy", "mrp_last_error",
                       "mrp_phase_variants_from_tagged_reads", "mrp_partition_reads_by_haplotype"):
                getattr(Y, fn).argtypes = getattr(L, fn).argtypes
                getattr(Y, fn).restype = getattr(L, fn).restype
        ctx = C.c_void_p()
        if Y.mrp_context_create(0, C.byref(ctx)) != capi.MRP_OK:
            raise RuntimeError(Y.mrp_last_error().decode())
    else:
        gctx = capi.Context(0)
    ok = lambda rc: None if rc == capi.MRP_OK else (_ for _ in ()).throw(RuntimeError(Y.mrp_last_error().decode()))
    ptr = lambda x: None if x.size == 0 else x.ctypes.data
    rows = []
    for name, chunks, rests in shapes:
        structs = [capi.string_chunk_struct(c) for c in chunks]
        times, info_at, dig = [], {}, None
        if a.filtered_leg == "a":
            assembled = None
            for rep in range(a.reps + 1):
                args = capi.StringChunkArgs(chunks, False, structs)
                st = capi.StringChunksStats()
                t0 = time.perf_counter()
                ok(Y.mrp_phase_string_chunks(ctx, args.n, args.arr, C.byref(f), C.byref(r), 4, 512, 0.0, C.byref(params), 0, args.res, args.hp, args.pp, None, C.byref(st)))
                ms = 1e3 * (time.perf_counter() - t0)
                if assembled is None:  # the warm-up call: the two host assemblies, once (the tags are the same in every call)
                    front = args.results()
                    variants, psites, strands, tags, n_all = chain_sites(chunks, rests, front)
                    V, vkeep = capi._haptag_sites(variants)
                    P, pkeep = capi._haptag_sites(psites)
                    assembled = True
                else:
                    for i in range(args.n):
                        Y.mrp_phase_result_destroy(args.res[i])
                state, cis, trans = np.zeros(len(variants), np.int32), np.zeros(len(variants)), np.zeros(len(variants))
                hap, h1, h2 = np.zeros(n_all, np.int32), np.zeros(n_all), np.zeros(n_all)
                sv, sp = capi.PairHmmStats(), capi.PairHmmStats()
                t0 = time.perf_counter()
                ok(Y.mrp_phase_variants_from_tagged_reads(ctx, C.byref(f), C.byref(r), C.byref(V), n_all, ptr(strands), ptr(tags), 4, 512, ptr(state), ptr(cis), ptr(trans),
                                                          C.byref(sv)))
                ok(Y.mrp_partition_reads_by_haplotype(ctx, C.byref(f), C.byref(r), C.byref(P), n_all, ptr(strands), 4, ptr(hap), ptr(h1), ptr(h2), C.byref(sp)))
                ms += 1e3 * (time.perf_counter() - t0)
                pairs = [int(x.pairs_lane + x.pairs_wave) for x in (st.pairhmm, sv, sp)]
                info = dict(pairs_front=pairs[0], pairs_variants=pairs[1], pairs_partition=pairs[2], pairs=sum(pairs), front_ms=round(st.total_ms, 2),
                            variants_ms=round(sv.total_ms, 2), partition_ms=round(sp.total_ms, 2),
                            pairhmm_kernel_ms=round(st.pairhmm.kernel_ms + sv.kernel_ms + sp.kernel_ms, 2))
                if rep == 0:
                    tagged = tags != 0
                    dig = hashlib.sha256(b"".join(x.tobytes() for x in (np.where(tagged, tags, hap), np.where(tagged, 0.0, h1), np.where(tagged, 0.0, h2), state, cis, trans))).hexdigest()
                else:
                    times.append(ms)
                    info_at[ms] = info
        else:
            rstructs = [capi.string_chunk_rest_struct(c, x) for c, x in zip(chunks, rests)]
            for rep in range(a.reps + 1):
                args = capi.StringFilteredArgs(chunks, rests, False, structs, rstructs)
                st = capi.StringFilteredStats()
                t0 = time.perf_counter()
                capi._check(L.mrp_phase_string_chunks_with_filtered(gctx.h, args.n, args.arr, args.rarr, C.byref(f), C.byref(r), 4, 512, 0.0, C.byref(params), 0, args.res,
                                                                    args.hp, args.pp, None, args.fout, C.byref(st)))
                ms = 1e3 * (time.perf_counter() - t0)
                out = args.results()
                info = dict(pairs=int(st.pairs_scored), pairs_speculative=int(st.pairs_speculative), pairs_read_by_results=int(st.pairs_read_by_results),
                            filtered_kernels_ms=round(st.filtered_ms, 3), pairhmm_kernel_ms=round(st.chunks.pairhmm.kernel_ms, 2), host_ms=round(st.chunks.host_ms, 2),
                            phase_ms=round(st.chunks.total_ms - st.chunks.host_ms, 2))
                if rep == 0:
                    cat = lambda k: np.concatenate([o["filtered"][k] for o in out])
                    dig = hashlib.sha256(b"".join(cat(k).tobytes() for k in ("read_hap", "h1", "h2", "variant_state", "cis", "trans"))).hexdigest()
                else:
                    times.append(ms)
                    info_at[ms] = info
        med = sorted(times)[len(times) // 2]
        rows.append(dict(shape=name, chunks=len(chunks), reps_ms=[round(x, 2) for x in times], median_ms=round(med, 2), digest=dig, **info_at[med]))
        print(f"leg {a.filtered_leg} {name}: {rows[-1]['reps_ms']} ms", file=sys.stderr, flush=True)
    if ctx is not None:
        Y.mrp_context_destroy(ctx)
    else:
        gctx.close()
    with open(a.leg_out, "w") as fh:
        json.dump(rows, fh)


def filtered_probe(a):
    import pickle
    out = a.out or os.path.join(ROOT, "profiles", "string_chunks", "filtered.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    import tempfile
    shapes = filtered_shapes(a.small, a.large)
    fd, inputs = tempfile.mkstemp(suffix=".pkl")  # the legs read the same inputs; removed whatever happens
    try:
        with os.fdopen(fd, "wb") as fh:
            pickle.dump(shapes, fh, protocol=4)
        print("inputs written", file=sys.stderr, flush=True)
        runs = filtered_legs(a, out, inputs)
    finally:
        os.remove(inputs)
    filtered_report(a, out, shapes, runs)


def filtered_legs(a, out, inputs):
    runs = {"a": [], "b": []}
    for leg in ["a", "b"] * a.rounds:
        path = f"{out}.leg_{leg}"
        cmd = [sys.executable, os.path.abspath(__file__), "--filtered-leg", leg, "--leg-out", path, "--inputs", inputs, "--reps", str(a.reps)]
        if leg == "a" and a.yardstick_lib:
            cmd += ["--yardstick-lib", os.path.abspath(a.yardstick_lib)]
        subprocess.run(cmd, check=True, timeout=a.leg_timeout, cwd=ROOT)  # one GPU process at a time; a failed leg ends the probe
        with open(path) as fh:
            runs[leg].append(json.load(fh))
        os.remove(path)
    return runs


def filtered_report(a, out, shapes, runs):
    rows = []
    for i, (name, chunks, rests) in enumerate(shapes):
        legs = {}
        for leg in ("a", "b"):
            per = [p[i] for p in runs[leg]]
            times = sorted(t for r in per for t in r["reps_ms"])
            med = times[len(times) // 2]
            at = min(per, key=lambda r: abs(r["median_ms"] - med))
            legs[leg] = dict({k: v for k, v in at.items() if k not in ("shape", "chunks", "reps_ms", "median_ms", "digest")}, reps_ms=[r["reps_ms"] for r in per],
                             median_ms=med, min_ms=times[0], max_ms=times[-1], digest=per[0]["digest"] if len({r["digest"] for r in per}) == 1 else None)
        ca, nb = legs["a"], legs["b"]
        bound = ca["median_ms"] + (ca["max_ms"] - ca["min_ms"])
        rows.append(dict(shape=name, chunks=len(chunks), sites=sum(len(c.bubbles) for c in chunks), primary_reads=sum(len(c.read_names) for c in chunks),
                         filtered_reads=sum(len(x["forward_strand"]) for x in rests), filtered_variants=sum(len(x["variants"]) for x in rests),
                         chain=ca, one_call=nb, one_call_over_chain=round(nb["median_ms"] / ca["median_ms"], 3),
                         condition="one call's median <= chain's median + chain's (max - min)", bound_ms=round(bound, 2), condition_met=bool(nb["median_ms"] <= bound),
                         pairs_one_call_over_chain=round(nb["pairs"] / max(ca["pairs"], 1), 3),
                         pairs_scored_over_read_by_results=round(nb["pairs"] / max(nb["pairs"] - nb["pairs_speculative"] + nb["pairs_read_by_results"], 1), 3),
                         outputs_equal=bool(ca["digest"] is not None and ca["digest"] == nb["digest"])))
    row = dict(probe="string_chunks_filtered", device=0, cpu=cpu_model(), reps=a.reps, processes_per_leg=a.rounds,
               yardstick="the chain of existing calls of " + ("the library given as --yardstick-lib" if a.yardstick_lib else "this build"), shapes=rows)
    print(json.dumps(row), flush=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(row, indent=1) + "\n")
    if not all(s_["outputs_equal"] for s_ in rows):
        raise SystemExit("the legs' outputs differ")


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def queue_probe(a):
    out = a.out or os.path.join(ROOT, "profiles", "string_chunks", "queue.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    runs = {}
    for leg, env_extra in [("a", {}), ("b", {"MRP_QUEUE_LANES": "1"}), ("c", {}), ("d", {})] * a.rounds:
        env = {k: v for k, v in os.environ.items() if k != "MRP_QUEUE_LANES"}
        env.update(env_extra)
        path = f"{out}.leg_{leg}"
        cmd = [sys.executable, os.path.abspath(__file__), "--queue-leg", leg, "--leg-out", path, "--small", str(a.small), "--large", str(a.large),
               "--long", str(a.long), "--lane-batch", str(a.lane_batch), "--reps", str(a.reps), "--host-threads", str(a.host_threads)]
        if leg == "a" and a.yardstick_lib:
            cmd += ["--yardstick-lib", os.path.abspath(a.yardstick_lib)]
        subprocess.run(cmd, check=True, env=env, timeout=a.leg_timeout, cwd=ROOT)  # one GPU process at a time; a failed leg ends the probe
        with open(path) as fh:
            runs.setdefault(leg, []).append(json.load(fh))
        os.remove(path)
    legs = {}
    for leg, per_process in runs.items():  # a leg's processes as one sample: the median and the spread over all their timed calls
        legs[leg] = []
        for rows in zip(*per_process):
            times = sorted(t for r in rows for t in r["reps_ms"])
            med = times[len(times) // 2]
            at_median = min(rows, key=lambda r: abs(r["median_ms"] - med))
            row = dict(at_median, reps_ms=[r["reps_ms"] for r in rows], process_medians_ms=[r["median_ms"] for r in rows], median_ms=med,
                       spread_pct=round(100.0 * (times[-1] - times[0]) / med, 1), digest=rows[0]["digest"] if len({r["digest"] for r in rows}) == 1 else None)
            legs[leg].append(row)
    shapes = []
    strip = lambda d: {k: v for k, v in d.items() if k not in ("shape", "chunks", "units", "digest")}
    for ra, rb, rc, rd in zip(legs["a"], legs["b"], legs["c"], legs["d"]):
        shapes.append(dict(shape=ra["shape"], chunks=ra["chunks"], units=ra["units"], one_call=strip(ra), queue_1_lane=strip(rb), queue_default_lanes=strip(rc),
                           queue_default_lanes_caller_batches=strip(rd), queue_caller_batches_over_one_call=round(rd["median_ms"] / ra["median_ms"], 3),
                           queue_1_lane_over_one_call=round(rb["median_ms"] / ra["median_ms"], 3),
                           queue_default_lanes_over_one_call=round(rc["median_ms"] / ra["median_ms"], 3),
                           outputs_equal=bool(ra["digest"] is not None and ra["digest"] == rb["digest"] == rc["digest"] == rd["digest"])))
    row = dict(probe="string_chunks_queue", device=0, cpu=cpu_model(), reps=a.reps, processes_per_leg=a.rounds, caller_batch=a.lane_batch, host_threads=a.host_threads or "library default",
               yardstick="mrp_phase_string_chunks of " + ("the library given as --yardstick-lib" if a.yardstick_lib else "this build"), shapes=shapes)
    print(json.dumps(row), flush=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(row) + "\n")
    if not all(s["outputs_equal"] for s in shapes):
        raise SystemExit("the legs' outputs differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=96, help="chunks of the config-2 shape")
    ap.add_argument("--large", type=int, default=12, help="chunks of 2 000 sites")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/string_chunks/probe.json, with --queue profiles/string_chunks/queue.json")
    ap.add_argument("--queue", action="store_true", help="the work queue over string chunks against the one call (see above)")
    ap.add_argument("--long", type=int, default=1536, help="--queue: chunks of the long queue (the first shape repeated)")
    ap.add_argument("--yardstick-lib", default=None, help="--queue: the library whose one call is leg (a)")
    ap.add_argument("--leg-timeout", type=int, default=400, help="--queue: seconds a leg's process may take")
    ap.add_argument("--lane-batch", type=int, default=192, help="--queue: chunks per batch of leg (d)")
    ap.add_argument("--rounds", type=int, default=2, help="--queue: processes per leg, run in turn (a b c d a b c d): timings of one shape differ more between processes than within one")
    ap.add_argument("--host-threads", type=int, default=0, help="--queue: mrp_set_host_threads before the legs (the queue: per device); 0 = the library's choice")
    ap.add_argument("--filtered", action="store_true", help="the back half inside the call against the chain of existing calls (see above)")
    ap.add_argument("--filtered-leg", choices=("a", "b"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--inputs", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--queue-leg", choices=("a", "b", "c", "d"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.filtered_leg:
        return filtered_leg(a)
    if a.filtered:
        if a.rounds == 2:
            a.rounds = 3  # (a b a b a b unless asked otherwise)
        return filtered_probe(a)
    if a.queue_leg:
        return queue_leg(a)
    if a.queue:
        return queue_probe(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "string_chunks", "probe.json")
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    shapes = probe_shapes(a.small, a.large)
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
