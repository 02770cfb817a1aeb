"""mrp_extract_read_substrings at margin phase's shape: 96 chunks of 100 kb with 10 kb overlaps, 30x, reads of median
~15 kb, a het variant every ~1 kb (a few distinct synthetic chunks, repeated).  Reports the wall time of the call (median
of --reps), kernel time (HIP events), bytes uploaded and the host share; aligned bases and CIGAR ops per second; a parity
sample of --parity chunks against the reference's walk (tests/extract_oracle.py); and the same chunks through
mrp_phase_string_chunks, for scale.  Prints one JSON line and writes it to --out.

    python tools/extract_probe.py [--chunks 96] [--distinct 4] [--reps 3] [--parity 16] [--cache FILE] [--out profiles/extract/probe.json]

--cache keeps the generated chunks and their oracle results (numpy pickle) so that a later run skips the slow Python parts.
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from margin_amd import capi, synth  # noqa: E402
from tests import extract_oracle as eo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=96)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parity", type=int, default=16)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract", "probe.json"))
    a = ap.parse_args()
    opts = capi.shipped_extract_options()
    key = (a.distinct, 1)
    if a.cache and os.path.exists(a.cache):
        with open(a.cache, "rb") as f:
            cached = pickle.load(f)
        assert cached["key"] == key
        distinct, oracle = cached["chunks"], cached["oracle"]
    else:
        t = time.perf_counter()
        distinct = [synth.make_aligned_chunk(seed, overlap_bp=120_000, margin_bp=10_000, coverage=30.0, read_len=(5_000, 25_000),
                                             variant_every=1_000, sv_share=0.02, oddities=False) for seed in range(a.distinct)]
        oracle = [eo.as_arrays(x) for x in eo.extract(distinct, opts)]
        print(f"generated {a.distinct} chunks and their oracle results in {time.perf_counter() - t:.0f} s", file=sys.stderr)
        if a.cache:
            with open(a.cache, "wb") as f:
                pickle.dump(dict(key=key, chunks=distinct, oracle=oracle), f)
    chunks = [distinct[i % a.distinct] for i in range(a.chunks)]
    built = [capi.aligned_chunk_struct(c) for c in chunks]
    with capi.Context(0) as ctx:
        capi.extract_read_substrings(ctx, chunks[:2], opts)  # warm-up: module load, pools
        walls, stats, got = [], [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            got, st = capi.extract_read_substrings(ctx, chunks, opts, structs=built)
            walls.append((time.perf_counter() - t) * 1e3)
            stats.append(st)
        bad = 0
        for i in range(min(a.parity, a.chunks)):
            w = oracle[i % a.distinct]
            bad += any(not np.array_equal(got[i][k], v) for k, v in w.items())
        scs = [capi.string_chunk_from_extracted(g, c.read_names, c.read_forward_strand)[0] for g, c in zip(got, chunks)]
        fwd = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
        params = capi.Params.from_reference_names(synth.shipped_phase_params())
        capi.phase_string_chunks(ctx, scs, fwd, fwd.reverse_complement(), params)
        t = time.perf_counter()
        _, pst = capi.phase_string_chunks(ctx, scs, fwd, fwd.reverse_complement(), params)
        phase_ms = (time.perf_counter() - t) * 1e3
    k = int(np.argsort(walls)[len(walls) // 2])
    st = stats[k]
    wall = walls[k]
    res = dict(chunks=a.chunks, distinct=a.distinct, reads=int(st.reads), cigar_ops=int(st.cigar_ops), aligned_bases=int(st.aligned_bases),
               substrings=int(st.entries), wall_ms=round(wall, 2), walls_ms=[round(x, 2) for x in walls], call_total_ms=round(st.total_ms, 2),
               kernel_ms=round(st.kernel_ms, 3), host_ms=round(st.host_ms, 2), host_share=round(st.host_ms / st.total_ms, 3),
               bytes_uploaded=int(st.bytes_uploaded), aligned_bases_per_s=round(st.aligned_bases / (wall / 1e3)),
               cigar_ops_per_s=round(st.cigar_ops / (wall / 1e3)), parity=f"{min(a.parity, a.chunks) - bad}/{min(a.parity, a.chunks)}",
               bubbles=int(sum(len(s.bubbles) for s in scs)), phase_string_chunks_ms=round(phase_ms, 2), phase_total_ms=round(pst.total_ms, 2))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
