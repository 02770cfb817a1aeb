#!/usr/bin/env python3
"""Timing probe of mrp_forward_probabilities on the alignment pairs of config-2 chunks (2 000 sites x ~30 reads x 2 alleles
per chunk): kernel time (HIP events), call time, cell updates per second, optional oracle check and CPU timing.
With --wide N --wide-len L instead: N unanchored pairs of L x L on a context with wide pairs on (L <= 2 047: the pair-per-wave
kernel, beyond: the pair-per-workgroup kernel), warm, the median kernel time of --repeat runs and cells/s."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from margin_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--sites", type=int, default=2000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check", type=int, default=2000, help="pairs compared with the oracle")
    ap.add_argument("--wide", type=int, default=0, help="score this many unanchored pairs of --wide-len x --wide-len with wide pairs on")
    ap.add_argument("--wide-len", type=int, default=2060)
    args = ap.parse_args()
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    models = [f, f.reverse_complement()]
    if args.wide:
        return wide(args, models)
    t0 = time.time()
    bubbles = []
    for c in range(args.chunks):
        bubbles += synth.make_bubble_strings(seed=c + 1, n_sites=args.sites, coverage=args.coverage)
    pool, xo, xl, yo, yl, mi = synth.pairs_from_bubbles(bubbles)
    print(f"synth {time.time() - t0:.1f}s: {len(xo)} pairs, pool {pool.size} B", flush=True)
    ctx = capi.Context(0)
    for r in range(args.repeat):
        out, st = capi.forward_probabilities(ctx, models, pool, xo, xl, yo, yl, mi)
        print(f"run {r}: kernel {st.kernel_ms:.3f} ms, call {st.total_ms:.2f} ms, {len(xo) / st.kernel_ms * 1e3:.3e} pairs/s, "
              f"{st.cells / st.kernel_ms * 1e3:.3e} cells/s (kernel), {len(xo) / st.total_ms * 1e3:.3e} pairs/s (call); lane {st.pairs_lane} wave {st.pairs_wave}",
              flush=True)
    if args.check:
        from oracle import pairhmm as ph
        rng = np.random.default_rng(0)
        pick = np.sort(rng.choice(len(out), size=min(args.check, len(out)), replace=False))
        om = [ph.Model.from_buffer_copy(bytes(m)) for m in models]
        t0 = time.perf_counter()
        ref = ph.forward_batch(om, pool, xo[pick], xl[pick], yo[pick], yl[pick], mi[pick])
        dt = time.perf_counter() - t0
        print(f"oracle: {len(pick) / dt:.3e} pairs/s on one core; identical={bool((ref == out[pick]).all())}", flush=True)


def wide(args, models):
    rng = np.random.default_rng(args.wide_len)
    n, ln = args.wide, args.wide_len
    strings = []
    for _ in range(n):
        a = synth.random_sequence(rng, ln)
        b = synth.evolve_sequence(rng, a, 0.02, 0.01, 0.01)
        strings += [a, np.concatenate([b, synth.random_sequence(rng, ln)])[:ln]]
    pool = np.concatenate(strings)
    xo = np.arange(n, dtype=np.int64) * 2 * ln
    xl = np.full(n, ln, np.int32)
    mi = (np.arange(n) % 2).astype(np.uint8)
    ctx = capi.Context(0)
    ctx.set_wide_pairs(1)
    capi.forward_probabilities(ctx, models, pool, xo, xl, xo + ln, xl, mi)  # warm: code objects, the context's pool
    ms = []
    for r in range(max(1, args.repeat)):
        out, st = capi.forward_probabilities(ctx, models, pool, xo, xl, xo + ln, xl, mi)
        ms.append(st.kernel_ms)
    med = float(np.median(ms))
    pairs, _cells = ctx.wide_pair_count()
    print(f"wide probe: {n} pairs of {ln} x {ln}, {'pair-per-workgroup' if pairs else 'pair-per-wave'} kernel: kernel ms {[round(x, 3) for x in ms]}, "
          f"median {med:.3f} ms, {st.cells / med * 1e3:.3e} cells/s, finite={bool(np.isfinite(out).all())}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
