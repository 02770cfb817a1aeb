#!/usr/bin/env python3
"""Timing probe of mrp_posterior_aligned_pairs: kernel time (HIP events) of its forward and traceback kernels, pairs/s and band cells/s
of each, the bytes that return per pair, and beside them mrp_forward_probabilities on the same pairs in the same run.
Two shapes: --short N pairs of 100 x ~97 with the reference's default parameters (one traceback each), --long N pairs of
--long-len x --long-len anchored on the diagonal every 16 symbols (a band of 37 cells; a traceback every 1 000 diagonals).
--wide adds a third: unanchored pairs of --wide-len x --wide-len (2 500: a widest diagonal of 2 501 cells, one traceback over the whole
matrix), as many as the default posterior workspace holds, on the pair-per-workgroup kernels (posterior wide pairs on), with
mrp_forward_probabilities' pair-per-workgroup kernel (wide pairs on) beside them.
--rle runs every shape a second time in the same run with run-length emissions (mrp_posterior_aligned_pairs_rle,
mrp_forward_probabilities_rle): the same strings with counts 1 + geometric and the shipped repeat matrix of
tests/golden/repeat_matrix_r94_g507.npz, and prints the run-length kernels' times with their ratio to the nucleotide ones.
--tiny N (with --rle) adds what the pair-per-lane kernel is for, N unanchored pairs of 25 x ~25, to the forward entries alone, three
times: the nucleotide entry (a pair per lane), the run-length entry as it is by default (a pair per wave), and the run-length entry with
mrp_context_set_rle_lane_pairs on (a pair per lane where every count is below the kernel's bound).  --tiny-len L: x strings of L symbols
in place of 25."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from margin_amd import capi, synth  # noqa: E402


def short_pairs(n, seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        sx = synth.random_sequence(rng, 100)
        pairs.append((sx, synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05), []))
    return pairs


def long_pairs(n, length, seed):
    rng = np.random.default_rng(seed)
    anchors = [(i, i) for i in range(8, length - 8, 16)]
    pairs = []
    for _ in range(n):
        sx = synth.random_sequence(rng, length)
        sy = sx.copy()
        hit = rng.random(length) < 0.15  # substitutions only: the diagonal anchors stay valid
        sy[hit] = rng.integers(0, 4, size=int(hit.sum()))
        pairs.append((sx, sy, anchors))
    return pairs


def wide_pairs(length, seed):
    """as many as fit MRP_POSTERIOR_DEFAULT_WORKSPACE together (24 B per cell of the whole matrix): one group, one launch"""
    n = max(1, (1 << 30) // (24 * (length + 1) ** 2))
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        sx = synth.random_sequence(rng, length)
        sy = sx.copy()
        hit = rng.random(length) < 0.15  # substitutions only: every pair has the same cells
        sy[hit] = rng.integers(0, 4, size=int(hit.sum()))
        pairs.append((sx, sy, []))
    return pairs


def pack(pairs):
    pool, xo, xl, yo, yl, ao, an, at = [], [], [], [], [], [0], [], 0
    for sx, sy, anchors in pairs:
        xo.append(at); xl.append(len(sx)); at += len(sx)
        yo.append(at); yl.append(len(sy)); at += len(sy)
        pool += [sx, sy]
        an += [v for a in anchors for v in a]
        ao.append(len(an) // 2)
    return (np.concatenate(pool), np.array(xo, np.int64), np.array(xl, np.int32), np.array(yo, np.int64), np.array(yl, np.int32),
            np.array(ao, np.int64), np.array(an, np.int64))


def shipped_repeat_model():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "repeat_matrix_r94_g507.npz")
    return capi.RepeatModel(np.load(path)["log_prob_F"], strand=1)


def probe(ctx, models, name, pairs, opt, repeat, rle=False):
    pool, xo, xl, yo, yl, ao, an = pack(pairs)
    n = len(pairs)
    rows, rle_rows = [], []
    if rle:
        rm = [shipped_repeat_model()]
        counts = np.minimum(np.random.default_rng(8).geometric(0.5, size=pool.size), rm[0].max_repeat - 1).astype(np.uint8)
    for r in range(repeat + 1):  # the first run warms the code objects and the context's pool
        match, _gx, _gy, total, st = capi.posterior_aligned_pairs(ctx, models, pool, xo, xl, yo, yl, None, ao, an, opt)
        ps = ctx.last_posterior()
        fwd, fst = capi.forward_probabilities(ctx, models, pool, xo, xl, yo, yl, None, ao, an, expansion=opt.expansion)
        if r:
            rows.append((ps.forward_ms, ps.traceback_ms, ps.total_ms, fst.kernel_ms, fst.total_ms))
        if rle:  # the same strings, in the same run
            rmatch, _gx, _gy, rtotal, _ = capi.posterior_aligned_pairs_rle(ctx, models, rm, pool, counts, xo, xl, yo, yl, None, ao, an, opt)
            rps = ctx.last_posterior()
            rfwd, rfst = capi.forward_probabilities_rle(ctx, models, rm, pool, counts, xo, xl, yo, yl, None, ao, an, expansion=opt.expansion)
            if r:
                rle_rows.append((rps.forward_ms, rps.traceback_ms, rps.total_ms, rfst.kernel_ms, rfst.total_ms))
    assert (total == fwd).all()
    f_ms, t_ms, call_ms, y_ms, ycall_ms = (float(np.median([row[k] for row in rows])) for k in range(5))
    print(f"{name}: {n} pairs, {ps.cells} band cells, {ps.traceback_cells} walked back, {ps.groups} group(s), with_gaps={int(opt.with_gaps)}, "
          f"{int(match['first'][-1])} match pairs", flush=True)
    print(f"  forward kernel   {f_ms:9.3f} ms  {n / f_ms * 1e3:.3e} pairs/s  {ps.cells / f_ms * 1e3:.3e} band cells/s", flush=True)
    print(f"  traceback kernel {t_ms:9.3f} ms  {n / t_ms * 1e3:.3e} pairs/s  {ps.traceback_cells / t_ms * 1e3:.3e} band cells/s", flush=True)
    print(f"  call             {call_ms:9.3f} ms  {n / call_ms * 1e3:.3e} pairs/s; {ps.downloaded_bytes / n:.1f} B downloaded per pair "
          f"({ps.candidates} candidates)", flush=True)
    print(f"  mrp_forward_probabilities on the same pairs: kernel {y_ms:.3f} ms  {fst.cells / y_ms * 1e3:.3e} cells/s, call {ycall_ms:.3f} ms "
          f"(lane {fst.pairs_lane}, wave {fst.pairs_wave})", flush=True)
    if rle:
        assert (rtotal == rfwd).all()
        rf_ms, rt_ms, rcall_ms, ry_ms, _ = (float(np.median([row[k] for row in rle_rows])) for k in range(5))
        print(f"  run-length emissions on the same strings ({int(rmatch['first'][-1])} match pairs; lane {rfst.pairs_lane}, wave {rfst.pairs_wave}):", flush=True)
        print(f"    forward kernel   {rf_ms:9.3f} ms  x{rf_ms / f_ms:.3f} of the nucleotide kernel", flush=True)
        print(f"    traceback kernel {rt_ms:9.3f} ms  x{rt_ms / t_ms:.3f}", flush=True)
        print(f"    call             {rcall_ms:9.3f} ms  x{rcall_ms / call_ms:.3f}", flush=True)
        print(f"    mrp_forward_probabilities_rle kernel {ry_ms:.3f} ms  x{ry_ms / y_ms:.3f} of mrp_forward_probabilities' (which runs {fst.pairs_lane} pairs a lane)",
              flush=True)


def tiny_forward(ctx, models, n, repeat, length=25):
    """N pairs of 25 x ~25: mrp_forward_probabilities (a pair per lane) against mrp_forward_probabilities_rle with run-length lane pairs
    off (a pair per wave, class 64) and on (a pair per lane for the pairs whose counts are all below the bound), the same strings in
    one run.  length: the x strings' (--tiny-len; the launch class of the lane kernels depends on it, mrp_rle_lane_caps)"""
    rng = np.random.default_rng(9)
    pairs = []
    for _ in range(n):
        sx = synth.random_sequence(rng, length)
        pairs.append((sx, synth.evolve_sequence(rng, sx, 0.05, 0.05, 0.05), []))
    pool, xo, xl, yo, yl, ao, an = pack(pairs)
    rm = [shipped_repeat_model()]
    counts = np.minimum(rng.geometric(0.5, size=pool.size), rm[0].max_repeat - 1).astype(np.uint8)
    rows = []
    for r in range(repeat + 1):
        _, a = capi.forward_probabilities(ctx, models, pool, xo, xl, yo, yl, expansion=20)
        off, b = capi.forward_probabilities_rle(ctx, models, rm, pool, counts, xo, xl, yo, yl, expansion=20)
        ctx.set_rle_lane_pairs(True)
        try:
            on, c = capi.forward_probabilities_rle(ctx, models, rm, pool, counts, xo, xl, yo, yl, expansion=20)
        finally:
            ctx.set_rle_lane_pairs(False)
        assert np.array_equal(on.view(np.int64), off.view(np.int64))
        if r:
            rows.append((a.kernel_ms, b.kernel_ms, c.kernel_ms))
    lane_ms, wave_ms, rle_lane_ms = (float(np.median([row[k] for row in rows])) for k in range(3))
    print(f"tiny: {n} pairs of {length} x ~{length}, {a.cells} cells: mrp_forward_probabilities kernel {lane_ms:.3f} ms (lane {a.pairs_lane}, wave {a.pairs_wave}), "
          f"mrp_forward_probabilities_rle kernel {wave_ms:.3f} ms (lane {b.pairs_lane}, wave {b.pairs_wave})  x{wave_ms / lane_ms:.3f}", flush=True)
    print(f"      with run-length lane pairs on: kernel {rle_lane_ms:.3f} ms (lane {c.pairs_lane}, wave {c.pairs_wave})  x{rle_lane_ms / wave_ms:.3f} of the switch off "
          f"(x{wave_ms / rle_lane_ms:.2f} faster), x{rle_lane_ms / lane_ms:.3f} of the nucleotide lane kernel", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short", type=int, default=4096)
    ap.add_argument("--long", type=int, default=256)
    ap.add_argument("--long-len", type=int, default=2000)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--wide-len", type=int, default=2500)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--with-gaps", type=int, default=0)
    ap.add_argument("--rle", action="store_true")
    ap.add_argument("--tiny", type=int, default=0)
    ap.add_argument("--tiny-len", type=int, default=25)
    args = ap.parse_args()
    models = [capi.PairHmm.default_nucleotide()]
    opt = capi.PosteriorOptions(with_gaps=bool(args.with_gaps))  # threshold 0.01, expansion 20, 1 000 / 40
    with capi.Context(0) as ctx:
        if args.short:
            probe(ctx, models, "short", short_pairs(args.short, 5), opt, args.repeat, args.rle)
        if args.long:
            probe(ctx, models, "long", long_pairs(args.long, args.long_len, 6), opt, args.repeat, args.rle)
        if args.tiny and args.rle:
            tiny_forward(ctx, models, args.tiny, args.repeat, args.tiny_len)
        if args.wide:
            ctx.set_posterior_wide_pairs(True)
            ctx.set_wide_pairs(True)  # the yardstick's own switch
            before = ctx.posterior_wide_count()
            probe(ctx, models, "wide", wide_pairs(args.wide_len, 7), opt, args.repeat, args.rle)
            after = ctx.posterior_wide_count()
            print(f"  the pair-per-workgroup kernels took {after[0] - before[0]} pairs, {after[1] - before[1]} band cells over {args.repeat + 1} runs", flush=True)


if __name__ == "__main__":
    main()
