#!/usr/bin/env python3
"""Timing probe of mrp_ml_repeat_counts on one polish chunk's worth: --nodes consensus nodes (70 000: a 100 kb chunk) under --reads reads
that span the consensus, one match per read and node plus --secondary (0.1) times as many secondary matches of a neighbouring node, run
lengths 1 + geometric(0.5) with +-1 noise, random weights and strands, the shipped r9.4 g507 matrix; unphased and phased (a random half of
the reads in the haplotype, s = log(0.0001)).

Reports the stats' four times (upload, ordering, estimate: HIP events; total: host wall time of the call) as the median of --runs warm
runs, made --repeats times.  Beside them, the yardstick: the same loop as a plain sequential C restatement on one host thread
(tools/hostcheck/repeat_counts_host_check.cpp built with -DRC_TIMING_ONLY, no sanitizers; the fastest of three), on the same arrays, whose
counts and log probabilities must equal the device's bit for bit -- the probe fails otherwise."""
import argparse
import json
import math
import os
import statistics
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from margin_amd import capi  # noqa: E402
from tests import repeat_count_cases as cases  # noqa: E402
from tests import rle_cases as rc  # noqa: E402

HOST_SRC = os.path.join(ROOT, "tools", "hostcheck", "repeat_counts_host_check.cpp")
HOST_EXE = os.path.join(ROOT, "tools", "hostcheck", "repeat_counts_host_time")


def host_program():
    if not os.path.exists(HOST_EXE) or os.path.getmtime(HOST_EXE) < os.path.getmtime(HOST_SRC):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DRC_TIMING_ONLY", HOST_SRC, "-o", HOST_EXE])
    return HOST_EXE


def chunk(nodes, reads, secondary, seed):
    """-> the flat arguments of capi.ml_repeat_counts for one consensus"""
    cons, matches = cases.spanning_consensus(np.random.default_rng(seed), nodes, reads, secondary=secondary)
    y_len = np.array([len(c) for c in cons["read_counts"]], np.int32)
    y_off = np.concatenate([[0], np.cumsum(y_len)[:-1]]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum([len(m) for m in matches])]).astype(np.int64)
    m = np.concatenate(matches)
    return dict(node_first=np.array([0, nodes], np.int64), symbols=cons["symbols"], read_first=np.array([0, reads], np.int64),
                counts=np.concatenate(cons["read_counts"]), y_off=y_off, y_len=y_len, read_forward_strand=cons["strands"],
                matches=dict(first=first, x=m[:, 0].astype(np.int32), y=m[:, 1].astype(np.int32), weight=m[:, 2].astype(np.int32)))


def write_host_file(path, table, p, walk_backwards, hap, s):
    def vec(f, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        f.write(struct.pack("<q", a.size))
        f.write(a.tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<iiid", table.shape[1], int(walk_backwards), int(hap is not None), float(s)))
        vec(f, table, np.float64); vec(f, p["symbols"], np.uint8); vec(f, p["counts"], np.uint8); vec(f, p["read_forward_strand"], np.uint8)
        vec(f, hap if hap is not None else np.zeros(len(p["y_off"]), np.uint8), np.uint8)
        vec(f, p["y_off"], np.int64); vec(f, p["matches"]["first"], np.int64); vec(f, np.zeros(len(p["y_off"]), np.int32), np.int32)
        vec(f, p["matches"]["x"], np.int32); vec(f, p["matches"]["y"], np.int32); vec(f, p["matches"]["weight"], np.int32)


def fnv(lp):
    h = 1469598103934665603
    for bits in lp.view(np.uint64).tolist():
        h = ((h ^ bits) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=70000)
    ap.add_argument("--reads", type=int, default=40)
    ap.add_argument("--secondary", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    table = rc.shipped_matrix()
    p = chunk(a.nodes, a.reads, a.secondary, a.seed)
    hap = np.random.default_rng(a.seed + 1).integers(0, 2, size=a.reads).astype(np.uint8)
    out = dict(nodes=a.nodes, reads=a.reads, matches=int(p["matches"]["first"][-1]), legs={})
    exe = host_program()
    with capi.Context(0) as ctx, tempfile.TemporaryDirectory() as tmp:
        for leg, h, s in (("unphased", None, 0.0), ("phased", hap, math.log(0.0001))):
            call = lambda: capi.ml_repeat_counts(ctx, table, walk_backwards=True, read_in_hap=h, log_het_substitution=s, **p)
            count, lp, length, st = call()  # cold
            medians = []
            for _ in range(a.repeats):
                runs = [call()[3] for _ in range(a.runs)]
                medians.append({k: statistics.median(getattr(r, k) for r in runs) for k in ("upload_ms", "ordering_ms", "estimate_ms", "total_ms")})
            path = os.path.join(tmp, leg + ".bin")
            write_host_file(path, table, p, True, h, s)
            host_ms, host_sum, host_hash = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.split()
            if int(host_sum) != int(length[0]) or int(host_hash, 16) != fnv(lp):
                raise SystemExit(f"{leg}: the sequential restatement and the device differ ({host_sum} vs {int(length[0])})")
            out["legs"][leg] = dict(medians=medians, host_ms=float(host_ms), observations=st.observations, nodes_observed=st.nodes_observed,
                                    candidates=st.candidates, bytes_uploaded=st.bytes_uploaded, bytes_downloaded=st.bytes_downloaded,
                                    non_rle_length=int(length[0]))
            print(f"{leg}: {st.observations} observations of {st.nodes_observed} nodes, {st.candidates} candidates, {st.bytes_uploaded} B up, "
                  f"{st.bytes_downloaded} B down; equal to the sequential restatement bit for bit")
            for i, m in enumerate(medians):
                print(f"  run {i}: upload {m['upload_ms']:.3f} ms, ordering {m['ordering_ms']:.3f} ms, estimate {m['estimate_ms']:.3f} ms, total {m['total_ms']:.3f} ms")
            print(f"  sequential C on one host thread: {float(host_ms):.1f} ms")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
