#!/usr/bin/env python3
"""Timing probe of mrp_poa_augment on one polish chunk's worth: --nodes reference positions (70 000: a 100 kb chunk) under --reads reads
that span them, the three lists from the seeded noise model of tests/poa_cases.py (substitutions, short indels, homopolymer-length errors,
low-weight alternatives beside the path), R of the shipped r9.4 g507 matrix, then mrp_poa_consensus on the result.

Reports the stats' stage times (HIP events), the host's check time and the call's wall time as the median of --runs warm runs, made
--repeats times, and the consensus walk's time.  Beside them, the yardstick: the same loops as a plain sequential C restatement on one
host thread (tools/hostcheck/poa_host_check.cpp built with -DPOA_TIMING_ONLY -O2, no sanitizers; the fastest of three) over the same
arrays, whose every output must equal the device's bit for bit -- the probe fails otherwise."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from margin_amd import capi  # noqa: E402
from tests import poa_cases as cases  # noqa: E402
from tests import rle_cases as rc  # noqa: E402

HOST_SRC = os.path.join(ROOT, "tools", "hostcheck", "poa_host_check.cpp")
HOST_EXE = os.path.join(ROOT, "tools", "hostcheck", "poa_host_time")
NAMES = ("node_first", "symbols", "ref_counts", "read_first", "read_symbols", "read_counts", "y_off", "y_len", "read_forward_strand", "matches",
         "deletes", "inserts")
OUT_ORDER = (("base_weight", np.float64), ("base_pick", np.int32), ("repeat_count_pick", np.int32), ("insert_first", np.int64), ("insert_str_off", np.int64),
             ("insert_str_len", np.int32), ("insert_weight_forward", np.float64), ("insert_weight_reverse", np.float64), ("insert_n_observations", np.int64),
             ("pool_symbols", np.uint8), ("pool_counts", np.int32), ("delete_first", np.int64), ("delete_length", np.int32),
             ("delete_weight_forward", np.float64), ("delete_weight_reverse", np.float64), ("delete_n_observations", np.int64), ("totals", np.float64))
STAGES = ("check_ms", "upload_ms", "sets_ms", "enumerate_ms", "group_ms", "picks_ms", "total_ms")


def host_program():
    if not os.path.exists(HOST_EXE) or os.path.getmtime(HOST_EXE) < os.path.getmtime(HOST_SRC):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPOA_TIMING_ONLY", HOST_SRC, "-o", HOST_EXE])
    return HOST_EXE


def write_host_file(path, R, p, x_shift, compare, merge, penalty):
    with open(path, "wb") as f:
        f.write(struct.pack("<6q", R, len(p["node_first"]) - 1, p["read_symbols"].size, int(compare), int(merge), len(p["y_off"])))
        f.write(struct.pack("<d", penalty))
        for k, dt in (("node_first", np.int64), ("symbols", np.uint8), ("ref_counts", np.uint8), ("read_first", np.int64), ("read_symbols", np.uint8),
                      ("read_counts", np.uint8), ("y_off", np.int64), ("y_len", np.int32), ("read_forward_strand", np.uint8)):
            f.write(np.ascontiguousarray(p[k], dtype=dt).tobytes())
        f.write(np.ascontiguousarray(x_shift, dtype=np.int32).tobytes())
        for k in ("matches", "deletes", "inserts"):
            f.write(np.ascontiguousarray(p[k]["first"], dtype=np.int64).tobytes())
            for q in ("x", "y", "weight"):
                f.write(np.ascontiguousarray(p[k][q], dtype=np.int32).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=70000)
    ap.add_argument("--reads", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    R, penalty = rc.R_SHIPPED, 0.5
    args, x_shift = cases.pack([cases.noisy_consensus(np.random.default_rng(a.seed), a.nodes, a.reads, R)])
    p = dict(zip(NAMES, args))
    exe = host_program()
    with capi.Context(0) as ctx, tempfile.TemporaryDirectory() as tmp:
        call = lambda: capi.poa_augment(ctx, R, x_shift=x_shift, reference_base_penalty=penalty, **p)
        got = call()  # cold
        st = got["stats"]
        medians = []
        for _ in range(a.repeats):
            runs = [call()["stats"] for _ in range(a.runs)]
            medians.append({k: statistics.median(getattr(r, k) for r in runs) for k in STAGES})
        walks = []
        for _ in range(a.runs):
            t = time.perf_counter()
            s, c, _ = capi.poa_consensus(got, 0, a.nodes, True)
            walks.append((time.perf_counter() - t) * 1e3)
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        write_host_file(src, R, p, x_shift, True, True, penalty)
        host_ms = min(float(subprocess.run([exe, src, dst], capture_output=True, text=True, check=True).stdout) for _ in range(3))
        with open(dst, "rb") as f:
            host = f.read()
        device = b"".join(np.ascontiguousarray(got[k], dtype=dt).tobytes() for k, dt in OUT_ORDER)
        if host != device:
            raise SystemExit(f"the sequential restatement and the device differ ({len(host)} B against {len(device)} B)")
    out = dict(nodes=a.nodes, reads=a.reads, matches=st.matches, deletes=st.deletes, inserts=st.inserts, complete_inserts=st.complete_inserts,
               complete_deletes=st.complete_deletes, distinct_inserts=st.distinct_inserts, distinct_deletes=st.distinct_deletes, longest_run=st.longest_run,
               table_slots=st.table_slots, bytes_uploaded=st.bytes_uploaded, bytes_downloaded=st.bytes_downloaded, medians=medians, host_ms=host_ms,
               consensus_ms=statistics.median(walks), consensus_length=int(len(s)))
    print(f"{st.matches} matches, {st.deletes} deletes, {st.inserts} inserts of {a.reads} reads over {a.nodes} positions; {st.complete_inserts} complete "
          f"inserts ({st.distinct_inserts} distinct), {st.complete_deletes} complete deletes ({st.distinct_deletes} distinct), longest run {st.longest_run}; "
          f"{st.table_slots} table slots, {st.bytes_uploaded} B up, {st.bytes_downloaded} B down; equal to the sequential restatement bit for bit")
    for i, m in enumerate(medians):
        print(f"  run {i}: " + ", ".join(f"{k[:-3]} {m[k]:.3f} ms" for k in STAGES))
    print(f"  sequential C on one host thread: {host_ms:.1f} ms; mrp_poa_consensus (host): {out['consensus_ms']:.1f} ms, {len(s)} run-length symbols")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
