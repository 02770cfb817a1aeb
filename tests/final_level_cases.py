"""Inputs that put the two kernels behind every mrp_phase_reads_many call -- the trace back and the genome fragment kernel of the
final level (mrp_traceback_kernel, mrp_fragment_kernel) -- on their tile sizes and branches.  TEST INFRASTRUCTURE ONLY.

A case is a small synth.Chunk, the parameters it is phased with and the refinement round limits it is run at; facts(name) returns
what the case must exhibit, computed from the oracle alone (OracleChunk.phase with its captured forward-backward jobs) and from the
chunk's arrays.  tests/test_final_level_cases.py asserts the facts without a device, tests/test_gpu_final_level.py runs the rows on
one.  Builders, oracle chunks and oracle runs are cached: each is made once per process, whichever module asks first.

The edges (mrp_engine_final.hip):
  rounds        the refinement stops at max_iterations or at the first round that moves nothing; the lists swap between two buffers
                every moving round and are copied back after an odd number of them.  Six chunks whose last moving round m is
                0, 1, 2, 3, 4 and 5, each at the limits 0, m - 1, m, m + 1 and 10.
  column tiles  a fragment thread owns ceil(K / 1024) columns; the trace back flushes the chosen cells every 1 024 columns.
                Final hmms of 1, 2, 1 023, 1 024, 1 025 and more than 2 048 columns.
  read search   a column's reads are found by binary search among the chunk's reads, in LDS up to 6 144 reads and in HBM above:
                6 144, 6 145 and 8 653 reads.
  list tiles    a thread owns ceil((n1 + n2) / 1024) entries of the two read lists in a round's compactions: 1 024 and 1 025.
  filter        the reads the coverage filter took out are re-added by one thread, a tie going to reads1: a 40x chunk at
                maxCoverageDepth 12, some of whose reads carry one constant profile byte (such a read ties wherever it lies).
  pool order    the search order is the identity unless the profile bytes lie in another order than the reads: a rounds chunk
                with its pool rebuilt in a seeded permutation, with gaps.
  alleles       sites of MRP_MAX_ALLELES alleles next to biallelic ones in one column.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from margin_amd import synth
from oracle import orc

FRAG_T = 1024            # threads of the fragment kernel = columns / list entries per trip; the trace back's flush tile
FRAG_LDS_READS = 6144    # reads whose pool offsets the fragment kernel searches in LDS
MRP_PRUNE_MAX_S = 116    # cells a pruned column keeps at most (mrp_engine.h)
MRP_MAX_ALLELES = 16     # include/margin_rphmm.h
SHIPPED_ROUNDS = 10
ROUND_SCAN = 12          # last_moving_round is looked for in 1..12
CONSTANT_BYTE = 77       # the profile byte of the reads that tie with every haplotype


@dataclasses.dataclass(frozen=True)
class Case:
    build: object          # () -> synth.Chunk
    limit: int             # maxPartitionsInAColumn (even; minPartitionsInAColumn = 0)
    rounds: tuple          # the roundsOfIterativeRefinement the case is run at
    depth: int = 64        # maxCoverageDepth
    twin: str = None       # a case whose results this one's must equal


def params(limit: int, rounds: int, depth: int = 64) -> dict:
    pd = synth.shipped_phase_params()
    pd.update(minPartitionsInAColumn=0, maxPartitionsInAColumn=limit, roundsOfIterativeRefinement=rounds, maxCoverageDepth=depth)
    return pd


def _round_limits(m: int) -> tuple:
    """0, m - 1, m, m + 1 and the shipped 10, duplicates dropped: no refinement, a cut while reads still move, the limit on the last
    moving round, the early break, the shipped limit"""
    return tuple(sorted({r for r in (0, m - 1, m, m + 1, SHIPPED_ROUNDS) if r >= 0}))


def _truncated(chunk, n: int):
    """the same sites and pool under the first n reads (pool offsets stay valid)"""
    return dataclasses.replace(chunk, reads=list(chunk.reads[:n]))


# ---- rounds ----

# last moving round -> (maxPartitionsInAColumn, allele error, seed) of a 40-site, 30x chunk
ROUNDS_SPECS = {0: (8, 0.05, 1), 1: (4, 0.05, 0), 2: (4, 0.3, 4), 3: (4, 0.3, 0), 4: (4, 0.3, 1), 5: (4, 0.3, 5)}


@functools.lru_cache(maxsize=None)
def rounds_chunk(m: int):
    _, err, seed = ROUNDS_SPECS[m]
    return synth.make_ont_chunk(seed, region_bp=20_000, n_sites=40, coverage=30, allele_error=err)


# ---- column tiles ----

N_SPANNING, N_HALF = 14, 9


@functools.lru_cache(maxsize=None)
def spanning_chunk(halves: int):
    """Four sites under N_SPANNING reads that span all of them: one column.  halves > 0: that many further reads over the first two
    sites only (a prefix of a spanning read's bytes is a read over a prefix of its sites): two columns."""
    c = synth.make_ont_chunk(seed=2, region_bp=400, n_sites=4, coverage=40, median_len=3000.0, sigma=0.2, min_len=2000, max_len=5000,
                             allele_error=0.2)
    full = [r for r in c.reads if r.ref_start == 0 and r.length == 4]
    assert len(full) >= N_SPANNING + halves
    two = int(c.allele_offset[2] - c.allele_offset[0])
    reads = full[:N_SPANNING] + [dataclasses.replace(r, name=r.name + "_half", length=2, nbytes=two) for r in full[N_SPANNING:N_SPANNING + halves]]
    return dataclasses.replace(c, reads=reads)


# final K -> (sites, seed) of a 10x chunk of short reads
TILE_SPECS = {1023: (1184, 0), 1024: (1175, 1), 1025: (1169, 1), 2097: (2400, 0)}


@functools.lru_cache(maxsize=None)
def tile_chunk(k: int):
    n, seed = TILE_SPECS[k]
    return synth.make_ont_chunk(seed, region_bp=n * 500, n_sites=n, coverage=10, median_len=1500.0, sigma=0.3, min_len=600, max_len=4000)


# ---- read search ----

@functools.lru_cache(maxsize=None)
def many_reads_chunk():
    """900 sites under 8 653 short, noisy reads"""
    return synth.make_ont_chunk(seed=3, region_bp=450_000, n_sites=900, coverage=18, median_len=700.0, sigma=0.2, min_len=500, max_len=1200,
                                allele_error=0.3)


@functools.lru_cache(maxsize=None)
def reads_chunk(n: int):
    c = many_reads_chunk()
    return c if n == len(c.reads) else _truncated(c, n)


# ---- list tiles ----

@functools.lru_cache(maxsize=None)
def noisy_chunk():
    """120 sites under about 1 450 short, noisy reads"""
    return synth.make_ont_chunk(seed=8, region_bp=60_000, n_sites=120, coverage=18, median_len=700.0, sigma=0.2, min_len=500, max_len=1200,
                                allele_error=0.3)


@functools.lru_cache(maxsize=None)
def listed_chunk(n: int):
    return _truncated(noisy_chunk(), n)


# ---- coverage filter ----

FILTER_SEED = 3
# reads of the filter chunk whose profile bytes are all CONSTANT_BYTE: the oracle's filter discards the first three and keeps the last
CONSTANT_READS = (0, 1, 3, 2)


@functools.lru_cache(maxsize=None)
def filter_chunk():
    c = synth.make_ont_chunk(FILTER_SEED, region_bp=20_000, n_sites=40, coverage=40, allele_error=0.3)
    pool = c.pool.copy()
    for i in CONSTANT_READS:
        r = c.reads[i]
        pool[r.pool_off:r.pool_off + r.nbytes] = CONSTANT_BYTE
    return dataclasses.replace(c, pool=pool)


# ---- pool out of read order ----

PERMUTED_TWIN = 3


@functools.lru_cache(maxsize=None)
def permuted_chunk():
    """rounds_chunk(PERMUTED_TWIN) with the reads' profile bytes laid out in a seeded permutation of the read order, 1-7 random bytes
    in front of each; the reads, their order and their bytes are the twin's"""
    c = rounds_chunk(PERMUTED_TWIN)
    rng = np.random.default_rng(17)
    parts, at, off = [], 0, {}
    for i in rng.permutation(len(c.reads)):
        gap = rng.integers(0, 256, size=int(rng.integers(1, 8))).astype(np.uint8)
        r = c.reads[int(i)]
        parts += [gap, c.pool[r.pool_off:r.pool_off + r.nbytes]]
        off[int(i)] = at + len(gap)
        at += len(gap) + r.nbytes
    reads = [dataclasses.replace(r, pool_off=off[i]) for i, r in enumerate(c.reads)]
    return dataclasses.replace(c, pool=np.concatenate(parts), reads=reads)


# ---- allele counts ----

@functools.lru_cache(maxsize=None)
def alleles_chunk():
    return synth.make_ont_chunk(seed=6, region_bp=30_000, n_sites=60, coverage=25, allele_choices=(2, 3, MRP_MAX_ALLELES),
                                allele_probs=(0.5, 0.25, 0.25))


CASES = {f"rounds_m{m}": Case(functools.partial(rounds_chunk, m), ROUNDS_SPECS[m][0], _round_limits(m)) for m in ROUNDS_SPECS}
CASES.update({
    "columns_1": Case(functools.partial(spanning_chunk, 0), 8, (SHIPPED_ROUNDS,)),
    "columns_2": Case(functools.partial(spanning_chunk, N_HALF), 8, (SHIPPED_ROUNDS,)),
    **{f"columns_{k}": Case(functools.partial(tile_chunk, k), 8, (SHIPPED_ROUNDS,)) for k in TILE_SPECS},
    "reads_6144": Case(functools.partial(reads_chunk, FRAG_LDS_READS), 8, (SHIPPED_ROUNDS,)),
    "reads_6145": Case(functools.partial(reads_chunk, FRAG_LDS_READS + 1), 8, (SHIPPED_ROUNDS,)),
    "reads_8653": Case(functools.partial(reads_chunk, 8653), 8, (SHIPPED_ROUNDS,)),
    "listed_1024": Case(functools.partial(listed_chunk, FRAG_T), 8, (SHIPPED_ROUNDS,)),
    "listed_1025": Case(functools.partial(listed_chunk, FRAG_T + 1), 8, (SHIPPED_ROUNDS,)),
    # (1 round besides 0 and 10: after an odd number of rounds a tied read that moved is on the other list, after an even number only
    # further back on its own)
    "filter": Case(filter_chunk, 4, (0, 1, SHIPPED_ROUNDS), depth=12),
    "permuted_pool": Case(permuted_chunk, ROUNDS_SPECS[PERMUTED_TWIN][0], _round_limits(PERMUTED_TWIN), twin=f"rounds_m{PERMUTED_TWIN}"),
    "alleles": Case(alleles_chunk, 8, (SHIPPED_ROUNDS,)),
})
ROWS = [(name, r) for name, case in CASES.items() for r in case.rounds]
ROW_IDS = [f"{name}-{r}" for name, r in ROWS]
LARGEST = "reads_8653"
HOST_PATH_MAX_READS = 1100   # the cases of at most this many reads are run on the per-chunk host path as well:
HOST_PATH_CASES = tuple(n for n in CASES if not n.startswith(("columns_1023", "columns_1024", "columns_1025", "columns_2097", "reads_")))


def _parameter_sets() -> dict:
    out = {}
    for name, rounds in ROWS:
        out.setdefault((CASES[name].limit, CASES[name].depth, rounds), []).append((name, rounds))
    return {k: v for k, v in out.items() if len(v) > 1}


# (limit, depth, rounds) -> the rows phased with these parameters, where there is more than one: they are phased in one call as well
PARAMETER_SETS = _parameter_sets()
GROUPED = (CASES[LARGEST].limit, CASES[LARGEST].depth, SHIPPED_ROUNDS)  # the set of the largest chunk: run as two concurrent batches


def chunk(name: str):
    return CASES[name].build()


def case_params(name: str, rounds: int) -> dict:
    return params(CASES[name].limit, rounds, CASES[name].depth)


@functools.lru_cache(maxsize=None)
def oracle_chunk(name: str):
    """(kept for the life of the process: every run of the case goes through it)"""
    orc.lib()
    return orc.OracleChunk(chunk(name))


_final_job = {}


@functools.lru_cache(maxsize=None)
def oracle(name: str, rounds: int) -> dict:
    """the oracle's phasing of the case at this round limit (without its jobs: final_job keeps what is needed of them)"""
    res = oracle_chunk(name).phase(case_params(name, rounds), capture_jobs=(rounds == 0))
    jobs = res.pop("jobs")
    if rounds == 0:
        j = jobs[-1]
        _final_job[name] = dict(n_columns=int(j["n_columns"]), max_cells=int(np.diff(j["col_cell_off"]).max()),
                                read_ids=sorted(set(int(r) for r in j["read_ids"])), col_ref_start=j["col_ref_start"].copy(),
                                col_length=j["col_length"].copy())
    return res


def final_job(name: str) -> dict:
    """of the last forward-backward job of the case (the final hmm; the round limit does not change it): its columns, its largest
    column's cells, the reads its columns hold"""
    oracle(name, 0)
    return _final_job[name]


def _result(res) -> tuple:
    return res["reads1"], res["reads2"], res["hap1"].tobytes(), res["hap2"].tobytes()


def read_sums(c, read, res) -> tuple:
    """getLogProbOfReadGivenHaplotype (genomeFragment.c:71-89) for both haplotype strings of a result, as byte sums: the log
    probabilities are minus these over 30, so the read goes to reads2 where the first sum is the larger, else (a tie too) to reads1"""
    s1 = s2 = 0
    first = int(c.allele_offset[read.ref_start])
    for i in range(read.length):
        j = i + read.ref_start - res["ref_start"]
        if 0 <= j < res["length"]:
            at = read.pool_off + int(c.allele_offset[read.ref_start + i]) - first
            s1 += int(c.pool[at + int(res["hap1"][j])])
            s2 += int(c.pool[at + int(res["hap2"][j])])
    return s1, s2


@functools.lru_cache(maxsize=None)
def facts(name: str) -> dict:
    """final_K, final_max_cells, n_reads, listed (reads on the two lists at 0 rounds, before the re-adding), discarded (the chunk's
    reads that no column of the final hmm holds), both_sides (reads on both lists at 0 rounds), last_moving_round (the largest r in
    1..12 at which the oracle's reads1, reads2, hap1, hap2 differ from those at r - 1 rounds), moved_1_to_2 / moved_2_to_1 (kept
    reads that changed lists between 0 rounds and 1 round), sides (per round limit the case is run at and per discarded read: its two
    byte sums under that result's haplotypes and the lists the oracle put it on), results (the oracle's results at 0, 1, ... rounds
    up to the end of the scan).

    A round that moves nothing ends the refinement (genomeFragment.c:196), and every round limit above it gives the same result; a
    round that moves a read changes a list.  So the scan stops at the first r whose result equals that of r - 1."""
    c = chunk(name)
    fj = final_job(name)
    r0 = oracle(name, 0)
    kept = set(fj["read_ids"])
    discarded = [i for i in range(len(c.reads)) if i not in kept]
    gone = set(discarded)
    results, last = [r0], 0
    for r in range(1, ROUND_SCAN + 1):
        results.append(oracle(name, r))
        if _result(results[-1]) == _result(results[-2]):
            break
        last = r
    r1 = results[1]
    on = lambda res, k: set(res[k]) - gone
    sides = {}
    for rounds in CASES[name].rounds:
        res = oracle(name, rounds)
        sides[rounds] = {i: dict(sums=read_sums(c, c.reads[i], res), on1=i in res["reads1"], on2=i in res["reads2"]) for i in discarded}
    return dict(final_K=fj["n_columns"], final_max_cells=fj["max_cells"], n_reads=len(c.reads),
                listed=len(r0["reads1"]) + len(r0["reads2"]) - len(discarded), kept=len(kept), discarded=discarded,
                both_sides=sorted(set(r0["reads1"]) & set(r0["reads2"])), last_moving_round=last,
                moved_1_to_2=len(on(r0, "reads1") & on(r1, "reads2")), moved_2_to_1=len(on(r0, "reads2") & on(r1, "reads1")),
                sides=sides, results=results)


def columns_with_site_kinds(name: str) -> int:
    """columns of the final hmm that hold a site of MRP_MAX_ALLELES alleles and a biallelic one"""
    c, fj = chunk(name), final_job(name)
    n = 0
    for s, ln in zip(fj["col_ref_start"], fj["col_length"]):
        a = c.allele_number[int(s):int(s) + int(ln)]
        n += bool((a == MRP_MAX_ALLELES).any() and (a == 2).any())
    return n
