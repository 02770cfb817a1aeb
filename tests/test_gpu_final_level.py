"""The trace back and the genome fragment kernel of the final level at their edges, against the oracle.

Every mrp_phase_reads_many call ends in mrp_traceback_kernel and mrp_fragment_kernel; what a caller keeps -- haplotype strings,
genotypes, supports, reads1 and reads2 -- is what these two return.  The launch census sees each as one slot; the branches inside
them (LDS or HBM read search, columns and list entries per thread, the parity of the moving rounds, the round limit, the re-adding
of filtered reads, the pool order) are reached by the rows of tests/final_level_cases.py, whose facts tests/test_final_level_cases.py
asserts from the oracle alone.  One module-scoped fixture with a context of its own runs every (case, round limit) row in a call
of its own, census read and reset around it, then the rows of at most HOST_PATH_MAX_READS reads on the per-chunk host path, then
all rows that share their parameters in one call per parameter set (the set of the largest chunk as two concurrent batches), then the
largest row again.  Nothing more is launched behind a failed call: the steps behind it record that they were not run."""
import time

import numpy as np
import pytest

from margin_amd import capi
from tests import final_level_cases as fc
from tests.test_gpu_resident import PHASE_KEYS

pytestmark = pytest.mark.gpu

SETS, GROUPED = fc.PARAMETER_SETS, fc.GROUPED
SET_IDS = [f"limit{k[0]}-depth{k[1]}-rounds{k[2]}" for k in SETS]
HOST_ROWS = [(n, r) for n, r in fc.ROWS if n in fc.HOST_PATH_CASES]


@pytest.fixture(scope="module")
def runs(orc):
    t0 = time.perf_counter()
    rows, host, sets, repeat = {}, {}, {}, {}
    failed = None

    def step(label, store, key, fn):
        nonlocal failed
        rec = dict(error=None)
        if failed:  # nothing more is launched behind a failed call
            rec["error"] = f"not run: {failed} failed"
        else:
            try:
                fn(rec)
            except capi.MrpError as e:  # that step's finding
                rec["error"] = repr(e)
                rec["code"] = e.code
                failed = label
        store[key] = rec

    with capi.Context(0) as ctx:
        dchunks = {}

        def dchunk(name):
            if name not in dchunks:
                dchunks[name] = capi.DeviceChunk.from_chunk(ctx, fc.chunk(name))
            return dchunks[name]

        def one_row(name, rounds):
            def fn(rec):
                d = dchunk(name)
                ctx.launch_census(reset=True)
                (rec["phase"],), rec["stats"] = capi.phase_reads_many(ctx, [d], [fc.chunk(name)], capi.Params.from_reference_names(fc.case_params(name, rounds)))
                rec["census"] = ctx.launch_census(reset=True)
            return fn

        for name, rounds in fc.ROWS:
            step(f"row {name}-{rounds}", rows, (name, rounds), one_row(name, rounds))
        for name, rounds in HOST_ROWS:
            step(f"host path of {name}-{rounds}", host, (name, rounds),
                 lambda rec, name=name, rounds=rounds: rec.update(phase=capi.phase_reads(ctx, dchunk(name), fc.chunk(name), capi.Params.from_reference_names(fc.case_params(name, rounds)))))
        for key, members in SETS.items():
            def fn(rec, key=key, members=members):
                ctx.set_phase_groups(2 if key == GROUPED else 0)
                try:
                    ctx.launch_census(reset=True)
                    rec["phase"], rec["stats"] = capi.phase_reads_many(ctx, [dchunk(n) for n, _ in members], [fc.chunk(n) for n, _ in members],
                                                                       capi.Params.from_reference_names(fc.params(key[0], key[2], key[1])))
                    rec["census"] = ctx.launch_census(reset=True)
                finally:
                    ctx.set_phase_groups(0)
            step(f"one call of {key}", sets, key, fn)
        step("repeat", repeat, "repeat", one_row(fc.LARGEST, fc.SHIPPED_ROUNDS))
        for d in dchunks.values():
            d.close()
    seconds = time.perf_counter() - t0
    print(f"final level rows: {len(rows)} rows, {len(host)} host path runs, {len(sets)} one-call sets in {seconds:.1f} s")
    return dict(rows=rows, host=host, sets=sets, repeat=repeat["repeat"], seconds=seconds)


def _same(got, ref, what=""):
    assert got["ref_start"] == ref["ref_start"] and got["length"] == ref["length"], what
    for k in PHASE_KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), (what, k)
    assert got["reads1"] == ref["reads1"] and got["reads2"] == ref["reads2"], what  # ordered: order is what the compactions can get wrong


@pytest.mark.parametrize("name,rounds", fc.ROWS, ids=fc.ROW_IDS)
def test_every_row_equals_the_oracle(runs, name, rounds):
    """ref_start, length, every result array and both read lists in order, with == (max-plus mode is bit-exact)"""
    row = runs["rows"][(name, rounds)]
    assert row["error"] is None, row["error"]
    _same(row["phase"], fc.oracle(name, rounds), "oracle")


@pytest.mark.parametrize("name,rounds", fc.ROWS, ids=fc.ROW_IDS)
def test_every_row_came_from_the_device_kernels(runs, name, rounds):
    """the chunk stayed on the resident path, and the call launched the trace back and the fragment kernel: the result is the device
    fragment kernel's, not the host's finish_phase_parts"""
    row = runs["rows"][(name, rounds)]
    assert row["error"] is None, row["error"]
    st, census = row["stats"], row["census"]
    assert st.resident == 1 and st.fallback_chunks == 0
    assert census["traceback"] >= 1 and census["fragments"] >= 1


@pytest.mark.parametrize("name,rounds", HOST_ROWS, ids=[f"{n}-{r}" for n, r in HOST_ROWS])
def test_small_rows_equal_the_per_chunk_host_path(runs, name, rounds):
    """a second opinion from rphmm_result.c"""
    row, other = runs["rows"][(name, rounds)], runs["host"][(name, rounds)]
    assert row["error"] is None, row["error"]
    assert other["error"] is None, other["error"]
    _same(row["phase"], other["phase"], "host path")


@pytest.mark.parametrize("rounds", fc.CASES["permuted_pool"].rounds)
def test_a_pool_out_of_read_order_changes_nothing(runs, rounds):
    """the search order of the fragment kernel is a real permutation here (the host sorts the reads by pool offset); the reads and
    their bytes are the twin's, and so is every result"""
    row, twin = runs["rows"][("permuted_pool", rounds)], runs["rows"][(fc.CASES["permuted_pool"].twin, rounds)]
    assert row["error"] is None, row["error"]
    assert twin["error"] is None, twin["error"]
    _same(row["phase"], twin["phase"], "twin")
    _same(row["phase"], fc.oracle("permuted_pool", rounds), "oracle")


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
def test_rows_of_one_parameter_set_in_one_call_give_each_rows_own_result(runs, key):
    """chunks of different sizes share the final level's launches: a workgroup of the fragment kernel per chunk, the chunk above
    6 144 reads beside small ones.  The set of the largest chunk runs as two concurrent batches: two trace backs, two fragment
    launches."""
    rec = runs["sets"][key]
    assert rec["error"] is None, rec["error"]
    st = rec["stats"]
    assert st.resident == 1 and st.fallback_chunks == 0
    assert len(rec["phase"]) == len(SETS[key])
    for (name, rounds), got in zip(SETS[key], rec["phase"]):
        _same(got, fc.oracle(name, rounds), f"oracle, {name}")
        own = runs["rows"][(name, rounds)]
        assert own["error"] is None, own["error"]
        _same(got, own["phase"], f"own call, {name}")
    batches = 2 if key == GROUPED else 1
    assert rec["census"]["traceback"] == batches and rec["census"]["fragments"] == batches


def test_a_repeat_of_the_largest_row_equals_the_first_call(runs):
    first, again = runs["rows"][(fc.LARGEST, fc.SHIPPED_ROUNDS)], runs["repeat"]
    assert first["error"] is None, first["error"]
    assert again["error"] is None, again["error"]
    _same(again["phase"], first["phase"], "first call")
