"""Every launch class of the device-resident merge against the oracle.

The resident path picks its kernels by size class, level by level (mrp_launch_prune: five instantiations x three chain modes;
mrp_launch_cross_emit: three plans and two table sizes; the recursion's narrow / mid / wide classes; the single-wave kernel).  Every
class is its own register blocking, barrier pattern and LDS layout, and a whole-call comparison with the oracle covers only the
classes the call happened to run.  The launch census (mrp_context_launch_census) says which those were.  One module-scoped fixture
runs a matrix over one small chunk -- 40 sites, 30x, 69 reads: columns of up to 116 x 116 cells need no more -- and records, per row,
the results and the census delta; the tests compare the results with the oracle alone and then hold the census to account: every
slot the library names has run, except those the table below shows unreachable by arithmetic.  A launch class added later fails
test_every_launch_class_ran_somewhere_in_the_matrix until a row reaches it.

Rows: maxPartitionsInAColumn in LIMITS with minPartitionsInAColumn = 0 (even limits only: an odd one cuts complement pairs and sends
the chunk to the hashing path, another subject), each in four modes -- the default (unit levels), test hook bit 3 (the general chain
over per-cell arrays), test hook bit 4 (the chain on complement pairs over per-cell arrays), includeInvertedPartitions = 0 (the general
chain in production) -- two rows with the ancestor substitution model at the merge levels (the two-kernel cross product, per-cell
arrays without any hook: what a caller of mrp_get_rp_hmms_resident with includeAncestorSubProb reaches).  mrp_phase_reads_many
switches that model off below the final level, as the reference does (bubbleGraph.c:2733), so the ancestor rows reach their levels
through the pruned-hmm step, which they run with the model ON against the oracle's getRPHmms with the model on; their phase step is
the default mode's.  One more row, the same region at 14x, reaches the cross product + emission plan of modes 1 + 2 (see ROWS).  The bound of a level is a product of min(2^depth, limit) per parent, so a limit L puts the largest level at
exactly L x L cells."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests.test_gpu_pipeline import assert_same_hmm
from tests.test_gpu_resident import PHASE_KEYS

pytestmark = pytest.mark.gpu

LIMITS = (16, 64, 68, 80, 100, 104, 116)
# mode -> (test hooks, parameter overrides, PruneParams.pairs of its merge levels as the census names it)
MODES = {
    "units": (0, {}, "units"),
    "general_chain": (8, {}, "general"),
    "pairs_over_cells": (16, {}, "pairs_over_cells"),
    "not_inverted": (0, dict(includeInvertedPartitions=0), "general"),
    "ancestor_model": (0, dict(includeAncestorSubProb=1), "pairs_over_cells"),
    "units_at_14x": (0, {}, "units"),
}
COVERAGE = {"units_at_14x": 14}  # every other mode: 30
# (16, units_at_14x): the same region at 14x (35 reads).  The one plan of the cross product + emission kernel the 30x rows do not reach is
# modes 1 + 2: a level most of whose hmms are the single-wave kernel's (columns of at most 128 cells by the static bounds, i.e. at
# most 3 reads on one side and any number on the other) while some column can exceed a wave.  At 30x the hmms of four and more reads
# are nearly all deeper than that; at 14x the third merge level is such a mix.
ROWS = [(limit, mode) for limit in LIMITS for mode in ("units", "general_chain", "pairs_over_cells", "not_inverted")] + \
       [(104, "ancestor_model"), (116, "ancestor_model"), (16, "units_at_14x")]
ROW_IDS = [f"{limit}-{mode}" for limit, mode in ROWS]
PER_CELL_MODES = ("general_chain", "pairs_over_cells", "not_inverted", "ancestor_model")

# Launch classes no input reaches, each with the arithmetic that says so.  A slot that stays zero and is not listed here fails.
UNREACHABLE = {
    # a unit level holds (cells + 1) / 2 entries; cells <= 116 x 116 = 13 456 (MRP_PRUNE_MAX_S), so held <= 6 728 < 10 241
    "prune_1024_units": "held <= (116 * 116 + 1) / 2 = 6 728, the class starts at 10 241",
}

PRUNE_CLASSES = ("prune_256", "prune_512x32", "prune_512x10_two_groups", "prune_512x10_one_group", "prune_1024")


def _oracle_key(limit, mode):
    # the hooks change no result: their rows share the default mode's oracle run
    return limit, ("units" if mode in ("general_chain", "pairs_over_cells") else mode)


def _params(limit, mode, **over):
    pd = synth.shipped_phase_params()
    pd.update(minPartitionsInAColumn=0, maxPartitionsInAColumn=limit)
    pd.update(MODES[mode][1])
    pd.update(over)
    return pd


def _hmm_params(limit, mode):
    # the pruned-hmm step: without the ancestor model (as test_resident_get_rp_hmms_matches_oracle), except in the rows that are about it
    return _params(limit, mode) if mode == "ancestor_model" else _params(limit, mode, includeAncestorSubProb=0)


@pytest.fixture(scope="module")
def matrix(orc):
    chunks = {cov: synth.make_ont_chunk(seed=5, region_bp=20_000, n_sites=40, coverage=cov) for cov in {30, *COVERAGE.values()}}
    strands_of = {cov: [[i for i, r in enumerate(c.reads) if r.strand == s] for s in (1, 0)] for cov, c in chunks.items()}
    ocs = {cov: orc.OracleChunk(c) for cov, c in chunks.items()}
    oracle = {}
    for limit, mode in ROWS:
        key = _oracle_key(limit, mode)
        if key in oracle:
            continue
        oc, strands = ocs[COVERAGE.get(key[1], 30)], strands_of[COVERAGE.get(key[1], 30)]
        ref = oc.phase(_params(*key), capture_jobs=True)
        jobs = ref.pop("jobs")
        hp = orc.make_params(_hmm_params(*key))
        oracle[key] = dict(
            phase=ref,
            max_column=max(int(np.diff(j["col_cell_off"]).max()) for j in jobs),
            max_merge_column=max(int(np.diff(j["mcol_cell_off"]).max()) for j in jobs if j["n_columns"] > 1),
            hmms=[[orc.flatten(h, oc.pool_off) for h in oc.get_rp_hmms(hp, idx)] for idx in strands])
    rows = {}
    with capi.Context(0) as ctx:
        dchunks = {cov: capi.DeviceChunk.from_chunk(ctx, c) for cov, c in chunks.items()}
        ctx.launch_census(reset=True)
        failed = None
        for limit, mode in ROWS:
            row = dict(hmms=[], error=None)
            if failed:  # nothing more is launched behind a failed call
                row["error"] = f"not run: row {failed} failed"
                rows[(limit, mode)] = row
                continue
            cov = COVERAGE.get(mode, 30)
            chunk, dchunk, strands = chunks[cov], dchunks[cov], strands_of[cov]
            ctx.set_test_hooks(MODES[mode][0])
            try:
                hparams = capi.Params.from_reference_names(_hmm_params(limit, mode))
                for idx in strands:
                    got = capi.get_rp_hmms_resident(ctx, dchunk, chunk, hparams, idx)
                    row["hmms"].append([capi.hmm_to_flat(h) for h in got])
                    for h in got:
                        capi.hmm_destroy(h)
                row["census_hmms"] = ctx.launch_census(reset=True)
                (row["phase"],), row["stats"] = capi.phase_reads_many(ctx, [dchunk], [chunk], capi.Params.from_reference_names(_params(limit, mode)))
                row["census_phase"] = ctx.launch_census(reset=True)
            except capi.MrpError as e:  # that row's finding; the rows behind it say that they were not run
                row["error"] = repr(e)
                failed = f"{limit}-{mode}"
            finally:
                ctx.set_test_hooks(0)
            rows[(limit, mode)] = row
        after_reset = ctx.launch_census()
        for d in dchunks.values():
            d.close()
    for oc in ocs.values():
        oc.close()
    return dict(rows=rows, oracle=oracle, after_reset=after_reset, names=capi.launch_class_names())


def _census(row):
    assert row["error"] is None, row["error"]
    return {k: row["census_hmms"][k] + row["census_phase"][k] for k in row["census_hmms"]}


@pytest.mark.parametrize("limit,mode", sorted(set(_oracle_key(*r) for r in ROWS)), ids=lambda v: str(v))
def test_the_oracle_runs_reach_the_sizes_the_rows_are_for(matrix, limit, mode):
    """Conditions on the inputs, decided by the oracle alone: the largest column the oracle's forward-backward jobs hold is the
    square of the limit, and from 80 on the largest merge column exceeds 4 096 cells (the recursion's wide class)."""
    o = matrix["oracle"][(limit, mode)]
    assert o["max_column"] == limit * limit
    if limit >= 80:
        assert o["max_merge_column"] > 4096


@pytest.mark.parametrize("limit,mode", ROWS, ids=ROW_IDS)
def test_pruned_hmms_equal_the_oracle(matrix, limit, mode):
    """mrp_get_rp_hmms_resident per strand against the oracle's getRPHmms, array for array."""
    row, ref = matrix["rows"][(limit, mode)], matrix["oracle"][_oracle_key(limit, mode)]["hmms"]
    assert row["error"] is None, row["error"]
    assert len(row["hmms"]) == len(ref) == 2
    for got_strand, ref_strand in zip(row["hmms"], ref):
        assert len(got_strand) == len(ref_strand)
        for hg, hr in zip(got_strand, ref_strand):
            assert_same_hmm(hr, hg, values=False)


@pytest.mark.parametrize("limit,mode", ROWS, ids=ROW_IDS)
def test_phase_results_equal_the_oracle(matrix, limit, mode):
    """mrp_phase_reads_many against the oracle's phasing: every result array and both read sets, with == (max-plus mode is
    bit-exact); the call stayed on the resident path with every chunk."""
    row, ref = matrix["rows"][(limit, mode)], matrix["oracle"][_oracle_key(limit, mode)]["phase"]
    assert row["error"] is None, row["error"]
    got, st = row["phase"], row["stats"]
    assert st.resident == 1 and st.fallback_chunks == 0
    assert got["ref_start"] == ref["ref_start"] and got["length"] == ref["length"]
    for k in PHASE_KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), k
    assert got["reads1"] == ref["reads1"] and got["reads2"] == ref["reads2"]


def test_every_launch_class_ran_somewhere_in_the_matrix(matrix):
    """Census completeness: every slot the library names is non-zero over the matrix, except the classes UNREACHABLE explains; those
    are indeed zero.  (The names come from the library: mrp_launch_class_name.)"""
    names = matrix["names"]
    assert len(names) == len(set(names)) >= 29 and set(UNREACHABLE) <= set(names)
    total = dict.fromkeys(names, 0)
    reached_by = {n: [] for n in names}
    for (limit, mode), row in matrix["rows"].items():
        for n, c in _census(row).items():
            total[n] += c
            if c:
                reached_by[n].append(f"{limit}-{mode}")
    print({n: reached_by[n] for n in names})
    never = [n for n in names if total[n] == 0 and n not in UNREACHABLE]
    assert not never, never
    assert not [n for n in UNREACHABLE if total[n] != 0]
    assert sum(matrix["after_reset"].values()) == 0  # a read with reset leaves nothing behind


@pytest.mark.parametrize("chain", ["general", "pairs_over_cells"])
def test_the_classes_no_earlier_test_launched_ran_here(matrix, chain):
    """The 1 024-thread prune class (a per-cell level above 10 240 cells: limits 104 and 116) and the two-group 16-byte-load class (a
    per-cell level of 4 097..5 120 cells: 68 x 68 = 4 624), in the general chain and in the chain on pairs over per-cell arrays; the
    recursion's wide class on a per-cell level at 116."""
    modes = ("general_chain", "not_inverted") if chain == "general" else ("pairs_over_cells", "ancestor_model")
    for limit, mode in ROWS:
        if mode not in modes:
            continue
        c = _census(matrix["rows"][(limit, mode)])
        if limit in (104, 116):
            assert c[f"prune_1024_{chain}"] > 0, (limit, mode)
        if limit == 68:
            assert c[f"prune_512x10_two_groups_{chain}"] > 0, (limit, mode)
        if limit == 116:
            assert c["sweep_wide"] > 0, (limit, mode)


def test_the_ancestor_rows_ran_the_two_kernel_cross_product_at_every_merge_level(matrix):
    for limit in (104, 116):
        c = matrix["rows"][(limit, "ancestor_model")]["census_hmms"]
        assert c["cross_two_kernels"] > 0 and c["prune_1024_pairs_over_cells"] > 0
        assert not [n for n in c if n.startswith("cross_emit_") and c[n]]
        assert not [n for n in c if n.startswith("prune_") and not n.startswith("prune_back") and not n.endswith("pairs_over_cells") and c[n]]


@pytest.mark.parametrize("limit,lower", [(16, "prune_256"), (64, "prune_512x32")])
def test_a_level_exactly_on_a_threshold_runs_the_lower_class(matrix, limit, lower):
    """Per-cell arrays at limits 16 and 64 put what the prune kernel's streaming waves hold exactly on 256 and 4 096 (the oracle's
    largest column says the columns really get there): the class that ends there ran, and no class above it."""
    assert matrix["oracle"][(limit, "units")]["max_column"] == limit * limit
    above = PRUNE_CLASSES[PRUNE_CLASSES.index(lower) + 1:]
    for mode in ("general_chain", "pairs_over_cells", "not_inverted"):
        c = _census(matrix["rows"][(limit, mode)])
        assert c[f"{lower}_{MODES[mode][2]}"] > 0, mode
        assert not [n for n in c if n.startswith(tuple(a + "_" for a in above)) and c[n]], mode
        assert not [n for n in c if n.startswith("prune_") and not n.startswith("prune_back") and not n.endswith("_" + MODES[mode][2]) and c[n]], mode


def test_the_census_sums_the_sibling_contexts(matrix):
    """Eight chunks as two concurrent batches: one runs on the context, one on its sibling, each with a final level of its own, so the
    call launches the trace back twice; as one batch, once."""
    assert not [k for k, row in matrix["rows"].items() if row["error"]]  # (nothing more is launched behind a failed call)
    chunks = [synth.make_ont_chunk(seed=31 + i, region_bp=10_000, n_sites=20, coverage=12) for i in range(8)]  # (fewer than four chunks a batch run as one)
    params = capi.Params.from_reference_names(synth.shipped_phase_params())
    with capi.Context(0) as ctx:
        dchunks = [capi.DeviceChunk.from_chunk(ctx, c) for c in chunks]
        seen = {}
        for groups in (1, 2):
            ctx.set_phase_groups(groups)
            ctx.launch_census(reset=True)
            _, st = capi.phase_reads_many(ctx, dchunks, chunks, params)
            assert st.resident == 1 and st.fallback_chunks == 0
            seen[groups] = ctx.launch_census()
        assert seen[1]["traceback"] == 1 and seen[2]["traceback"] == 2
        assert seen[2]["mini"] > seen[1]["mini"] > 0
        for d in dchunks:
            d.close()
