"""Hmms of one, two and three columns in every wide class of the prune kernel, against the oracle.

Every role of mrp_prune_kernel runs its own loop over the columns and all of them pass the same barriers: one after the prologue, one
per column, one or two behind the last column.  The edges of that schedule are the shortest hmms -- the list stages run up to three
columns behind the chain, and the two groups of bin-streaming waves alternate over the columns -- and the launch-class matrix
(test_gpu_launch_classes.py) reaches the wide classes only with hmms of eleven and more columns.  Here: chunks of one to five sites at
30x (33 or 34 reads), whose last merge levels are hmms of 1, 2, 3 and 4 columns as wide as the limit allows, at the limits whose
L x L cells select the classes 512x32, two groups, one group and 1 024 threads on per-cell arrays, under the chain on units, the general
chain and the chain on pairs over per-cell arrays.  Results are compared as the matrix compares them."""
import numpy as np
import pytest

from margin_amd import capi, synth
from tests.test_gpu_launch_classes import MODES, _params
from tests.test_gpu_pipeline import assert_same_hmm
from tests.test_gpu_resident import PHASE_KEYS

# (no module mark: the conditions on the inputs are the oracle's alone and run without a GPU; the comparisons are marked one by one)

# sites of the chunk -> columns of its widest hmms (decided by the oracle: test_the_oracle_has_the_short_wide_hmms)
COLUMNS_OF = {1: 1, 2: 2, 4: 3, 5: 4}
# limit -> the prune class of a per-cell level of limit x limit cells
CLASS_OF = {64: "prune_512x32", 68: "prune_512x10_two_groups", 80: "prune_512x10_one_group", 116: "prune_1024"}
SHORT_MODES = ("units", "general_chain", "pairs_over_cells")
ROWS = [(sites, limit, mode) for sites in COLUMNS_OF for limit in CLASS_OF for mode in SHORT_MODES]
ROW_IDS = [f"{sites}sites-{limit}-{mode}" for sites, limit, mode in ROWS]


@pytest.fixture(scope="module")
def short_oracle(orc):
    """The chunks and what the oracle makes of them; no device."""
    chunks = {n: synth.make_ont_chunk(seed=5, region_bp=2000, n_sites=n, coverage=30) for n in COLUMNS_OF}
    strands_of = {n: [[i for i, r in enumerate(c.reads) if r.strand == s] for s in (1, 0)] for n, c in chunks.items()}
    oracle = {}
    for n, chunk in chunks.items():
        oc = orc.OracleChunk(chunk)
        for limit in CLASS_OF:  # (the hooks change no result: the three modes share an oracle run)
            ref = oc.phase(_params(limit, "units"), capture_jobs=True)
            jobs = ref.pop("jobs")
            hp = orc.make_params(_params(limit, "units", includeAncestorSubProb=0))
            oracle[(n, limit)] = dict(
                phase=ref,
                wide=[(int(j["n_columns"]), int(np.diff(j["col_cell_off"]).max())) for j in jobs if np.diff(j["col_cell_off"]).max() > 256],
                hmms=[[orc.flatten(h, oc.pool_off) for h in oc.get_rp_hmms(hp, idx)] for idx in strands_of[n]])
        oc.close()
    return dict(chunks=chunks, strands_of=strands_of, oracle=oracle)


def _check_the_short_wide_hmms(oracle, limit):
    wide = [w for n in COLUMNS_OF for w in oracle[(n, limit)]["wide"]]
    columns = {c for c, _ in wide}
    assert {1, 2, 3} <= columns and max(columns) >= 4
    for n, cols in COLUMNS_OF.items():
        # the level of limit x limit cells -- the one that launches CLASS_OF[limit] -- holds an hmm of exactly COLUMNS_OF[n] columns, and
        # the chunk has no hmm of more columns: whatever class ran on this chunk ran on hmms that short
        assert (cols, limit * limit) in oracle[(n, limit)]["wide"], n
        assert max(c for c, _ in oracle[(n, limit)]["wide"]) == cols, n


@pytest.fixture(scope="module")
def short(short_oracle):
    chunks, strands_of, oracle = short_oracle["chunks"], short_oracle["strands_of"], short_oracle["oracle"]
    for limit in CLASS_OF:  # before anything is launched
        _check_the_short_wide_hmms(oracle, limit)
    rows = {}
    with capi.Context(0) as ctx:
        dchunks = {n: capi.DeviceChunk.from_chunk(ctx, c) for n, c in chunks.items()}
        ctx.launch_census(reset=True)
        failed = None
        for sites, limit, mode in ROWS:
            row = dict(hmms=[], error=None)
            if failed:  # nothing more is launched behind a failed call
                row["error"] = f"not run: row {failed} failed"
                rows[(sites, limit, mode)] = row
                continue
            chunk, dchunk = chunks[sites], dchunks[sites]
            ctx.set_test_hooks(MODES[mode][0])
            try:
                hparams = capi.Params.from_reference_names(_params(limit, mode, includeAncestorSubProb=0))
                for idx in strands_of[sites]:
                    got = capi.get_rp_hmms_resident(ctx, dchunk, chunk, hparams, idx)
                    row["hmms"].append([capi.hmm_to_flat(h) for h in got])
                    for h in got:
                        capi.hmm_destroy(h)
                (row["phase"],), row["stats"] = capi.phase_reads_many(ctx, [dchunk], [chunk], capi.Params.from_reference_names(_params(limit, mode)))
                row["census"] = ctx.launch_census(reset=True)
            except capi.MrpError as e:
                row["error"] = repr(e)
                failed = f"{sites}sites-{limit}-{mode}"
            finally:
                ctx.set_test_hooks(0)
            rows[(sites, limit, mode)] = row
        for d in dchunks.values():
            d.close()
    return dict(rows=rows, oracle=oracle)


@pytest.mark.parametrize("limit", sorted(CLASS_OF))
def test_the_oracle_has_the_short_wide_hmms(short_oracle, limit):
    """Conditions on the inputs, decided by the oracle alone, on the CPU: at every limit its forward-backward jobs hold hmms wider than
    256 cells (the wide classes) of exactly 1, 2 and 3 columns and of at least 4; the chunk of n sites has one of COLUMNS_OF[n] columns
    whose widest column is the square of the limit, and none of more columns."""
    _check_the_short_wide_hmms(short_oracle["oracle"], limit)


@pytest.mark.gpu
@pytest.mark.parametrize("sites,limit,mode", ROWS, ids=ROW_IDS)
def test_short_hmms_equal_the_oracle(short, sites, limit, mode):
    """mrp_get_rp_hmms_resident per strand array for array, and mrp_phase_reads_many with == (max-plus mode is bit-exact), on the
    resident path; on per-cell arrays the level of limit x limit cells ran the class the limit is here for -- on an hmm of COLUMNS_OF[sites]
    columns, since a launch takes every hmm of its level and the oracle's conditions put the short hmm in that level."""
    row, ref = short["rows"][(sites, limit, mode)], short["oracle"][(sites, limit)]
    assert row["error"] is None, row["error"]
    assert len(row["hmms"]) == len(ref["hmms"]) == 2
    for got_strand, ref_strand in zip(row["hmms"], ref["hmms"]):
        assert len(got_strand) == len(ref_strand)
        for hg, hr in zip(got_strand, ref_strand):
            assert_same_hmm(hr, hg, values=False)
    got, st = row["phase"], row["stats"]
    assert st.resident == 1 and st.fallback_chunks == 0
    assert got["ref_start"] == ref["phase"]["ref_start"] and got["length"] == ref["phase"]["length"]
    for k in PHASE_KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref["phase"][k])).all(), k
    assert got["reads1"] == ref["phase"]["reads1"] and got["reads2"] == ref["phase"]["reads2"]
    if mode != "units":
        assert row["census"][f"{CLASS_OF[limit]}_{MODES[mode][2]}"] > 0
