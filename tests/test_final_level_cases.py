"""What the cases of tests/final_level_cases.py exhibit, asserted from the oracle alone (no device): every tile size and branch of
the trace back and the genome fragment kernel that tests/test_gpu_final_level.py is there for is really in the inputs it runs.  A
change of margin_amd.synth that empties a case fails here, not silently on the device.

Two branches of the kernels are unreachable on the resident path, and the rows show it:

UNREACHABLE
  the trace back's path for columns above 128 cells.  The final hmm is the fusion of a tiling path (stRPHmm_fuse, hmm.c:283-372): its
    columns are columns of hmms that the merge level below has pruned, or gap columns of one cell, and fusing multiplies nothing.  A
    pruned column keeps at most maxPartitionsInAColumn cells, and the resident path takes limits up to MRP_PRUNE_MAX_S = 116 only
    (above it a chunk goes to the hashing path, which has no device trace back).  So a final column holds at most 116 cells:
    test_no_final_column_exceeds_the_pruned_size.
  a read on both lists of the first sightings.  The trace back follows merge cells, and a cell feeds a merge cell only if it agrees
    with it on every read the two columns share (the masks of hmm.c:196-214): along a valid path a read is on one side in every
    column that holds it.  The kernel's "in both" case needs inconsistent columns, which no path has:
    test_no_read_is_on_both_sides_without_refinement.
A row that contradicted either would be a finding about the reference, not a reason to drop the row."""
import numpy as np
import pytest

from tests import final_level_cases as fc

NAMES = list(fc.CASES)


def test_the_rows_are_what_the_module_says():
    """even limits of 4 or 8 without a lower bound, the round limits 0, m - 1, m, m + 1 and 10 per rounds chunk"""
    for name, case in fc.CASES.items():
        assert case.limit in (4, 8), name
        pd = fc.case_params(name, case.rounds[0])
        assert pd["minPartitionsInAColumn"] == 0 and pd["maxPartitionsInAColumn"] == case.limit and pd["maxCoverageDepth"] == case.depth
    assert [fc.CASES[f"rounds_m{m}"].rounds for m in range(6)] == [(0, 1, 10), (0, 1, 2, 10), (0, 1, 2, 3, 10), (0, 2, 3, 4, 10), (0, 3, 4, 5, 10), (0, 4, 5, 6, 10)]
    assert len(fc.ROWS) == len(set(fc.ROWS)) == sum(len(c.rounds) for c in fc.CASES.values())
    assert set(fc.HOST_PATH_CASES) == {n for n in fc.CASES if len(fc.chunk(n).reads) <= fc.HOST_PATH_MAX_READS}


def test_the_grouped_set_mixes_the_largest_chunk_with_small_ones():
    """the rows phased with the largest chunk's parameters go into one call as two concurrent batches: that takes eight chunks
    (fewer than four chunks a batch run as one batch), and puts a chunk above 6 144 reads beside chunks of a few dozen"""
    names = [n for n, _ in fc.PARAMETER_SETS[fc.GROUPED]]
    assert fc.LARGEST in names and len(names) >= 8
    sizes = [len(fc.chunk(n).reads) for n in names]
    assert max(sizes) > fc.FRAG_LDS_READS and min(sizes) < 100
    assert all(len(rows) > 1 for rows in fc.PARAMETER_SETS.values())
    assert {(n, r) for rows in fc.PARAMETER_SETS.values() for n, r in rows} <= set(fc.ROWS)


@pytest.mark.parametrize("name", NAMES)
def test_no_final_column_exceeds_the_pruned_size(name):
    f = fc.facts(name)
    assert 1 <= f["final_max_cells"] <= fc.CASES[name].limit <= fc.MRP_PRUNE_MAX_S


@pytest.mark.parametrize("name", NAMES)
def test_no_read_is_on_both_sides_without_refinement(name):
    f = fc.facts(name)
    assert f["both_sides"] == []
    assert f["listed"] == f["kept"] == f["n_reads"] - len(f["discarded"])  # every kept read is on exactly one list


@pytest.mark.parametrize("m", sorted(fc.ROUNDS_SPECS))
def test_rounds_chunks_stop_moving_where_they_should(m):
    """last moving round 0, 1, 2, 3, 4 and 5: with the limits 0, m - 1, m, m + 1 and 10 that is a cut while reads still move, an odd
    and an even number of moving rounds, the early break and no refinement; every limit up to m gives a result of its own"""
    name = f"rounds_m{m}"
    f = fc.facts(name)
    assert f["last_moving_round"] == m and not f["discarded"]
    results = [fc._result(fc.oracle(name, r)) for r in fc.CASES[name].rounds]
    distinct = {r if r < m else m for r in fc.CASES[name].rounds}
    assert len(set(map(repr, results))) == len(distinct)
    assert fc._result(fc.oracle(name, 10)) == fc._result(fc.oracle(name, m))


def test_rounds_chunks_move_reads_both_ways_in_one_round():
    both = [m for m in fc.ROUNDS_SPECS if fc.facts(f"rounds_m{m}")["moved_1_to_2"] > 0 and fc.facts(f"rounds_m{m}")["moved_2_to_1"] > 0]
    assert len(both) >= 1 and set(both) >= {1, 2, 3, 4, 5}
    f0 = fc.facts("rounds_m0")
    assert f0["moved_1_to_2"] == f0["moved_2_to_1"] == 0


def test_column_tiles():
    """final hmms of 1, 2, 1 023, 1 024, 1 025 and more than 2 048 columns; the long ones move reads, so the column flips of a round
    run over more than one trip of the kernel's threads"""
    assert [fc.facts(f"columns_{k}")["final_K"] for k in (1, 2, 1023, 1024, 1025)] == [1, 2, fc.FRAG_T - 1, fc.FRAG_T, fc.FRAG_T + 1]
    assert fc.facts("columns_2097")["final_K"] == 2097 > 2 * fc.FRAG_T
    one = fc.chunk("columns_1")
    assert all(r.ref_start == 0 and r.length == one.n_sites for r in one.reads) and len(one.reads) == fc.N_SPANNING
    for k in (1023, 1024, 1025, 2097):
        assert fc.facts(f"columns_{k}")["last_moving_round"] >= 1


def test_read_search_sizes():
    """6 144 reads (the last size searched in LDS), 6 145 (the first searched in HBM) and all 8 653, each with moving rounds"""
    for n in (fc.FRAG_LDS_READS, fc.FRAG_LDS_READS + 1, 8653):
        f = fc.facts(f"reads_{n}")
        assert f["n_reads"] == f["listed"] == n and f["last_moving_round"] >= 1
        assert f["moved_1_to_2"] > 0 and f["moved_2_to_1"] > 0
    assert len(fc.many_reads_chunk().reads) == 8653


def test_list_tiles():
    """1 024 and 1 025 listed reads with a moving round: the compactions run with one and with two entries per thread"""
    for n in (fc.FRAG_T, fc.FRAG_T + 1):
        f = fc.facts(f"listed_{n}")
        assert f["listed"] == n and f["last_moving_round"] >= 1 and f["moved_1_to_2"] > 0 and f["moved_2_to_1"] > 0


def test_coverage_filter_case():
    """the filter discards reads; at either round limit some go to either side and some tie, and the oracle puts every tie on reads1;
    three of the constant-byte reads are discarded (and tie), the fourth is kept and stays where it is in every round; the kept
    reads move"""
    f = fc.facts("filter")
    assert len(f["discarded"]) > 0 and f["last_moving_round"] >= 1
    assert fc.CASES["filter"].rounds == (0, 1, fc.SHIPPED_ROUNDS) and fc.CASES["filter"].depth == 12
    for rounds, per in f["sides"].items():
        to1 = [i for i, v in per.items() if v["sums"][0] < v["sums"][1]]
        to2 = [i for i, v in per.items() if v["sums"][0] > v["sums"][1]]
        tie = [i for i, v in per.items() if v["sums"][0] == v["sums"][1]]
        assert to1 and to2 and tie, rounds
        assert all(per[i]["on1"] and not per[i]["on2"] for i in to1 + tie), rounds
        assert all(per[i]["on2"] and not per[i]["on1"] for i in to2), rounds
        assert set(fc.CONSTANT_READS[:3]) <= set(tie), rounds
        assert any(per[i]["sums"][0] > 0 for i in tie), rounds  # (not only reads that cover nothing of the fragment)
    kept = fc.CONSTANT_READS[3]
    assert kept not in f["discarded"]
    sides = {(kept in res["reads1"], kept in res["reads2"]) for res in f["results"]}
    assert len(sides) == 1 and sides <= {(True, False), (False, True)}
    c = fc.chunk("filter")
    for res in f["results"]:  # it ties under every result's haplotypes, over sites of the fragment: a move test with >= would move it
        s1, s2 = fc.read_sums(c, c.reads[kept], res)
        assert s1 == s2 > 0
    for i in fc.CONSTANT_READS:
        assert (c.pool[c.reads[i].pool_off:c.reads[i].pool_off + c.reads[i].nbytes] == fc.CONSTANT_BYTE).all()


def test_permuted_pool_case():
    """the pool is out of read order, with gaps; the reads' bytes are the twin's, and so is the oracle's result at every round limit"""
    c, t = fc.chunk("permuted_pool"), fc.chunk(fc.CASES["permuted_pool"].twin)
    off = np.array([r.pool_off for r in c.reads])
    assert (np.diff(off) < 0).sum() > len(off) // 4
    spans = sorted((r.pool_off, r.pool_off + r.nbytes) for r in c.reads)
    assert spans[0][0] > 0 and all(b[0] > a[1] for a, b in zip(spans, spans[1:])) and spans[-1][1] == len(c.pool)
    for r, q in zip(c.reads, t.reads):
        assert (r.name, r.ref_start, r.length, r.strand, r.nbytes) == (q.name, q.ref_start, q.length, q.strand, q.nbytes)
        assert (c.pool[r.pool_off:r.pool_off + r.nbytes] == t.pool[q.pool_off:q.pool_off + q.nbytes]).all()
    assert fc.CASES["permuted_pool"].rounds == fc.CASES[fc.CASES["permuted_pool"].twin].rounds
    for rounds in fc.CASES["permuted_pool"].rounds:
        a, b = fc.oracle("permuted_pool", rounds), fc.oracle(fc.CASES["permuted_pool"].twin, rounds)
        assert fc._result(a) == fc._result(b)
        for k in ("genotype", "ancestor", "support1", "support2", "genotype_probs", "hap_probs1", "hap_probs2"):
            assert (a[k] == b[k]).all(), k


def test_allele_counts_case():
    c = fc.chunk("alleles")
    assert set(c.allele_number.tolist()) == {2, 3, fc.MRP_MAX_ALLELES}
    assert fc.columns_with_site_kinds("alleles") >= 1
