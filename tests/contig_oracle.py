"""What margin phase does with a contig after its chunk loop (phase.c:475-535), restated in plain Python over dicts and sets.
TEST INFRASTRUCTURE ONLY: the definition mrp_final_read_tags, mrp_stitch_values and mrp_close_contig are held to.  Built on
oracle/frame_oracle.py's Stitcher and phase_sets and on tests/variant_records_oracle.py's contig_variants, none of which is restated.

A chunk is a dict: read_names, read_id, hap (the phasing's tags, 1 / 2 / 0 / -1), phred, filtered (dict with read_hap: the chunk's reads,
then its filtered reads) and filtered_read (the chunk's read index of every filtered read) -- or filtered None for the haplotag tool --,
and for the variants roots = (primary root entries, filtered root entries) as tests/variant_records_oracle.py makes them (or None) and
range = (chunk_start, chunk_end)."""
from __future__ import annotations

import numpy as np

from oracle import frame_oracle as fo
from tests import variant_records_oracle as vo

REASONS = {"Same": 0, "NoHet": 1, "MissingConcordancy": 2, "UnlikelyConcordancy": 3, "Discordancy": 4}


def final_tags(ch: dict) -> list:
    """the haplotype set a chunk read ends in, 1 / 2 / 0.  phase.c:413: the reads the phasing tagged keep their tag; phase.c:419-436: the
    filtered reads and the primary reads the phasing left untagged are haplotagged afterwards and join readsBelongingToHap1 / 2.  The back
    half's result of a filtered read lies behind the chunk's reads, in list order; its primary index holds 0."""
    n = len(ch["read_names"])
    if ch.get("filtered") is None:  # tagFromPhasedVcf.c: the call's tags are the sets
        return [int(h) if h in (1, 2) else 0 for h in ch["hap"]]
    read_hap = [int(x) for x in ch["filtered"]["read_hap"]]
    at = list(range(n))
    for k, r in enumerate(ch["filtered_read"]):
        at[int(r)] = n + k
    return [int(h) if h in (1, 2) else read_hap[at[r]] for r, h in enumerate(ch["hap"])]


def printed(phred: float) -> float:
    """genomeFragment.c:117 prints the score with "%f"; getReadNames, stitching.c:300, parses the field with strtof into a double.  (The
    text has six decimals: it is never closer to the middle of two floats than 2^-44 of its size without being that middle exactly, so
    rounding it to double first and to float second gives strtof's float.)"""
    return float(np.float32(float("%f" % float(phred))))


def partition_lines(ch: dict, tags=None):
    """stitching.c:887-917 as getReadNames (:288-303) reads it back: per haplotype {read name: value}.  :896 / :909 print the reads of the
    genome fragment's own partition with their score (here: the reads the phasing itself tagged); :898-903 / :911-916 print every other
    read of the set -- the ones the back half tagged -- with -1.0.  With no fragment (tagFromPhasedVcf.c:340-348) every value is -1.0."""
    tags = final_tags(ch) if tags is None else tags
    own = ch.get("filtered") is not None
    lines = ({}, {})
    for r, name in enumerate(ch["read_names"]):
        if tags[r] not in (1, 2):
            continue
        assert name not in lines[tags[r] - 1]  # :298
        lines[tags[r] - 1][name] = printed(ch["phred"][r]) if own and ch["hap"][r] in (1, 2) else -1.0
    return lines


def close_contig(chunks, primary_reads_only=False, prevent_switching=False, rules=(2, 0.05, 0.5)) -> dict:
    """mergeContigChunkz (stitching.c:1413-1502: the first chunk's sets are the start, every later chunk goes through
    chunkToStitch_phaseAdjacentChunks), the final sets of stitching.c:1664-1671, updateHaplotypeSwitchingInVcfEntries and writePhasedVcf's
    phase set rules.  -> dict(switched, counts, final (name -> 1 / 2), final_hap per chunk, moved (names that changed sets at some chunk),
    variants, phase_sets [(phase set, reason code)])"""
    st = fo.Stitcher()
    switched, counts, moved = [], [], set()
    for c, ch in enumerate(chunks):
        l1, l2 = partition_lines(ch)
        before = {nm: 1 for nm in st.readsInHap1}
        before.update({nm: 2 for nm in st.readsInHap2})
        sw, cnt = st.chunk(l1, l2, primary_only=primary_reads_only, do_not_switch=prevent_switching or c == 0)  # stitching.c:1586
        moved |= {nm for nm, h in before.items() if nm in (st.readsInHap2 if h == 1 else st.readsInHap1)}
        switched.append(int(sw))
        counts.append(tuple(cnt))
    assert not set(st.readsInHap1) & set(st.readsInHap2)
    final = {nm: 1 for nm in st.readsInHap1}  # :1666-1671
    final.update({nm: 2 for nm in st.readsInHap2})
    out = dict(switched=switched, counts=counts, final=final, moved=moved,
               final_hap=[np.array([final.get(nm, 0) for nm in ch["read_names"]], np.int8) for ch in chunks], variants=[], phase_sets=[])
    if any(ch.get("roots") is not None for ch in chunks):
        roots = [ch["roots"] if ch.get("roots") is not None else ([], []) for ch in chunks]
        out["variants"] = vo.contig_variants(roots, [ch["range"] for ch in chunks], switched, [ch["read_id"] for ch in chunks])
        out["phase_sets"] = [(s, REASONS[why]) for s, why in fo.phase_sets(out["variants"], *rules)]
    return out


def assert_closed_equal(got: dict, want: dict, where=""):
    """capi.close_contig's dict against close_contig's: integers, sets as sorted lists, floats as bits"""
    assert got["switched"] == want["switched"], (where, got["switched"], want["switched"])
    assert got["counts"] == want["counts"], (where, got["counts"], want["counts"])
    assert len(got["final_hap"]) == len(want["final_hap"])
    for c, (g, w) in enumerate(zip(got["final_hap"], want["final_hap"])):
        assert g.dtype == np.int8 and np.array_equal(g, w), (where, c, g, w)
    assert len(got["variants"]) == len(want["variants"]), where
    for v, o in zip(got["variants"], want["variants"]):
        assert (v["pos"], v["gt1"], v["gt2"], v["chunk"], v["site"]) == (o["pos"], o["gt1"], o["gt2"], o["chunk"], o["site"]), where
        assert v["alleleIdxToReads"] == [sorted(s) for s in o["alleleIdxToReads"]], where
        for k, ko in (("genotype_log_prob", "genotypeProb"), ("hap1_log_prob", "haplotype1Prob"), ("hap2_log_prob", "haplotype2Prob")):
            assert np.float32(v[k]).view(np.uint32) == np.float32(o[ko]).view(np.uint32), (where, k)
    assert got["phase_sets"] == want["phase_sets"], where
