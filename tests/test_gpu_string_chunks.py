"""mrp_phase_string_chunks on the device: read and allele strings in, haplotypes, read partitions and HP tags out, against the
four-call chain it replaces (mrp_allele_read_supports -> mrp_profile_seqs_from_bubbles + mrp_reference_from_bubbles ->
mrp_chunk_create + mrp_phase_reads_many -> mrp_assign_reads_to_haplotypes) and against the chain of oracles."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import string_filtered_cases as sf
from tests.test_pairhmm import omodel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT_KEYS = ("ref_start", "length", "hap1", "hap2", "genotype", "ancestor", "genotype_probs", "hap_probs1", "hap_probs2", "support1", "support2",
               "reads1", "reads2", "hmm_forward", "hmm_backward", "n_sweeps")


def models():
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    return f, f.reverse_complement()


def params(**over):
    pd = synth.shipped_phase_params()
    pd.update(over)
    return capi.Params.from_reference_names(pd)


def mixed_chunks(n=48):
    """the generator's options in turn, a chunk without bubbles and bubbles without substrings among them"""
    out = []
    for i in range(n):
        if i == 5:
            out.append(synth.StringChunk(bubbles=[], read_names=["lonely_a", "lonely_b"], read_forward_strand=np.array([1, 0], np.uint8),
                                         hap=np.zeros(2, int), truth=[]))
            continue
        out.append(synth.make_string_chunk(seed=100 + i, n_sites=int(40 + (i * 7) % 60), coverage=int(12 + i % 5 * 4), multi_allelic=0.25 if i % 3 == 0 else 0.0,
                                           duplicate_rate=0.2 if i % 4 == 1 else 0.0, sv_sites=1 if i % 8 == 2 else 0, orphan_reads=3 if i % 5 == 3 else 0,
                                           empty_bubbles=2 if i % 6 == 4 else 0))
    return out


def assert_same(got, ref, chunks, profiles=True):
    assert len(got) == len(ref)
    for i, (g, r, c) in enumerate(zip(got, ref, chunks)):
        for k in RESULT_KEYS:
            a, b = g["result"][k], r["result"][k]
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (i, k)
            else:
                assert a == b, (i, k)
        assert (g["hap"] == r["hap"]).all(), i
        np.testing.assert_allclose(g["phred"], r["phred"], rtol=1e-9, atol=0, err_msg=str(i))
        in_bubble = {int(x) for _al, rs, _sb in c.bubbles for x in rs}
        for q in range(len(c.read_names)):
            if q not in in_bubble:
                assert g["hap"][q] == -1 and g["phred"][q] == 0.0
        if profiles:
            gp, rp = g["profile"], r["profile"]
            assert gp["seqs"] == rp["seqs"], i
            for k in ("read_of_seq", "pool", "allele_number", "sub", "prior"):
                assert gp[k].dtype == rp[k].dtype and (gp[k] == rp[k]).all(), (i, k)


def test_mixed_chunks_against_the_chain(gpu_ctx):
    f, r = models()
    chunks = mixed_chunks(48)
    p = params()
    got, st = capi.phase_string_chunks(gpu_ctx, chunks, f, r, p, min_phred=3, profiles=True)
    ref, rst = capi.phase_string_chunks_chain(gpu_ctx, chunks, f, r, p, min_phred=3)
    assert_same(got, ref, chunks)
    assert st.phase.resident == 1 and rst.resident == 1
    assert st.pairhmm.pairs_lane > 0 and st.pairhmm.pairs_wave > 0  # the SV alleles go to the pair-per-wave kernel
    assert st.profile_ms > 0 and st.assign_ms > 0 and st.total_ms >= st.host_ms > 0
    # the options did what they say
    assert any(len(al) > 2 for c in chunks for al, _rs, _sb in c.bubbles)
    assert any(len(rs) == 0 for c in chunks for _al, rs, _sb in c.bubbles)
    assert (np.concatenate([g["hap"] for g in got]) == -1).sum() >= 10
    tagged = np.concatenate([g["hap"] for g in got])
    assert ((tagged == 1) | (tagged == 2)).sum() > 0.8 * len(tagged)


def test_a_call_without_pairs(gpu_ctx, monkeypatch):
    """the pair-HMM launch, the profile-byte kernel and the HP kernel are all skipped: the call still equals the chain"""
    # the chain helper hands NULL for an empty array, which mrp_allele_read_supports refuses even when no bubble has a substring:
    # give it the empty read arrays a caller in C would pass (arguments 10-12: read_off, read_len, read_forward_strand)
    L = capi.load()
    supports, nothing = L.mrp_allele_read_supports, np.zeros(1, np.int64)
    monkeypatch.setattr(L, "mrp_allele_read_supports",
                        lambda *a: supports(*[nothing.ctypes.data if x is None and 10 <= i <= 12 else x for i, x in enumerate(a)]))
    f, r = models()
    chunks = sf.no_pair_chunks()
    p = params()
    got, st = capi.phase_string_chunks(gpu_ctx, chunks, f, r, p, min_phred=3, profiles=True)
    ref, _ = capi.phase_string_chunks_chain(gpu_ctx, chunks, f, r, p, min_phred=3)
    assert st.pairhmm.pairs_lane + st.pairhmm.pairs_wave == 0 and st.pairhmm.cells == 0
    assert all(len(g["profile"]["seqs"]) == 0 for g in got)
    assert all(g["hap"].shape == (len(c.read_names),) and (g["hap"] == -1).all() and (g["phred"] == 0).all() for g, c in zip(got, chunks))
    assert_same(got, ref, chunks)


def test_one_chunk_against_the_oracles(gpu_ctx, orc):
    """pair-HMM (oracle) -> getProfileSeqs (oracle) -> phasing (oracle) -> phaseBamChunkReads (oracle)"""
    from oracle import frame_oracle as fo
    f, r = models()
    c = synth.make_string_chunk(seed=9, n_sites=130, coverage=30, multi_allelic=0.2, duplicate_rate=0.1, orphan_reads=2)
    (got,), st = capi.phase_string_chunks(gpu_ctx, [c], f, r, params(), min_phred=0, profiles=True)
    strands = c.read_forward_strand
    sups = [ph.allele_read_supports(omodel(f), omodel(r), al, sb, [bool(strands[x]) for x in rs]) if rs else np.zeros((len(al), 0), np.float32)
            for al, rs, sb in c.bubbles]
    fb = [fo.Bubble(len(al), rs, np.asarray(s_).reshape(-1).tolist()) for (al, rs, _sb), s_ in zip(c.bubbles, sups)]
    pseqs = fo.get_profile_seqs(fb)
    prof = got["profile"]
    assert list(pseqs.keys()) == prof["read_of_seq"].tolist()
    assert (np.array([b for p in pseqs.values() for b in p["probs"]], dtype=np.uint8) == prof["pool"]).all()
    an, sub, prior = fo.get_reference(fb, 0.0)
    assert (prof["allele_number"] == np.array(an)).all() and (prof["sub"] == np.array(sub)).all() and (prof["prior"] == np.array(prior)).all()
    off = np.concatenate([[0], np.cumsum(prof["allele_number"])]).astype(np.int64)
    reads = [synth.Read(name=q["name"], ref_start=q["ref_start"], length=q["length"], strand=q["forward_strand"], hap=0, pool_off=q["pool_offset"],
                        nbytes=int(off[q["ref_start"] + q["length"]] - off[q["ref_start"]])) for q in prof["seqs"]]
    chunk = synth.Chunk(allele_number=prof["allele_number"], allele_offset=off, sub=prof["sub"], prior=prof["prior"], pool=prof["pool"], reads=reads)
    oc = orc.OracleChunk(chunk)
    ref = oc.phase(synth.shipped_phase_params())
    oc.close()
    for k in ("hap1", "hap2", "genotype", "ancestor"):
        assert (np.asarray(got["result"][k]) == np.asarray(ref[k])).all(), k
    ro = prof["read_of_seq"]
    assert got["result"]["reads1"] == [int(ro[q]) for q in ref["reads1"]] and got["result"]["reads2"] == [int(ro[q]) for q in ref["reads2"]]
    gf = dict(reads1={int(ro[q]) for q in ref["reads1"]}, reads2={int(ro[q]) for q in ref["reads2"]}, hap1=ref["hap1"], hap2=ref["hap2"],
              refStart=int(ref["ref_start"]), length=int(ref["length"]))
    h1, h2, phreds = fo.phase_bam_chunk_reads(gf, {int(ro[s]): p for s, p in enumerate(pseqs.values())}, off, 0)
    for q in range(len(c.read_names)):
        want = 1 if q in h1 else (2 if q in h2 else (0 if q in phreds else -1))
        assert got["hap"][q] == want, q
        if q in phreds:
            assert got["phred"][q] == pytest.approx(phreds[q], rel=1e-9, abs=1e-12)
    truth_agree = sum(1 for q in range(len(c.read_names)) if got["hap"][q] in (1, 2) and got["hap"][q] - 1 == c.hap[q])
    tagged = int(((got["hap"] == 1) | (got["hap"] == 2)).sum())
    assert tagged > 0.9 * len(ro) and max(truth_agree, tagged - truth_agree) >= 0.9 * tagged


def test_outside_the_resident_range(gpu_ctx):
    """maxPartitionsInAColumn = 200: the hashing path reads the host copy of the device-built pool"""
    f, r = models()
    chunks = [synth.make_string_chunk(seed=300 + i, n_sites=30, coverage=10, multi_allelic=0.2 * i) for i in range(2)]
    p = params(maxPartitionsInAColumn=200, minPartitionsInAColumn=200)
    got, st = capi.phase_string_chunks(gpu_ctx, chunks, f, r, p, profiles=True)
    ref, rst = capi.phase_string_chunks_chain(gpu_ctx, chunks, f, r, p)
    assert st.phase.resident == 0 and rst.resident == 0
    assert_same(got, ref, chunks)


def test_oversize_pair_is_refused_and_the_context_stays_usable(gpu_ctx):
    f, r = models()
    rng = np.random.default_rng(4)
    big = synth.random_sequence(rng, 2100)
    c = synth.StringChunk(bubbles=[([big, big.copy()], [0], [big.copy()])], read_names=["long"], read_forward_strand=np.ones(1, np.uint8),
                          hap=np.zeros(1, int), truth=[0])
    with pytest.raises(capi.MrpError) as e:  # unanchored (sv_threshold above the lengths): a 2 101-cell diagonal
        capi.phase_string_chunks(gpu_ctx, [c], f, r, params(), sv_threshold=100_000)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    chunks = [synth.make_string_chunk(seed=41, n_sites=50, coverage=16)]
    got, _ = capi.phase_string_chunks(gpu_ctx, chunks, f, r, params(), profiles=True)
    ref, _ = capi.phase_string_chunks_chain(gpu_ctx, chunks, f, r, params())
    assert_same(got, ref, chunks)


_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1])
from margin_amd import capi
from tests.test_gpu_string_chunks import mixed_chunks, models, params
lib = capi.load()
lib.mrp_set_host_threads(int(sys.argv[2]))
f, r = models()
with capi.Context(0) as ctx:
    got, st = capi.phase_string_chunks(ctx, mixed_chunks(24), f, r, params(), min_phred=3, profiles=True)
pickle.dump(got, open(sys.argv[3], "wb"))
"""


def test_repeatable_and_independent_of_host_threads(gpu_ctx, tmp_path):
    f, r = models()
    chunks = mixed_chunks(24)
    a, _ = capi.phase_string_chunks(gpu_ctx, chunks, f, r, params(), min_phred=3, profiles=True)
    b, _ = capi.phase_string_chunks(gpu_ctx, chunks, f, r, params(), min_phred=3, profiles=True)
    assert_same(a, b, chunks)
    for g, h in zip(a, b):
        assert (g["phred"] == h["phred"]).all()
    for n in (1, 16):  # the process-wide host pool is sized once per process: a fresh process each
        path = tmp_path / f"threads{n}.pkl"
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(n), str(path)], check=True, timeout=600, cwd=ROOT)
        other = pickle.load(open(path, "rb"))
        assert_same(other, a, chunks)
        for g, h in zip(other, a):
            assert (g["phred"] == h["phred"]).all()
