"""GPU parity of the filtered-read haplotagging and filtered-variant phasing (mrp_partition_reads_by_haplotype,
mrp_phase_variants_from_tagged_reads) against tests/haptag_oracle.py: decisions and states identical, totals within
1e-9 * max(1, |oracle|) (device log / exp are not glibc's; the pair-HMM values themselves are bit-identical)."""
import ctypes as C

import numpy as np
import pytest

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import haptag_oracle as ho

pytestmark = pytest.mark.gpu


def models():
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    r = f.reverse_complement()
    return f, r, ph.Model.from_buffer_copy(bytes(f)), ph.Model.from_buffer_copy(bytes(r))


def close(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return bool((np.abs(got - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))).all())


def snp_alleles(rng, n_alleles=2, flank=12):
    ref = synth.random_sequence(rng, 2 * flank + 1)
    out = [ref]
    for k in range(1, n_alleles):
        a = ref.copy()
        if k == 1:
            a[flank] = (a[flank] + 1 + rng.integers(0, 3)) % 4
        else:  # an indel allele
            a = np.concatenate([ref[:flank], synth.random_sequence(rng, int(rng.integers(1, 6))), ref[flank + 1:]]) if k == 2 else ref[np.arange(len(ref)) != flank]
        out.append(a)
    return out


def make_chunk(rng, read_base, n_sites=40, n_reads=36, duplicate_rate=0.25, sv_sites=(), hom_rate=0.15, empty_rate=0.1):
    """Partition input of one chunk: reads keep their identity (hap, strand, span) across sites; a read's substring at a site
    is a noisy copy of the allele its haplotype carries (or, with duplicate_rate, a copy of an earlier read's substring there).
    Returns (sites, read_forward_strand of the chunk's reads)."""
    haps, strands = rng.integers(0, 2, size=n_reads), rng.random(n_reads) < 0.5
    spans = []
    for _ in range(n_reads):
        a = int(rng.integers(0, n_sites))
        spans.append((a, int(min(n_sites - 1, a + rng.integers(0, 12)))))
    # two reads that span no het site: they only cover the last site, which is homozygous
    spans[0] = spans[1] = (n_sites, n_sites)
    sites = []
    for i in range(n_sites + 1):
        if i in sv_sites:
            flank = synth.random_sequence(rng, 520)
            alleles = [flank, np.concatenate([flank[:260], synth.random_sequence(rng, int(rng.integers(60, 300))), flank[260:]])]
        else:
            alleles = snp_alleles(rng)
        hom = i == n_sites or (i not in sv_sites and rng.random() < hom_rate)
        cmp_ = (1, 1) if hom else ((0, 1) if rng.random() < 0.5 else (1, 0))
        entries = []
        if i < n_sites and i not in sv_sites and rng.random() < empty_rate:
            sites.append((alleles, cmp_, entries))
            continue
        for r in range(n_reads):
            if not spans[r][0] <= i <= spans[r][1]:
                continue
            if entries and rng.random() < duplicate_rate:
                sub = entries[int(rng.integers(0, len(entries)))][1].copy()
            else:
                al = alleles[cmp_[haps[r]]]
                sub = synth.evolve_sequence(rng, al, 0.04, 0.02, 0.02) if i not in sv_sites else synth.evolve_sequence(rng, al, 0.01, 0.005, 0.005)
            entries.append((read_base + r, sub))
        sites.append((alleles, cmp_, entries))
    return sites, strands


def test_partition_several_chunks_in_one_call(gpu_ctx):
    rng = np.random.default_rng(31)
    f, r, of, orv = models()
    sites, strands = [], []
    for c in range(3):
        s, st_ = make_chunk(rng, len(strands), sv_sites=(5, 17) if c == 1 else ())
        sites += s
        strands += st_.tolist()
    n_reads = len(strands) + 4  # four reads of the call have no entry anywhere
    strands += [True, False, True, False]
    hap, h1, h2, st = capi.partition_reads_by_haplotype(gpu_ctx, f, r, sites, n_reads, strands)
    rhap, rh1, rh2 = ho.partition_filtered_reads(of, orv, sites, n_reads, strands)
    n_dup = sum(len(e) - len({bytes(x) for _, x in e}) for _, c_, e in sites if c_[0] != c_[1])
    mixed = sum(1 for _, c_, e in sites if c_[0] != c_[1] for i, (a, x) in enumerate(e) for b, y in e[i + 1:]
                if bytes(x) == bytes(y) and strands[a] != strands[b])
    assert n_dup > 20 and mixed > 5
    assert st.pairs_wave > 0 and st.pairs_lane > 0  # the SV-like alleles (> 100 symbols) take the pair-per-wave kernel
    assert any(c_[0] == c_[1] and e for _, c_, e in sites) and any(not e for _, c_, e in sites)
    ho.assert_margins_decisive(rh1, rh2, "partition")
    assert close(h1, rh1) and close(h2, rh2)
    assert (hap == rhap).all()
    assert (rhap == 0).sum() >= 6 and (rhap == 1).sum() > 10 and (rhap == 2).sum() > 10
    assert (h1[-4:] == 0).all() and (hap[-4:] == 0).all()


def make_variants(rng, n_variants=60, n_reads=40, sv_every=20):
    haps, strands = rng.integers(0, 2, size=n_reads), rng.random(n_reads) < 0.5
    read_hap = np.where(rng.random(n_reads) < 0.75, haps + 1, 0).astype(np.int32)  # a quarter untagged
    read_hap[rng.random(n_reads) < 0.1] = 7  # "anything else" is untagged too
    variants = []
    for v in range(n_variants):
        kind = v % 6
        if v % sv_every == sv_every - 1:
            flank = synth.random_sequence(rng, 540)
            alleles = [flank, np.concatenate([flank[:270], synth.random_sequence(rng, 150), flank[270:]])]
        else:
            alleles = snp_alleles(rng, int(rng.integers(2, 5)))
        g = rng.choice(len(alleles), size=2, replace=False).tolist()
        if kind == 4:
            g = [g[0], g[0]]  # homozygous
        carrier = [g[0], g[1]] if rng.random() < 0.5 else [g[1], g[0]]  # which allele each true haplotype carries
        entries = []
        if kind != 5 or v % 12 == 5:  # every other kind-5 variant has no entries
            reads = rng.choice(n_reads, size=int(rng.integers(3, 10)), replace=False)
            if kind == 3:  # only untagged reads
                reads = [q for q in range(n_reads) if read_hap[q] not in (1, 2)][:4]
            for q in sorted(int(x) for x in reads):
                if entries and rng.random() < 0.3:
                    sub = entries[int(rng.integers(0, len(entries)))][1].copy()
                else:
                    al = alleles[carrier[haps[q]]]
                    sub = synth.evolve_sequence(rng, al, 0.04, 0.02, 0.02) if len(al) < 100 else synth.evolve_sequence(rng, al, 0.01, 0.005, 0.005)
                entries.append((q, sub))
        if kind == 2:  # the same substring on a hap-1 and a hap-2 read only: an exact tie
            t1, t2 = [q for q in range(n_reads) if read_hap[q] == 1][0], [q for q in range(n_reads) if read_hap[q] == 2][0]
            sub = synth.evolve_sequence(rng, alleles[g[0]])
            entries = [(min(t1, t2), sub), (max(t1, t2), sub.copy())]
        variants.append((alleles, tuple(g), entries))
    return variants, strands, read_hap


def test_phase_variants(gpu_ctx):
    rng = np.random.default_rng(47)
    f, r, of, orv = models()
    variants, strands, read_hap = make_variants(rng)
    n_reads = len(strands)
    state, cis, trans, st = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, n_reads, strands, read_hap)
    rstate, rcis, rtrans = ho.phase_filtered_variants(of, orv, variants, n_reads, strands, read_hap)
    assert st.pairs_wave > 0 and st.pairs_lane > 0
    assert {int(x) for x in rstate} == {ho.NOT_VISITED, ho.CIS, ho.TRANS, ho.TIE}
    assert any(s_ == ho.TIE and c_ != 0 for s_, c_ in zip(rstate, rcis))  # a tie of equal supports, not only of no tagged entry
    ho.assert_margins_decisive(rcis, rtrans, "phasing")
    assert close(cis, rcis) and close(trans, rtrans)
    assert (state == rstate).all()
    assert ((cis == trans) == (rcis == rtrans)).all()
    # the anchored pairs: without the threshold the long alleles take their whole matrix and the totals move
    _, cis_full, _, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, n_reads, strands, read_hap, sv_threshold=10 ** 6)
    sv = [i for i, (al, g, e) in enumerate(variants) if max(len(a) for a in al) > 512 and g[0] != g[1] and any(read_hap[q] in (1, 2) for q, _ in e)]
    assert sv and all(cis_full[i] != cis[i] for i in sv)


def test_phase_variants_duplicates_across_strands(gpu_ctx):
    """a duplicated substring: the first TAGGED entry's strand picks the state machine, an untagged one before it does not"""
    rng = np.random.default_rng(5)
    f, r, of, orv = models()
    variants = []
    for _ in range(30):
        alleles = snp_alleles(rng, 3)
        sub = synth.evolve_sequence(rng, alleles[1])
        variants.append((alleles, (1, 2), [(0, sub), (1, sub.copy()), (2, sub.copy()), (3, synth.evolve_sequence(rng, alleles[2]))]))
    strands, read_hap = [True, False, True, False], [0, 2, 1, 2]
    state, cis, trans, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, 4, strands, read_hap)
    rstate, rcis, rtrans = ho.phase_filtered_variants(of, orv, variants, 4, strands, read_hap)
    ho.assert_margins_decisive(rcis, rtrans)
    assert (state == rstate).all() and close(cis, rcis) and close(trans, rtrans)
    # read 1 (the first tagged, reverse strand) owns the scores: the strand of untagged read 0 changes nothing, read 1's does
    _, cis0, trans0, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, 4, [False, False, True, False], read_hap)
    assert (cis0 == cis).all() and (trans0 == trans).all()
    _, cis1, _, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, 4, [True, True, True, False], read_hap)
    assert (cis1 != cis).sum() > len(variants) // 2


def raw_call(fn, ctx, f, r, sites, strands, read_hap, n_out):
    """the C entry with its outputs pre-filled, so that a result the call did not write shows: (decision, total a, total b, stats)"""
    S, keep = capi._haptag_sites(sites)
    sd = np.ascontiguousarray(strands, dtype=np.uint8)
    dec, a, b = np.full(n_out, 99, np.int32), np.full(n_out, 9.0), np.full(n_out, 9.0)
    st = capi.PairHmmStats()
    if read_hap is None:
        rc = fn(ctx.h, C.byref(f), C.byref(r), C.byref(S), sd.size, sd.ctypes.data, 4, dec.ctypes.data, a.ctypes.data, b.ctypes.data, C.byref(st))
    else:
        rh = np.ascontiguousarray(read_hap, dtype=np.int32)
        rc = fn(ctx.h, C.byref(f), C.byref(r), C.byref(S), sd.size, sd.ctypes.data, rh.ctypes.data, 4, 512, dec.ctypes.data, a.ctypes.data, b.ctypes.data,
                C.byref(st))
    capi._check(rc)
    return dec, a, b, st


def test_partition_without_an_active_site(gpu_ctx):
    """the one site compares an allele with itself: no pair is scored, the reduction runs over nothing"""
    rng = np.random.default_rng(3)
    f, r, of, orv = models()
    alleles = snp_alleles(rng)
    sites = [(alleles, (1, 1), [(0, alleles[1].copy()), (1, alleles[0].copy())])]
    rhap, rh1, rh2 = ho.partition_filtered_reads(of, orv, sites, 2, [True, False])
    assert list(rhap) == [0, 0] and list(rh1) == [0.0, 0.0] and list(rh2) == [0.0, 0.0]
    hap, h1, h2, st = raw_call(capi.load().mrp_partition_reads_by_haplotype, gpu_ctx, f, r, sites, [1, 0], None, 2)
    assert st.pairs_lane + st.pairs_wave == 0 and st.cells == 0
    assert hap.tolist() == [0, 0] and h1.tolist() == [0.0, 0.0] and h2.tolist() == [0.0, 0.0]


def test_phase_variants_without_a_tagged_entry(gpu_ctx):
    """a heterozygous variant whose only entry is an untagged read: visited, but nothing is scored -- a tie of two empty sums"""
    rng = np.random.default_rng(4)
    f, r, of, orv = models()
    alleles = snp_alleles(rng)
    variants = [(alleles, (0, 1), [(0, alleles[1].copy())])]
    rstate, rcis, rtrans = ho.phase_filtered_variants(of, orv, variants, 1, [True], [0])
    assert list(rstate) == [ho.TIE] and list(rcis) == [0.0] and list(rtrans) == [0.0]
    state, cis, trans, st = raw_call(capi.load().mrp_phase_variants_from_tagged_reads, gpu_ctx, f, r, variants, [1], [0], 1)
    assert st.pairs_lane + st.pairs_wave == 0 and st.cells == 0
    assert state.tolist() == [ho.TIE] and cis.tolist() == [0.0] and trans.tolist() == [0.0]


def test_end_to_end_chunk_loop(gpu_ctx, orc):
    """strings -> allele_read_supports -> profile seqs -> phase_reads_many -> read assignment; the withheld reads (as
    downsampling leaves them) and the unassigned ones partitioned against the fragment's alleles; then filtered
    multi-allelic variants phased with the union of the tagged reads.  Every decision against the same chain of oracles."""
    from oracle import frame_oracle as fo
    rng = np.random.default_rng(91)
    f, r, of, orv = models()
    n_sites, n_reads = 120, 110
    truth = rng.integers(0, 2, size=n_sites)
    haps, strands = rng.integers(0, 2, size=n_reads), rng.random(n_reads) < 0.5
    spans = []
    for _ in range(n_reads):
        a = int(rng.integers(0, n_sites - 5))
        spans.append((a, int(min(n_sites - 1, a + rng.integers(4, 40)))))
    kept = [q for q in range(n_reads) if rng.random() < 0.7]
    withheld = [q for q in range(n_reads) if q not in kept]
    kidx = {q: i for i, q in enumerate(kept)}
    site_alleles, site_subs = [], []
    for i in range(n_sites):
        ref = synth.random_sequence(rng, 25)
        alt = ref.copy()
        alt[12] = (alt[12] + 1 + rng.integers(0, 3)) % 4
        subs = {}
        for q, (a, b) in enumerate(spans):
            if a <= i <= b:
                allele = truth[i] if haps[q] == 0 else 1 - truth[i]
                subs[q] = synth.evolve_sequence(rng, alt if allele else ref, 0.04, 0.02, 0.02)
        site_alleles.append([ref, alt])
        site_subs.append(subs)
    # 1. the phasing of the kept reads
    bubbles = [(al, [s[q] for q in kept if q in s], [bool(strands[q]) for q in kept if q in s]) for al, s in zip(site_alleles, site_subs)]
    br = [[kidx[q] for q in kept if q in s] for s in site_subs]
    sup, _ = capi.allele_read_supports(gpu_ctx, f, r, bubbles)
    an = [2] * n_sites
    seqs, pool = capi.profile_seqs_from_bubbles(an, br, sup, len(kept))
    a_num, sub, prior = capi.reference_from_bubbles(an, br, sup, 0.0)
    off = np.concatenate([[0], np.cumsum(a_num)]).astype(np.int64)
    reads = [synth.Read(name=f"r{s_['read']:04d}", ref_start=s_["ref_start"], length=s_["length"], strand=int(strands[kept[s_["read"]]]),
                        hap=int(haps[kept[s_["read"]]]), pool_off=s_["pool_offset"],
                        nbytes=int(off[s_["ref_start"] + s_["length"]] - off[s_["ref_start"]])) for s_ in seqs]
    chunk = synth.Chunk(allele_number=a_num, allele_offset=off, sub=sub, prior=prior, pool=pool, reads=reads)
    pd = synth.shipped_phase_params()
    dchunk = capi.DeviceChunk.from_chunk(gpu_ctx, chunk)
    (got,), _ = capi.phase_reads_many(gpu_ctx, [dchunk], [chunk], capi.Params.from_reference_names(pd))
    dchunk.close()
    recs, _ = capi.read_records(chunk)
    ahap, _ = capi.assign_reads_to_haplotypes(a_num, pool, recs, len(reads), got, min_phred=0)
    oc = orc.OracleChunk(chunk)
    ref = oc.phase(pd)
    oc.close()
    pseqs = {i: dict(refStart=x.ref_start, length=x.length, probs=chunk.pool[x.pool_off:x.pool_off + x.nbytes].tolist()) for i, x in enumerate(chunk.reads)}
    ogf = dict(refStart=ref["ref_start"], length=ref["length"], hap1=ref["hap1"], hap2=ref["hap2"], reads1=set(ref["reads1"]), reads2=set(ref["reads2"]))
    o1, o2, _ = fo.phase_bam_chunk_reads(ogf, pseqs, off.tolist(), 0)
    ohap = np.array([1 if i in o1 else 2 if i in o2 else 0 for i in range(len(reads))])
    assert (np.where((ahap == 1) | (ahap == 2), ahap, 0) == ohap).all()

    def tags(assigned):  # per original read: 1 / 2 from the phasing, 0 otherwise
        t = np.zeros(n_reads, dtype=np.int32)
        for i, s_ in enumerate(seqs):
            t[kept[s_["read"]]] = assigned[i] if assigned[i] in (1, 2) else 0
        return t
    dtag, otag = tags(ahap), tags(ohap)
    # 2. the filtered reads: withheld plus those the phasing left untagged, against the fragment's hap1 / hap2 alleles
    filtered = sorted(set(withheld) | {q for q in kept if dtag[q] == 0})

    def partition_sites(gf):
        out = []
        for j in range(gf["length"]):
            i = gf["ref_start"] + j
            out.append((site_alleles[i], (int(gf["hap1"][j]), int(gf["hap2"][j])), [(q, site_subs[i][q]) for q in filtered if q in site_subs[i]]))
        return out
    psites = partition_sites(got)
    assert len(psites) > 50
    phap, ph1, ph2, _ = capi.partition_reads_by_haplotype(gpu_ctx, f, r, psites, n_reads, strands)
    rphap, rph1, rph2 = ho.partition_filtered_reads(of, orv, partition_sites(ref), n_reads, strands)
    ho.assert_margins_decisive(rph1, rph2, "partition")
    assert (phap == rphap).all() and close(ph1, rph1) and close(ph2, rph2)
    assert ((phap[withheld] == 1) | (phap[withheld] == 2)).mean() > 0.7
    # 3. filtered multi-allelic variants, phased with the union of the tagged reads
    dunion = np.where(np.isin(np.arange(n_reads), filtered), phap, dtag)
    ounion = np.where(np.isin(np.arange(n_reads), filtered), rphap, otag)
    assert (dunion == ounion).all()
    variants = []
    for v in range(40):
        i = int(rng.integers(0, n_sites))
        alleles = snp_alleles(rng, int(rng.integers(3, 5)))
        g = rng.choice(len(alleles), size=2, replace=False).tolist()
        entries = []
        for q in sorted(site_subs[i]):
            carried = g[truth[i]] if haps[q] == 0 else g[1 - truth[i]]
            entries.append((q, synth.evolve_sequence(rng, alleles[carried], 0.04, 0.02, 0.02)))
        variants.append((alleles, tuple(g), entries))
    state, cis, trans, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, variants, n_reads, strands, dunion)
    rstate, rcis, rtrans = ho.phase_filtered_variants(of, orv, variants, n_reads, strands, ounion)
    ho.assert_margins_decisive(rcis, rtrans, "phasing")
    assert (state == rstate).all() and close(cis, rcis) and close(trans, rtrans)
    assert ((rstate == ho.CIS) | (rstate == ho.TRANS)).mean() > 0.8


def test_unanchored_pair_over_the_diagonal_limit_is_refused(gpu_ctx):
    f, r, _, _ = models()
    rng = np.random.default_rng(2)
    big = synth.random_sequence(rng, 2100)
    sites = [([big, synth.random_sequence(rng, 30)], (0, 1), [(0, big.copy())])]
    with pytest.raises(capi.MrpError) as e:  # the partition never anchors: a 2 101-cell diagonal
        capi.partition_reads_by_haplotype(gpu_ctx, f, r, sites, 1, [True])
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    with pytest.raises(capi.MrpError) as e:  # phasing with the threshold above the strings: unanchored as well
        capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, sites, 1, [True], [1], sv_threshold=10 ** 6)
    assert e.value.code == capi.MRP_ERR_UNSUPPORTED
    # the context is unharmed, and the same site anchored past the threshold goes through
    state, _, _, _ = capi.phase_variants_from_tagged_reads(gpu_ctx, f, r, sites, 1, [True], [1], sv_threshold=512)
    assert state[0] in (ho.CIS, ho.TRANS, ho.TIE)
    with pytest.raises(capi.MrpError) as e:
        capi.partition_reads_by_haplotype(gpu_ctx, f, r, sites, 1, [True], expansion=3)
    assert e.value.code == capi.MRP_ERR_ARG
