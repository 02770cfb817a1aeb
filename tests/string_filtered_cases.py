"""Inputs of the mrp_phase_string_chunks_with_filtered tests and the yardstick they are compared against: the chain of the
EXISTING calls -- mrp_phase_string_chunks over the primary reads, then host-assembled sites into
mrp_phase_variants_from_tagged_reads (tags: the primary tags only) and mrp_partition_reads_by_haplotype (participants: the
filtered reads in index order, then the primary reads the phasing left untagged, in index order; sites: the fragment's bubbles
with the fragment's hap1 / hap2 alleles), assembled as tests/test_gpu_haptag.py::test_end_to_end_chunk_loop assembles them."""
import numpy as np

from margin_amd import capi, synth

MIN_PHRED = 40  # a read over one or two sites stays below it: primary reads the phasing leaves untagged


def split_chunk(seed: int, **opts):
    """A synthetic chunk whose reads are split into primary and filtered ones (about half each, as maxDepth = 32 leaves 60x data),
    with filtered variants at some of its sites.  Returns (synth.StringChunk of the primary reads, rest dict for
    capi.string_chunk_rest_struct)."""
    n_variants = opts.pop("n_variants", 6)
    full = synth.make_string_chunk(seed=seed, span=(1, 14), **opts)
    rng = np.random.default_rng([seed, 23])
    n = len(full.read_names)
    is_filtered = rng.random(n) < 0.5
    new_index = np.zeros(n, dtype=np.int64)
    new_index[~is_filtered] = np.arange(int((~is_filtered).sum()))
    new_index[is_filtered] = np.arange(int(is_filtered.sum()))
    n_primary = int((~is_filtered).sum())
    bubbles, fsubs = [], []
    hom = int(rng.integers(0, len(full.bubbles))) if len(full.bubbles) > 4 else -1
    for b, (alleles, reads, subs) in enumerate(full.bubbles):
        if b == hom and max(len(a) for a in alleles) < 100:  # every read carries allele 0 here: a homozygous site of the fragment
            subs = [synth._noisy_copy(rng, alleles[0], 0.02, 0.01, 0.01) for _ in subs]
        bubbles.append((alleles, [int(new_index[r]) for r in reads if not is_filtered[r]], [s for r, s in zip(reads, subs) if not is_filtered[r]]))
        fsubs.append(sorted(((int(new_index[r]), s) for r, s in zip(reads, subs) if is_filtered[r]), key=lambda x: x[0]))
    primary = synth.StringChunk(bubbles=bubbles, read_names=[nm for nm, f in zip(full.read_names, is_filtered) if not f],
                                read_forward_strand=np.ascontiguousarray(full.read_forward_strand[~is_filtered]), hap=full.hap[~is_filtered],
                                truth=full.truth)
    variants = []
    sites = [b for b in range(len(full.bubbles)) if full.bubbles[b][1]]
    long_sites = [b for b in sites if max(len(a) for a in full.bubbles[b][0]) > 512]
    for v in range(n_variants if sites else 0):
        b = sites[int(rng.integers(0, len(sites)))]
        if v == 0 and long_sites:
            b = long_sites[0]  # a chunk with an SV bubble has a filtered variant of SV length there
        alleles0, reads, _subs = full.bubbles[b]
        long_site = max(len(a) for a in alleles0) > 512
        if long_site:  # the SV bubble's own alleles: pairs past sv_threshold, anchored when variants are phased
            alleles, g = [a.copy() for a in alleles0], [0, 1]
        else:
            ref = synth.random_sequence(rng, 25)
            alleles = [ref]
            for k in range(1, int(rng.integers(2, 5))):
                alt = ref.copy()
                alt[(10 + 3 * k) % 25] = (alt[(10 + 3 * k) % 25] + k) % 4
                alleles.append(alt)
            g = rng.choice(len(alleles), size=2, replace=False).tolist()
        kind = v % 6
        if kind == 4:
            g = [g[0], g[0]]  # homozygous: not visited
        entries = []
        for r in reads:  # in the order of the original reads: primary and filtered ones interleaved
            if kind == 3 and not is_filtered[r]:
                continue  # only filtered reads: no tagged entry, a tie
            if entries and rng.random() < 0.3:
                sub = entries[int(rng.integers(0, len(entries)))][1].copy()
            else:
                al = alleles[g[int(full.hap[r])]]
                sub = synth._noisy_copy(rng, al, 0.04, 0.02, 0.02) if len(al) < 100 else synth._noisy_copy(rng, al, 0.01, 0.005, 0.005)
            entries.append((int(new_index[r]) + (n_primary if is_filtered[r] else 0), sub))
        if kind == 5:
            entries = []  # no entries: not visited
        variants.append((alleles, (int(g[0]), int(g[1])), entries))
    rest = dict(forward_strand=np.ascontiguousarray(full.read_forward_strand[is_filtered]), fsubs=fsubs, variants=variants)
    return primary, rest


def filtered_chunks(n=26):
    """mixed shapes: multi-allelic sites, duplicated substrings (classes across strands, across primary and filtered reads), an SV
    bubble in a few, orphan reads, empty bubbles; chunk 4 has an empty rest, chunk 9 no bubbles and an empty rest"""
    chunks, rests = [], []
    for i in range(n):
        if i == 9:
            chunks.append(synth.StringChunk(bubbles=[], read_names=["lonely_a", "lonely_b"], read_forward_strand=np.array([1, 0], np.uint8),
                                            hap=np.zeros(2, int), truth=[]))
            rests.append(None)
            continue
        c, r = split_chunk(400 + i, n_sites=int(30 + (i * 37) % 90), coverage=int(24 + i % 4 * 8), multi_allelic=0.3 if i % 3 == 0 else 0.0,
                           duplicate_rate=0.25 if i % 2 == 1 else 0.05, sv_sites=1 if i % 8 == 2 else 0, orphan_reads=3 if i % 5 == 3 else 0,
                           empty_bubbles=2 if i % 6 == 4 else 0)
        chunks.append(c)
        rests.append(None if i == 4 else r)
    return chunks, rests


def no_pair_chunks():
    """a chunk of 3 reads and no bubble, a chunk of 2 bubbles without a substring: no pair, no profile sequence in the whole call"""
    rng = np.random.default_rng(12)
    lonely = synth.StringChunk(bubbles=[], read_names=["a0", "a1", "a2"], read_forward_strand=np.array([1, 0, 1], np.uint8), hap=np.zeros(3, int), truth=[])
    bubbles = [([synth.random_sequence(rng, 25), synth.random_sequence(rng, 25)], [], []) for _ in range(2)]
    bare = synth.StringChunk(bubbles=bubbles, read_names=["b0", "b1"], read_forward_strand=np.array([1, 0], np.uint8), hap=np.zeros(2, int), truth=[0, 0])
    return [lonely, bare]


def chain(ctx, chunks, rests, f, r, p, min_phred=MIN_PHRED, expansion=4, sv_threshold=512):
    """The yardstick.  Returns (front: phase_string_chunks' list, back: per chunk dict(read_hap, h1, h2, variant_state, cis, trans,
    psites, tagged) -- psites the partition's sites, for the checks on the inputs)."""
    front, _ = capi.phase_string_chunks(ctx, chunks, f, r, p, min_phred=min_phred, expansion=expansion, sv_threshold=sv_threshold, profiles=True)
    back = []
    for c, rest, g in zip(chunks, rests, front):
        n_primary = len(c.read_names)
        tags = np.where((g["hap"] == 1) | (g["hap"] == 2), g["hap"], 0).astype(np.int32)
        if rest is None:
            back.append(dict(read_hap=tags, h1=np.zeros(n_primary), h2=np.zeros(n_primary), variant_state=np.zeros(0, np.int32), cis=np.zeros(0),
                             trans=np.zeros(0), psites=[], tagged=tags))
            continue
        n_filtered = len(rest["forward_strand"])
        n_all = n_primary + n_filtered
        strands = np.concatenate([c.read_forward_strand, rest["forward_strand"]]).astype(np.uint8)
        tagged = np.concatenate([tags, np.zeros(n_filtered, np.int32)])
        # variants first, with the primary tags only (phase.c:413)
        if rest["variants"]:
            state, cis, trans, _ = capi.phase_variants_from_tagged_reads(ctx, f, r, rest["variants"], n_all, strands, tagged, expansion=expansion,
                                                                         sv_threshold=sv_threshold)
        else:
            state, cis, trans = np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
        # then the reads (phase.c:419-436)
        res = g["result"]
        psites = []
        for j in range(int(res["length"])):
            b = int(res["ref_start"]) + j
            alleles, reads, subs = c.bubbles[b]
            entries = [(n_primary + fr, sub) for fr, sub in rest["fsubs"][b]]
            entries += [(q, sub) for q, sub in sorted(zip(reads, subs), key=lambda x: x[0]) if tags[q] == 0]
            psites.append((alleles, (int(res["hap1"][j]), int(res["hap2"][j])), entries))
        hap, h1, h2, _ = capi.partition_reads_by_haplotype(ctx, f, r, psites, n_all, strands, expansion=expansion)
        is_tagged = tagged != 0
        back.append(dict(read_hap=np.where(is_tagged, tagged, hap).astype(np.int32), h1=np.where(is_tagged, 0.0, h1), h2=np.where(is_tagged, 0.0, h2),
                         variant_state=state, cis=cis, trans=trans, psites=psites, tagged=tagged))
    return front, back


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_back_identical(got, back):
    """decisions identical, totals bit for bit"""
    assert len(got) == len(back)
    for i, (g, b) in enumerate(zip(got, back)):
        o = g["filtered"]
        for k in ("read_hap", "variant_state"):
            assert o[k].dtype == np.int32 and o[k].shape == b[k].shape and (o[k] == b[k]).all(), (i, k)
        for k in ("h1", "h2", "cis", "trans"):
            assert o[k].shape == b[k].shape and (bits(o[k]) == bits(b[k])).all(), (i, k, float(np.abs(o[k] - b[k]).max()))
