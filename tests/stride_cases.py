"""Inputs that make the kernels of the alignment front take a second trip: more than 64 parts per work item (a wave's lanes
stride over them 64 at a time) and more work items than the grid cap (the waves stride over them).  TEST INFRASTRUCTURE ONLY.

Every builder comes with a function that returns the facts its case must exhibit, computed from the references alone
(tests/extract_oracle.py, tests/haplotag_aligned_oracle.py, oracle.pairhmm, a Python restatement of the k-mer chain's walk);
tests/test_stride_cases.py asserts them without a device, tests/test_gpu_front_strides.py runs the cases on one.  Builders and
oracle results are cached: a chunk is generated once per process, whichever module asks first."""
from __future__ import annotations

import functools

import numpy as np

from margin_amd import capi, synth
from oracle import pairhmm as ph
from tests import extract_cases as ec
from tests import extract_oracle as eo
from tests import haplotag_aligned_oracle as hao

OPTS = dict(ec.OPTS)           # expansion_small 2, expansion_sv 6
K = 20                         # KMER_SIZE
GRID_CAP = 65_536              # ex_rank / ex_gather / ha_owners / ec_classes / ak_chain
PHM_GRID_CAP = 16_384          # phm_wave_kernel
BOUNDARY_COUNTS = (63, 64, 65, 127, 128, 129, 200)
BUCKET_SIZES = (63, 64, 65, 128, 129)
CIGAR_OPS = (63, 64, 65, 128, 129)


# ---- A. extraction ----

def make_chunk(reference: str, overlap_start: int, variants, reads, chunk_start=None, chunk_end=None):
    """tests/extract_cases.make over a reference and overlap range of the caller's.  variants: [(genome pos, alleles, is_sv)];
    reads: [(pos, cigar text, mapq, flag)]; a read's bases cycle A C G T from its first base (soft clip included)"""
    cf, sf, cig, seq, pos, flag, mapq, lq = [0], [0], [], [], [], [], [], []
    for p, text, mq, fl in reads:
        w = ec.cigar(text)
        n = ec.qlen(w)
        packed = synth.pack_seq(np.array((1, 2, 4, 8), np.uint8)[np.arange(n) % 4])
        cig += w
        seq.append(packed)
        cf.append(cf[-1] + len(w))
        sf.append(sf[-1] + len(packed))
        pos.append(p); flag.append(fl); mapq.append(mq); lq.append(n)
    end = overlap_start + len(reference)
    return synth.AlignedChunk(overlap_start=overlap_start, overlap_end=end, chunk_start=overlap_start if chunk_start is None else chunk_start,
                              chunk_end=end if chunk_end is None else chunk_end, reference=reference,
                              variant_pos=np.array([v[0] for v in variants], np.int64), alleles=[list(v[1]) for v in variants],
                              is_sv=np.array([v[2] for v in variants], np.uint8), read_pos=np.array(pos, np.int64),
                              flag=np.array(flag, np.uint16), mapq=np.array(mapq, np.uint8), l_qseq=np.array(lq, np.int32),
                              cigar_first=np.array(cf, np.int64), cigar=np.array(cig, np.uint32), seq_first=np.array(sf, np.int64),
                              seq=np.concatenate(seq) if seq else np.zeros(0, np.uint8), read_names=[f"stride{k}" for k in range(len(reads))])


def random_reference(seed: int, n: int) -> str:
    return "".join("ACGT"[int(c)] for c in np.random.default_rng(seed).integers(0, 4, size=n))


def snp_everywhere(reference: str, overlap_start: int, sv=()):
    """a biallelic SNP at every position of the slice; sv: slice positions whose variant carries the SV flag"""
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    sv = set(sv)
    return [(overlap_start + p, [c, nxt[c]], 1 if p in sv else 0) for p, c in enumerate(reference)]


OVL = 1_000                    # genome position of the small chunks' slice
LONG_START = 5                 # slice position of the 200-entry read: its candidates 64 and 128 carry the SV flag
SV_CANDIDATES = (64, 128)
BUCKET_AT = dict(zip(BUCKET_SIZES, (220, 250, 280, 310, 340)))  # slice position of each stack of identical reads
BUCKET_READ = 10               # ... of "10M" reads: the variants at its ten positions get one substring from each


@functools.lru_cache(maxsize=None)
def boundary_chunk():
    """A1: a 400 bp slice with a SNP at every position: a read kM has k entries.  Reads with exactly BOUNDARY_COUNTS entries (one
    starting and one ending with a soft clip, one of low mapq, one =/X read with an insertion and a deletion past its 64th entry),
    two SV-flagged variants that are candidates 64 and 128 of the longest read, and stacks of identical short reads of BUCKET_SIZES
    reads each, of mixed mapq and strand, in round-robin order"""
    ref = random_reference(41, 400)
    variants = snp_everywhere(ref, OVL, sv=[LONG_START + c for c in SV_CANDIDATES])
    long_reads = [(OVL + LONG_START, "200M", 60, 0), (OVL + 4, "63M", 60, 0x10), (OVL + 3, "4S64M", 60, 0), (OVL + 6, "65M3S", 60, 0),
                  (OVL + 7, "127M", 3, 0), (OVL + 8, "128M", 60, 0), (OVL + 9, "70=1X10=2I15=3D30=", 60, 0x10)]
    stacks = []
    for i in range(max(BUCKET_SIZES)):
        for size in BUCKET_SIZES:
            if i < size:
                stacks.append((OVL + BUCKET_AT[size], f"{BUCKET_READ}M", 3 if i % 3 == 1 else 60, 0x10 if i % 2 else 0))
    return make_chunk(ref, OVL, variants, long_reads[:4] + stacks + long_reads[4:])


@functools.lru_cache(maxsize=None)
def boundary_oracle():
    return eo.extract([boundary_chunk()], OPTS)[0]


def boundary_facts() -> dict:
    """entries per read; per SV candidate of the longest read (read 0) its number counted from the read's first entry, its
    substring's length, the length its own window would give and the length from the carried maximum of the window starts; per
    stack its buckets' sizes, whether entry_read ascends, and the read statuses inside"""
    x = boundary_oracle()
    a = eo.as_arrays(x)
    start, stop = a["ref_aln_start"], a["ref_aln_stop_incl"]
    carry = []
    for c in SV_CANDIDATES:                                   # read 0 is all M without clip: sequence advance = reference advance
        v = LONG_START + c
        lo, hi = int(a["entry_first"][v]), int(a["entry_first"][v + 1])
        e = lo + a["entry_read"][lo:hi].tolist().index(0)
        before = int(start[LONG_START:v].max())
        carry.append(dict(candidate=v - LONG_START, length=int(a["entry_len"][e]), own_window=int(stop[v] - start[v]),
                          before=before, own_start=int(start[v]), predecessor_start=int(start[v - 1]),
                          from_carry=int(stop[v] - max(int(start[v]), before))))
    buckets = {}
    for size, at in BUCKET_AT.items():
        per = []
        for v in range(at, at + BUCKET_READ):
            reads = a["entry_read"][a["entry_first"][v]:a["entry_first"][v + 1]]
            per.append(dict(n=len(reads), ascending=bool((np.diff(reads) > 0).all()), statuses=set(a["read_status"][reads].tolist())))
        buckets[size] = per
    return dict(entries_per_read=a["read_n_substrings"].tolist(), status=a["read_status"].tolist(), carry=carry, buckets=buckets)


def block_cigar(n_ops: int, lead, trail) -> str:
    """lead + alternating 1M 1I 2M 1D + trail, n_ops ops in all, the last body op an M"""
    pat = ("1M", "1I", "2M", "1D")
    body = [pat[i % 4] for i in range(n_ops - len(lead) - len(trail))]
    if body[-1] in ("1I", "1D"):
        body[-1] = "2M"
    return "".join(list(lead) + body + list(trail))


@functools.lru_cache(maxsize=None)
def cigar_chunk():
    """A2: the slice of A1 (one SV-flagged variant) under reads whose CIGARs have exactly CIGAR_OPS ops: H S body S H (the end-clip
    search starts in the last block; the last op of the first block of 64 is a sequence op), S body S (the ops shifted by
    one: a reference op there), one read with H S in front and no clip behind, and one with an N op and 65 ops (the loop-bound rule of
    extract_cases case 5 over a long CIGAR)"""
    ref = random_reference(41, 400)
    variants = snp_everywhere(ref, OVL, sv=[70])
    reads = []
    for k, n in enumerate(CIGAR_OPS):
        reads.append((OVL + 3 + k, block_cigar(n, ("2H", "3S"), ("3S", "2H")), 60 if k != 1 else 3, 0x10 if k % 2 else 0))
        reads.append((OVL + 20 + k, block_cigar(n, ("3S",), ("3S",)), 60, 0))
    reads.append((OVL + 11, block_cigar(65, ("2H", "3S"), ()), 60, 0))
    reads.append((OVL + 12, block_cigar(65, ("4M", "10N"), ()), 60, 0x10))
    return make_chunk(ref, OVL, variants, reads)


def cigar_facts() -> dict:
    c = cigar_chunk()
    x = eo.extract([c], OPTS)[0]
    n_ops = np.diff(c.cigar_first).tolist()
    with_n = [r for r in range(len(n_ops)) if any((w & 15) == eo.N for w in c.cigar[c.cigar_first[r]:c.cigar_first[r + 1]])]
    return dict(n_ops=n_ops, entries_per_read=x["read_n_substrings"].tolist(), n_read=with_n,
                n_read_aligned=[eo.aligned_read_length([int(w) for w in c.cigar[c.cigar_first[r]:c.cigar_first[r + 1]]], int(c.l_qseq[r]))[0] for r in with_n],
                n_read_ref_steps=[sum(int(w) >> 4 for w in c.cigar[c.cigar_first[r]:c.cigar_first[r + 1]] if (int(w) & 15) in (eo.M, eo.D, eo.N, eo.EQ, eo.X)) for r in with_n])


DENSE_SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def dense_chunk(seed: int):
    """A3: 90x coverage over 4 kb with a variant every 24 bases: reads with more than 128 entries, variants with more than 64"""
    return synth.make_aligned_chunk(seed, overlap_bp=4000, margin_bp=200, coverage=90.0, read_len=(3000, 6000), variant_every=24)


def option_sets():
    """the three option sets of tests/test_gpu_extract.py"""
    return [capi.shipped_extract_options(),
            dict(expansion_small=4, expansion_sv=64, min_mapq=20, include_secondary=1, include_supplementary=1),
            dict(expansion_small=0, expansion_sv=0, min_mapq=0, include_secondary=0, include_supplementary=1)]


@functools.lru_cache(maxsize=None)
def dense_oracle(seed: int, k: int = 0):
    return eo.extract([dense_chunk(seed)], option_sets()[k])[0]


def dense_facts(seed: int) -> dict:
    x = dense_oracle(seed, 0)
    per_read = np.asarray(x["read_n_substrings"])
    per_var = np.array([len(e) for e in x["entries"]])
    return dict(reads=len(per_read), variants=len(per_var), entries=int(per_read.sum()), reads_over_64=int((per_read > 64).sum()),
                reads_over_128=int((per_read > 128).sum()), max_per_read=int(per_read.max()), variants_over_64=int((per_var > 64).sum()),
                max_per_variant=int(per_var.max()))


WIDE_BP = 66_000
WIDE_READS = ((10, "150M", 60, 0), (65_640, "100M", 60, 0), (65_720, "60M2I40M", 60, 0x10), (65_644, "90M", 60, 0))


@functools.lru_cache(maxsize=None)
def wide_chunk():
    """A4 (ii), B1: a 66 000 bp slice with a SNP at every position, so more variants than the grid cap of the kernels that run a wave
    per variant, under four reads: one near the start and three past variant 65 536.  The 100M and the 90M read start four bases
    apart, so their bases agree wherever both lie: equal substrings at one site"""
    ref = random_reference(43, WIDE_BP)
    return make_chunk(ref, OVL, snp_everywhere(ref, OVL), [(OVL + p, c, q, f) for p, c, q, f in WIDE_READS])


@functools.lru_cache(maxsize=None)
def wide_oracle():
    return eo.extract([wide_chunk()], OPTS)[0]


def wide_facts() -> dict:
    x = wide_oracle()
    has = np.array([len(e) > 0 for e in x["entries"]])
    return dict(variants=len(has), entries=int(np.sum(x["read_n_substrings"])), entries_per_read=np.asarray(x["read_n_substrings"]).tolist(),
                with_entries_below_cap=int(has[:GRID_CAP].sum()), with_entries_past_cap=int(has[GRID_CAP:].sum()))


def wide_genotypes():
    return np.tile(np.array([[0, 1]], np.int32), (WIDE_BP, 1))


def pair_hmm_models():
    """margin phase's forward and reverse-strand read models -> (capi forward, capi reverse, oracle forward, oracle reverse)"""
    f = capi.PairHmm.from_margin_hmm(*synth.margin_phase_pair_hmm_arrays())
    r = f.reverse_complement()
    return f, r, ph.Model.from_buffer_copy(bytes(f)), ph.Model.from_buffer_copy(bytes(r))


@functools.lru_cache(maxsize=None)
def wide_haplotag_oracle():
    _, _, of, orv = pair_hmm_models()
    return hao.haplotag([wide_chunk()], [wide_genotypes()], OPTS, of, orv)[0]


def wide_owner_facts() -> dict:
    """the sites past the grid cap: their entries and the distinct substrings among them (the owners)"""
    w = wide_haplotag_oracle()
    sites = w["sites"][GRID_CAP:]
    return dict(entries=sum(len(s[2]) for s in sites), owners=sum(len({bytes(x) for _, x in s[2]}) for s in sites),
                sites_per_read=np.asarray(w["extracted"]["read_n_substrings"]).tolist())


# ---- B2. equal substring classes ----

TAIL_SITES = 40


@functools.lru_cache(maxsize=None)
def class_sites():
    """65 536 sites with no or one entry, then 40 built as the `sites` fixture of tests/test_gpu_substring_classes.py builds its
    own: 1, 2, 63, 64, 65 and 130 entries (a few distinct strings many times over), all equal, none equal, two strings with one key"""
    from tests.test_gpu_substring_classes import same_key_pair
    rng = np.random.default_rng(23)
    sym = lambda n: rng.integers(0, 5, size=n).astype(np.uint8)
    out = [[sym(int(rng.integers(0, 12)))] if rng.random() < 0.5 else [] for _ in range(GRID_CAP)]
    p, q = same_key_pair()
    tail = []
    for rep in range(5):
        for n in (1, 2, 63, 64, 65, 130):
            base = [sym(int(rng.integers(1, 40))) for _ in range(max(1, n // 6))]
            tail.append([base[int(rng.integers(0, len(base)))].copy() if rng.random() < 0.8 else sym(int(rng.integers(0, 40))) for _ in range(n)])
    for n in (70, 64, 129):
        one = sym(25)
        tail.append([one.copy() for _ in range(n)])                                                    # all equal
    for n in (70, 65, 125):
        tail.append([np.concatenate([sym(12), np.array([k % 5, k // 5 % 5, k // 25], np.uint8)]) for k in range(n)])  # none equal
    for n in (0, 20, 62, 63):                                                                          # one key, different bytes
        tail.append([sym(8) for _ in range(n)] + [p, q, p.copy(), sym(8), q.copy()])
    assert len(tail) == TAIL_SITES
    return out + tail


# ---- C. k-mer anchors ----

def walk(x, y):
    """getKmerAlignmentAnchors' chain (pairwiseAligner.c:1580-1600) restated -> per record dict(x, y, score, back, high, passed
    (the records its walk back looked at), stopped (the walk ended at a chainable running maximum), stop_dist / best_dist (how far
    back the stop / the record it points to lay; 1 = the record before it, 0 = none))"""
    x, y = np.ascontiguousarray(x, np.uint8), np.ascontiguousarray(y, np.uint8)
    first = {}
    for i in range(len(x) - K + 1):
        first.setdefault(x[i:i + K].tobytes(), i)
    recs, top = [], 0
    for j in range(len(y) - K + 1 if len(x) >= K else 0):
        xi = first.get(y[j:j + K].tobytes())
        if xi is None:
            continue
        score, back, passed, stopped = 1, -1, 0, False
        for q in range(len(recs) - 1, -1, -1):
            passed += 1
            if recs[q]["x"] < xi:
                if recs[q]["score"] + 1 > score:
                    score, back = recs[q]["score"] + 1, q
                if recs[q]["high"]:
                    stopped = True
                    break
        recs.append(dict(x=xi, y=j, score=score, back=back, high=score >= top, passed=passed, stopped=stopped,
                         stop_dist=passed if stopped else 0, best_dist=len(recs) - back if back >= 0 else 0))
        top = max(top, score)
    return recs


def walk_anchors(recs) -> np.ndarray:
    """the chain of the last running maximum, ascending, as k-mer centres (:1605-1617)"""
    q = max((i for i, r in enumerate(recs) if r["high"]), default=-1)
    out = []
    while q != -1:
        out.append((recs[q]["x"] + K // 2, recs[q]["y"] + K // 2))
        q = recs[q]["back"]
    return np.array(out[::-1], np.int64).reshape(-1, 2)


X_SEP, Y_SEP = np.array([5], np.uint8), np.array([6], np.uint8)


def _arrange(rng, x_names, y_names):
    """x: the named blocks of K random symbols in this order, each followed by the byte 5; y: the named blocks in that order, each
    followed by the byte 6.  K-mers are compared byte by byte, whatever the symbol, so only a whole block is a shared k-mer: a
    window across a junction holds a 5 in x and a 6 in y.  A pair then has one record per block of y.  -> (x, y, x position by name)"""
    blk = {n: synth.random_sequence(rng, K) for n in x_names}
    pos = {n: (K + 1) * i for i, n in enumerate(x_names)}
    return (np.concatenate([p for n in x_names for p in (blk[n], X_SEP)]), np.concatenate([p for n in y_names for p in (blk[n], Y_SEP)]), pos)


def long_walk_pair(n_blocks: int = 300, seed: int = 51):
    """C1: y = block 0 of x, then blocks n - 1 .. 10 in descending order, then block 5: every record's walk runs back to record 0,
    a running maximum and so its stop"""
    rng = np.random.default_rng(seed)
    x, y, _ = _arrange(rng, list(range(n_blocks)), [0] + list(range(n_blocks - 1, 9, -1)) + [5])
    return x, y


def far_best_pair(seed: int = 52, n_low: int = 70):
    """C2: y = 40 ascending blocks (a chain of score 40 ending in a running maximum), then n_low blocks whose x lies before all
    of those and descends (score 1 each, no running maximum, chainable for what follows), then a block whose x lies behind all"""
    rng = np.random.default_rng(seed)
    low, mid = [f"L{i}" for i in range(n_low)], [f"M{i}" for i in range(40)]
    x, y, _ = _arrange(rng, low + mid + ["F"], mid + low[::-1] + ["F"])
    return x, y


def tie_pair(seed: int = 53, n_fill: int = 70):
    """C3: the record F has two chainable predecessors of score 2, Pn right before it and Pf beyond n_fill records that are not
    chainable for F; no running maximum is chainable for F, so its walk passes both and runs to the first record.  Blocks behind
    F put it on the chain that is reported.  -> (x, y, x position by name)"""
    rng = np.random.default_rng(seed)
    fill, high, tail = [f"X{i}" for i in range(n_fill)], [f"H{i}" for i in range(5)], [f"T{i}" for i in range(10)]
    x_names = ["a1", "Pn", "a0", "Pf", "F"] + tail + fill + high
    y_names = high + ["a0", "Pf"] + fill[::-1] + ["a1", "Pn", "F"] + tail
    return _arrange(rng, x_names, y_names)


def anchor_cases():
    x3, y3, _ = tie_pair()
    return [("long walk", *long_walk_pair()), ("far best", *far_best_pair()), ("tie", x3, y3)]


N_REAL = 64


@functools.lru_cache(maxsize=None)
def many_pairs():
    """C4: 65 536 + 64 pairs.  Pairs 0..63 and 65 536..65 599 are real and mutually different (C1-C3 among them, an evolved, an
    identical and an unrelated pair, and evolved pairs of 60-300 symbols); the rest are too short for a k-mer (0-19 symbols out of
    one small pool).  A wave that ran one of the first 64 runs one of the last 64 next.  -> (pool, x_off, x_len, y_off, y_len,
    indices of the real pairs, their (x, y))"""
    rng = np.random.default_rng(61)
    rs = lambda n: synth.random_sequence(rng, n)

    def real(special):
        out = list(special)
        a = rs(300)
        out += [(a, synth.evolve_sequence(rng, a)), (a, a.copy()), (rs(200), rs(200))]
        while len(out) < N_REAL:
            a = rs(int(rng.integers(60, 301)))
            out.append((a, synth.evolve_sequence(rng, a, 0.01, 0.005, 0.005)))
        return out
    t1, t2 = tie_pair(), tie_pair(seed=63, n_fill=66)
    head = real([long_walk_pair(), far_best_pair(), t1[:2]])
    tail = real([far_best_pair(seed=62, n_low=80), t2[:2], long_walk_pair(150, seed=64)])
    n = GRID_CAP + N_REAL
    small = rs(40)
    x_len, y_len = rng.integers(0, K, size=n).astype(np.int32), rng.integers(0, K, size=n).astype(np.int32)
    x_off, y_off = rng.integers(0, 21, size=n).astype(np.int64), rng.integers(0, 21, size=n).astype(np.int64)
    idx = list(range(N_REAL)) + list(range(GRID_CAP, n))
    parts, at = [small], len(small)
    for i, (x, y) in zip(idx, head + tail):
        x_off[i], x_len[i], y_off[i], y_len[i] = at, len(x), at + len(x), len(y)
        parts += [x, y]
        at += len(x) + len(y)
    return np.concatenate(parts).astype(np.uint8), x_off, x_len, y_off, y_len, idx, head + tail


# ---- D. pair-per-wave kernel ----

N_MODELS = 200
N_LONG = 12


def many_models():
    """200 models, made as test_many_models of tests/test_gpu_pairhmm.py makes them: their emission tables leave the
    pair-per-lane kernel no room, so every pair takes the pair-per-wave kernel"""
    t, tr, em = synth.margin_phase_pair_hmm_arrays()
    f = capi.PairHmm.from_margin_hmm(t, tr, em)
    base = [f, f.reverse_complement(), capi.PairHmm.default_nucleotide()]
    out = []
    for i in range(N_MODELS):
        m = base[i % 3].copy()
        m.gap_open_x -= 0.01 * i
        m.e_match[5] -= 0.003 * i
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def wave_pairs():
    """16 384 + 200 random pairs of 0-30 symbols and, spread over the list, twelve evolved pairs of 101-300 symbols (a second
    launch class) -> (pool, x_off, x_len, y_off, y_len, model index)"""
    rng = np.random.default_rng(31)
    n = PHM_GRID_CAP + 200 + N_LONG
    x_len, y_len = rng.integers(0, 31, size=n).astype(np.int32), rng.integers(0, 31, size=n).astype(np.int32)
    x_off = np.zeros(n, np.int64)
    x_off[1:] = np.cumsum(x_len[:-1] + y_len[:-1])
    y_off = x_off + x_len
    at = int(x_off[-1] + x_len[-1] + y_len[-1])
    parts = [synth.random_sequence(rng, at, n_rate=0.03)]
    for i in np.linspace(5, n - 7, N_LONG).astype(int):
        a = synth.random_sequence(rng, int(rng.integers(101, 301)), n_rate=0.03)
        b = synth.evolve_sequence(rng, a)[:300]
        b = np.concatenate([b, synth.random_sequence(rng, max(0, 101 - len(b)))])
        x_off[i], x_len[i], y_off[i], y_len[i] = at, len(a), at + len(a), len(b)
        parts += [a, b]
        at += len(a) + len(b)
    return np.concatenate(parts).astype(np.uint8), x_off, x_len, y_off, y_len, rng.integers(0, N_MODELS, size=n).astype(np.uint8)


def wave_facts() -> dict:
    """an unanchored pair's widest diagonal has min(lx, ly) + 1 cells; the launch classes hold up to 64, 256, 1 024, 2 048"""
    _, _, x_len, _, y_len, _ = wave_pairs()
    width = np.minimum(x_len, y_len) + 1
    return dict(pairs=len(width), first_class=int((width <= 64).sum()), second_class=int(((width > 64) & (width <= 256)).sum()),
                wider=int((width > 256).sum()), long_pairs=int((np.maximum(x_len, y_len) > 100).sum()))
