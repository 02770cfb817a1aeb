/*
 * mrp_string_chunks.hip -- the string-chunk calls built on the pair-HMM (mrp_pairhmm.h): mrp_phase_string_chunks, the front of the chunk
 * loop in one device-resident call (profile bytes and HP tags by kernels over the chunks' device pool), and the same with the filtered
 * back half (mrp_phase_string_chunks_with_filtered: the filtered-read / filtered-variant loops, bubbleGraph.c:1749-2351, over records a
 * kernel makes from what the phasing decided); the front / run steps a work queue drives (mrp_internal.h).  gfx950 only; compiled
 * with -ffp-contract=off.
 */
#include <cmath>
#include <string>

#include "mrp_pairhmm.h"

#pragma clang fp contract(off)

namespace {

/* ---- mrp_phase_string_chunks: profile bytes and HP tags on the device ------------------------------------------------------
 *
 * Exactness of the profile bytes.  The byte of bubbleGraph.c:2429-2435 (rphmm_frame.c mrp_profile_seqs_from_bubbles) is
 * min(255, (int64) roundf((float) (30 (total - lp)))) with lp the float support and total = logAddExact over the alleles in
 * allele order.  Everything but total is exact IEEE arithmetic on both sides (the narrowing to float, the fp64 subtraction and
 * product -- not contracted in this file --, the conversion to float, roundf, and the x86 conversion restated below).  total
 * takes one exp and one log per allele after the first: the device's (ocml) and glibc's double exp / log are both faithfully
 * rounded, so total can differ from the host's in its last bit, 2^-52 relative: about 1e-14 absolute for the values here (|total|
 * below 10^3).  That moves 30 (total - lp) by less than 1e-12, and the byte changes only if the fp64 value lies that close to a
 * point where its float rounding crosses a half integer; float spacing below 256 is at least 2^-16, so the chance is below
 * 1e-7 per byte, and the supports are the same floats on both sides.  The tests compare every byte of the chain's pool. */
static __device__ __forceinline__ int64_t sc_f32_to_i64_x86(float v) { /* (int64_t) of a float as x86-64 converts it (cvttss2si) */
    if (!(v >= -9223372036854775808.0f && v < 9223372036854775808.0f)) return INT64_MIN;
    return (int64_t) v;
}

struct ScByteItem { /* one (bubble, read substring): where its bytes go in the device pool, the first pair of its owner */
    int64_t dst;
    int32_t pair;      /* the owner's pair with allele 0 of the bubble; alleles follow */
    int32_t n_alleles;
};

/* bubbleGraph.c:2421-2435 over the supports of bubbleGraph.c:1421-1464: a lane per (bubble, substring) */
__global__ void __launch_bounds__(256) sc_profile_bytes_kernel(const ScByteItem *__restrict__ items, int64_t n_items, const double *__restrict__ lp,
                                                               uint8_t *__restrict__ pool) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const ScByteItem it = items[i];
    const double *p = lp + it.pair;
    double total = -__builtin_inf();
    for (int32_t k = 0; k < it.n_alleles; k++) total = ht_log_add_exact(total, (double) (float) p[k]); /* the float store of :1464 */
    uint8_t *dst = pool + it.dst;
    for (int32_t k = 0; k < it.n_alleles; k++) {
        const float f = (float) p[k];
        const int64_t l = sc_f32_to_i64_x86(roundf((float) (30.0 * (total - (double) f))));
        dst[k] = (uint8_t) (l > 255 ? 255 : l);
    }
}

struct ScHapItem { /* one profile sequence of one chunk */
    int64_t pool;   /* its bytes in the device pool */
    int64_t aoff;   /* its chunk's allele offsets (n_sites + 1) in the offsets table */
    int64_t hap;    /* its chunk's haplotype strings: hap1 then hap2, frag_length each */
    int32_t ref_start, length, frag_start, frag_length;
    int32_t side;   /* 1 / 2: in reads1 / only in reads2 of the fragment, 0: in neither */
    int32_t pad;
};

/* stGenomeFragment_phaseBamChunkReads (genomeFragment.c:234-276) with getLogProbOfReadGivenHaplotype (:71-89) and
 * getLogProbabilityOfBeingInPartition (:91-100), as mrp_assign_reads_to_haplotypes states them: a lane per sequence.  The
 * sums of bytes are integers, exact in fp64 in any order; one exp and one log follow (relative error ~1e-16). */
__global__ void __launch_bounds__(256) sc_assign_kernel(const ScHapItem *__restrict__ items, int64_t n_items, const int64_t *__restrict__ aoff,
                                                        const uint64_t *__restrict__ haps, const uint8_t *__restrict__ pool, int64_t min_phred,
                                                        int8_t *__restrict__ hap_out, double *__restrict__ phred_out) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const ScHapItem it = items[i];
    if (it.side == 0) { hap_out[i] = -1; phred_out[i] = 0.0; return; }
    /* :255-259: the first haplotype handed over for a hap1 read is haplotypeString2, i.e. the OTHER one */
    const uint64_t *mine = haps + it.hap + (it.side == 1 ? 0 : it.frag_length), *other = haps + it.hap + (it.side == 1 ? it.frag_length : 0);
    const int64_t *ao = aoff + it.aoff + it.ref_start;
    const uint8_t *bytes = pool + it.pool;
    int32_t lo = it.frag_start - it.ref_start, hi = it.frag_start + it.frag_length - it.ref_start;
    if (lo < 0) lo = 0;
    if (hi > it.length) hi = it.length;
    double ta = 0.0, tb = 0.0;
    for (int32_t s = lo; s < hi; s++) {
        const int64_t o = ao[s] - ao[0], A = ao[s + 1] - ao[s];
        const int64_t j = (int64_t) s + it.ref_start - it.frag_start;
        const uint64_t ho = other[j], hm = mine[j];
        if (ho < (uint64_t) A) ta -= bytes[o + (int64_t) ho]; /* (a haplotype allele is always one of the site's) */
        if (hm < (uint64_t) A) tb -= bytes[o + (int64_t) hm];
    }
    const double a = ta / 30.0, b = tb / 30.0;
    const double lp = a - ht_log_add_exact(a, b);
    const double phred = -10 * lp / 2.302585; /* :260 */
    hap_out[i] = phred < (double) min_phred ? 0 : (int8_t) it.side;
    phred_out[i] = phred;
}

/* what the host works out for one chunk beside the pair-HMM kernels: bubbleGraph_getProfileSeqs' layout (bubbleGraph.c:2356-2381)
 * and bubbleGraph_getReference's tables (:2443-2474), as rphmm_frame.c computes them */
struct ScLayout {
    std::vector<mrp_read> seqs;
    std::vector<int32_t> read_of_seq, seq_of;
    std::vector<int64_t> aoff; /* n_bubbles + 1 */
    int64_t pool_bytes = 0;
    std::vector<uint32_t> an;
    std::vector<uint16_t> sub, prior;
};

/* (uint16_t) of a float as gcc/x86-64 converts it (rphmm_frame.c) */
uint16_t sc_f32_to_u16_x86(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return 0;
    return (uint16_t) (uint32_t) (int32_t) v;
}

/* MRP_ERR_ARG for a malformed chunk; seen: scratch of n_reads entries */
int sc_check_chunk(const char *who, int64_t c, const mrp_string_chunk &S, std::vector<int64_t> &seen) {
    if (S.n_bubbles < 0 || S.n_reads < 0 || S.pool_bytes < 0 || S.n_reads >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes", who, (long long) c);
    if (S.n_reads > 0 && (!S.read_names || !S.read_forward_strand)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    for (int64_t r = 0; r < S.n_reads; r++)
        if (!S.read_names[r]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %lld has no name", who, (long long) c, (long long) r);
    if (S.n_bubbles == 0) return MRP_OK;
    if (!S.allele_first || !S.sub_first || (S.pool_bytes > 0 && !S.pool)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    if (S.allele_first[0] != 0 || S.sub_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets must start at 0", who, (long long) c);
    for (int64_t b = 0; b < S.n_bubbles; b++) {
        const int64_t na = S.allele_first[b + 1] - S.allele_first[b], ns = S.sub_first[b + 1] - S.sub_first[b];
        if (na < 1 || na > 65535 || ns < 0)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets not ascending or no allele at bubble %lld", who, (long long) c, (long long) b);
    }
    const int64_t n_alleles = S.allele_first[S.n_bubbles], n_subs = S.sub_first[S.n_bubbles];
    if (!S.allele_off || !S.allele_len || (n_subs > 0 && (!S.sub_off || !S.sub_len || !S.sub_read)))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    for (int64_t j = 0; j < n_alleles; j++)
        if (S.allele_len[j] < 0 || S.allele_off[j] < 0 || S.allele_off[j] + S.allele_len[j] > S.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: allele %lld lies outside the pool", who, (long long) c, (long long) j);
    seen.assign((size_t) S.n_reads, -1);
    for (int64_t b = 0; b < S.n_bubbles; b++)
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            if (S.sub_len[k] < 0 || S.sub_off[k] < 0 || S.sub_off[k] + S.sub_len[k] > S.pool_bytes)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read substring %lld lies outside the pool", who, (long long) c, (long long) k);
            const int32_t r = S.sub_read[k];
            if (r < 0 || r >= S.n_reads)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: substring %lld names read %d of %lld", who, (long long) c, (long long) k, r, (long long) S.n_reads);
            if (seen[(size_t) r] == b) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %d appears twice in bubble %lld", who, (long long) c, r, (long long) b);
            seen[(size_t) r] = b;
        }
    return MRP_OK;
}

void sc_layout(const mrp_string_chunk &S, double het_substitution_probability, ScLayout &Lc) {
    const int64_t nb = S.n_bubbles, n_reads = S.n_reads;
    std::vector<int64_t> first((size_t) n_reads, -1), last((size_t) n_reads, -1);
    Lc.seq_of.assign((size_t) n_reads, -1);
    Lc.read_of_seq.clear();
    for (int64_t b = 0; b < nb; b++)
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            const int32_t r = S.sub_read[k];
            if (first[(size_t) r] < 0) { first[(size_t) r] = b; Lc.seq_of[(size_t) r] = (int32_t) Lc.read_of_seq.size(); Lc.read_of_seq.push_back(r); }
            last[(size_t) r] = b;
        }
    Lc.aoff.assign((size_t) nb + 1, 0);
    Lc.an.resize((size_t) nb);
    int64_t n_sub = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int64_t A = S.allele_first[b + 1] - S.allele_first[b];
        Lc.an[(size_t) b] = (uint32_t) A;
        Lc.aoff[(size_t) b + 1] = Lc.aoff[(size_t) b] + A;
        n_sub += A * A;
    }
    const int64_t n_seqs = (int64_t) Lc.read_of_seq.size();
    Lc.seqs.assign((size_t) n_seqs, mrp_read{});
    int64_t pool_bytes = 0;
    for (int64_t q = 0; q < n_seqs; q++) { /* stProfileSeq_constructEmptyProfile profileSeq.c:13-29 */
        const int32_t r = Lc.read_of_seq[(size_t) q];
        mrp_read &m = Lc.seqs[(size_t) q];
        m.name = S.read_names[r];
        m.ref_start = (int32_t) first[(size_t) r];
        m.length = (int32_t) (last[(size_t) r] - first[(size_t) r] + 1);
        m.forward_strand = S.read_forward_strand[r] ? 1 : 0;
        m.pool_offset = pool_bytes;
        pool_bytes += Lc.aoff[(size_t) last[(size_t) r] + 1] - Lc.aoff[(size_t) first[(size_t) r]];
    }
    Lc.pool_bytes = pool_bytes;
    /* bubbleGraph.c:2458-2467 */
    const uint16_t off = sc_f32_to_u16_x86(roundf((float) (-log(het_substitution_probability) * 30.0)));
    Lc.sub.assign((size_t) n_sub, 0);
    Lc.prior.assign((size_t) Lc.aoff[(size_t) nb], 0);
    int64_t o = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int64_t A = Lc.an[(size_t) b];
        for (int64_t j = 0; j < A; j++)
            for (int64_t k = 0; k < A; k++) Lc.sub[(size_t) (o + j * A + k)] = j == k ? 0 : off;
        o += A * A;
    }
}

struct FsChunk { /* what the phasing decided for a chunk: where its haplotype strings are (hap1 then hap2, frag_length each) */
    int64_t hap;
    int32_t frag_start, frag_length;
};
constexpr int FS_TILE = 256; /* classes per pass of the LDS owner table */

/* the tag of a read where the HP kernel wrote it: read_seq = its profile sequence, -1 a primary read in no bubble, -2 a filtered read */
static __device__ __forceinline__ int fs_tag(const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags, int32_t read) {
    const int32_t q = read_seq[read];
    return q >= 0 ? (int) tags[q] : -1;
}

/* A wave per site, behind sc_assign_kernel.  Decides the site's activity and its two alleles (bubbles: the fragment's hap1 / hap2
 * allele, bubbleGraph.c:1780; variants: gt1 / gt2), each entry's participation (bubbles: filtered reads and untagged primary
 * reads; variants: tagged primary reads, :2226-2235), per class the owning entry (bubbles: the last-listed participant, :1816-1819;
 * variants: the first, :2221) and from the owner's strand the two pairs.  One record per entry, live or not. */
__global__ void __launch_bounds__(64) sc_filtered_sites_kernel(const FsSite *__restrict__ sites, const FsEntry *__restrict__ ent,
                                                               const int32_t *__restrict__ cbase, const int32_t *__restrict__ pidx,
                                                               const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags,
                                                               const FsChunk *__restrict__ chunks, const uint64_t *__restrict__ haps,
                                                               HtEntry *__restrict__ rec, uint8_t *__restrict__ used) {
    __shared__ int32_t tab[FS_TILE];
    const FsSite st = sites[blockIdx.x];
    const int lane = (int) threadIdx.x;
    const bool variant = st.bubble < 0;
    bool active = st.visited != 0;
    int32_t a1 = 0, a2 = 1;
    if (!variant) {
        const FsChunk ch = chunks[st.chunk];
        const int32_t j = st.bubble - ch.frag_start;
        active = j >= 0 && j < ch.frag_length;
        if (active) {
            const uint64_t h1 = haps[ch.hap + j], h2 = haps[ch.hap + ch.frag_length + j];
            active = h1 != h2 && h1 < (uint64_t) st.n_alleles && h2 < (uint64_t) st.n_alleles;
            a1 = (int32_t) h1;
            a2 = (int32_t) h2;
        }
    }
    const FsEntry *e = ent + st.entry_first;
    HtEntry *out = rec + st.entry_first;
    for (int32_t i = lane; i < st.n_entries; i += 64) out[i] = HtEntry{0, 0, 0, 0};
    if (!active) return; /* (the same for every lane of the block) */
    for (int32_t t0 = 0; t0 < st.n_classes; t0 += FS_TILE) {
        for (int i = lane; i < FS_TILE; i += 64) tab[i] = variant ? INT32_MAX : -1;
        __syncthreads();
        for (int32_t i = lane; i < st.n_entries; i += 64) {
            const FsEntry x = e[i];
            const int tag = fs_tag(read_seq, tags, x.read);
            const bool tagged = !(x.flags & 2) && (tag == 1 || tag == 2);
            const bool takes_part = variant ? tagged : !tagged;
            if (!takes_part || x.cls < t0 || x.cls >= t0 + FS_TILE) continue;
            const int32_t v = x.key * 2 + (x.flags & 1);
            if (variant) atomicMin(&tab[x.cls - t0], v);
            else atomicMax(&tab[x.cls - t0], v);
        }
        __syncthreads();
        for (int32_t i = lane; i < st.n_entries; i += 64) {
            const FsEntry x = e[i];
            const int tag = fs_tag(read_seq, tags, x.read);
            const bool tagged = !(x.flags & 2) && (tag == 1 || tag == 2);
            const bool takes_part = variant ? tagged : !tagged;
            if (!takes_part || x.cls < t0 || x.cls >= t0 + FS_TILE) continue;
            const int32_t owner = tab[x.cls - t0];
            const int32_t block = cbase[2 * (st.cls_first + x.cls) + (owner & 1)];
            const int32_t pa = pidx[block + a1], pb = pidx[block + a2];
            out[i] = HtEntry{pa, pb, tag == 1 ? 1 : 0, 1};
            if (used) { used[pa] = 1; used[pb] = 1; }
        }
        __syncthreads();
    }
}

/* ht_partition_kernel over a read's static candidate list (its entries at bubbles, in bubble order): records that are not live
 * are skipped.  A primary read the phasing tagged keeps its tag. */
__global__ void __launch_bounds__(256) fs_partition_kernel(const int64_t *__restrict__ first, const int32_t *__restrict__ cand,
                                                           const HtEntry *__restrict__ e, const double *__restrict__ lp,
                                                           const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags, int64_t n_reads,
                                                           int32_t *__restrict__ hap, double *__restrict__ h1, double *__restrict__ h2) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int tag = fs_tag(read_seq, tags, (int32_t) r);
    if (read_seq[r] != -2 && (tag == 1 || tag == 2)) { hap[r] = tag; h1[r] = 0.0; h2[r] = 0.0; return; }
    double t1 = 0.0, t2 = 0.0;
    for (int64_t i = first[r]; i < first[r + 1]; i++) {
        const HtEntry x = e[cand[i]];
        if (x.live) ht_partition_term(lp, x, t1, t2);
    }
    hap[r] = ht_hap(t1, t2);
    h1[r] = t1;
    h2[r] = t2;
}

/* ht_phase_kernel over a variant's entries in order, the records that are not live skipped */
__global__ void __launch_bounds__(256) fs_phase_kernel(const FsSite *__restrict__ sites, const HtEntry *__restrict__ e, const double *__restrict__ lp,
                                                       int64_t n_variants, int32_t *__restrict__ state, double *__restrict__ cis,
                                                       double *__restrict__ trans) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_variants) return;
    const FsSite st = sites[v];
    double c = 0.0, t = 0.0;
    for (int64_t i = st.entry_first; i < st.entry_first + st.n_entries; i++) {
        const HtEntry x = e[i];
        if (x.live) ht_phase_term(lp, x, c, t);
    }
    state[v] = ht_state(st.visited != 0, c, t);
    cis[v] = c;
    trans[v] = t;
}

/* The phased variant records (updateOriginalVcfEntriesWithBubbleData, vcf.c:511-592; the update that ends
 * bubbleGraph_phaseVcfEntriesFromHaplotaggedReads, bubbleGraph.c:2298-2343), behind fs_phase_kernel.  A wave per site; lanes run over
 * the site's entries where the extraction left them, 64 a pass.  A primary site is updated when its bubble lies inside the fragment
 * (its gt: the fragment's hap1 / hap2 allele there); a filtered site follows its state.  An entry is listed when its read is a primary
 * read of the chunk (kept, let through by the mask; at a filtered site kept by the rest's extraction too) that the HP kernel tagged 1 or
 * 2.  The two lists are stable compactions (ballot + prefix popcount, a running base across the passes): a count pass, then hap1 fills
 * the site's slots from the front and hap2 ends at their end.  n_slots counts the site's entries of primary reads, so n1 + n2 <=
 * n_slots; a store outside the site's slots is skipped all the same.  Plain vector stores only; every loop is bounded by the site's
 * entry count and uniform across the wave. */
static __device__ __forceinline__ int rc_entry_tag(const RcSite &st, bool variant, int32_t g, const uint8_t *__restrict__ status,
                                                   const uint8_t *__restrict__ take, const int32_t *__restrict__ read_seq,
                                                   const int8_t *__restrict__ tags, int32_t &read) {
    if (variant && status[g] != MRP_READ_KEPT) return 0; /* (entries of reads the rest's extraction did not keep are not listed) */
    const int32_t p = g - st.read_shift;
    read = p - st.read_base;
    if (status[p] != MRP_READ_KEPT || (take && !take[p])) return 0;
    const int tag = fs_tag(read_seq, tags, p);
    return tag == 1 || tag == 2 ? tag : 0;
}

__global__ void __launch_bounds__(64) rc_records_kernel(const RcSite *__restrict__ sites, const int64_t *__restrict__ entry_first,
                                                        const int32_t *__restrict__ entry_read, const uint8_t *__restrict__ status,
                                                        const uint8_t *__restrict__ take, const int32_t *__restrict__ read_seq,
                                                        const int8_t *__restrict__ tags, const FsChunk *__restrict__ chunks,
                                                        const uint64_t *__restrict__ haps, const int32_t *__restrict__ var_state,
                                                        RcOut *__restrict__ out, int32_t *__restrict__ slots) {
    const RcSite st = sites[blockIdx.x];
    const int lane = (int) threadIdx.x;
    const bool variant = st.state >= 0;
    int32_t state = MRP_RECORD_UNTOUCHED, g1 = -2, g2 = -2;
    if (!variant) {
        if (st.bubble >= 0) {
            const FsChunk ch = chunks[st.chunk];
            const int32_t j = st.bubble - ch.frag_start;
            if (j >= 0 && j < ch.frag_length) { /* vcf.c:520, :558-563 */
                state = MRP_RECORD_UPDATED;
                g1 = (int32_t) haps[ch.hap + j];
                g2 = (int32_t) haps[ch.hap + ch.frag_length + j];
            }
        }
    } else {
        const int32_t vs = var_state[st.state];
        if (vs == MRP_VARIANT_TIE) { state = MRP_RECORD_CLEARED; g1 = -1; g2 = -1; }      /* bubbleGraph.c:2298-2321 */
        else if (vs == MRP_VARIANT_CIS) { state = MRP_RECORD_UPDATED; g1 = st.gt1; g2 = st.gt2; }   /* :2303-2305 */
        else if (vs == MRP_VARIANT_TRANS) { state = MRP_RECORD_UPDATED; g1 = st.gt2; g2 = st.gt1; } /* :2306-2309 */
    }
    int32_t n1 = 0, n2 = 0;
    if (state == MRP_RECORD_UPDATED && st.n_slots > 0) { /* (the same for every lane of the wave) */
        const int64_t a = entry_first[st.var], b = entry_first[st.var + 1];
        for (int64_t p0 = a; p0 < b; p0 += 64) {
            const int64_t p = p0 + lane;
            int32_t read = 0;
            const int tag = p < b ? rc_entry_tag(st, variant, entry_read[p], status, take, read_seq, tags, read) : 0;
            n1 += (int32_t) __popcll(__ballot(tag == 1));
            n2 += (int32_t) __popcll(__ballot(tag == 2));
        }
        const uint64_t below = (1ull << lane) - 1;
        int32_t b1 = 0, b2 = st.n_slots - n2;
        int32_t *dst = slots + st.slot_first;
        for (int64_t p0 = a; p0 < b; p0 += 64) {
            const int64_t p = p0 + lane;
            int32_t read = 0;
            const int tag = p < b ? rc_entry_tag(st, variant, entry_read[p], status, take, read_seq, tags, read) : 0;
            const uint64_t m1 = __ballot(tag == 1), m2 = __ballot(tag == 2);
            const int32_t at = tag == 1 ? b1 + (int32_t) __popcll(m1 & below) : b2 + (int32_t) __popcll(m2 & below);
            if (tag != 0 && at >= 0 && at < st.n_slots) dst[at] = read;
            b1 += (int32_t) __popcll(m1);
            b2 += (int32_t) __popcll(m2);
        }
    }
    if (lane == 0) out[blockIdx.x] = RcOut{state, g1, g2, n1, n2};
}

bool sc_rest_empty(const mrp_string_chunk_rest &R) { return R.n_filtered == 0 && R.n_variants == 0; }

/* MRP_ERR_ARG for a malformed rest of chunk c (the chunk itself has passed sc_check_chunk) */
int sc_check_rest(const char *who, int64_t c, const mrp_string_chunk &S, const mrp_string_chunk_rest &R) {
    const long long cc = (long long) c;
    if (R.n_filtered < 0 || R.n_variants < 0 || R.pool_bytes < 0 || S.n_reads + R.n_filtered >= (1ll << 30))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes of the rest", who, cc);
    if ((R.n_filtered > 0 && !R.forward_strand) || (R.pool_bytes > 0 && !R.pool)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    if (R.n_filtered > 0 && S.n_bubbles > 0 && !R.fsub_first) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest (fsub_first)", who, cc);
    if (R.fsub_first && S.n_bubbles > 0) {
        if (R.fsub_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets of the rest must start at 0", who, cc);
        for (int64_t b = 0; b < S.n_bubbles; b++)
            if (R.fsub_first[b + 1] < R.fsub_first[b])
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring offsets not ascending at bubble %lld", who, cc, (long long) b);
        const int64_t n = R.fsub_first[S.n_bubbles];
        if (n > 0 && (!R.fsub_off || !R.fsub_len || !R.fsub_read)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = R.fsub_first[b]; k < R.fsub_first[b + 1]; k++) {
                if (R.fsub_len[k] < 0 || R.fsub_off[k] < 0 || R.fsub_off[k] + R.fsub_len[k] > R.pool_bytes)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring %lld lies outside the pool", who, cc, (long long) k);
                const int32_t r = R.fsub_read[k];
                if (r < 0 || r >= R.n_filtered)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring %lld names read %d of %lld", who, cc, (long long) k, r, (long long) R.n_filtered);
                if (k > R.fsub_first[b] && R.fsub_read[k - 1] == r)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered read %d appears twice in bubble %lld", who, cc, r, (long long) b);
                if (k > R.fsub_first[b] && R.fsub_read[k - 1] > r)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered reads of bubble %lld are not in ascending order", who, cc, (long long) b);
            }
    }
    if (R.n_variants == 0) return MRP_OK;
    if (!R.valle_first || !R.ventry_first || !R.gt) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    if (R.valle_first[0] != 0 || R.ventry_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets of the rest must start at 0", who, cc);
    for (int64_t v = 0; v < R.n_variants; v++) {
        const int64_t na = R.valle_first[v + 1] - R.valle_first[v], ne = R.ventry_first[v + 1] - R.ventry_first[v];
        if (na < 0 || ne < 0 || ne >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets not ascending at variant %lld", who, cc, (long long) v);
        if (R.gt[2 * v] < 0 || R.gt[2 * v] >= na || R.gt[2 * v + 1] < 0 || R.gt[2 * v + 1] >= na)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant %lld has a genotype allele it does not have", who, cc, (long long) v);
    }
    const int64_t n_alleles = R.valle_first[R.n_variants], n_entries = R.ventry_first[R.n_variants];
    if ((n_alleles > 0 && (!R.valle_off || !R.valle_len)) || (n_entries > 0 && (!R.ventry_read || !R.ventry_off || !R.ventry_len)))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    for (int64_t j = 0; j < n_alleles; j++)
        if (R.valle_len[j] < 0 || R.valle_off[j] < 0 || R.valle_off[j] + R.valle_len[j] > R.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant allele %lld lies outside the pool", who, cc, (long long) j);
    for (int64_t k = 0; k < n_entries; k++) {
        if (R.ventry_len[k] < 0 || R.ventry_off[k] < 0 || R.ventry_off[k] + R.ventry_len[k] > R.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant entry %lld lies outside the pool", who, cc, (long long) k);
        if (R.ventry_read[k] < 0 || R.ventry_read[k] >= S.n_reads + R.n_filtered)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant entry %lld names read %d of %lld", who, cc, (long long) k, R.ventry_read[k],
                                 (long long) (S.n_reads + R.n_filtered));
    }
    return MRP_OK;
}

}  // namespace

/* ---- mrp_phase_string_chunks in three steps (mrp_internal.h): its own body below, and what a lane of the work queue runs per
 * batch (mrp_queue.cpp) -- the checks of every chunk first, the front of batch n + 1 beside the device work of batch n. */

int mrp_string_chunks_check(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                            int64_t expansion, const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                            const mrp_string_chunk_rest *rest, const char *who) {
    if (n_chunks < 0 || (n_chunks > 0 && (!chunks || !out || !hap_out)) || !forward_model || !reverse_model || !params)
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    for (int64_t c = 0; c < n_chunks; c++)
        if (chunks[c].n_reads > 0 && (!hap_out[c] || (phred_out && !phred_out[c]))) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output", who, (long long) c);
    {
        std::vector<int> rcs((size_t) n_chunks, MRP_OK);
        std::vector<std::string> msgs((size_t) n_chunks);
        mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
            std::vector<int64_t> seen;
            rcs[(size_t) c] = sc_check_chunk(who, c, chunks[c], seen);
            if (rcs[(size_t) c] == MRP_OK && rest) rcs[(size_t) c] = sc_check_rest(who, c, chunks[c], rest[c]);
            if (rcs[(size_t) c] != MRP_OK) msgs[(size_t) c] = mrp_last_error();
        });
        for (int64_t c = 0; c < n_chunks; c++)
            if (rcs[(size_t) c] != MRP_OK) return mrp_set_error(rcs[(size_t) c], "%s", msgs[(size_t) c].c_str());
    }
    return MRP_OK;
}

/* MRP_ERR_UNSUPPORTED as phm_classify raises it, from the strings alone -- without the owners, the pair list or the sort (a
 * duplicate substring has its owner's strings, so looking at every substring changes nothing).  A diagonal of a pair holds at
 * most min(lx, ly) + 1 cells, band or not: only pairs with BOTH strings at the limit are looked at, their anchors (above
 * sv_threshold, bubbleGraph.c:1448-1451) and bands made as the front makes them.  wide_pairs (mrp_queue_set_wide_pairs): such a pair
 * is refused only beyond the caps of the pair-per-workgroup kernel. */
int mrp_string_chunks_check_pairs(int64_t n_chunks, const mrp_string_chunk *chunks, int64_t expansion, int64_t sv_threshold,
                                  const mrp_string_chunk_rest *rest, const char *who, int wide_pairs) {
    std::vector<int> rcs((size_t) n_chunks, MRP_OK);
    std::vector<std::string> msgs((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        std::vector<int64_t> anc;
        std::vector<int32_t> Lb, Rb;
        int &rcc = rcs[(size_t) c];
        /* one pair: x = allele, y = substring; what: "bubble" / "variant" and its index.  Leaves rcc set on a refusal. */
        auto pair = [&](const uint8_t *x, int64_t lx, const uint8_t *y, int64_t ly, bool anchored, const char *what, int64_t idx) {
            if (std::min(lx, ly) < PHM_WAVE_MAX_WIDTH) return;
            anc.clear();
            if (anchored) kmer_anchors(x, lx, y, ly, anc);
            int width = (int) std::min<int64_t>(std::min(lx, ly) + 1, INT32_MAX);
            int64_t cells = (lx + 1) * (ly + 1);
            if (!anc.empty()) {
                if (lx + ly >= (1ll << 30)) { rcc = mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who); return; }
                Lb.resize((size_t) (lx + ly + 1));
                Rb.resize((size_t) (lx + ly + 1));
                const int rc = band_closed_form(anc.data(), (int64_t) anc.size() / 2, lx, ly, expansion, Lb.data(), Rb.data(), &cells, &width);
                if (rc != MRP_OK) {
                    rcc = mrp_set_error(rc, "%s: chunk %lld: a pair of %s %lld has invalid anchors (pairwiseAligner.c:206-211)", who, (long long) c, what, (long long) idx);
                    return;
                }
            }
            if (width > PHM_WAVE_MAX_WIDTH && wide_pairs) {
                char which[96];
                snprintf(which, sizeof(which), "chunk %lld: a pair of %s %lld", (long long) c, what, (long long) idx);
                rcc = phm_wide_caps(who, which, width, cells);
            } else if (width > PHM_WAVE_MAX_WIDTH)
                rcc = mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: chunk %lld: a pair of %s %lld has a diagonal of %d cells (limit %d)", who, (long long) c, what,
                                    (long long) idx, width, PHM_WAVE_MAX_WIDTH);
        };
        for (int64_t b = 0; b < S.n_bubbles && rcc == MRP_OK; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1] && rcc == MRP_OK; k++)
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1] && rcc == MRP_OK; j++)
                    pair(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], S.sub_len[k] > sv_threshold || S.allele_len[j] > sv_threshold,
                         "bubble", b);
        if (rest && !sc_rest_empty(rest[c])) {
            /* the back half's pairs: every substring of a bubble, primary or filtered, against every allele without anchors (the
             * partition never anchors, bubbleGraph.c:1832); a variant's entries of primary reads against its two gt alleles */
            const mrp_string_chunk_rest &R = rest[c];
            for (int64_t b = 0; b < S.n_bubbles && rcc == MRP_OK; b++)
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1] && rcc == MRP_OK; j++) {
                    for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1] && rcc == MRP_OK; k++)
                        pair(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], false, "bubble", b);
                    for (int64_t k = R.fsub_first ? R.fsub_first[b] : 0; k < (R.fsub_first ? R.fsub_first[b + 1] : 0) && rcc == MRP_OK; k++)
                        pair(S.pool + S.allele_off[j], S.allele_len[j], R.pool + R.fsub_off[k], R.fsub_len[k], false, "bubble", b);
                }
            for (int64_t v = 0; v < R.n_variants && rcc == MRP_OK; v++) {
                if (R.gt[2 * v] == R.gt[2 * v + 1]) continue;
                for (int64_t k = R.ventry_first[v]; k < R.ventry_first[v + 1] && rcc == MRP_OK; k++) {
                    if (R.ventry_read[k] >= S.n_reads) continue;
                    for (int w = 0; w < 2 && rcc == MRP_OK; w++) {
                        const int64_t j = R.valle_first[v] + R.gt[2 * v + w];
                        pair(R.pool + R.valle_off[j], R.valle_len[j], R.pool + R.ventry_off[k], R.ventry_len[k],
                             R.ventry_len[k] > sv_threshold || R.valle_len[j] > sv_threshold, "variant", v);
                    }
                }
            }
        }
        if (rcc != MRP_OK) msgs[(size_t) c] = mrp_last_error();
    });
    for (int64_t c = 0; c < n_chunks; c++)
        if (rcs[(size_t) c] != MRP_OK) return mrp_set_error(rcs[(size_t) c], "%s", msgs[(size_t) c].c_str());
    return MRP_OK;
}

void mrp_string_front_destroy(mrp_string_front *F) { delete F; }

/* The static half of the back half, made with the front (host only): per chunk with a rest its sites (bubbles, then variants), their
 * entries grouped into classes of equal substrings (the sort of substring_owners), and one pair per (class, strand that occurs in
 * the class, allele) some outcome of the phasing could read -- for a bubble every allele, never anchored; for a variant its two gt
 * alleles, anchored past sv_threshold, and only classes and strands of primary reads (a filtered read is never tagged).  A pair
 * the front already scores (same substring, same strand's model, not anchored) is referred to, not added.  The new pairs go behind
 * the front's own in its pair list. */
struct FsLocal { /* one task's share; pidx: a pair of the front (>= 0) or ~(index among the task's new pairs) */
    std::vector<FsEntry> entries;
    std::vector<FsSite> bsites, vsites;
    std::vector<int32_t> cbase;
    std::vector<int64_t> pidx;
    PhmPairList pairs;
    std::vector<int64_t> anchored; /* classes by id: the new pairs past sv_threshold, whose anchors are found on the device */
};
/* a task: a run of bubbles or of variants of one chunk (a chunk of 2 000 sites is sixteen tasks, not one) */
struct FsTask { int64_t c; bool variants; int64_t lo, hi; };

static void sc_filtered_task(const mrp_string_front *F, const mrp_string_chunk_rest *rest, int64_t sv_threshold, const std::vector<int64_t> &rpool_base,
                             const FsTask &T, FsLocal &Lc) {
    const mrp_string_front::Scratch &X = F->scratch;
    const uint8_t *gpool = F->gpool.data();
    const int64_t c = T.c;
    const mrp_string_chunk &S = F->chunks[c];
    const mrp_string_chunk_rest &R = rest[c];
    const int64_t pb = F->pool_base[(size_t) c], rb = rpool_base[(size_t) c], sb = F->sub_base[(size_t) c];
    const bool by_id = X.classes_by_id; /* the symbols lie in HBM: equal substrings of a site carry equal ids */
    struct Item { int64_t off; int32_t len; int64_t prim_sub; bool may_own; int64_t id; };
    std::vector<Item> items;
    std::vector<int32_t> order;
    auto same = [&](int32_t a, int32_t d) {
        const Item &x = items[(size_t) a], &y = items[(size_t) d];
        return by_id ? x.id == y.id : x.len == y.len && memcmp(gpool + x.off, gpool + y.off, (size_t) x.len) == 0;
    };
    /* classes of the items that may own (entries [e0, e0 + items.size()) of Lc.entries); per class and strand block(cls, rev, rep):
     * adds the (class, strand)'s pairs and returns where its block starts in Lc.pidx */
    auto classes = [&](size_t e0, FsSite &st, auto block) {
        order.clear();
        for (size_t i = 0; i < items.size(); i++)
            if (items[i].may_own) order.push_back((int32_t) i);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t d) {
            const Item &x = items[(size_t) a], &y = items[(size_t) d];
            if (by_id) return x.id != y.id ? x.id < y.id : a < d; /* (another numbering of the classes: only the order of the pairs differs) */
            if (x.len != y.len) return x.len < y.len;
            const int cmp = memcmp(gpool + x.off, gpool + y.off, (size_t) x.len);
            return cmp != 0 ? cmp < 0 : a < d;
        });
        st.cls_first = (int64_t) Lc.cbase.size() / 2;
        int32_t n_cls = 0;
        for (size_t i = 0; i < order.size(); n_cls++) {
            size_t j = i + 1;
            while (j < order.size() && same(order[i], order[j])) j++;
            int64_t prim = -1;
            bool has[2] = {false, false};
            for (size_t q = i; q < j; q++) {
                FsEntry &e = Lc.entries[e0 + (size_t) order[q]];
                e.cls = n_cls;
                has[e.flags & 1] = true;
                if (prim < 0) prim = items[(size_t) order[q]].prim_sub;
            }
            for (int rev = 0; rev < 2; rev++) Lc.cbase.push_back(has[rev] ? (int32_t) block(rev, items[(size_t) order[i]], prim) : -1);
            i = j;
        }
        st.n_classes = n_cls;
    };
    auto new_pair = [&](int64_t xo, int32_t xl, int64_t yo, int32_t yl, int rev, bool anchored) {
        Lc.pidx.push_back(~Lc.pairs.size());
        if (anchored && by_id) Lc.anchored.push_back(Lc.pairs.size());
        Lc.pairs.add(xo, xl, yo, yl, rev, anchored && !by_id ? gpool : nullptr);
    };
    for (int64_t b = T.variants ? T.hi : T.lo; b < T.hi; b++) {
        FsSite st{};
        st.entry_first = (int64_t) Lc.entries.size();
        st.chunk = (int32_t) c;
        st.bubble = (int32_t) b;
        st.n_alleles = (int32_t) (S.allele_first[b + 1] - S.allele_first[b]);
        st.visited = 1;
        items.clear();
        /* listing order of the partition: the filtered reads in index order, then the primary reads in index order */
        for (int64_t k = R.fsub_first ? R.fsub_first[b] : 0; k < (R.fsub_first ? R.fsub_first[b + 1] : 0); k++) {
            const int32_t fr = R.fsub_read[k];
            Lc.entries.push_back(FsEntry{0, (int32_t) (S.n_reads + fr), fr, (R.forward_strand[fr] ? 0 : 1) | 2});
            items.push_back(Item{rb + R.fsub_off[k], R.fsub_len[k], -1, true, by_id ? X.fsub_cls[(size_t) c][(size_t) k] : -1});
        }
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            const int32_t r = S.sub_read[k];
            Lc.entries.push_back(FsEntry{0, r, (int32_t) (R.n_filtered + r), S.read_forward_strand[r] ? 0 : 1});
            items.push_back(Item{pb + S.sub_off[k], S.sub_len[k], sb + k, true, by_id ? X.sub_cls[(size_t) (sb + k)] : -1});
        }
        st.n_entries = (int32_t) items.size();
        classes((size_t) st.entry_first, st, [&](int rev, const Item &rep, int64_t prim) {
            const int64_t at = (int64_t) Lc.pidx.size();
            /* the front's own pairs of this substring: its owner's strand, anchored past sv_threshold (bubbleGraph.c:1448-1451) */
            int prim_rev = -1;
            if (prim >= 0) {
                const int64_t po = X.owner[(size_t) prim] - sb;
                prim_rev = S.read_forward_strand[S.sub_read[po]] ? 0 : 1;
            }
            for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1]; j++) {
                if (prim_rev == rev && !(rep.len > sv_threshold || S.allele_len[j] > sv_threshold))
                    Lc.pidx.push_back(F->pair_first[(size_t) prim] + (j - S.allele_first[b]));
                else
                    new_pair(pb + S.allele_off[j], S.allele_len[j], rep.off, rep.len, rev, false);
            }
            return at;
        });
        Lc.bsites.push_back(st);
    }
    for (int64_t v = T.variants ? T.lo : T.hi; v < T.hi; v++) {
        FsSite st{};
        st.entry_first = (int64_t) Lc.entries.size();
        st.chunk = (int32_t) c;
        st.bubble = -1;
        st.n_alleles = 2;
        st.n_entries = (int32_t) (R.ventry_first[v + 1] - R.ventry_first[v]);
        st.visited = R.gt[2 * v] != R.gt[2 * v + 1] && st.n_entries > 0;
        items.clear();
        for (int64_t k = R.ventry_first[v]; k < R.ventry_first[v + 1]; k++) {
            const int32_t r = R.ventry_read[k];
            const bool filtered = r >= S.n_reads;
            const bool fwd = filtered ? R.forward_strand[r - S.n_reads] != 0 : S.read_forward_strand[r] != 0;
            Lc.entries.push_back(FsEntry{0, r, (int32_t) (k - R.ventry_first[v]), (fwd ? 0 : 1) | (filtered ? 2 : 0)});
            items.push_back(Item{rb + R.ventry_off[k], R.ventry_len[k], -1, st.visited && !filtered, by_id ? X.ventry_cls[(size_t) c][(size_t) k] : -1});
        }
        classes((size_t) st.entry_first, st, [&](int rev, const Item &rep, int64_t) {
            const int64_t at = (int64_t) Lc.pidx.size();
            for (int w = 0; w < 2; w++) {
                const int64_t j = R.valle_first[v] + R.gt[2 * v + w];
                new_pair(rb + R.valle_off[j], R.valle_len[j], rep.off, rep.len, rev, rep.len > sv_threshold || R.valle_len[j] > sv_threshold); /* bubbleGraph.c:2253-2263 */
            }
            return at;
        });
        Lc.vsites.push_back(st);
    }
}

int sc_filtered_front(mrp_string_front *F, const mrp_string_chunk_rest *rest, int64_t sv_threshold, const std::vector<int64_t> &rpool_base) {
    static const char *who = "mrp_phase_string_chunks_with_filtered";
    const int64_t n_chunks = F->n_chunks;
    const mrp_string_chunk *chunks = F->chunks;
    mrp_string_front::Filtered &Q = F->fil;
    mrp_string_front::Scratch &X = F->scratch;
    Q.on = true;
    Q.rest = rest;
    Q.n_primary_pairs = F->n_pairs;
    Q.read_base.assign((size_t) n_chunks + 1, 0);
    Q.var_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        Q.read_base[(size_t) c + 1] = Q.read_base[(size_t) c] + chunks[c].n_reads + rest[c].n_filtered;
        Q.var_base[(size_t) c + 1] = Q.var_base[(size_t) c] + rest[c].n_variants;
    }
    if (Q.read_base[(size_t) n_chunks] >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 reads in one call", who);
    std::vector<FsTask> tasks;
    constexpr int64_t TASK_SITES = 128;
    for (int64_t c = 0; c < n_chunks; c++) {
        if (sc_rest_empty(rest[c])) continue;
        for (int64_t lo = 0; lo < chunks[c].n_bubbles; lo += TASK_SITES) tasks.push_back(FsTask{c, false, lo, std::min(chunks[c].n_bubbles, lo + TASK_SITES)});
        for (int64_t lo = 0; lo < rest[c].n_variants; lo += TASK_SITES) tasks.push_back(FsTask{c, true, lo, std::min(rest[c].n_variants, lo + TASK_SITES)});
    }
    std::vector<FsLocal> loc(tasks.size());
    mrp_parallel_for((int64_t) tasks.size(), 1, [&](int64_t ti) { sc_filtered_task(F, rest, sv_threshold, rpool_base, tasks[(size_t) ti], loc[(size_t) ti]); });
    /* ---- side by side: entries, class tables and blocks task by task; the sites as bubbles of every chunk, then variants */
    int64_t n_entries = 0, n_cbase = 0, n_pidx = 0, n_new = 0, n_b = 0, n_v = 0;
    for (const FsLocal &Lc : loc) {
        n_entries += (int64_t) Lc.entries.size(); n_cbase += (int64_t) Lc.cbase.size(); n_pidx += (int64_t) Lc.pidx.size(); n_new += Lc.pairs.size();
        n_b += (int64_t) Lc.bsites.size(); n_v += (int64_t) Lc.vsites.size();
    }
    if (F->n_pairs + n_new >= (1ll << 31) || n_entries >= (1ll << 31) || n_pidx >= (1ll << 31) || n_cbase >= (1ll << 31) || n_b + n_v >= (1ll << 31))
        return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs or entries in one call", who);
    Q.entries.resize((size_t) n_entries);
    Q.cbase.resize((size_t) n_cbase);
    Q.pidx.resize((size_t) n_pidx);
    Q.sites.resize((size_t) (n_b + n_v));
    Q.n_bsites = n_b;
    int64_t e0 = 0, c0 = 0, p0 = 0, b0 = 0, v0 = n_b, pair0 = F->n_pairs;
    for (size_t ti = 0; ti < tasks.size(); ti++) {
        const FsLocal &Lc = loc[ti];
        const int64_t c = tasks[ti].c;
        for (size_t i = 0; i < Lc.entries.size(); i++) {
            FsEntry e = Lc.entries[i];
            e.read += (int32_t) Q.read_base[(size_t) c];
            Q.entries[(size_t) e0 + i] = e;
        }
        for (size_t i = 0; i < Lc.cbase.size(); i++) Q.cbase[(size_t) c0 + i] = Lc.cbase[i] < 0 ? -1 : Lc.cbase[i] + (int32_t) p0;
        for (size_t i = 0; i < Lc.pidx.size(); i++) Q.pidx[(size_t) p0 + i] = (int32_t) (Lc.pidx[i] >= 0 ? Lc.pidx[i] : pair0 + ~Lc.pidx[i]);
        for (const FsSite &st : Lc.bsites) { FsSite g = st; g.entry_first += e0; g.cls_first += c0 / 2; Q.sites[(size_t) b0++] = g; }
        for (const FsSite &st : Lc.vsites) { FsSite g = st; g.entry_first += e0; g.cls_first += c0 / 2; Q.sites[(size_t) v0++] = g; }
        for (int64_t q : Lc.anchored) X.anchored_new.push_back(pair0 + q);
        X.pairs.append(Lc.pairs);
        e0 += (int64_t) Lc.entries.size(); c0 += (int64_t) Lc.cbase.size(); p0 += (int64_t) Lc.pidx.size(); pair0 += Lc.pairs.size();
    }
    F->n_pairs = pair0;
    /* a read's entries at bubbles in bubble order (a counting sort by read, filled in site order) */
    const int64_t n_reads_all = Q.read_base[(size_t) n_chunks];
    Q.cand_first.assign((size_t) n_reads_all + 1, 0);
    for (int64_t s = 0; s < n_b; s++)
        for (int64_t i = Q.sites[(size_t) s].entry_first; i < Q.sites[(size_t) s].entry_first + Q.sites[(size_t) s].n_entries; i++)
            Q.cand_first[(size_t) Q.entries[(size_t) i].read + 1]++;
    for (int64_t r = 0; r < n_reads_all; r++) Q.cand_first[(size_t) r + 1] += Q.cand_first[(size_t) r];
    Q.cand.resize((size_t) Q.cand_first[(size_t) n_reads_all]);
    std::vector<int64_t> fill(Q.cand_first.begin(), Q.cand_first.end() - 1);
    for (int64_t s = 0; s < n_b; s++)
        for (int64_t i = Q.sites[(size_t) s].entry_first; i < Q.sites[(size_t) s].entry_first + Q.sites[(size_t) s].n_entries; i++)
            Q.cand[(size_t) fill[(size_t) Q.entries[(size_t) i].read]++] = (int32_t) i;
    return MRP_OK;
}

int mrp_string_front_create(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest, const mrp_pair_hmm *forward_model,
                            const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, int wide_pairs, mrp_string_front **front_out) {
    const char *who = rest ? "mrp_phase_string_chunks_with_filtered" : "mrp_phase_string_chunks";
    const double t_begin = now_ms();
    *front_out = nullptr;
    mrp_string_front *F = new (std::nothrow) mrp_string_front();
    if (!F) return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks: out of host memory");
    struct Drop { mrp_string_front *f; ~Drop() { delete f; } } drop{F}; /* (an early return) */
    F->n_chunks = n_chunks;
    F->chunks = chunks;
    /* ---- the pairs of every chunk, one symbol pool: bubble b of chunk c is global bubble bubble_base[c] + b */
    std::vector<int64_t> &pool_base = F->pool_base, &sub_base = F->sub_base, bubble_base((size_t) n_chunks + 1, 0);
    pool_base.assign((size_t) n_chunks + 1, 0);
    sub_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        pool_base[(size_t) c + 1] = pool_base[(size_t) c] + chunks[c].pool_bytes;
        bubble_base[(size_t) c + 1] = bubble_base[(size_t) c] + chunks[c].n_bubbles;
        sub_base[(size_t) c + 1] = sub_base[(size_t) c] + (chunks[c].n_bubbles ? chunks[c].sub_first[chunks[c].n_bubbles] : 0);
    }
    const int64_t n_bub = bubble_base[(size_t) n_chunks], n_subs = sub_base[(size_t) n_chunks];
    HostVec<uint8_t> &gpool = F->gpool;
    /* the rests' symbols behind the chunks' (a rest that points at its chunk's pool reads it there) */
    std::vector<int64_t> rpool_base((size_t) n_chunks, 0);
    int64_t gpool_bytes = pool_base[(size_t) n_chunks];
    auto rest_has_own_pool = [&](int64_t c) { return !(rest[c].pool == chunks[c].pool && rest[c].pool_bytes == chunks[c].pool_bytes); };
    if (rest)
        for (int64_t c = 0; c < n_chunks; c++) {
            rpool_base[(size_t) c] = pool_base[(size_t) c];
            if (sc_rest_empty(rest[c]) || !rest_has_own_pool(c)) continue;
            rpool_base[(size_t) c] = gpool_bytes;
            gpool_bytes += rest[c].pool_bytes;
        }
    gpool.resize((size_t) gpool_bytes);
    mrp_string_front::Scratch &X = F->scratch;
    std::vector<int64_t> &g_sub_first = X.g_sub_first, &g_sub_off = X.g_sub_off;
    std::vector<int32_t> &g_sub_len = X.g_sub_len;
    g_sub_first.assign((size_t) n_bub + 1, 0);
    g_sub_off.resize((size_t) n_subs);
    g_sub_len.resize((size_t) n_subs);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        if (S.pool_bytes) memcpy(gpool.data() + pool_base[(size_t) c], S.pool, (size_t) S.pool_bytes);
        if (rest && !sc_rest_empty(rest[c]) && rest_has_own_pool(c) && rest[c].pool_bytes)
            memcpy(gpool.data() + rpool_base[(size_t) c], rest[c].pool, (size_t) rest[c].pool_bytes);
        for (int64_t b = 0; b < S.n_bubbles; b++) g_sub_first[(size_t) (bubble_base[(size_t) c] + b + 1)] = sub_base[(size_t) c] + S.sub_first[b + 1];
        const int64_t ns = sub_base[(size_t) c + 1] - sub_base[(size_t) c];
        for (int64_t k = 0; k < ns; k++) {
            g_sub_off[(size_t) (sub_base[(size_t) c] + k)] = pool_base[(size_t) c] + S.sub_off[k];
            g_sub_len[(size_t) (sub_base[(size_t) c] + k)] = S.sub_len[k];
        }
    });
    /* cachedScores (bubbleGraph.c:1418,1431-1441): the first substring of the bubble with given symbols owns the scores */
    std::vector<int64_t> &owner = X.owner;
    substring_owners(n_bub, g_sub_first.data(), gpool.data(), g_sub_off.data(), g_sub_len.data(), nullptr, false, owner);
    /* the owners' pairs, chunk by chunk in parallel: pair_first[k] = the pair of owner k with the bubble's allele 0 */
    std::vector<int64_t> pair_base((size_t) n_chunks + 1, 0), &pair_first = F->pair_first;
    pair_first.assign((size_t) n_subs, -1);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_string_chunk &S = chunks[c];
        int64_t np = 0;
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++)
                if (owner[(size_t) (sub_base[(size_t) c] + k)] == sub_base[(size_t) c] + k) np += S.allele_first[b + 1] - S.allele_first[b];
        pair_base[(size_t) c + 1] = pair_base[(size_t) c] + np;
    }
    const int64_t n_pairs = pair_base[(size_t) n_chunks];
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    PhmPairList &pairs = X.pairs;
    std::vector<std::vector<int64_t>> &chunk_anchors = X.chunk_anchors;
    pairs.resize(n_pairs);
    chunk_anchors.resize((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        const int64_t pb = pool_base[(size_t) c], sb = sub_base[(size_t) c];
        int64_t p = pair_base[(size_t) c];
        std::vector<int64_t> &anc = chunk_anchors[(size_t) c];
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
                if (owner[(size_t) (sb + k)] != sb + k) continue;
                pair_first[(size_t) (sb + k)] = p;
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1]; j++, p++) {
                    const size_t before = anc.size();
                    if (S.sub_len[k] > sv_threshold || S.allele_len[j] > sv_threshold) /* bubbleGraph.c:1448-1451 */
                        kmer_anchors(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], anc);
                    pairs.set(p, pb + S.allele_off[j], S.allele_len[j], pb + S.sub_off[k], S.sub_len[k], S.read_forward_strand[S.sub_read[k]] ? 0 : 1,
                              (int64_t) (anc.size() - before) / 2);
                }
            }
    });
    pairs.counts_to_offsets();
    for (auto &v : chunk_anchors) pairs.anchors.insert(pairs.anchors.end(), v.begin(), v.end());
    for (int64_t k = 0; k < n_subs; k++) /* duplicates read their owner's pairs */
        if (owner[(size_t) k] != k) pair_first[(size_t) k] = pair_first[(size_t) owner[(size_t) k]];

    F->n_subs = n_subs;
    F->n_pairs = n_pairs;
    if (rest) { /* the back half's sites; its speculative pairs join the list behind the front's own */
        const int rc = sc_filtered_front(F, rest, sv_threshold, rpool_base);
        if (rc != MRP_OK) return rc;
    }
    if (F->n_pairs > 0) {
        const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
        const int rc = phm_classify(who, models, 2, (int64_t) gpool.size(), pairs.view(), expansion, 0, 0, wide_pairs, F->L);
        if (rc != MRP_OK) return rc;
    }
    F->front_ms = now_ms() - t_begin;
    drop.f = nullptr;
    *front_out = F;
    return MRP_OK;
}

namespace {

/* One run of a front: everything the queued work reads or writes until the stream has drained -- the stream, the device and pinned
 * buffers, the host sources of the uploads, the events, the layouts -- and the chunks and results that are the run's until it hands
 * them over.  The destructor drains the stream first, then deletes the chunks and whatever was not handed over; the buffers' own
 * destructors follow, so mrp_string_front_run reclaims the pool once the ScRun is gone and no block can be forgotten.
 * The steps run in the order mrp_string_front_run lists them; each queues its work on ctx->stream in the order written. */
struct ScRun {
    mrp_context *const ctx;
    mrp_string_front *const F;
    mrp_string_chunks_stats *const stats;
    mrp_string_filtered_stats *const filtered_stats;
    const int64_t n_chunks, n_subs, n_pairs;
    const mrp_string_chunk *const chunks;
    hipStream_t s = nullptr; /* set once the device is current: from then on the destructor drains it */
    enum { EV_PAIRS_END, EV_BYTES_BEGIN, EV_BYTES_END, EV_POOL_HOME, EV_TAGS_BEGIN, EV_BACK_BEGIN, EV_BACK_END, EV_REC_BEGIN, EV_REC_END, N_EV };
    hipEvent_t ev[N_EV] = {};
    PhmDev D; /* the pair-HMM's device half: D.d_out holds the log probabilities every later kernel reads */
    DevBufGroup arrays;
    DevBuf<ScByteItem> d_items{arrays};
    DevBuf<uint8_t> d_pool{arrays};
    DevBuf<int64_t> d_aoff{arrays};
    DevBuf<uint64_t> d_haps{arrays};
    DevBuf<ScHapItem> d_hitems{arrays};
    DevBuf<int8_t> d_hap{arrays};
    DevBuf<double> d_phred{arrays};
    PinnedBuf h_pool, h_res;
    int8_t *h_hap = nullptr;
    double *h_phred = nullptr;
    std::vector<ScLayout> lay;
    std::vector<int64_t> dpool_base, aoff_base, seq_base, hap_base; /* n_chunks + 1: chunk c's share of the call's arrays */
    int64_t dpool_bytes = 0, n_seqs_all = 0;
    HostVec<ScByteItem> items;
    HostVec<int64_t> aoff_all;
    HostVec<uint64_t> haps;
    HostVec<ScHapItem> hitems;
    mrp_chunk_block blk;
    std::vector<mrp_chunk *> dch;
    std::vector<mrp_phase_result *> res;
    double phase_ms = 0; /* host wall time inside mrp_phase_reads_many */

    /* The back half's share: its static tables, what the phasing decided per chunk, a record per entry, the results.
     * Its four methods are called where the run has the matching step of its own; `on` false makes each a no-op. */
    struct Back {
        const mrp_string_front::Filtered &Q;
        mrp_filtered_out *const out;
        const bool on, count_used;
        int64_t n_reads = 0, n_vars = 0;
        size_t n_tot = 0, n_i32 = 0;
        DevBufGroup arrays;
        DevBuf<FsEntry> d_ent{arrays};
        DevBuf<FsSite> d_sites{arrays};
        DevBuf<FsChunk> d_chunks{arrays};
        DevBuf<int32_t> d_cbase{arrays}, d_pidx{arrays}, d_cand{arrays}, d_read_seq{arrays}, d_hap{arrays};
        DevBuf<int64_t> d_cand_first{arrays};
        DevBuf<HtEntry> d_rec{arrays};
        DevBuf<double> d_tot{arrays};
        DevBuf<uint8_t> d_used{arrays};
        HostVec<int32_t> read_seq;
        HostVec<FsChunk> fchunks;
        PinnedBuf h_res;
        double *h_tot = nullptr;
        int32_t *h_hap = nullptr;
        uint8_t *h_used = nullptr;
        float ms = 0.f;
        Back(const mrp_string_front::Filtered &q, mrp_filtered_out *o, bool stats) : Q(q), out(o), on(q.on && o != nullptr), count_used(on && stats) {}
        int upload_static(ScRun &R);
        int alloc_results(ScRun &R);
        int launch(ScRun &R);
        int hand_over(ScRun &R, mrp_profile_out *profiles_out);
    } back;

    /* The records' share: the site table and the tags' index go up with the static tables, the kernel follows the back
     * half's, 20 B per site and 4 B per slot come back.  `on` false makes each method a no-op. */
    struct Rec {
        mrp_string_front::Records &Q;
        const bool on;
        size_t n_sites = 0;
        DevBufGroup arrays;
        DevBuf<RcSite> d_sites{arrays};
        DevBuf<int32_t> d_read_seq{arrays}, d_slots{arrays};
        DevBuf<FsChunk> d_chunks{arrays};
        DevBuf<RcOut> d_out{arrays};
        HostVec<int32_t> read_seq;
        HostVec<FsChunk> fchunks;
        PinnedBuf h_res;
        explicit Rec(mrp_string_front::Records &q) : Q(q), on(q.on) {}
        int upload_static(ScRun &R);
        int alloc_results(ScRun &R);
        int launch(ScRun &R);
        int hand_over(ScRun &R);
    } rec;

    ScRun(mrp_context *c, mrp_string_front *f, mrp_string_chunks_stats *st, mrp_filtered_out *filtered_out, mrp_string_filtered_stats *fst)
        : ctx(c), F(f), stats(st), filtered_stats(fst), n_chunks(f->n_chunks), n_subs(f->n_subs), n_pairs(f->n_pairs), chunks(f->chunks),
          dch((size_t) f->n_chunks, nullptr), res((size_t) f->n_chunks, nullptr), back(f->fil, filtered_out, fst != nullptr), rec(f->rec) {
        /* the one place that binds the run's device buffers to the context's pool (D: phm_enqueue) */
        arrays.bind(&ctx->pool);
        back.arrays.bind(&ctx->pool);
        rec.arrays.bind(&ctx->pool);
    }
    ~ScRun() {
        if (s) (void) hipStreamSynchronize(s);
        for (mrp_chunk *ch : dch) delete ch;
        for (mrp_phase_result *r : res) mrp_phase_result_destroy(r);
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
    }
    int begin();
    int enqueue_pairhmm();
    int layout_and_items(double het_substitution_probability);
    int profile_bytes();
    int chunks_and_phase(const mrp_params *params);
    int hp_tags(int64_t min_phred);
    int download();
    int hand_over(mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out);
};

int ScRun::begin() {
    PHM_HIP(hipSetDevice(ctx->device));
    s = ctx->stream;
    for (hipEvent_t &x : ev) PHM_HIP(hipEventCreate(&x));
    return MRP_OK;
}

/* the pair-HMM kernels over the front's launch classes; EV_PAIRS_END behind them */
int ScRun::enqueue_pairhmm() {
    if (n_pairs > 0) {
        const int64_t pool_bytes = F->device_pool ? F->device_pool_bytes : (int64_t) F->gpool.size();
        const int rc = phm_enqueue(ctx, F->gpool.data(), pool_bytes, n_pairs, F->L, D, stats ? &stats->pairhmm : nullptr, F->device_pool);
        if (rc != MRP_OK) return rc;
    } else {
        PHM_HIP(hipEventRecord(ctx->ev[0], s));
    }
    PHM_HIP(hipEventRecord(ev[EV_PAIRS_END], s));
    return MRP_OK;
}

/* on the host, beside the pair-HMM kernels: the layout of every chunk (the index arrays only) and where each (bubble, substring)'s
 * bytes go.  Every chunk's pool lies in one device buffer, with mrp_chunk_create's tail slack (mrp_pack_kernel reads a read's last
 * bytes a dword at a time) and 256-byte alignment. */
int ScRun::layout_and_items(double het_substitution_probability) {
    lay.resize((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) { sc_layout(chunks[c], het_substitution_probability, lay[(size_t) c]); });
    dpool_base.assign((size_t) n_chunks + 1, 0);
    aoff_base.assign((size_t) n_chunks + 1, 0);
    seq_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        dpool_base[(size_t) c + 1] = (dpool_base[(size_t) c] + lay[(size_t) c].pool_bytes + MRP_POOL_TAIL_PAD + 255) & ~(int64_t) 255;
        aoff_base[(size_t) c + 1] = aoff_base[(size_t) c] + chunks[c].n_bubbles + 1;
        seq_base[(size_t) c + 1] = seq_base[(size_t) c] + (int64_t) lay[(size_t) c].seqs.size();
    }
    dpool_bytes = dpool_base[(size_t) n_chunks];
    n_seqs_all = seq_base[(size_t) n_chunks];
    items.resize((size_t) n_subs);
    aoff_all.resize((size_t) aoff_base[(size_t) n_chunks]);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        const ScLayout &Lc = lay[(size_t) c];
        const int64_t sb = F->sub_base[(size_t) c];
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
                const mrp_read &q = Lc.seqs[(size_t) Lc.seq_of[(size_t) S.sub_read[k]]];
                ScByteItem &it = items[(size_t) (sb + k)];
                it.dst = dpool_base[(size_t) c] + q.pool_offset + (Lc.aoff[(size_t) b] - Lc.aoff[(size_t) q.ref_start]);
                it.pair = (int32_t) F->pair_first[(size_t) (sb + k)];
                it.n_alleles = (int32_t) Lc.an[(size_t) b];
            }
        std::copy(Lc.aoff.begin(), Lc.aoff.end(), aoff_all.begin() + aoff_base[(size_t) c]);
    });
    return MRP_OK;
}

/* the profile bytes, written into the chunks' device pool; the host copy comes back behind them (EV_POOL_HOME) */
int ScRun::profile_bytes() {
    PHM_HIP(d_items.upload(items, s));
    PHM_HIP(d_aoff.upload(aoff_all, s));
    int rc = back.upload_static(*this); /* the static tables of the back half go up with the rest */
    if (rc == MRP_OK) rc = rec.upload_static(*this);
    if (rc != MRP_OK) return rc;
    PHM_HIP(d_pool.alloc((size_t) dpool_bytes));
    PHM_HIP(hipMemsetAsync(d_pool.p, 0, (size_t) dpool_bytes, s)); /* sites a read skips stay 0 */
    PHM_HIP(h_pool.reserve((size_t) dpool_bytes));
    PHM_HIP(hipEventRecord(ev[EV_BYTES_BEGIN], s));
    if (n_subs > 0) {
        hipLaunchKernelGGL(sc_profile_bytes_kernel, dim3((unsigned) ((n_subs + 255) / 256)), dim3(256), 0, s, d_items.p, n_subs, D.d_out.p, d_pool.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ev[EV_BYTES_END], s));
    PHM_HIP(hipMemcpyAsync(h_pool.p, d_pool.p, (size_t) dpool_bytes, hipMemcpyDeviceToHost, s));
    PHM_HIP(hipEventRecord(ev[EV_POOL_HOME], s)); /* the host copy is complete */
    return MRP_OK;
}

/* chunks over that pool (site tables staged and uploaded behind the download), then the phasing as it stands */
int ScRun::chunks_and_phase(const mrp_params *params) {
    std::vector<mrp_chunk_desc> descs((size_t) n_chunks);
    std::vector<const mrp_chunk_desc *> desc_ptr((size_t) n_chunks);
    std::vector<const uint8_t *> dev_pools((size_t) n_chunks);
    std::vector<const mrp_read *> rptr((size_t) n_chunks);
    std::vector<int64_t> nr((size_t) n_chunks);
    for (int64_t c = 0; c < n_chunks; c++) {
        const ScLayout &Lc = lay[(size_t) c];
        mrp_chunk_desc &d = descs[(size_t) c];
        d.n_sites = chunks[c].n_bubbles;
        d.allele_number = Lc.an.data();
        d.substitution_log_probs = Lc.sub.data();
        d.allele_prior_log_probs = Lc.prior.data();
        d.profile_pool = (const uint8_t *) h_pool.p + dpool_base[(size_t) c];
        d.pool_bytes = Lc.pool_bytes;
        d.reads = Lc.seqs.data();
        d.n_reads = (int64_t) Lc.seqs.size();
        desc_ptr[(size_t) c] = &d;
        dev_pools[(size_t) c] = d_pool.p + dpool_base[(size_t) c];
        rptr[(size_t) c] = Lc.seqs.data();
        nr[(size_t) c] = (int64_t) Lc.seqs.size();
    }
    int rc = mrp_chunk_block_create(ctx, n_chunks, desc_ptr.data(), dch.data(), &blk, 1, dev_pools.data());
    if (rc != MRP_OK) return rc;
    for (mrp_chunk *ch : dch) { ch->pool_host_ready = ev[EV_POOL_HOME]; ch->pool_host_pending.store(true); }
    std::vector<const mrp_chunk *> cptr(dch.begin(), dch.end());
    const double t0 = now_ms();
    rc = mrp_phase_reads_many(ctx, n_chunks, cptr.data(), rptr.data(), nr.data(), params, res.data(), stats ? &stats->phase : nullptr);
    phase_ms = now_ms() - t0;
    return rc;
}

/* HP tags over the same device pool: the fragments' haplotype strings go up, one lane per sequence; the back half follows the HP
 * kernel on the same stream and reads the tags and the haplotype strings where they are */
int ScRun::hp_tags(int64_t min_phred) {
    hap_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) hap_base[(size_t) c + 1] = hap_base[(size_t) c] + 2 * (int64_t) res[(size_t) c]->length;
    haps.resize((size_t) hap_base[(size_t) n_chunks]);
    hitems.resize((size_t) n_seqs_all);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_phase_result *g = res[(size_t) c];
        const ScLayout &Lc = lay[(size_t) c];
        const int64_t ns = (int64_t) Lc.seqs.size();
        if (g->length > 0) {
            std::copy(g->haplotype_string1, g->haplotype_string1 + g->length, haps.begin() + hap_base[(size_t) c]);
            std::copy(g->haplotype_string2, g->haplotype_string2 + g->length, haps.begin() + hap_base[(size_t) c] + g->length);
        }
        std::vector<int32_t> side((size_t) ns, 0);
        for (int64_t q = 0; q < g->n_reads2; q++) /* a read found in both sets counts as hap1 (genomeFragment.c:253) */
            if (g->reads2[q] >= 0 && g->reads2[q] < ns) side[(size_t) g->reads2[q]] = 2;
        for (int64_t q = 0; q < g->n_reads1; q++)
            if (g->reads1[q] >= 0 && g->reads1[q] < ns) side[(size_t) g->reads1[q]] = 1;
        for (int64_t q = 0; q < ns; q++) {
            ScHapItem &it = hitems[(size_t) (seq_base[(size_t) c] + q)];
            it.pool = dpool_base[(size_t) c] + Lc.seqs[(size_t) q].pool_offset;
            it.aoff = aoff_base[(size_t) c];
            it.hap = hap_base[(size_t) c];
            it.ref_start = Lc.seqs[(size_t) q].ref_start;
            it.length = Lc.seqs[(size_t) q].length;
            it.frag_start = g->ref_start;
            it.frag_length = g->length;
            it.side = side[(size_t) q];
            it.pad = 0;
        }
    }
    PHM_HIP(d_haps.upload(haps, s));
    PHM_HIP(d_hitems.upload(hitems, s));
    PHM_HIP(d_hap.alloc((size_t) n_seqs_all));
    PHM_HIP(d_phred.alloc((size_t) n_seqs_all));
    PHM_HIP(h_res.reserve((size_t) n_seqs_all * 9 + 16));
    h_hap = (int8_t *) h_res.p;
    h_phred = (double *) ((char *) h_res.p + (((size_t) n_seqs_all + 7) & ~(size_t) 7));
    /* the back half's buffers, device and pinned, before the HP kernel is queued: no allocation between it and the back half */
    int rc = back.alloc_results(*this);
    if (rc == MRP_OK) rc = rec.alloc_results(*this);
    if (rc != MRP_OK) return rc;
    PHM_HIP(hipEventRecord(ev[EV_TAGS_BEGIN], s));
    if (n_seqs_all > 0) {
        hipLaunchKernelGGL(sc_assign_kernel, dim3((unsigned) ((n_seqs_all + 255) / 256)), dim3(256), 0, s, d_hitems.p, n_seqs_all, d_aoff.p, d_haps.p,
                           d_pool.p, min_phred, d_hap.p, d_phred.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ctx->ev[1], s));
    if (n_seqs_all > 0) {
        PHM_HIP(hipMemcpyAsync(h_hap, d_hap.p, (size_t) n_seqs_all, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h_phred, d_phred.p, (size_t) n_seqs_all * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    rc = back.launch(*this);
    return rc == MRP_OK ? rec.launch(*this) : rc;
}

/* the downloads queued behind their kernels have landed once the stream has drained */
int ScRun::download() {
    PHM_HIP(hipStreamSynchronize(s));
    /* (read before anything is handed over: an error leaves profiles_out / filtered_out zeroed) */
    if (back.on && filtered_stats) PHM_HIP(hipEventElapsedTime(&back.ms, ev[EV_BACK_BEGIN], ev[EV_BACK_END]));
    if (rec.on) PHM_HIP(hipEventElapsedTime(&rec.Q.ms, ev[EV_REC_BEGIN], ev[EV_REC_END]));
    return MRP_OK;
}

/* back to the caller's reads; the results are the caller's from the last line on */
int ScRun::hand_over(mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out) {
    for (int64_t c = 0; c < n_chunks; c++) {
        const ScLayout &Lc = lay[(size_t) c];
        mrp_phase_result *g = res[(size_t) c];
        for (int64_t r = 0; r < chunks[c].n_reads; r++) {
            hap_out[c][r] = -1;
            if (phred_out) phred_out[c][r] = 0.0;
        }
        for (size_t q = 0; q < Lc.seqs.size(); q++) {
            const int32_t r = Lc.read_of_seq[q];
            hap_out[c][r] = h_hap[seq_base[(size_t) c] + (int64_t) q];
            if (phred_out) phred_out[c][r] = h_phred[seq_base[(size_t) c] + (int64_t) q];
        }
        for (int64_t q = 0; q < g->n_reads1; q++) g->reads1[q] = Lc.read_of_seq[(size_t) g->reads1[q]];
        for (int64_t q = 0; q < g->n_reads2; q++) g->reads2[q] = Lc.read_of_seq[(size_t) g->reads2[q]];
    }
    if (profiles_out)
        for (int64_t c = 0; c < n_chunks; c++) {
            const ScLayout &Lc = lay[(size_t) c];
            mrp_profile_out &P = profiles_out[c];
            P.n_seqs = (int64_t) Lc.seqs.size();
            P.pool_bytes = Lc.pool_bytes;
            P.seqs = (mrp_read *) sc_dup(Lc.seqs.data(), sizeof(mrp_read) * Lc.seqs.size());
            P.read_of_seq = (int32_t *) sc_dup(Lc.read_of_seq.data(), sizeof(int32_t) * Lc.read_of_seq.size());
            P.pool = (uint8_t *) sc_dup((const uint8_t *) h_pool.p + dpool_base[(size_t) c], (size_t) Lc.pool_bytes);
            P.allele_number = (uint32_t *) sc_dup(Lc.an.data(), sizeof(uint32_t) * Lc.an.size());
            P.substitution = (uint16_t *) sc_dup(Lc.sub.data(), sizeof(uint16_t) * Lc.sub.size());
            P.prior = (uint16_t *) sc_dup(Lc.prior.data(), sizeof(uint16_t) * Lc.prior.size());
            if (!P.seqs || !P.read_of_seq || !P.pool || !P.allele_number || !P.substitution || !P.prior) {
                for (int64_t q = 0; q <= c; q++) mrp_profile_out_clear(&profiles_out[q]);
                return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks: out of host memory");
            }
        }
    int rc = rec.hand_over(*this); /* (into the front: nothing of the caller's is written) */
    if (rc == MRP_OK) rc = back.hand_over(*this, profiles_out);
    if (rc != MRP_OK) return rc;
    if (stats) {
        float ms = 0.f;
        if (n_pairs > 0) { PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ev[EV_PAIRS_END])); stats->pairhmm.kernel_ms = ms; stats->pairhmm.cells = F->L.cells; }
        PHM_HIP(hipEventElapsedTime(&ms, ev[EV_BYTES_BEGIN], ev[EV_BYTES_END]));
        stats->profile_ms = ms;
        PHM_HIP(hipEventElapsedTime(&ms, ev[EV_TAGS_BEGIN], ctx->ev[1]));
        stats->assign_ms = ms;
    }
    for (int64_t c = 0; c < n_chunks; c++) { out[c] = res[(size_t) c]; res[(size_t) c] = nullptr; }
    return MRP_OK;
}

/* the static tables; a read's tag is its sequence's (read_seq: -1 a primary read in no bubble, -2 a filtered read) */
int ScRun::Back::upload_static(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    n_reads = Q.read_base[(size_t) R.n_chunks];
    n_vars = Q.var_base[(size_t) R.n_chunks];
    n_tot = 2 * (size_t) (n_reads + n_vars);
    n_i32 = (size_t) (n_reads + n_vars);
    read_seq.resize((size_t) n_reads);
    for (int64_t c = 0; c < R.n_chunks; c++) {
        const int64_t rb = Q.read_base[(size_t) c];
        for (int64_t r = 0; r < R.chunks[c].n_reads; r++) {
            const int32_t q = R.lay[(size_t) c].seq_of[(size_t) r];
            read_seq[(size_t) (rb + r)] = q < 0 ? -1 : (int32_t) (R.seq_base[(size_t) c] + q);
        }
        for (int64_t r = 0; r < Q.rest[c].n_filtered; r++) read_seq[(size_t) (rb + R.chunks[c].n_reads + r)] = -2;
    }
    PHM_HIP(d_ent.upload(Q.entries, s));
    PHM_HIP(d_sites.upload(Q.sites, s));
    PHM_HIP(d_cbase.upload(Q.cbase, s));
    PHM_HIP(d_pidx.upload(Q.pidx, s));
    PHM_HIP(d_cand_first.upload(Q.cand_first, s));
    PHM_HIP(d_cand.upload(Q.cand, s));
    PHM_HIP(d_read_seq.upload(read_seq, s));
    return MRP_OK;
}

/* what the phasing decided per chunk goes up; then every buffer of the results.  Totals: h1 | h2 of the reads, then cis | trans of
 * the variants; decisions: the reads', then the variants'. */
int ScRun::Back::alloc_results(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    fchunks.resize((size_t) R.n_chunks);
    for (int64_t c = 0; c < R.n_chunks; c++)
        fchunks[(size_t) c] = FsChunk{R.hap_base[(size_t) c], (int32_t) R.res[(size_t) c]->ref_start, (int32_t) R.res[(size_t) c]->length};
    PHM_HIP(d_chunks.upload(fchunks, s));
    PHM_HIP(d_rec.alloc(Q.entries.size()));
    PHM_HIP(d_tot.alloc(n_tot));
    PHM_HIP(d_hap.alloc(n_i32));
    PHM_HIP(h_res.reserve(n_tot * sizeof(double) + n_i32 * sizeof(int32_t) + (count_used ? (size_t) R.n_pairs : 0) + 16));
    h_tot = (double *) h_res.p;
    h_hap = (int32_t *) (h_tot + n_tot);
    h_used = (uint8_t *) (h_hap + n_i32);
    if (count_used) {
        PHM_HIP(d_used.alloc((size_t) R.n_pairs));
        PHM_HIP(hipMemsetAsync(d_used.p, 0, (size_t) std::max<int64_t>(R.n_pairs, 1), s));
    }
    return MRP_OK;
}

int ScRun::Back::launch(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    const int64_t n_sites = (int64_t) Q.sites.size();
    PHM_HIP(hipEventRecord(R.ev[EV_BACK_BEGIN], s));
    if (n_sites > 0) {
        hipLaunchKernelGGL(sc_filtered_sites_kernel, dim3((unsigned) n_sites), dim3(64), 0, s, d_sites.p, d_ent.p, d_cbase.p, d_pidx.p, d_read_seq.p,
                           R.d_hap.p, d_chunks.p, R.d_haps.p, d_rec.p, count_used ? d_used.p : nullptr);
        PHM_HIP(hipGetLastError());
    }
    double *d_h1 = d_tot.p, *d_h2 = d_tot.p + n_reads, *d_cis = d_tot.p + 2 * n_reads, *d_trans = d_cis + n_vars;
    if (n_reads > 0) {
        hipLaunchKernelGGL(fs_partition_kernel, dim3((unsigned) ((n_reads + 255) / 256)), dim3(256), 0, s, d_cand_first.p, d_cand.p, d_rec.p, R.D.d_out.p,
                           d_read_seq.p, R.d_hap.p, n_reads, d_hap.p, d_h1, d_h2);
        PHM_HIP(hipGetLastError());
    }
    if (n_vars > 0) {
        hipLaunchKernelGGL(fs_phase_kernel, dim3((unsigned) ((n_vars + 255) / 256)), dim3(256), 0, s, d_sites.p + Q.n_bsites, d_rec.p, R.D.d_out.p, n_vars,
                           d_hap.p + n_reads, d_cis, d_trans);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(R.ev[EV_BACK_END], s));
    if (n_tot > 0) {
        PHM_HIP(hipMemcpyAsync(h_tot, d_tot.p, n_tot * sizeof(double), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h_hap, d_hap.p, n_i32 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (count_used && R.n_pairs > 0) PHM_HIP(hipMemcpyAsync(h_used, d_used.p, (size_t) R.n_pairs, hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

int ScRun::Back::hand_over(ScRun &R, mrp_profile_out *profiles_out) {
    if (!on) return MRP_OK;
    const double *h_h1 = h_tot, *h_h2 = h_tot + n_reads, *h_cis = h_tot + 2 * n_reads, *h_trans = h_cis + n_vars;
    bool ok = true;
    for (int64_t c = 0; c < R.n_chunks && ok; c++) {
        mrp_filtered_out &O = out[c];
        const int64_t rb = Q.read_base[(size_t) c], nr = Q.read_base[(size_t) c + 1] - rb, vb = Q.var_base[(size_t) c], nv = Q.var_base[(size_t) c + 1] - vb;
        O.n_reads = nr;
        O.n_variants = nv;
        O.read_hap = (int32_t *) sc_dup(h_hap + rb, sizeof(int32_t) * (size_t) nr);
        O.h1 = (double *) sc_dup(h_h1 + rb, sizeof(double) * (size_t) nr);
        O.h2 = (double *) sc_dup(h_h2 + rb, sizeof(double) * (size_t) nr);
        O.variant_state = (int32_t *) sc_dup(h_hap + n_reads + vb, sizeof(int32_t) * (size_t) nv);
        O.cis = (double *) sc_dup(h_cis + vb, sizeof(double) * (size_t) nv);
        O.trans = (double *) sc_dup(h_trans + vb, sizeof(double) * (size_t) nv);
        ok = O.read_hap && O.h1 && O.h2 && O.variant_state && O.cis && O.trans;
    }
    if (!ok) {
        for (int64_t c = 0; c < R.n_chunks; c++) {
            mrp_filtered_out_clear(&out[c]);
            if (profiles_out) mrp_profile_out_clear(&profiles_out[c]);
        }
        return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks_with_filtered: out of host memory");
    }
    if (R.filtered_stats) {
        mrp_string_filtered_stats &T = *R.filtered_stats;
        T.filtered_ms += ms;
        T.pairs_scored += R.n_pairs;
        T.pairs_speculative += R.n_pairs - Q.n_primary_pairs;
        for (int64_t p = Q.n_primary_pairs; p < R.n_pairs; p++) T.pairs_read_by_results += h_used[p] ? 1 : 0;
    }
    return MRP_OK;
}

/* the records: the site table and, per primary read of the call, where the HP kernel writes its tag */
int ScRun::Rec::upload_static(ScRun &R) {
    if (!on) return MRP_OK;
    n_sites = Q.sites.size();
    read_seq.resize((size_t) Q.read_first[(size_t) R.n_chunks]);
    for (int64_t c = 0; c < R.n_chunks; c++)
        for (int64_t r = 0; r < R.chunks[c].n_reads; r++) {
            const int32_t q = R.lay[(size_t) c].seq_of[(size_t) r];
            read_seq[(size_t) (Q.read_first[(size_t) c] + r)] = q < 0 ? -1 : (int32_t) (R.seq_base[(size_t) c] + q);
        }
    PHM_HIP(d_sites.upload(Q.sites, R.s));
    PHM_HIP(d_read_seq.upload(read_seq, R.s));
    return MRP_OK;
}

/* where the fragments' haplotype strings lie goes up; the results' buffers, device and pinned, before the HP kernel is queued */
int ScRun::Rec::alloc_results(ScRun &R) {
    if (!on) return MRP_OK;
    fchunks.resize((size_t) R.n_chunks);
    for (int64_t c = 0; c < R.n_chunks; c++)
        fchunks[(size_t) c] = FsChunk{R.hap_base[(size_t) c], (int32_t) R.res[(size_t) c]->ref_start, (int32_t) R.res[(size_t) c]->length};
    PHM_HIP(d_chunks.upload(fchunks, R.s));
    PHM_HIP(d_out.alloc(n_sites));
    PHM_HIP(d_slots.alloc((size_t) Q.n_slots));
    PHM_HIP(h_res.reserve(n_sites * sizeof(RcOut) + (size_t) Q.n_slots * sizeof(int32_t) + 16));
    return MRP_OK;
}

int ScRun::Rec::launch(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    if (!R.back.on) return fail(MRP_ERR_ARG, "mrp_phase_aligned_chunks_with_records: the records follow the back half");
    PHM_HIP(hipEventRecord(R.ev[EV_REC_BEGIN], s));
    if (n_sites > 0) {
        hipLaunchKernelGGL(rc_records_kernel, dim3((unsigned) n_sites), dim3(64), 0, s, d_sites.p, Q.entry_first, Q.entry_read, Q.read_status, Q.take,
                           d_read_seq.p, R.d_hap.p, d_chunks.p, R.d_haps.p, R.back.d_hap.p + R.back.n_reads, d_out.p, d_slots.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(R.ev[EV_REC_END], s));
    if (n_sites > 0) PHM_HIP(hipMemcpyAsync(h_res.p, d_out.p, n_sites * sizeof(RcOut), hipMemcpyDeviceToHost, s));
    if (Q.n_slots > 0)
        PHM_HIP(hipMemcpyAsync((uint8_t *) h_res.p + n_sites * sizeof(RcOut), d_slots.p, (size_t) Q.n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

int ScRun::Rec::hand_over(ScRun &R) {
    if (!on) return MRP_OK;
    const RcOut *o = (const RcOut *) h_res.p;
    const int32_t *sl = (const int32_t *) ((const uint8_t *) h_res.p + n_sites * sizeof(RcOut));
    Q.out.assign(o, o + n_sites);
    Q.slots.assign(sl, sl + Q.n_slots);
    return MRP_OK;
}

}  // namespace

int mrp_string_front_run(mrp_context *ctx, mrp_string_front *F, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                         mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                         mrp_string_chunks_stats *stats, mrp_filtered_out *filtered_out, mrp_string_filtered_stats *filtered_stats) {
    const double t_begin = now_ms();
    int rc;
    double phase_ms;
    {
        ScRun R(ctx, F, stats, filtered_out, filtered_stats);
        rc = R.begin();
        if (rc == MRP_OK) rc = R.enqueue_pairhmm();
        if (rc == MRP_OK) rc = R.layout_and_items(het_substitution_probability);
        if (rc == MRP_OK) rc = R.profile_bytes();
        if (rc == MRP_OK) rc = R.chunks_and_phase(params);
        if (rc == MRP_OK) rc = R.hp_tags(min_phred);
        if (rc == MRP_OK) rc = R.download();
        if (rc == MRP_OK) rc = R.hand_over(out, hap_out, phred_out, profiles_out);
        phase_ms = R.phase_ms;
    }
    /* the stream has drained and every buffer of the run is back in the pool (after a refused run as well) */
    ctx->pool.reclaim();
    if (rc == MRP_OK && stats) { /* the whole call, its teardown included */
        stats->total_ms = F->front_ms + (now_ms() - t_begin);
        stats->host_ms = stats->total_ms - phase_ms;
    }
    return rc;
}

/* What the two entries share, from the checks on: rest, filtered_out and filtered_stats are NULL for the plain call */
static int sc_phase_chunks(const char *who, double t_begin, mrp_context *ctx, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest,
                           const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                           double het_substitution_probability, const mrp_params *params, int64_t min_phred, mrp_phase_result **out, int8_t *const *hap_out,
                           double *const *phred_out, mrp_profile_out *profiles_out, mrp_string_chunks_stats *stats, mrp_filtered_out *filtered_out,
                           mrp_string_filtered_stats *filtered_stats) {
    /* ---- checks (host only, before the context: a malformed call is refused the same with or without a device) */
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, rest, who);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the pair-HMM path has no CPU fallback)", who);
    for (int64_t c = 0; c < n_chunks; c++) out[c] = nullptr;
    if (profiles_out) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    if (n_chunks == 0) return MRP_OK;
    mrp_string_front *F = nullptr;
    rc = mrp_string_front_create(n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold, ctx->wide_pairs, &F);
    if (rc != MRP_OK) return rc;
    F->front_ms = now_ms() - t_begin;
    rc = mrp_string_front_run(ctx, F, het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, stats, filtered_out, filtered_stats);
    mrp_string_front_destroy(F);
    return rc;
}

extern "C" {

int mrp_string_chunk_units(const mrp_string_chunk *chunk, int64_t *units_out) {
    if (!chunk || !units_out || chunk->n_bubbles < 0 || (chunk->n_bubbles > 0 && !chunk->sub_first))
        return mrp_set_error(MRP_ERR_ARG, "mrp_string_chunk_units: null argument or bad sizes");
    *units_out = chunk->n_bubbles ? chunk->sub_first[chunk->n_bubbles] : 0;
    return MRP_OK;
}

int mrp_phase_string_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model,
                            const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                            const mrp_params *params, int64_t min_phred, mrp_phase_result **out, int8_t *const *hap_out,
                            double *const *phred_out, mrp_profile_out *profiles_out, mrp_string_chunks_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    return sc_phase_chunks("mrp_phase_string_chunks", t_begin, ctx, n_chunks, chunks, nullptr, forward_model, reverse_model, expansion, sv_threshold,
                           het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, stats, nullptr, nullptr);
}

int mrp_phase_string_chunks_with_filtered(mrp_context *ctx, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest,
                                          const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                          double het_substitution_probability, const mrp_params *params, int64_t min_phred, mrp_phase_result **out,
                                          int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out, mrp_filtered_out *filtered_out,
                                          mrp_string_filtered_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks > 0 && (!rest || !filtered_out)) return fail(MRP_ERR_ARG, "mrp_phase_string_chunks_with_filtered: null argument or bad sizes");
    if (filtered_out && n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    return sc_phase_chunks("mrp_phase_string_chunks_with_filtered", t_begin, ctx, n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold,
                           het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, stats ? &stats->chunks : nullptr,
                           filtered_out, stats);
}

}  // extern "C"
