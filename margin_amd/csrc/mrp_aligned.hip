/*
 * mrp_aligned.hip -- the composites over the extraction's result in HBM (ha_owners_kernel, ec_classes_kernel): the haplotagging of aligned
 * reads from a phased VCF (mrp_haplotag_aligned_chunks), the phasing of aligned chunks (mrp_phase_aligned_chunks; its k-mer anchors are
 * made by mrp_anchors.hip) and the same with the filtered back half (mrp_phase_aligned_chunks_with_filtered).  The pair-HMM and the string
 * run they queue come through mrp_pairhmm.h.  gfx950 only; compiled with -ffp-contract=off.
 */
#include "mrp_pairhmm.h"

#pragma clang fp contract(off)

namespace {

/* cachedScores of bubbleGraph_partitionFilteredReadsFromPhasedVcfEntries (bubbleGraph.c:2044-2072) on the device, over the arrays the
 * extraction left in HBM (mrp_extract_device): a wave per site, a lane per entry with a lane stride (a site may hold more entries than
 * a wave has lanes).  An entry takes part if its read is MRP_READ_KEPT and, with a mask, take[read] is set (the caller's downsampling in
 * mrp_phase_aligned_chunks; NULL: every kept read); owner[p] = the LAST entry of the site that takes part and has
 * p's substring (b->reads is filled by popping, :2012-2014), p itself if none follows, -1 for an entry that takes no part.  Pass one
 * gives every entry a key (length, hash of the symbols); pass two walks the site from its end and compares symbols wherever the keys
 * agree: the hash only skips comparisons.  Every loop is bounded by the site's entry count or the substring's length; the barrier
 * between the passes is the wave's own workgroup's, and both passes of a site are run by the same wave. */
constexpr uint64_t HA_NO_KEY = ~0ull;
__global__ void __launch_bounds__(PHM_WAVE) ha_owners_kernel(const int64_t *__restrict__ first, int64_t n_sites, const int32_t *__restrict__ read,
                                                             const uint8_t *__restrict__ status, const int64_t *__restrict__ len,
                                                             const int64_t *__restrict__ off, const uint8_t *__restrict__ sym,
                                                             const uint8_t *__restrict__ take, uint64_t *key, int32_t *__restrict__ owner) {
    const int lane = threadIdx.x;
    for (int64_t v = blockIdx.x; v < n_sites; v += gridDim.x) {
        const int64_t a = first[v], b = first[v + 1];
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            uint64_t k = HA_NO_KEY;
            const int32_t r = read[p];
            if (status[r] == MRP_READ_KEPT && (!take || take[r])) {
                const uint8_t *x = sym + off[p];
                const int64_t n = len[p];
                uint32_t h = 2166136261u;
                for (int64_t i = 0; i < n; i++) h = (h ^ x[i]) * 16777619u;
                k = (uint64_t) n << 32 | h;
            }
            key[p] = k;
        }
        __syncthreads();
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint64_t k = key[p];
            int32_t o = -1;
            if (k != HA_NO_KEY) {
                o = (int32_t) p;
                const uint8_t *x = sym + off[p];
                const int64_t n = len[p];
                for (int64_t q = b - 1; q > p; q--) {
                    if (key[q] != k) continue;
                    const uint8_t *y = sym + off[q];
                    int64_t i = 0;
                    while (i < n && x[i] == y[i]) i++;
                    if (i == n) {
                        o = (int32_t) q;
                        break;
                    }
                }
            }
            owner[p] = o;
        }
    }
}

/* The classes of equal substrings of every site (what sc_filtered_task finds by sorting host symbols), over symbols that lie in HBM: a wave
 * per site, lanes striding over the site's entries, waves striding over the sites, as ha_owners_kernel.  Pass one gives EVERY entry of the
 * site a key (length, FNV-1a of the symbols) -- no mask: who may own is decided later, from indices.  Pass two gives entry p its
 * representative rep[p]: the lowest entry q <= p of the site with p's length and bytes, found by walking the site from its start and
 * comparing symbols only where the keys agree (the hash only skips comparisons; two distinct strings with one key are told apart by
 * their bytes).  Every loop is bounded by the site's entry count or a substring's length; stores are plain vector stores; the barrier
 * between the passes is the wave's own workgroup's.  LenT: int32 lengths (the public seam) or the extraction's int64 ones. */
template <typename LenT>
__global__ void __launch_bounds__(PHM_WAVE) ec_classes_kernel(const int64_t *__restrict__ first, int64_t n_sites, const LenT *__restrict__ len,
                                                              const int64_t *__restrict__ off, const uint8_t *__restrict__ sym, uint64_t *key,
                                                              int32_t *__restrict__ rep) {
    const int lane = threadIdx.x;
    for (int64_t v = blockIdx.x; v < n_sites; v += gridDim.x) {
        const int64_t a = first[v], b = first[v + 1];
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint8_t *x = sym + off[p];
            const int64_t n = len[p];
            uint32_t h = 2166136261u;
            for (int64_t i = 0; i < n; i++) h = (h ^ x[i]) * 16777619u;
            key[p] = (uint64_t) n << 32 | h;
        }
        __syncthreads();
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint64_t k = key[p];
            const uint8_t *x = sym + off[p];
            const int64_t n = len[p];
            int32_t o = (int32_t) p;
            for (int64_t q = a; q < p; q++) {
                if (key[q] != k) continue;
                const uint8_t *y = sym + off[q];
                int64_t i = 0;
                while (i < n && x[i] == y[i]) i++;
                if (i == n) {
                    o = (int32_t) q;
                    break;
                }
            }
            rep[p] = o;
        }
    }
}

}  // namespace

/* ec_classes_kernel over a host pool: upload, one launch, 4 B per entry back */
extern "C" int mrp_equal_substring_classes(mrp_context *ctx, int64_t n_sites, const int64_t *entry_first, const uint8_t *pool, int64_t pool_bytes,
                                           const int64_t *off, const int32_t *len, int32_t *rep_out) {
    static const char *who = "mrp_equal_substring_classes";
    if (n_sites < 0 || pool_bytes < 0 || !entry_first || (pool_bytes > 0 && !pool)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (entry_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: entry_first must start at 0", who);
    for (int64_t v = 0; v < n_sites; v++)
        if (entry_first[v + 1] < entry_first[v]) return mrp_set_error(MRP_ERR_ARG, "%s: entry_first not ascending at site %lld", who, (long long) v);
    const int64_t n_ent = entry_first[n_sites];
    if (n_ent >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 entries in one call", who);
    if (n_ent > 0 && (!off || !len || !rep_out)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    for (int64_t p = 0; p < n_ent; p++)
        if (len[p] < 0 || off[p] < 0 || off[p] + len[p] > pool_bytes) return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld lies outside the symbol pool", who, (long long) p);
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the classes are found on the device; there is no CPU fallback)", who);
    if (n_ent == 0) return MRP_OK;
    {
        PHM_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DevBuf<uint8_t> d_pool;
        DevBuf<int64_t> d_first, d_off;
        DevBuf<int32_t> d_len, d_rep;
        DevBuf<uint64_t> d_key;
        d_pool.pool = d_first.pool = d_off.pool = d_len.pool = d_rep.pool = d_key.pool = &ctx->pool;
        Drain drain{s};
        PHM_HIP(d_pool.alloc((size_t) pool_bytes));
        PHM_HIP(d_first.alloc((size_t) n_sites + 1));
        PHM_HIP(d_off.alloc((size_t) n_ent));
        PHM_HIP(d_len.alloc((size_t) n_ent));
        PHM_HIP(d_key.alloc((size_t) n_ent));
        PHM_HIP(d_rep.alloc((size_t) n_ent));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_first.p, entry_first, 8 * ((size_t) n_sites + 1), hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_off.p, off, 8 * (size_t) n_ent, hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_len.p, len, 4 * (size_t) n_ent, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ec_classes_kernel<int32_t>, dim3((unsigned) std::min<int64_t>(n_sites, 65536)), dim3(PHM_WAVE), 0, s, d_first.p, n_sites, d_len.p,
                           d_off.p, d_pool.p, d_key.p, d_rep.p);
        PHM_HIP(hipGetLastError());
        HostVec<int32_t> rep((size_t) n_ent); /* (rep_out is written only on success) */
        PHM_HIP(hipMemcpyAsync(rep.data(), d_rep.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipStreamSynchronize(s));
        memcpy(rep_out, rep.data(), 4 * (size_t) n_ent);
    }
    ctx->pool.reclaim();
    return MRP_OK;
}

/* ---- mrp_haplotag_aligned_chunks: the staged extraction (mrp_internal.h) with the partition of mrp_partition_reads_by_haplotype reading
 * its result where it lies in HBM.  One device pool holds the call's allele strings, then the substrings the
 * gather writes behind them; the owners of equal substrings are found there (ha_owners_kernel); the host gets per entry its read, length
 * and owner and per read its status, and makes from them what needs no symbol: the pair list (ht_build_pairs' order), the launch classes
 * (phm_classify reads offsets and lengths only for unanchored pairs) and the per-read entry lists of ht_partition_kernel. */
namespace {

/* What the composites over aligned chunks share (mrp_haplotag_aligned_chunks, mrp_phase_aligned_chunks): the staged extraction gathering
 * behind the allele strings in the call's one device pool, the owners kernel over it and what comes back from it -- indices, no symbol. */
struct AlignedFront {
    const char *const who;
    mrp_context *ctx; /* (a front made ahead of its run gets it when it is staged) */
    const int64_t n_chunks;
    const mrp_aligned_chunk *const chunks;
    mrp_extract_run *X = nullptr;
    hipStream_t s = nullptr; /* set once the device is current: from then on the destructor drains it */
    hipEvent_t ev[2] = {nullptr, nullptr}; /* around the owners kernel */
    mrp_extract_device D{};
    int64_t allele_bytes = 0, pool_bytes = 0, n_alleles = 0, downloaded = 0;
    PinnedBuf h_sym, h_back;
    HostVec<int64_t> a_off, y_off;
    HostVec<int32_t> a_len;
    HostVec<uint8_t> forward;
    DevBufGroup arrays;
    DevBuf<uint8_t> d_sym{arrays}, d_take{arrays};
    DevBuf<uint64_t> d_key{arrays};
    DevBuf<int32_t> d_owner{arrays};
    /* what came back after the owners kernel */
    const uint8_t *k_status = nullptr;
    const int64_t *k_first = nullptr, *k_len = nullptr;
    const int32_t *k_read = nullptr, *k_owner = nullptr;
    /* a mask made on the device (the downsampling, PaRun::downsampled_owners): d_take holds it before the owners kernel; its first
     * mask_reads bytes and the mask_chunks per-chunk flags behind d_mask_flag come back with the rest (k_flag is not aligned) */
    int64_t mask_reads = -1, mask_chunks = 0;
    const int32_t *d_mask_flag = nullptr;
    const uint8_t *k_take = nullptr, *k_flag = nullptr;

    AlignedFront(const char *w, mrp_context *c, int64_t n, const mrp_aligned_chunk *ch) : who(w), ctx(c), n_chunks(n), chunks(ch) {}
    ~AlignedFront() {
        if (s) (void) hipStreamSynchronize(s);
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
        mrp_extract_run_destroy(X);
    }
    int check_front(const mrp_extract_options *options, mrp_extract_stats *extract_stats, bool null_argument, int64_t expansion);
    int extract();
    int owners(const HostVec<uint8_t> *take);
    void offsets_and_strands();
};

struct HaRun : AlignedFront {
    const int32_t *const *const gt;
    mrp_haplotag_aligned_stats *const stats;
    PinnedBuf h_res;
    HostVec<int64_t> first;
    HostVec<HtEntry> ent;
    HtPairs P;
    PhmLaunch H;
    PhmDev L; /* L.d_out holds the log probabilities the partition kernel reads */
    HtPartitionDev B;

    HaRun(mrp_context *c, int64_t n, const mrp_aligned_chunk *ch, const int32_t *const *g, mrp_haplotag_aligned_stats *st)
        : AlignedFront("mrp_haplotag_aligned_chunks", c, n, ch), gt(g), stats(st) {}
    ~HaRun() {
        if (s) (void) hipStreamSynchronize(s); /* before the pinned result buffer goes */
    }
    int check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
              int8_t *const *hap_out, double *const *h1_out, double *const *h2_out, int sv_split);
    int pairs();
    int score(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion);
    int hand_over(int8_t *const *hap_out, double *const *h1_out, double *const *h2_out);
};

/* how both checks open: the extraction's run and its MRP_ERR_ARG, then the caller's own null arguments (one is missing) and the expansion */
int AlignedFront::check_front(const mrp_extract_options *options, mrp_extract_stats *extract_stats, bool null_argument, int64_t expansion) {
    X = mrp_extract_run_create(who, n_chunks, chunks, options, extract_stats);
    if (!X) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int rc = mrp_extract_run_check_args(X, true);
    if (rc == MRP_OK) rc = mrp_extract_run_check_chunks(X);
    if (rc != MRP_OK) return rc;
    if (null_argument) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    return MRP_OK;
}

/* every MRP_ERR_ARG of the call, then the two refused modes: nothing here looks at the context (sv_split: its setting, 0 for none) */
int HaRun::check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                 int8_t *const *hap_out, double *const *h1_out, double *const *h2_out, int sv_split) {
    const int rc = check_front(options, stats ? &stats->extract : nullptr, !forward_model || !reverse_model || (n_chunks > 0 && (!gt || !hap_out)), expansion);
    if (rc != MRP_OK) return rc;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        if (C.n_reads > 0 && (!hap_out[c] || (h1_out && !h1_out[c]) || (h2_out && !h2_out[c])))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output array", who, (long long) c);
        if (C.n_variants > 0 && !gt[c]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null genotypes", who, (long long) c);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t k = C.allele_first[v + 1] - C.allele_first[v];
            for (int w = 0; w < 2; w++)
                if (gt[c][2 * v + w] < 0 || gt[c][2 * v + w] >= k)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, variant %lld: genotype %d outside its %lld alleles", who, (long long) c, (long long) v,
                                         gt[c][2 * v + w], (long long) k);
        }
    }
    return mrp_extract_run_check_modes(X, sv_split);
}

/* the extraction up to its second half, gathering behind the allele strings in the call's one device pool */
int AlignedFront::extract() {
    int rc = mrp_extract_run_stage(X, ctx);
    if (rc != MRP_OK) return rc;
    s = ctx->stream;
    arrays.bind(&ctx->pool);
    for (hipEvent_t &x : ev) PHM_HIP(hipEventCreate(&x));
    rc = mrp_extract_run_first_half(X);
    int64_t n_ent = 0, n_bases = 0;
    if (rc == MRP_OK) rc = mrp_extract_run_totals(X, &n_ent, &n_bases);
    if (rc != MRP_OK) return rc;
    downloaded += 16;
    allele_bytes = mrp_extract_run_allele_bytes(X);
    pool_bytes = allele_bytes + n_bases;
    for (int64_t c = 0; c < n_chunks; c++) n_alleles += chunks[c].n_variants ? chunks[c].allele_first[chunks[c].n_variants] : 0;
    a_off.resize((size_t) n_alleles);
    a_len.resize((size_t) n_alleles);
    PHM_HIP(h_sym.reserve(std::max<size_t>((size_t) allele_bytes, 1)));
    mrp_extract_run_alleles(X, (uint8_t *) h_sym.p, a_off.data(), a_len.data());
    PHM_HIP(d_sym.alloc((size_t) pool_bytes));
    if (allele_bytes) PHM_HIP(hipMemcpyAsync(d_sym.p, h_sym.p, (size_t) allele_bytes, hipMemcpyHostToDevice, s));
    rc = mrp_extract_run_second_half(X, d_sym.p, allele_bytes);
    if (rc != MRP_OK) return rc;
    mrp_extract_run_device(X, &D);
    return MRP_OK;
}

/* the owners on the device (take: NULL, or per read of the call whether it may take part; mask_reads >= 0: the mask is in d_take
 * already); back come the per-read status and per entry its read, length and owner -- not the symbols -- and of a mask made on the
 * device its first mask_reads bytes and the chunks' flags */
int AlignedFront::owners(const HostVec<uint8_t> *take) {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants, n_reads = D.n_reads;
    const bool device_mask = mask_reads >= 0;
    PHM_HIP(d_key.alloc((size_t) n_ent));
    PHM_HIP(d_owner.alloc((size_t) n_ent));
    if (take) PHM_HIP(d_take.upload(*take, s));
    PHM_HIP(hipEventRecord(ev[0], s));
    if (n_ent > 0) {
        hipLaunchKernelGGL(ha_owners_kernel, dim3((unsigned) std::min<int64_t>(n_var, 65536)), dim3(PHM_WAVE), 0, s, D.entry_first, n_var, D.entry_read,
                           D.read_status, D.entry_len, D.entry_off, D.symbols, take || device_mask ? (const uint8_t *) d_take.p : nullptr, d_key.p, d_owner.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ev[1], s));
    const size_t b_first = 0, b_len = b_first + 8 * ((size_t) n_var + 1), b_read = b_len + 8 * (size_t) n_ent, b_owner = b_read + 4 * (size_t) n_ent,
                 b_status = b_owner + 4 * (size_t) n_ent, b_take = b_status + (size_t) n_reads, b_flag = b_take + (device_mask ? (size_t) mask_reads : 0),
                 b_end = b_flag + 4 * (size_t) mask_chunks;
    PHM_HIP(h_back.reserve(b_end));
    uint8_t *hk = (uint8_t *) h_back.p;
    PHM_HIP(hipMemcpyAsync(hk + b_first, D.entry_first, 8 * ((size_t) n_var + 1), hipMemcpyDeviceToHost, s));
    if (n_ent) {
        PHM_HIP(hipMemcpyAsync(hk + b_len, D.entry_len, 8 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(hk + b_read, D.entry_read, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(hk + b_owner, d_owner.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
    }
    if (n_reads) PHM_HIP(hipMemcpyAsync(hk + b_status, D.read_status, (size_t) n_reads, hipMemcpyDeviceToHost, s));
    if (device_mask && mask_reads) PHM_HIP(hipMemcpyAsync(hk + b_take, d_take.p, (size_t) mask_reads, hipMemcpyDeviceToHost, s));
    if (mask_chunks) PHM_HIP(hipMemcpyAsync(hk + b_flag, d_mask_flag, 4 * (size_t) mask_chunks, hipMemcpyDeviceToHost, s));
    PHM_HIP(hipStreamSynchronize(s));
    downloaded += (int64_t) b_end;
    if (device_mask) { k_take = hk + b_take; k_flag = hk + b_flag; }
    k_first = (const int64_t *) (hk + b_first);
    k_len = (const int64_t *) (hk + b_len);
    k_read = (const int32_t *) (hk + b_read);
    k_owner = (const int32_t *) (hk + b_owner);
    k_status = hk + b_status;
    return MRP_OK;
}

/* where every entry's symbols lie in the device pool (behind the allele strings, in entry order), and every read's strand */
void AlignedFront::offsets_and_strands() {
    const int64_t n_ent = D.n_entries;
    y_off.resize((size_t) n_ent);
    int64_t at = allele_bytes;
    for (int64_t p = 0; p < n_ent; p++) { y_off[(size_t) p] = at; at += k_len[p]; }
    forward.resize((size_t) D.n_reads);
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) forward[(size_t) (D.read_first[c] + r)] = (chunks[c].flag[r] & 0x10) == 0;
}

/* on the host, from indices and lengths alone: the two pairs of every owner at an active site in ht_build_pairs' order (the model from
 * the owner's strand), and every read's entries in site order */
int HaRun::pairs() {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants, n_reads = D.n_reads;
    offsets_and_strands();
    std::vector<uint8_t> active((size_t) n_var, 0);
    P.pair_of.assign((size_t) n_ent, -1);
    first.assign((size_t) n_reads + 1, 0);
    int64_t n_active = 0, n_scored = 0, n_owners = 0, abase = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t g = D.variant_first[c] + v;
            if (gt[c][2 * v] == gt[c][2 * v + 1]) continue; /* bubbleGraph.c:1975 */
            int64_t k = 0;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++)
                if (k_owner[p] >= 0) { k++; first[(size_t) k_read[p] + 1]++; }
            if (!k) continue; /* :1989 */
            active[(size_t) g] = 1;
            n_active++;
            n_scored += k;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                if (k_owner[p] != p) continue;
                n_owners++;
                P.pair_of[(size_t) p] = P.list.size();
                for (int w = 0; w < 2; w++) { /* never anchored (:2027) */
                    const int64_t j = abase + C.allele_first[v] + gt[c][2 * v + w];
                    P.list.add(a_off[(size_t) j], a_len[(size_t) j], y_off[(size_t) p], (int32_t) k_len[p], forward[(size_t) k_read[p]] ? 0 : 1, nullptr);
                }
            }
        }
        abase += C.n_variants ? C.allele_first[C.n_variants] : 0;
    }
    for (int64_t r = 0; r < n_reads; r++) first[(size_t) r + 1] += first[(size_t) r];
    ent.resize((size_t) first[(size_t) n_reads]);
    std::vector<int64_t> fill(first.begin(), first.end() - 1);
    for (int64_t g = 0; g < n_var; g++) {
        if (!active[(size_t) g]) continue;
        for (int64_t p = k_first[g + 1] - 1; p >= k_first[g]; p--) { /* b->reads order (:2076) */
            if (k_owner[p] < 0) continue;
            const int64_t q = P.pair_of[(size_t) k_owner[p]];
            ent[(size_t) fill[(size_t) k_read[p]]++] = HtEntry{(int32_t) q, (int32_t) q + 1, 0, 0};
        }
    }
    if (stats) {
        stats->sites = n_var;
        stats->active_sites = n_active;
        stats->entries = n_scored;
        stats->owners = n_owners;
    }
    return MRP_OK;
}

/* the pair-HMM kernels over the pool that is already on the device, then a lane per read over its entries; the results on their way back */
int HaRun::score(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion) {
    const int64_t n_reads = D.n_reads;
    mrp_pairhmm_stats *pst = stats ? &stats->pairhmm : nullptr;
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    if (P.list.size() > 0) { /* (MRP_ERR_UNSUPPORTED for a diagonal beyond the limit is raised by phm_classify, before anything is launched) */
        int rc = phm_classify(who, models, 2, pool_bytes, P.list.view(), expansion, 0, 0, ctx->wide_pairs, H);
        if (rc == MRP_OK) rc = phm_enqueue(ctx, nullptr, pool_bytes, P.list.size(), H, L, pst, d_sym.p);
        if (rc != MRP_OK) return rc;
    } else {
        if (stats) PHM_HIP(hipStreamSynchronize(s));
        PHM_HIP(hipEventRecord(ctx->ev[0], s));
    }
    const int rc = ht_partition_enqueue(ctx, s, first, ent, L.d_out.p, n_reads, B);
    if (rc != MRP_OK) return rc;
    PHM_HIP(h_res.reserve(std::max<size_t>(20 * (size_t) n_reads, 1)));
    if (n_reads > 0) {
        PHM_HIP(hipMemcpyAsync(h_res.p, B.d_h.p, 16 * (size_t) n_reads, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync((uint8_t *) h_res.p + 16 * (size_t) n_reads, B.d_hap.p, 4 * (size_t) n_reads, hipMemcpyDeviceToHost, s));
    }
    PHM_HIP(hipStreamSynchronize(s));
    downloaded += 20 * n_reads;
    return MRP_OK;
}

/* after the stream has drained: the outputs per chunk, the stats, the device arrays back to the pool */
int HaRun::hand_over(int8_t *const *hap_out, double *const *h1_out, double *const *h2_out) {
    const int64_t n_reads = D.n_reads;
    const double *k_h1 = (const double *) h_res.p, *k_h2 = k_h1 + n_reads;
    const int32_t *k_hap = (const int32_t *) (k_h2 + n_reads);
    if (stats) {
        float ms = 0.f;
        PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        stats->pairhmm.kernel_ms = ms;
        stats->pairhmm.cells = H.cells;
        PHM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stats->owners_ms = ms;
        stats->bytes_downloaded = downloaded;
        const int rc = mrp_extract_run_stats(X);
        if (rc != MRP_OK) return rc;
        mrp_extract_run_times(X, false);
    }
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) {
            const int64_t g = D.read_first[c] + r;
            const bool kept = k_status[g] == MRP_READ_KEPT;
            hap_out[c][r] = kept ? (int8_t) k_hap[g] : (int8_t) -1;
            if (h1_out) h1_out[c][r] = kept ? k_h1[g] : 0.0;
            if (h2_out) h2_out[c][r] = kept ? k_h2[g] : 0.0;
        }
    arrays.release();
    B.arrays.release();
    L.arrays.release();
    mrp_extract_run_release(X); /* (reclaims the context's pool) */
    return MRP_OK;
}

}  // namespace

/* ---- the call in steps (mrp_internal.h): the checks, the device steps up to the owners, the scoring and the outputs */
struct mrp_haplotag_front {
    const mrp_haplotag_args a;
    HaRun R;
    mrp_haplotag_front(const mrp_haplotag_args &args, mrp_haplotag_aligned_stats *st) : a(args), R(nullptr, args.n_chunks, args.chunks, args.gt, st) {}
};

/* every check of the call that needs no context, in the one call's order; the extraction's run it leaves holds the windows */
int mrp_haplotag_front_create(const mrp_haplotag_args *a, mrp_haplotag_aligned_stats *stats, mrp_haplotag_front **front_out) {
    *front_out = nullptr;
    mrp_haplotag_front *A = new (std::nothrow) mrp_haplotag_front(*a, stats);
    if (!A) return mrp_set_error(MRP_ERR_NOMEM, "mrp_haplotag_aligned_chunks: out of host memory");
    const int rc = A->R.check(a->options, a->forward_model, a->reverse_model, a->expansion, a->hap_out, a->h1_out, a->h2_out, a->sv_split);
    if (rc != MRP_OK) {
        delete A;
        return rc;
    }
    *front_out = A;
    return MRP_OK;
}

void mrp_haplotag_front_destroy(mrp_haplotag_front *front) { delete front; }

int mrp_haplotag_chunks_check(const mrp_haplotag_args *a) {
    mrp_haplotag_front *A = nullptr;
    const int rc = mrp_haplotag_front_create(a, nullptr, &A);
    mrp_haplotag_front_destroy(A);
    return rc;
}

/* on ctx: the extraction gathering behind the allele strings, the owners of equal substrings; indices and lengths come back */
int mrp_haplotag_front_stage(mrp_context *ctx, mrp_haplotag_front *A) {
    HaRun &R = A->R;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction and the pair-HMM have no CPU fallback)", R.who);
    R.ctx = ctx;
    const int rc = R.extract();
    return rc == MRP_OK ? R.owners(nullptr) : rc;
}

/* the pair list, the pair-HMM (which raises the 2 048-cell refusal before it launches) and the scoring over a staged front, the outputs */
int mrp_haplotag_front_run(mrp_haplotag_front *A) {
    HaRun &R = A->R;
    const mrp_haplotag_args &a = A->a;
    int rc = R.pairs();
    if (rc == MRP_OK) rc = R.score(a.forward_model, a.reverse_model, a.expansion);
    if (rc == MRP_OK) rc = R.hand_over(a.hap_out, a.h1_out, a.h2_out);
    return rc;
}

extern "C" int mrp_haplotag_aligned_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const int32_t *const *gt,
                                           const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                           int64_t expansion, int8_t *const *hap_out, double *const *h1_out, double *const *h2_out,
                                           mrp_haplotag_aligned_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    const mrp_haplotag_args a{n_chunks, chunks, gt, options, forward_model, reverse_model, expansion, hap_out, h1_out, h2_out,
                              ctx ? ctx->sv_split : 0}; /* (a NULL context counts as off) */
    mrp_haplotag_front *A = nullptr;
    int rc = mrp_haplotag_front_create(&a, stats, &A);
    if (rc == MRP_OK) rc = mrp_haplotag_front_stage(ctx, A);
    if (rc == MRP_OK) rc = mrp_haplotag_front_run(A);
    mrp_haplotag_front_destroy(A);
    if (rc != MRP_OK) return rc;
    if (stats) stats->total_ms = now_ms() - t_begin;
    return MRP_OK;
}

/* ---- mrp_phase_aligned_chunks: the staged extraction, the owners kernel with the caller's mask, the k-mer anchors on the device
 * (mrp_anchors.hip) and the string call's run over the pool where it lies in HBM.  The host makes, from indices
 * and lengths alone, what mrp_string_chunk_from_extracted and mrp_string_front_create make from the downloaded symbols: every chunk's
 * mrp_string_chunk index arrays (offsets into the device pool), the owners' pairs in the front's order, and which pairs are anchored. */
namespace {

struct PaRun : AlignedFront {
    const char *const *const *const read_names;
    const uint8_t *const *const keep;
    mrp_phase_aligned_stats *const stats;
    struct ChunkArrays { /* what the mrp_string_chunk of a chunk points into */
        std::vector<int64_t> a_first{0}, a_off, s_first{0}, s_off, bubble_variant;
        std::vector<int32_t> a_len, s_len, s_read;
        std::vector<uint8_t> forward;
    };
    std::vector<ChunkArrays> arr;
    std::vector<mrp_string_chunk> sc;
    std::vector<int64_t> anchored; /* the pairs with a string longer than sv_threshold, ascending */
    std::vector<int64_t *> bv_out; /* the copies of bubble_variant the caller gets */
    mrp_string_front F;
    int64_t n_bubbles = 0, n_used = 0, n_owners = 0, n_anchors = 0, n_anchor_runs = 0;
    double anchors_ms = 0;
    /* the chunks of the call: all of the extraction's chunk records, or (with the filtered back half, PfRun) their first half -- the
     * second half are the same reads over the rests' variants */
    const int64_t n_front;
    std::vector<int64_t> entry_of_sub; /* with the back half: substring of the call -> its entry */
    /* the downsampling to maxDepth (mrp_context_set_downsampling): > 0 makes the mask on the device */
    int64_t max_depth = 0;
    uint64_t downsampling_seed = 0;
    hipEvent_t dev[2] = {nullptr, nullptr}; /* around its kernel */
    HostVec<MrpDsChunk> ds_chunks;
    DevBuf<MrpDsChunk> d_ds_chunks{arrays};
    DevBuf<int32_t> d_ds_flag{arrays};

    PaRun(const char *w, mrp_context *c, int64_t n, const mrp_aligned_chunk *ch, const char *const *const *names, const uint8_t *const *k,
          mrp_phase_aligned_stats *st, int64_t front)
        : AlignedFront(w, c, n, ch), read_names(names), keep(k), stats(st), n_front(front) {}
    ~PaRun() {
        if (s) (void) hipStreamSynchronize(s); /* before ds_chunks goes */
        for (hipEvent_t x : dev)
            if (x) (void) hipEventDestroy(x);
        for (int64_t *p : bv_out) free(p);
    }
    /* read r of chunk c passes the mask: the one made on the device, or the caller's */
    bool taken(int64_t c, int64_t r) const { return k_take ? k_take[D.read_first[c] + r] != 0 : (!keep || !keep[c] || keep[c][r]); }
    int check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
              const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, int sv_split);
    int masked_owners();
    int downsampled_owners();
    int strings_and_pairs(int64_t sv_threshold);
    int anchors();
    int classify(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion);
    int hand_over(int64_t **bubble_variant_out);
};

/* every MRP_ERR_ARG of the call (the extraction's, then the string call's parameter checks), then the two refused modes: nothing
 * here looks at the context (sv_split: its setting, 0 for none) */
int PaRun::check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                 const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, int sv_split) {
    const int rc = check_front(options, stats ? &stats->extract : nullptr,
                               !forward_model || !reverse_model || !params || (n_chunks > 0 && (!out || !hap_out || !read_names)), expansion);
    if (rc != MRP_OK) return rc;
    for (int64_t c = 0; c < n_front; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        if (C.n_reads == 0) continue;
        if (!hap_out[c] || (phred_out && !phred_out[c])) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output", who, (long long) c);
        if (!read_names[c]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null read names", who, (long long) c);
        for (int64_t r = 0; r < C.n_reads; r++)
            if (!read_names[c][r]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %lld has no name", who, (long long) c, (long long) r);
    }
    for (int64_t c = 0; max_depth > 0 && keep && c < n_front; c++)
        if (keep[c])
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: a keep mask while the downsampling is on (mrp_context_set_downsampling): the mask is made on the device",
                                 who, (long long) c);
    return mrp_extract_run_check_modes(X, sv_split);
}

/* the owners among the kept reads the caller's mask lets through (one byte per read of the call; no mask anywhere: none uploaded) */
int PaRun::masked_owners() {
    if (max_depth > 0) return downsampled_owners();
    bool any = n_front < n_chunks; /* (the second half's records take no part in the front) */
    for (int64_t c = 0; keep && c < n_front; c++) any = any || (keep[c] && chunks[c].n_reads > 0);
    if (!any) return owners(nullptr);
    HostVec<uint8_t> take((size_t) D.n_reads);
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) take[(size_t) (D.read_first[c] + r)] = c >= n_front ? 0 : (keep && keep[c] ? (keep[c][r] != 0) : 1);
    return owners(&take);
}

/* the mask of phase.c:360-382 made on the device, between the gather and the owners kernel: a workgroup per chunk of the front reads the
 * statuses, the per-read entry counts and the walk bounds where the extraction left them (nothing per read is uploaded: 40 B per chunk
 * are) and writes the bytes the owners kernel reads as `take`; the second half's records take no part and get 0 */
int PaRun::downsampled_owners() {
    const int64_t n_mask = D.read_first[n_front];
    ds_chunks.resize((size_t) n_front);
    for (int64_t c = 0; c < n_front; c++)
        ds_chunks[(size_t) c] = MrpDsChunk{D.read_first[c], chunks[c].n_reads, chunks[c].n_variants, chunks[c].overlap_start, chunks[c].overlap_end};
    for (hipEvent_t &x : dev) PHM_HIP(hipEventCreate(&x));
    PHM_HIP(d_ds_chunks.upload(ds_chunks, s));
    PHM_HIP(d_ds_flag.alloc((size_t) n_front));
    PHM_HIP(d_take.alloc((size_t) D.n_reads));
    if (D.n_reads > n_mask) PHM_HIP(hipMemsetAsync(d_take.p + n_mask, 0, (size_t) (D.n_reads - n_mask), s));
    PHM_HIP(hipEventRecord(dev[0], s));
    PHM_HIP(mrp_downsample_launch(s, n_front, d_ds_chunks.p, MrpDsIn{nullptr, nullptr, D.read_entry_first, D.read_limit, D.read_limit_stride}, D.read_status,
                                  max_depth, downsampling_seed, nullptr, d_take.p, d_ds_flag.p));
    PHM_HIP(hipEventRecord(dev[1], s));
    mask_reads = n_mask;
    mask_chunks = n_front;
    d_mask_flag = d_ds_flag.p;
    return owners(nullptr);
}

/* bubbleGraph_constructFromVCFAndBamChunkReadVcfEntrySubstrings (bubbleGraph.c:1338-1400) over the device pool: a variant with an entry
 * that takes part is a bubble, its substrings those entries in descending order (:1391-1393); then mrp_string_front_create's pair list:
 * chunk by chunk, bubble by bubble, the owners in listing order, an owner's pairs allele by allele, the owner's strand picking the model */
int PaRun::strings_and_pairs(int64_t sv_threshold) {
    offsets_and_strands();
    const int64_t n_chunks = n_front;
    const bool back = n_front < AlignedFront::n_chunks;
    arr.resize((size_t) n_chunks);
    sc.assign((size_t) n_chunks, mrp_string_chunk{});
    std::vector<int64_t> &sub_base = F.sub_base, &pair_first = F.pair_first;
    sub_base.assign((size_t) n_chunks + 1, 0);
    pair_first.clear();
    std::vector<int64_t> sub_of((size_t) D.n_entries, -1); /* entry -> its substring in the call */
    PhmPairList &pairs = F.scratch.pairs;
    int64_t abase = 0, n_subs = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        ChunkArrays &A = arr[(size_t) c];
        A.forward.assign(forward.begin() + D.read_first[c], forward.begin() + D.read_first[c + 1]);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t g = D.variant_first[c] + v;
            int64_t k = 0;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) k += k_owner[p] >= 0;
            if (!k) continue; /* :1366-1371 nothing to phase with */
            const int64_t na = C.allele_first[v + 1] - C.allele_first[v];
            if (na > 65535) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant %lld has more than 65535 alleles", who, (long long) c, (long long) v);
            const int64_t a0 = (int64_t) A.a_off.size();
            for (int64_t a = C.allele_first[v]; a < C.allele_first[v + 1]; a++) {
                A.a_off.push_back(a_off[(size_t) (abase + a)]);
                A.a_len.push_back(a_len[(size_t) (abase + a)]);
            }
            for (int64_t p = k_first[g + 1] - 1; p >= k_first[g]; p--) {
                if (k_owner[p] < 0) continue;
                sub_of[(size_t) p] = n_subs++;
                if (back) { /* what the back half's static front reads: a substring's owner and its entry */
                    F.scratch.owner.push_back(sub_of[(size_t) k_owner[p]]);
                    entry_of_sub.push_back(p);
                }
                /* the pair of the substring's owner with the bubble's allele 0 (the owner is listed before its duplicates) */
                pair_first.push_back(k_owner[p] == p ? pairs.size() : pair_first[(size_t) sub_of[(size_t) k_owner[p]]]);
                A.s_off.push_back(y_off[(size_t) p]);
                A.s_len.push_back((int32_t) k_len[p]);
                A.s_read.push_back((int32_t) (k_read[p] - D.read_first[c]));
                if (k_owner[p] != p) continue;
                n_owners++;
                const int model = forward[(size_t) k_read[p]] ? 0 : 1;
                for (int64_t j = 0; j < na; j++) {
                    const int32_t al = A.a_len[(size_t) (a0 + j)];
                    if (k_len[p] > sv_threshold || al > sv_threshold) anchored.push_back(pairs.size()); /* bubbleGraph.c:1448-1451 */
                    pairs.add(A.a_off[(size_t) (a0 + j)], al, y_off[(size_t) p], (int32_t) k_len[p], model, nullptr);
                }
            }
            A.bubble_variant.push_back(v);
            A.a_first.push_back((int64_t) A.a_off.size());
            A.s_first.push_back((int64_t) A.s_off.size());
        }
        abase += C.n_variants ? C.allele_first[C.n_variants] : 0;
        sub_base[(size_t) c + 1] = n_subs;
        mrp_string_chunk &S = sc[(size_t) c];
        S.n_bubbles = (int64_t) A.bubble_variant.size();
        S.n_reads = C.n_reads;
        S.pool = nullptr; /* the symbols are in HBM */
        S.pool_bytes = pool_bytes;
        S.allele_first = A.a_first.data();
        S.allele_off = A.a_off.data();
        S.allele_len = A.a_len.data();
        S.sub_first = A.s_first.data();
        S.sub_off = A.s_off.data();
        S.sub_len = A.s_len.data();
        S.sub_read = A.s_read.data();
        S.read_names = read_names[c];
        S.read_forward_strand = A.forward.data();
        n_bubbles += S.n_bubbles;
    }
    n_used = n_subs;
    if (pairs.size() >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    F.n_chunks = n_chunks;
    F.chunks = sc.data();
    F.n_subs = n_subs;
    F.n_pairs = pairs.size();
    F.device_pool = d_sym.p;
    F.device_pool_bytes = pool_bytes;
    return MRP_OK;
}

/* getKmerAlignmentAnchors of the anchored pairs, in the device pool; run counts and the anchors (as diagonal runs) come back and join
 * the pair list */
int PaRun::anchors() {
    PhmPairList &pairs = F.scratch.pairs;
    const int64_t n = (int64_t) anchored.size();
    if (n == 0) return MRP_OK;
    std::vector<int64_t> xo((size_t) n), yo((size_t) n), off((size_t) n + 1, 0), anc;
    std::vector<int32_t> xl((size_t) n), yl((size_t) n);
    for (int64_t i = 0; i < n; i++) {
        const size_t q = (size_t) anchored[(size_t) i];
        xo[(size_t) i] = pairs.x_off[q]; xl[(size_t) i] = pairs.x_len[q]; yo[(size_t) i] = pairs.y_off[q]; yl[(size_t) i] = pairs.y_len[q];
    }
    int64_t bytes = 0;
    const int rc = mrp_kmer_anchors_on_device(ctx, who, d_sym.p, n, xo.data(), xl.data(), yo.data(), yl.data(), off.data(), anc, &anchors_ms, &bytes, &n_anchor_runs);
    if (rc != MRP_OK) return rc;
    downloaded += bytes;
    n_anchors = off[(size_t) n];
    for (int64_t i = 0; i < n; i++) pairs.anchor_off[(size_t) anchored[(size_t) i] + 1] = off[(size_t) i + 1] - off[(size_t) i];
    pairs.counts_to_offsets();
    pairs.anchors = std::move(anc);
    return MRP_OK;
}

/* the launch classes and the bands; raises the 2 048-cell refusal (wide pairs on for the context: the wide kernel's caps), before any
 * pair-HMM kernel */
int PaRun::classify(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion) {
    if (F.n_pairs == 0) return MRP_OK;
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    return phm_classify(who, models, 2, pool_bytes, F.scratch.pairs.view(), expansion, 0, 0, ctx->wide_pairs, F.L);
}

/* after the string run has handed its results over: the bubbles' variants, the stats, the device arrays back to the pool */
int PaRun::hand_over(int64_t **bubble_variant_out) {
    mrp_downsampling_stats &ds = ctx->last_downsampling;
    ds = mrp_downsampling_stats{};
    if (max_depth > 0) {
        float ms = 0.f;
        PHM_HIP(hipEventElapsedTime(&ms, dev[0], dev[1]));
        ds.downsample_ms = ms;
        ds.chunks = n_front;
        for (int64_t c = 0; c < n_front; c++) {
            int32_t flag = 0;
            memcpy(&flag, k_flag + 4 * c, 4);
            ds.chunks_downsampled += flag != 0;
            for (int64_t r = 0; r < chunks[c].n_reads; r++) ds.reads_discarded += k_status[D.read_first[c] + r] == MRP_READ_KEPT && !taken(c, r);
        }
        ds.bytes_downloaded = mask_reads + 4 * mask_chunks;
    }
    if (stats) {
        float ms = 0.f;
        PHM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stats->owners_ms = ms;
        stats->anchors_ms = anchors_ms;
        stats->variants = D.n_variants;
        stats->bubbles = n_bubbles;
        stats->entries = D.n_entries;
        stats->entries_used = n_used;
        stats->owners = n_owners;
        stats->pairs = F.n_pairs;
        stats->pairs_anchored = (int64_t) anchored.size();
        stats->anchors = n_anchors;
        stats->anchor_runs = n_anchor_runs;
        stats->front_bytes_downloaded = downloaded;
        const int rc = mrp_extract_run_stats(X);
        if (rc != MRP_OK) return rc;
        mrp_extract_run_times(X, false);
    }
    if (bubble_variant_out)
        for (int64_t c = 0; c < n_front; c++) { bubble_variant_out[c] = bv_out[(size_t) c]; bv_out[(size_t) c] = nullptr; }
    arrays.release();
    mrp_extract_run_release(X); /* (reclaims the context's pool) */
    return MRP_OK;
}

/* ---- mrp_phase_aligned_chunks_with_filtered: mrp_phase_aligned_chunks with the back half of the chunk loop.
 * One staged extraction runs over 2 * n_chunks chunk records: record c is chunk c, record n_chunks + c the same reads over the rest's
 * variants (extractReadSubstringsAtVariantPositions called the second time, phase.c:354-357).  Both gathers land behind both sets of
 * allele strings in the call's one device pool.  The front is PaRun's, over the first half; ec_classes_kernel runs over the sites of
 * both halves, and from its representatives, the statuses and the entry indices the host makes what mrp_string_chunk_rest_from_extracted
 * makes from downloaded symbols -- every chunk's rest as index arrays into the device pool -- and the back half's static front
 * (sc_filtered_front, its classes by id).  The anchored pairs of both halves go through the anchors kernel in one launch. */
struct PfRun : PaRun {
    const int64_t n; /* chunks of the call */
    const mrp_aligned_chunk_rest *const rest; /* NULL: the plain call, no second half */
    struct RestArrays { /* what the mrp_string_chunk_rest of a chunk points into */
        std::vector<uint8_t> forward;
        std::vector<int64_t> f_first{0}, f_off, va_first{0}, va_off, ve_first{0}, ve_off;
        std::vector<int32_t> f_len, f_read, va_len, gt, ve_read, ve_len, filtered_read;
    };
    std::vector<RestArrays> ra;
    std::vector<mrp_string_chunk_rest> rs;
    std::vector<int32_t *> fr_out; /* the copies of filtered_read the caller gets */
    hipEvent_t cev[2] = {nullptr, nullptr}; /* around the classes kernel */
    DevBufGroup class_arrays;
    DevBuf<uint64_t> d_ckey{class_arrays};
    DevBuf<int32_t> d_rep{class_arrays};
    PinnedBuf h_rep;
    int64_t n_filtered_reads = 0;

    PfRun(const char *w, mrp_context *c, int64_t n_, const mrp_aligned_chunk *records, const mrp_aligned_chunk_rest *r, const char *const *const *names,
          const uint8_t *const *k, mrp_phase_aligned_stats *st)
        : PaRun(w, c, r ? 2 * n_ : n_, records, names, k, st, n_), n(n_), rest(r) {}
    ~PfRun() {
        if (s) (void) hipStreamSynchronize(s); /* before the pinned buffer goes */
        for (hipEvent_t x : cev)
            if (x) (void) hipEventDestroy(x);
        for (int32_t *p : fr_out) free(p);
    }
    int check_rest() const;
    int classes();
    int rests();
    int filtered_front(int64_t sv_threshold);
    int record_sites();
    int records(mrp_phase_result *const *out, mrp_variant_records *records_out, mrp_phase_aligned_records_stats *rstats);
};

/* the rest's own MRP_ERR_ARG (its variants have passed the extraction's checks as the second half's records) */
int PfRun::check_rest() const {
    for (int64_t c = 0; c < n; c++) {
        const mrp_aligned_chunk_rest &R = rest[c];
        if (R.n_variants > 0 && !R.gt) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null genotypes of the rest", who, (long long) c);
        for (int64_t v = 0; v < R.n_variants; v++) {
            const int64_t k = R.allele_first[v + 1] - R.allele_first[v];
            for (int w = 0; w < 2; w++)
                if (R.gt[2 * v + w] < 0 || R.gt[2 * v + w] >= k)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, filtered variant %lld: genotype %d outside its %lld alleles", who, (long long) c,
                                         (long long) v, R.gt[2 * v + w], (long long) k);
        }
    }
    return MRP_OK;
}

/* the classes of equal substrings at the sites of both halves, queued behind the gather; 4 B per entry start on their way back (the
 * owners' wait covers them) */
int PfRun::classes() {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants;
    class_arrays.bind(&ctx->pool);
    for (hipEvent_t &x : cev) PHM_HIP(hipEventCreate(&x));
    PHM_HIP(d_ckey.alloc((size_t) n_ent));
    PHM_HIP(d_rep.alloc((size_t) n_ent));
    PHM_HIP(h_rep.reserve(std::max<size_t>(4 * (size_t) n_ent, 1)));
    PHM_HIP(hipEventRecord(cev[0], s));
    if (n_ent > 0) {
        hipLaunchKernelGGL(ec_classes_kernel<int64_t>, dim3((unsigned) std::min<int64_t>(n_var, 65536)), dim3(PHM_WAVE), 0, s, D.entry_first, n_var, D.entry_len,
                           D.entry_off, D.symbols, d_ckey.p, d_rep.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(cev[1], s));
    if (n_ent > 0) PHM_HIP(hipMemcpyAsync(h_rep.p, d_rep.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
    downloaded += 4 * n_ent;
    return MRP_OK;
}

/* mrp_string_chunk_rest_from_extracted over what came back: statuses, entry indices, lengths and representatives (the rules and their
 * reference lines are in include/margin_rphmm.h); offsets are into the device pool */
int PfRun::rests() {
    const int32_t *k_rep = (const int32_t *) h_rep.p;
    mrp_string_front::Scratch &X = F.scratch;
    ra.resize((size_t) n);
    rs.assign((size_t) n, mrp_string_chunk_rest{});
    X.fsub_cls.resize((size_t) n);
    X.ventry_cls.resize((size_t) n);
    X.sub_cls.resize(entry_of_sub.size());
    for (size_t k = 0; k < entry_of_sub.size(); k++) X.sub_cls[k] = k_rep[entry_of_sub[k]];
    int64_t abase = 0;
    for (int64_t c = 0; c < n; c++) abase += chunks[c].n_variants ? chunks[c].allele_first[chunks[c].n_variants] : 0;
    for (int64_t c = 0; c < n; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        const mrp_aligned_chunk_rest &Rc = rest[c];
        RestArrays &A = ra[(size_t) c];
        const int64_t nr = C.n_reads, nv = Rc.n_variants, r1 = D.read_first[c], r2 = D.read_first[n + c];
        auto primary = [&](int64_t r) { return k_status[r1 + r] == MRP_READ_KEPT && taken(c, r); };
        auto kind = [&](int64_t r) {
            if (k_status[r1 + r] == MRP_READ_FILTERED) return 0;
            if (k_status[r1 + r] == MRP_READ_KEPT) return primary(r) ? -1 : 1;
            return k_status[r2 + r] == MRP_READ_KEPT ? 2 : -1;
        };
        int64_t n_kind[3] = {0, 0, 0};
        for (int64_t r = 0; r < nr; r++) {
            const int k = kind(r);
            if (k >= 0) n_kind[k]++;
        }
        const int64_t nf = n_kind[0] + n_kind[1] + n_kind[2];
        n_filtered_reads += nf;
        if (nf == 0 && nv == 0) continue; /* the empty rest */
        std::vector<int32_t> findex((size_t) nr, -1);
        A.filtered_read.resize((size_t) nf);
        A.forward.resize((size_t) nf);
        int64_t at[3] = {0, n_kind[0], n_kind[0] + n_kind[1]};
        for (int64_t r = 0; r < nr; r++) {
            const int k = kind(r);
            if (k < 0) continue;
            findex[(size_t) r] = (int32_t) at[k]++;
            A.filtered_read[(size_t) findex[(size_t) r]] = (int32_t) r;
            A.forward[(size_t) findex[(size_t) r]] = forward[(size_t) (r1 + r)];
        }
        std::vector<int64_t> &fcls = X.fsub_cls[(size_t) c], &vcls = X.ventry_cls[(size_t) c];
        for (int64_t v : arr[(size_t) c].bubble_variant) {
            const int64_t g = D.variant_first[c] + v;
            for (int pass = 0; pass < 2; pass++)
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                    const int64_t r = k_read[p] - r1;
                    if (kind(r) != pass) continue;
                    A.f_off.push_back(y_off[(size_t) p]);
                    A.f_len.push_back((int32_t) k_len[p]);
                    A.f_read.push_back(findex[(size_t) r]);
                    fcls.push_back(k_rep[p]);
                }
            A.f_first.push_back((int64_t) A.f_off.size());
        }
        for (int64_t v = 0; v < nv; v++) {
            const int64_t g = D.variant_first[n + c] + v;
            for (int64_t a = Rc.allele_first[v]; a < Rc.allele_first[v + 1]; a++) {
                A.va_off.push_back(a_off[(size_t) (abase + a)]);
                A.va_len.push_back(a_len[(size_t) (abase + a)]);
            }
            A.va_first.push_back((int64_t) A.va_off.size());
            A.gt.push_back(Rc.gt[2 * v]);
            A.gt.push_back(Rc.gt[2 * v + 1]);
            if (Rc.variant_pos[v] >= C.chunk_start && Rc.variant_pos[v] < C.chunk_end) /* bubbleGraph.c:2179 */
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                    const int64_t r = k_read[p] - r2;
                    if (k_status[r2 + r] != MRP_READ_KEPT) continue;
                    A.ve_read.push_back(primary(r) ? (int32_t) r : (int32_t) (nr + findex[(size_t) r]));
                    A.ve_off.push_back(y_off[(size_t) p]);
                    A.ve_len.push_back((int32_t) k_len[p]);
                    vcls.push_back(k_rep[p]);
                }
            A.ve_first.push_back((int64_t) A.ve_off.size());
        }
        abase += nv ? Rc.allele_first[nv] : 0;
        mrp_string_chunk_rest &R = rs[(size_t) c];
        R.n_filtered = nf;
        R.forward_strand = A.forward.data();
        R.pool = nullptr; /* the symbols are in HBM */
        R.pool_bytes = pool_bytes;
        R.fsub_first = A.f_first.data();
        R.fsub_off = A.f_off.data();
        R.fsub_len = A.f_len.data();
        R.fsub_read = A.f_read.data();
        R.n_variants = nv;
        R.valle_first = A.va_first.data();
        R.valle_off = A.va_off.data();
        R.valle_len = A.va_len.data();
        R.gt = A.gt.data();
        R.ventry_first = A.ve_first.data();
        R.ventry_read = A.ve_read.data();
        R.ventry_off = A.ve_off.data();
        R.ventry_len = A.ve_len.data();
    }
    return MRP_OK;
}

/* the back half's static front from indices and classes alone; its pairs past sv_threshold join the front's anchored list */
int PfRun::filtered_front(int64_t sv_threshold) {
    F.pool_base.assign((size_t) n + 1, 0); /* every offset is the device pool's already */
    F.scratch.classes_by_id = true;
    const std::vector<int64_t> rpool_base((size_t) n, 0);
    const int rc = sc_filtered_front(&F, rs.data(), sv_threshold, rpool_base);
    if (rc != MRP_OK) return rc;
    anchored.insert(anchored.end(), F.scratch.anchored_new.begin(), F.scratch.anchored_new.end());
    return MRP_OK;
}

/* the records' site table: every variant of both halves, with a slot per entry of a primary read where the
 * site can be updated at all -- a primary variant with a bubble and a position inside the chunk (vcf.c:538-540), a filtered variant
 * inside the chunk (bubbleGraph.c:2179); the kernel reads the entries where the extraction left them */
int PfRun::record_sites() {
    mrp_string_front::Records &Q = F.rec;
    Q.on = true;
    Q.read_first.assign(D.read_first, D.read_first + n + 1);
    Q.entry_first = D.entry_first;
    Q.entry_read = D.entry_read;
    Q.read_status = D.read_status;
    Q.take = d_take.p;
    Q.sites.resize((size_t) D.n_variants);
    int64_t slots = 0;
    for (int64_t c = 0; c < n; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        const mrp_aligned_chunk_rest &Rc = rest[c];
        const int64_t r1 = D.read_first[c], r2 = D.read_first[n + c];
        auto primary = [&](int64_t r) { return k_status[r1 + r] == MRP_READ_KEPT && taken(c, r); };
        std::vector<int32_t> bubble_of((size_t) C.n_variants, -1);
        const std::vector<int64_t> &bv = arr[(size_t) c].bubble_variant;
        for (size_t b = 0; b < bv.size(); b++) bubble_of[(size_t) bv[b]] = (int32_t) b;
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t g = D.variant_first[c] + v;
            const bool inside = C.variant_pos[v] >= C.chunk_start && C.variant_pos[v] < C.chunk_end;
            RcSite st{g, slots, 0, (int32_t) c, inside ? bubble_of[(size_t) v] : -1, -1, 0, 0, 0, (int32_t) r1};
            if (st.bubble >= 0)
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) st.n_slots += primary(k_read[p] - r1);
            slots += st.n_slots;
            Q.sites[(size_t) g] = st;
        }
        for (int64_t v = 0; v < Rc.n_variants; v++) {
            const int64_t g = D.variant_first[n + c] + v;
            RcSite st{g, slots, 0, (int32_t) c, -1, (int32_t) (F.fil.var_base[(size_t) c] + v), Rc.gt[2 * v], Rc.gt[2 * v + 1], (int32_t) (r2 - r1), (int32_t) r1};
            if (Rc.variant_pos[v] >= C.chunk_start && Rc.variant_pos[v] < C.chunk_end)
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) st.n_slots += k_status[k_read[p]] == MRP_READ_KEPT && primary(k_read[p] - r2);
            slots += st.n_slots;
            Q.sites[(size_t) g] = st;
        }
    }
    Q.n_slots = slots;
    if (slots >= (1ll << 31) || D.n_reads >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 reads or list slots in one call", who);
    return MRP_OK;
}

/* the records per chunk from what the kernel brought back; the log values are the fragment's own floats (vcf.c:527-529), a filtered
 * record's -INFINITY (probability 0, bubbleGraph.c:2300-2302) */
int PfRun::records(mrp_phase_result *const *out, mrp_variant_records *records_out, mrp_phase_aligned_records_stats *rstats) {
    const mrp_string_front::Records &Q = F.rec;
    int64_t n_updated = 0, n_listed = 0;
    bool ok = true;
    for (size_t g = 0; g < Q.sites.size(); g++) { /* (before anything is handed over) */
        const RcOut &o = Q.out[g];
        if (o.n_hap1 < 0 || o.n_hap2 < 0 || (int64_t) o.n_hap1 + o.n_hap2 > Q.sites[g].n_slots)
            return mrp_set_error(MRP_ERR_HIP, "%s: site %lld: the records kernel listed %d + %d reads in %d slots", who, (long long) g, o.n_hap1, o.n_hap2,
                                 Q.sites[g].n_slots);
    }
    for (int64_t c = 0; c < n && ok; c++) {
        const int64_t np = chunks[c].n_variants, nv = rest[c].n_variants, ns = np + nv;
        int64_t listed = 0;
        for (int64_t i = 0; i < ns; i++) {
            const RcOut &o = Q.out[(size_t) (i < np ? D.variant_first[c] + i : D.variant_first[n + c] + (i - np))];
            listed += o.n_hap1 + o.n_hap2;
        }
        mrp_variant_records &R = records_out[c];
        const size_t m = (size_t) std::max<int64_t>(ns, 1);
        R.n_primary = np;
        R.n_filtered = nv;
        R.state = (uint8_t *) calloc(m, 1);
        R.gt = (int32_t *) calloc(2 * m, 4);
        R.genotype_log_prob = (float *) calloc(m, 4);
        R.hap1_log_prob = (float *) calloc(m, 4);
        R.hap2_log_prob = (float *) calloc(m, 4);
        R.read_first = (int64_t *) calloc((size_t) ns + 1, 8);
        R.n_hap1 = (int32_t *) calloc(m, 4);
        R.n_hap2 = (int32_t *) calloc(m, 4);
        R.reads = (int32_t *) calloc((size_t) std::max<int64_t>(listed, 1), 4);
        ok = R.state && R.gt && R.genotype_log_prob && R.hap1_log_prob && R.hap2_log_prob && R.read_first && R.n_hap1 && R.n_hap2 && R.reads;
        if (!ok) break;
        const mrp_phase_result *gf = out[c];
        int64_t at = 0;
        for (int64_t i = 0; i < ns; i++) {
            const int64_t g = i < np ? D.variant_first[c] + i : D.variant_first[n + c] + (i - np);
            const RcOut &o = Q.out[(size_t) g];
            const RcSite &st = Q.sites[(size_t) g];
            R.state[i] = (uint8_t) o.state;
            R.gt[2 * i] = o.gt1;
            R.gt[2 * i + 1] = o.gt2;
            R.n_hap1[i] = o.n_hap1;
            R.n_hap2[i] = o.n_hap2;
            if (i >= np && o.state != MRP_RECORD_UNTOUCHED) R.genotype_log_prob[i] = R.hap1_log_prob[i] = R.hap2_log_prob[i] = -INFINITY;
            if (i < np && o.state == MRP_RECORD_UPDATED) {
                const int64_t j = st.bubble - gf->ref_start;
                R.genotype_log_prob[i] = gf->genotype_probs[j];
                R.hap1_log_prob[i] = gf->haplotype_probs1[j];
                R.hap2_log_prob[i] = gf->haplotype_probs2[j];
            }
            const int32_t *sl = Q.slots.data() + st.slot_first;
            for (int32_t q = 0; q < o.n_hap1; q++) R.reads[at++] = sl[q];
            for (int32_t q = 0; q < o.n_hap2; q++) R.reads[at++] = sl[st.n_slots - o.n_hap2 + q];
            R.read_first[i + 1] = at;
            n_updated += o.state == MRP_RECORD_UPDATED;
        }
        n_listed += listed;
    }
    if (!ok) {
        for (int64_t c = 0; c < n; c++) mrp_variant_records_clear(&records_out[c]);
        return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    }
    if (rstats) {
        rstats->records_sites = (int64_t) Q.sites.size();
        rstats->records_updated = n_updated;
        rstats->reads_listed = n_listed;
        rstats->records_bytes_downloaded = (int64_t) (sizeof(RcOut) * Q.sites.size()) + 4 * Q.n_slots;
        rstats->records_ms = Q.ms;
    }
    return MRP_OK;
}

}  // namespace

/* ---- the two entries in steps (mrp_internal.h): the checks, the device steps up to the launch classes, the string run ------------
 * rest, filtered_out and filtered_read_out are NULL for the plain call, whose extraction records are its chunks. */
static std::vector<mrp_aligned_chunk> pa_records(const mrp_aligned_args &a) {
    std::vector<mrp_aligned_chunk> records;
    if (!a.rest || !a.chunks || a.n_chunks <= 0) return records;
    const int64_t n_chunks = a.n_chunks;
    /* the extraction's chunk records: the chunks, then the same reads over the rests' variants */
    records.resize((size_t) (2 * n_chunks));
    for (int64_t c = 0; c < n_chunks; c++) {
        records[(size_t) c] = a.chunks[c];
        mrp_aligned_chunk &R = records[(size_t) (n_chunks + c)];
        R = a.chunks[c];
        R.n_variants = a.rest[c].n_variants;
        R.variant_pos = a.rest[c].variant_pos;
        R.allele_first = a.rest[c].allele_first;
        R.allele_off = a.rest[c].allele_off;
        R.allele_len = a.rest[c].allele_len;
        R.allele_chars = a.rest[c].allele_chars;
        R.allele_bytes = a.rest[c].allele_bytes;
        R.is_sv = a.rest[c].is_sv;
    }
    return records;
}

struct mrp_aligned_front {
    const mrp_aligned_args a;
    const double t_begin;
    mrp_phase_aligned_stats *const stats;
    mrp_phase_aligned_filtered_stats *const fstats;
    const std::vector<mrp_aligned_chunk> records;
    PfRun R;
    mrp_aligned_front(const char *who, double t0, const mrp_aligned_args &args, mrp_phase_aligned_stats *st, mrp_phase_aligned_filtered_stats *fst)
        : a(args), t_begin(t0), stats(st), fstats(fst), records(pa_records(args)),
          R(who, nullptr, args.n_chunks, args.rest ? records.data() : args.chunks, args.rest, args.read_names, args.keep, st) {
        R.max_depth = args.max_depth;
        R.downsampling_seed = args.downsampling_seed;
    }
};

/* every check of the call that needs no context, in the one call's order (every MRP_ERR_ARG comes before the refused modes); the
 * extraction's run it leaves holds the windows */
int mrp_aligned_front_create(const char *who, double t_begin, const mrp_aligned_args *a, mrp_phase_aligned_stats *stats,
                             mrp_phase_aligned_filtered_stats *fstats, mrp_aligned_front **front_out) {
    *front_out = nullptr;
    mrp_aligned_front *A = new (std::nothrow) mrp_aligned_front(who, t_begin, *a, stats, fstats);
    if (!A) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int rc = A->R.check(a->options, a->forward_model, a->reverse_model, a->expansion, a->params, a->out, a->hap_out, a->phred_out, a->sv_split);
    if (a->rest && (rc == MRP_OK || rc == MRP_ERR_UNSUPPORTED)) {
        const int rc2 = A->R.check_rest();
        if (rc2 != MRP_OK) rc = rc2;
    }
    if (rc != MRP_OK) {
        delete A;
        return rc;
    }
    *front_out = A;
    return MRP_OK;
}

void mrp_aligned_front_destroy(mrp_aligned_front *front) { delete front; }

int mrp_aligned_chunks_check(const char *who, const mrp_aligned_args *a) {
    mrp_aligned_front *A = nullptr;
    const int rc = mrp_aligned_front_create(who, now_ms(), a, nullptr, nullptr, &A);
    mrp_aligned_front_destroy(A);
    return rc;
}

/* on ctx, up to the launch classes: extraction, classes, owners, the pair list, the rests, the anchors; raises the 2 048-cell refusal */
int mrp_aligned_front_stage(mrp_context *ctx, mrp_aligned_front *A) {
    PfRun &R = A->R;
    const mrp_aligned_args &a = A->a;
    const bool rest = a.rest != nullptr;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction and the pair-HMM have no CPU fallback)", R.who);
    R.ctx = ctx;
    int rc = R.extract();
    if (rc == MRP_OK && rest) rc = R.classes();
    if (rc == MRP_OK) rc = R.masked_owners();
    if (rc == MRP_OK) rc = R.strings_and_pairs(a.sv_threshold);
    if (rc == MRP_OK && rest) rc = R.rests();
    if (rc == MRP_OK && rest) rc = R.filtered_front(a.sv_threshold);
    if (rc == MRP_OK && rest && a.records_out) rc = R.record_sites();
    if (rc == MRP_OK) rc = R.anchors();
    if (rc == MRP_OK) rc = R.classify(a.forward_model, a.reverse_model, a.expansion);
    return rc;
}

/* the string run over a staged front, and the per-chunk lists; chunk_stats: NULL, or where the string run's stats go when the front
 * has no stats of its own (the work queue counts the per-chunk path's chunks from them) */
int mrp_aligned_front_run(mrp_aligned_front *A, mrp_string_chunks_stats *chunk_stats) {
    PfRun &R = A->R;
    const mrp_aligned_args &a = A->a;
    const char *who = R.who;
    mrp_context *ctx = R.ctx;
    const int64_t n_chunks = a.n_chunks;
    const bool rest = a.rest != nullptr;
    mrp_phase_aligned_stats *stats = A->stats;
    mrp_phase_aligned_filtered_stats *fstats = A->fstats;
    int rc = MRP_OK;
    /* (made before anything is handed over: an error returns nothing) */
    if (rest) R.fr_out.assign((size_t) n_chunks, nullptr);
    if (a.bubble_variant_out) R.bv_out.assign((size_t) n_chunks, nullptr);
    for (int64_t c = 0; c < n_chunks; c++) {
        if (rest) {
            std::vector<int32_t> fr = R.ra[(size_t) c].filtered_read;
            fr.push_back(-1); /* the end of the list */
            R.fr_out[(size_t) c] = (int32_t *) sc_dup(fr.data(), sizeof(int32_t) * fr.size());
            if (!R.fr_out[(size_t) c]) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
        }
        if (!a.bubble_variant_out) continue;
        std::vector<int64_t> bv = R.arr[(size_t) c].bubble_variant;
        bv.push_back(-1); /* the end of the list: the caller has no other way to the bubble count */
        R.bv_out[(size_t) c] = (int64_t *) sc_dup(bv.data(), sizeof(int64_t) * bv.size());
        if (!R.bv_out[(size_t) c]) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t c = 0; c < n_chunks; c++) a.out[c] = nullptr;
    if (a.profiles_out && n_chunks > 0) memset(a.profiles_out, 0, sizeof(*a.profiles_out) * (size_t) n_chunks);
    mrp_string_filtered_stats fst;
    memset(&fst, 0, sizeof(fst));
    if (n_chunks > 0) {
        /* the rest of the string call unchanged: pair-HMM over the device pool, layout beside it, profile bytes, phasing, HP tags */
        R.F.front_ms = now_ms() - A->t_begin;
        rc = mrp_string_front_run(ctx, &R.F, a.het_substitution_probability, a.params, a.min_phred, a.out, a.hap_out, a.phred_out, a.profiles_out,
                                  stats ? &stats->chunks : chunk_stats, a.filtered_out, fstats ? &fst : nullptr);
        if (rc != MRP_OK) return rc;
        if (a.records_out) {
            rc = R.records(a.out, a.records_out, a.records_stats);
            if (rc != MRP_OK) { /* an error returns nothing: what the string run handed over goes back */
                for (int64_t c = 0; c < n_chunks; c++) {
                    mrp_phase_result_destroy(a.out[c]);
                    a.out[c] = nullptr;
                    if (a.profiles_out) mrp_profile_out_clear(&a.profiles_out[c]);
                    mrp_filtered_out_clear(&a.filtered_out[c]);
                }
                return rc;
            }
        }
    }
    if (fstats) {
        float ms = 0.f;
        if (R.cev[1]) PHM_HIP(hipEventElapsedTime(&ms, R.cev[0], R.cev[1]));
        fstats->classes_ms = ms;
        fstats->filtered_ms = fst.filtered_ms;
        fstats->pairs_scored = fst.pairs_scored;
        fstats->pairs_speculative = fst.pairs_speculative;
        fstats->pairs_read_by_results = fst.pairs_read_by_results;
        fstats->filtered_variants = R.D.n_variants - R.D.variant_first[n_chunks];
        fstats->filtered_reads = R.n_filtered_reads;
        fstats->filtered_entries = R.D.n_entries - (n_chunks > 0 ? R.k_first[R.D.variant_first[n_chunks]] : 0);
    }
    rc = R.hand_over(a.bubble_variant_out);
    if (rc != MRP_OK) return rc;
    if (rest) {
        R.class_arrays.release();
        ctx->pool.reclaim();
        for (int64_t c = 0; c < n_chunks; c++) { a.filtered_read_out[c] = R.fr_out[(size_t) c]; R.fr_out[(size_t) c] = nullptr; }
    }
    if (stats) stats->total_ms = now_ms() - A->t_begin;
    return MRP_OK;
}

/* What the two entries share: front, stage, run, destroy */
static int pa_phase_chunks(const char *who, double t_begin, mrp_context *ctx, const mrp_aligned_args &a, mrp_phase_aligned_stats *stats,
                           mrp_phase_aligned_filtered_stats *fstats) {
    mrp_aligned_front *A = nullptr;
    int rc = mrp_aligned_front_create(who, t_begin, &a, stats, fstats, &A);
    if (rc == MRP_OK) rc = mrp_aligned_front_stage(ctx, A);
    if (rc == MRP_OK) rc = mrp_aligned_front_run(A, nullptr);
    mrp_aligned_front_destroy(A);
    return rc;
}

extern "C" int mrp_phase_aligned_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const char *const *const *read_names,
                                        const uint8_t *const *keep, const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                        const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                                        const mrp_params *params, int64_t min_phred, mrp_phase_result **out, int8_t *const *hap_out,
                                        double *const *phred_out, mrp_profile_out *profiles_out, int64_t **bubble_variant_out,
                                        mrp_phase_aligned_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    const mrp_aligned_args a{n_chunks, chunks, nullptr, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                             het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, nullptr, nullptr,
                             ctx ? ctx->sv_split : 0, nullptr, nullptr, ctx ? ctx->max_depth : 0, ctx ? ctx->downsampling_seed : 0}; /* (a NULL context counts as off) */
    return pa_phase_chunks("mrp_phase_aligned_chunks", t_begin, ctx, a, stats, nullptr);
}

extern "C" int mrp_phase_aligned_chunks_with_records(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                     const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                     const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                     int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                     mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                                     int64_t **bubble_variant_out, mrp_filtered_out *filtered_out, int32_t **filtered_read_out,
                                                     mrp_variant_records *records_out, mrp_phase_aligned_records_stats *stats) {
    static const char *who = "mrp_phase_aligned_chunks_with_records";
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks < 0 || n_chunks >= (1ll << 30) || (n_chunks > 0 && (!chunks || !rest || !filtered_out || !filtered_read_out || !records_out)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (n_chunks > 0) {
        memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
        memset(records_out, 0, sizeof(*records_out) * (size_t) n_chunks);
    }
    const mrp_aligned_args a{n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                             het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                             filtered_read_out, ctx ? ctx->sv_split : 0, records_out, stats, ctx ? ctx->max_depth : 0, ctx ? ctx->downsampling_seed : 0};
    return pa_phase_chunks(who, t_begin, ctx, a, stats ? &stats->filtered.aligned : nullptr, stats ? &stats->filtered : nullptr);
}

extern "C" int mrp_phase_aligned_chunks_with_filtered(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                      const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                      const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                      int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                      mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                                      int64_t **bubble_variant_out, mrp_filtered_out *filtered_out, int32_t **filtered_read_out,
                                                      mrp_phase_aligned_filtered_stats *stats) {
    static const char *who = "mrp_phase_aligned_chunks_with_filtered";
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks < 0 || n_chunks >= (1ll << 30) || (n_chunks > 0 && (!chunks || !rest || !filtered_out || !filtered_read_out)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    const mrp_aligned_args a{n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                             het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                             filtered_read_out, ctx ? ctx->sv_split : 0, nullptr, nullptr, ctx ? ctx->max_depth : 0, ctx ? ctx->downsampling_seed : 0};
    return pa_phase_chunks(who, t_begin, ctx, a, stats ? &stats->aligned : nullptr, stats);
}
