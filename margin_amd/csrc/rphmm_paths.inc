/*
 * rphmm_paths.inc -- the interval logic of coordination.c (stRPHmm_cmpFn, getTilingPaths, getOverlappingComponents) over
 * any hmm type that has ref_start and ref_length; included by rphmm_chunk.c for the flat host hmm (struct mrp_hmm) and by
 * rphmm_host.c for the compact shadows of the device-resident merge (struct rhmm).  Parameters:
 *     HMM_T            the hmm type
 *     PFX(name)        prefix of the generated names
 *     H_NAME_READ(h)   index of the read whose name breaks ties (first read of the hmm), -1 if it has none
 */

/* stRPHmm_cmpFn hmm.c:67-95 (single reference per chunk; pointer tie-break -> creation order) */
static int PFX(hmm_cmp)(const world *w, const HMM_T *a, const HMM_T *b) {
    if (a->ref_start != b->ref_start) return a->ref_start > b->ref_start ? 1 : -1;
    if (a->ref_length != b->ref_length) return b->ref_length > a->ref_length ? 1 : -1;
    const int32_t ra = H_NAME_READ(a), rb = H_NAME_READ(b);
    if (ra >= 0 && rb >= 0) {
        int i = strcmp(w->reads[ra].name, w->reads[rb].name);
        if (i != 0) return i;
    }
    return a > b ? 1 : (a < b ? -1 : 0);
}
static int PFX(hmm_overlap)(const HMM_T *a, const HMM_T *b) { /* hmm.c:1165-1190 */
    if (a->ref_start > b->ref_start) return PFX(hmm_overlap)(b, a);
    return a->ref_start + a->ref_length > b->ref_start;
}

typedef VEC(HMM_T *) PFX(hmm_vec);

static __thread const world *PFX(t_sort_world); /* qsort context of the calling thread */
static int PFX(hmm_cmp_qsort)(const void *a, const void *b) {
    return PFX(hmm_cmp)(PFX(t_sort_world), *(HMM_T *const *) a, *(HMM_T *const *) b);
}
static void PFX(sort_hmms)(const world *w, HMM_T **a, int64_t n) {
    {   /* a merged tiling path comes out of getOverlappingComponents in order, or nearly so: look before sorting */
        int64_t i = 1;
        while (i < n && (a[i - 1]->ref_start < a[i]->ref_start || PFX(hmm_cmp)(w, a[i - 1], a[i]) <= 0)) i++;
        if (i >= n) return;
    }
    if (n <= 24) { /* the members of an overlap component, a merged path: a handful -- insertion sort (stRPHmm_cmpFn is a total order) */
        for (int64_t i = 1; i < n; i++) {
            HMM_T *x = a[i];
            int64_t j = i;
            while (j > 0 && PFX(hmm_cmp)(w, a[j - 1], x) > 0) { a[j] = a[j - 1]; j--; }
            a[j] = x;
        }
        return;
    }
    /* Many (the leaves of a chunk): LSD radix sort on (refStart ascending, refLength descending) = the first two criteria of
     * stRPHmm_cmpFn in one 64-bit key, then the full comparison inside runs of equal keys (name, then address): rare. */
    typedef struct { uint64_t key; HMM_T *h; } PFX(keyed_hmm);
    PFX(keyed_hmm) *x = xmalloc(sizeof(*x) * (size_t) n * 2), *y = x + n;
    uint32_t max_start = 0, max_len = 0;
    for (int64_t i = 0; i < n; i++) {
        if ((uint32_t) a[i]->ref_start > max_start) max_start = (uint32_t) a[i]->ref_start;
        if ((uint32_t) a[i]->ref_length > max_len) max_len = (uint32_t) a[i]->ref_length;
    }
    for (int64_t i = 0; i < n; i++) { x[i].key = ((uint64_t) (uint32_t) a[i]->ref_start << 32) | (uint64_t) (max_len - (uint32_t) a[i]->ref_length); x[i].h = a[i]; }
    int bits_lo = 1, bits_hi = 1;
    while (bits_lo < 32 && (max_len >> bits_lo) != 0) bits_lo++;
    while (bits_hi < 32 && (max_start >> bits_hi) != 0) bits_hi++;
    for (int half = 0; half < 2; half++) { /* low word (length), then high word (start): 11 bits per pass */
        const int bits = half ? bits_hi : bits_lo, base = half ? 32 : 0;
        for (int sh = 0; sh < bits; sh += 11) {
            int64_t cnt[2049] = {0};
            for (int64_t i = 0; i < n; i++) cnt[((x[i].key >> (base + sh)) & 2047u) + 1]++;
            for (int q = 0; q < 2048; q++) cnt[q + 1] += cnt[q];
            for (int64_t i = 0; i < n; i++) y[cnt[(x[i].key >> (base + sh)) & 2047u]++] = x[i];
            PFX(keyed_hmm) *t = x; x = y; y = t;
        }
    }
    for (int64_t i = 0; i < n;) { /* ties */
        int64_t j = i + 1;
        while (j < n && x[j].key == x[i].key) j++;
        for (int64_t p = i + 1; p < j; p++) {
            PFX(keyed_hmm) v = x[p];
            int64_t q = p;
            while (q > i && PFX(hmm_cmp)(w, x[q - 1].h, v.h) > 0) { x[q] = x[q - 1]; q--; }
            x[q] = v;
        }
        i = j;
    }
    for (int64_t i = 0; i < n; i++) a[i] = x[i].h;
    free(x < y ? x : y);
    (void) PFX(hmm_cmp_qsort);
}

/* getTilingPaths coordination.c:186-222 (+ :19-55): consumes the array */
typedef VEC(PFX(hmm_vec) *) PFX(path_vec);
static PFX(path_vec) PFX(tiling_paths_sorted)(HMM_T *const *hmms, int64_t n) { /* hmms in stRPHmm_cmpFn order */
    /* The reference builds one path after the other: the first unused hmm, then again and again the first unused hmm that
     * starts at or behind the end of the path's last one (:19-55), until none is left.  The same paths come out of ONE pass
     * over the hmms in order, each going to the first path (in order of creation) whose last hmm ends at or before its start,
     * or opening a new path: path 1 takes exactly the hmms the reference's first walk takes (the first in order that fits
     * behind its last one), and so on for the rest.  n hmms x the number of paths (coverage depth) compares on a small array
     * instead of a scan over every overlapping hmm per step. */
    PFX(path_vec) paths = {0};
    if (n <= 0) return paths;
    int32_t ends_small[64], *ends = ends_small;
    int64_t ends_cap = 64;
    for (int64_t i = 0; i < n; i++) {
        HMM_T *h = hmms[i];
        const int32_t st = h->ref_start;
        int64_t k = 0;
        while (k < paths.n && ends[k] > st) k++;
        if (k == paths.n) {
            PFX(hmm_vec) *tp = xcalloc(1, sizeof(*tp));
            VEC_PUSH(paths, tp);
            if (paths.n > ends_cap) {
                int32_t *grown = xmalloc(sizeof(int32_t) * (size_t) ends_cap * 2);
                memcpy(grown, ends, sizeof(int32_t) * (size_t) ends_cap);
                if (ends != ends_small) free(ends);
                ends = grown; ends_cap *= 2;
            }
        }
        VEC_PUSH(*paths.a[k], h);
        ends[k] = st + h->ref_length;
    }
    if (ends != ends_small) free(ends);
    return paths;
}
static PFX(path_vec) PFX(tiling_paths_from)(const world *w, HMM_T **hmms, int64_t n) {
    PFX(sort_hmms)(w, hmms, n);
    return PFX(tiling_paths_sorted)(hmms, n);
}

typedef struct { PFX(hmm_vec) members; } PFX(component);
typedef VEC(PFX(component) *) PFX(comp_vec);

/* getOverlappingComponents coordination.c:69-184; components in creation order */
static PFX(comp_vec) PFX(overlapping_components)(const world *w, const PFX(hmm_vec) *tp1, const PFX(hmm_vec) *tp2) {
    PFX(comp_vec) comps = {0};
    /* component index per hmm of tp1 / tp2 */
    int64_t *c1 = xmalloc(sizeof(int64_t) * (size_t) (tp1->n + 1)), *c2 = xmalloc(sizeof(int64_t) * (size_t) (tp2->n + 1));
    for (int64_t i = 0; i < tp1->n; i++) c1[i] = -1;
    for (int64_t i = 0; i < tp2->n; i++) c2[i] = -1;
#define NEW_COMP(hmm, slot) do { PFX(component) *c_ = xcalloc(1, sizeof(PFX(component))); VEC_PUSH(c_->members, (hmm)); \
                                 (slot) = comps.n; VEC_PUSH(comps, c_); } while (0)
    int64_t j = 0;
    for (int64_t i = 0; i < tp2->n && i < 4; i++) __builtin_prefetch(tp2->a[i]);
    for (int64_t i = 0; i < tp1->n; i++) {
        HMM_T *h1 = tp1->a[i];
        if (i + 3 < tp1->n) __builtin_prefetch(tp1->a[i + 3]); /* (headers written a level ago, often on another core) */
        if (j + 4 < tp2->n) __builtin_prefetch(tp2->a[j + 4]);
        int64_t comp = -1, k = 0;
        while (j + k < tp2->n) {
            HMM_T *h2 = tp2->a[j + k];
            if (PFX(hmm_overlap)(h1, h2)) {
                k++;
                if (comp < 0) {
                    comp = c2[j + k - 1];
                    if (comp < 0) { NEW_COMP(h2, c2[j + k - 1]); comp = c2[j + k - 1]; }
                    VEC_PUSH(comps.a[comp]->members, h1);
                    c1[i] = comp;
                } else {
                    VEC_PUSH(comps.a[comp]->members, h2);
                    c2[j + k - 1] = comp;
                }
            } else {
                if (PFX(hmm_cmp)(w, h1, h2) < 0) {
                    if (comp < 0) { NEW_COMP(h1, c1[i]); comp = c1[i]; }
                    break;
                } else {
                    if (c2[j + k] < 0) NEW_COMP(h2, c2[j + k]);
                    j++;
                }
            }
        }
        if (comp < 0) NEW_COMP(h1, c1[i]);
    }
    while (j < tp2->n) {
        if (c2[j] < 0) NEW_COMP(tp2->a[j], c2[j]);
        j++;
    }
#undef NEW_COMP
    free(c1); free(c2);
    return comps;
}
