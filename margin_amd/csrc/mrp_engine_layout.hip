/*
 * mrp_engine_layout.hip -- column structure of a merge level (mrp_engine.h "column structure of a level, on the device") and, further
 * down, its layout.  A level's other stages: mrp_engine_cross.hip, mrp_engine_kernels.hip (prune), mrp_engine_small.hip,
 * mrp_engine_final.hip.
 */
#include "mrp_engine.h"
#include "mrp_wave.h"

/* what one side (tiling path) contributes to the child column [cs, ce): the piece of pieces_of_path / align_pieces of the
 * reference's stRPHmm_fuse (hmm.c:283-372) and stRPHmm_alignColumns (hmm.c:374-507) that holds cs */
struct SidePiece {
    const uint64_t *part; const uint32_t *np; const int32_t *ncells, *nmerge;
    const int64_t *rbo;      /* the parent column's read_byte_off entries */
    int64_t leaf_rbo;        /* leaf: the read's pool offset */
    int32_t delta_site;      /* first site of the parent column (rbo moves on by the alleles between it and cs) */
    uint8_t depth, out, paired, cont;
    bool leaf;
};
static __device__ SidePiece structure_side(const StructureIn &in, const mrp_xpar *path, int n_path, int32_t ref_end, int32_t cs, int32_t ce,
                                           int *bad) {
    SidePiece r;
    r.part = nullptr; r.np = nullptr; r.ncells = nullptr; r.nmerge = nullptr; r.rbo = nullptr; r.leaf_rbo = 0; r.delta_site = cs;
    r.depth = 0; r.out = MRP_CONN_ZERO; r.paired = 0; r.cont = 0; r.leaf = false;
    /* last hmm of the path that starts at or before cs */
    int lo = 0, hi = n_path;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (path[mid].start <= cs) lo = mid + 1; else hi = mid; }
    const int pi = lo - 1;
    if (pi < 0 || cs >= path[pi].end) { /* gap column (hmm.c:335-359, :396-462): one cell, partition 0, depth 0 */
        const int32_t gap_end = lo < n_path ? path[lo].start : ref_end;
        if (ce > gap_end) *bad = 1;
        r.out = ce < gap_end ? MRP_CONN_IDENT : MRP_CONN_ZERO; /* a gap cut in two: the accept-mask connector of a depth-0 column */
        return r;
    }
    const mrp_xpar p = path[pi];
    if (p.seg < 0) { /* stRPHmm_construct (hmm.c:97-133): one column {1, 0} over the read's sites */
        if (ce > p.end) *bad = 1;
        r.part = in.leaf_part; r.np = in.leaf_np; r.ncells = in.leaf_count;
        r.leaf = true; r.leaf_rbo = p.col0; r.delta_site = p.start; r.depth = 1;
        r.out = ce < p.end ? MRP_CONN_IDENT : MRP_CONN_ZERO;
        r.paired = r.out == MRP_CONN_IDENT ? 1 : 0;
        r.cont = r.paired;
        return r;
    }
    const SegDev sg = in.segs[p.seg];
    const ResCol *pc = sg.cols + p.col0;
    int a = 0, b = p.n_cols; /* last column of the parent that starts at or before cs */
    while (a < b) { const int mid = (a + b) >> 1; if (pc[mid].start <= cs) a = mid + 1; else b = mid; }
    const int k = a - 1;
    if (k < 0) { *bad = 1; return r; }
    const ResCol c = pc[k];
    const int32_t pe = k + 1 < p.n_cols ? pc[k + 1].start : p.end;
    if (ce > pe) *bad = 1;
    const int64_t col = p.col0 + k;
    r.part = sg.part + col * in.stride; r.np = sg.np + col * in.stride; r.ncells = sg.n_cells + col;
    r.rbo = sg.rbo + c.rbo_off; r.delta_site = c.start; r.depth = c.depth;
    if (ce < pe) { r.out = MRP_CONN_IDENT; r.paired = c.depth > 0 ? 1 : 0; }          /* column.c:86-101 */
    else if (k + 1 < p.n_cols) { r.out = MRP_CONN_REAL; r.paired = c.cont; r.nmerge = sg.n_merge + col; }
    else { r.out = MRP_CONN_ZERO; r.paired = 0; }                                       /* hmm.c:324-331 */
    r.cont = r.paired;
    return r;
}

__global__ void __launch_bounds__(256) mrp_structure_kernel(StructureIn in) {
    const int64_t col = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= in.n_cols) return;
    /* the hmm the column belongs to: last one whose first column is at or before col */
    int64_t lo = 0, hi = in.n_hmms;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (in.xd[mid].col0 <= col) lo = mid + 1; else hi = mid; }
    const XDesc x = in.xd[lo - 1];
    const int k = (int) (col - x.col0);
    const bool last = k + 1 == x.n_cols;
    int32_t cs = in.col_start[col], ce = last ? x.ref_end : in.col_start[col + 1];
    int bad = (ce <= cs || cs < x.ref_start || ce > x.ref_end) ? 1 : 0;
    if (bad) { cs = x.ref_start; ce = x.ref_end; } /* (the chunk's tables are read below whatever the flag says: inside the hmm's interval) */
    const mrp_xpar *pa = in.par + x.par0, *pb = pa + x.n_a;
    const SidePiece A = structure_side(in, pa, x.n_a, x.ref_end, cs, ce, &bad);
    const SidePiece B = structure_side(in, pb, x.n_b, x.ref_end, cs, ce, &bad);
    const DevChunk ch = in.chunks[x.chunk];
    const int depth = (int) A.depth + (int) B.depth;
    if (depth > MRP_MAX_READ_PARTITIONING_DEPTH) bad = 1;
    const int64_t read_off = x.read0 + in.col_roff[col];
    /* the host sized the column's slice of the read offsets from ITS depth: a disagreement must not run into the next column's */
    if (!last && depth != in.col_roff[col + 1] - in.col_roff[col]) bad = 1;
    if (!bad) { /* the column's reads: side A's then side B's (partitions.c:21-28); profileSeq.c:41-47 */
        int64_t *dst = in.rbo + read_off;
        const uint32_t a_cs = ch.allele_offset[cs];
        if (A.depth) {
            const int64_t delta = (int64_t) a_cs - (int64_t) ch.allele_offset[A.delta_site];
            if (A.leaf) dst[0] = A.leaf_rbo + delta;
            else for (int i = 0; i < A.depth; i++) dst[i] = A.rbo[i] + delta;
        }
        if (B.depth) {
            const int64_t delta = (int64_t) a_cs - (int64_t) ch.allele_offset[B.delta_site];
            if (B.leaf) dst[A.depth] = B.leaf_rbo + delta;
            else for (int i = 0; i < B.depth; i++) dst[A.depth + i] = B.rbo[i] + delta;
        }
    }
    PlanCol o;
    o.a_part = A.part; o.b_part = B.part; o.a_np = A.np; o.b_np = B.np;
    o.a_ncells = A.ncells; o.b_ncells = B.ncells; o.a_nmerge = A.nmerge; o.b_nmerge = B.nmerge;
    o.read_off = read_off;
    o.slot_off = x.slot0 + (int64_t) (ch.allele_offset[cs] - ch.allele_offset[x.ref_start]);
    o.site_start = cs; o.n_sites = ce - cs; o.depth = bad ? 0 : depth;
    o.n_slots = (int32_t) (ch.allele_offset[ce] - ch.allele_offset[cs]);
    o.chunk = x.chunk;
    const int32_t uniform = ch.same_until[cs] >= ce ? (int32_t) ch.allele_number[cs] : 0;
    o.uniform_alleles = uniform;
    o.d1 = bad ? 0 : A.depth; o.d2 = bad ? 0 : B.depth; o.out_a = A.out; o.out_b = B.out;
    o.out_a_paired = A.paired; o.out_b_paired = B.paired;
    o.need_planes = (!in.fused && (uniform == 0 || (x.flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB))) ? 1 : 0;
    o.last = last ? 1 : 0;
    o.pad = 0;
    if (bad) { o.a_part = nullptr; o.b_part = nullptr; o.a_np = nullptr; o.b_np = nullptr; o.a_ncells = nullptr; o.b_ncells = nullptr;
               o.a_nmerge = nullptr; o.b_nmerge = nullptr; o.out_a = o.out_b = MRP_CONN_ZERO; o.out_a_paired = o.out_b_paired = 0; }
    in.plan[col] = o;
    ResCol rc;
    rc.rbo_off = read_off; rc.start = cs; rc.depth = (uint8_t) o.depth; rc.cont = last ? 0 : (uint8_t) ((A.cont | B.cont) && !bad); rc.pad = 0;
    in.cols[col] = rc;
    in.col_hmm[col] = x.prune_pos;
    if (bad) { atomicOr(in.err, MRP_ENGINE_ERR_RANGE); atomicOr(in.err_hmm + x.prune_pos, MRP_ENGINE_ERR_RANGE); }
}

hipError_t mrp_launch_structure(const StructureIn &in, hipStream_t stream) {
    if (in.n_cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(mrp_structure_kernel, dim3((unsigned) ((in.n_cols + 255) / 256)), dim3(256), 0, stream, in);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------ */
/* layout of a level: sizes, offsets and kernel descriptors from the parents' counts           */
/* ------------------------------------------------------------------------------------------ */
static __device__ __forceinline__ int32_t layout_count(const int32_t *p, int32_t S) {
    if (!p) return 1;
    const int32_t v = *p;
    return v < 1 ? 1 : (v > S ? S : v); /* (a discarded parent may hold anything: the level stays within its static bounds) */
}

/* pass 1, one wave per hmm: C1, C2, Ma, Mb of every column; per hmm the sums the scan needs */
__global__ void __launch_bounds__(256) mrp_layout_count_kernel(const PlanCol *__restrict__ plan, const PlanHmm *__restrict__ ph, int64_t n_hmms,
                                                               int32_t S, uint32_t xflags, LayoutOut o) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t w = (int64_t) blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (w >= n_hmms) return;
    const PlanHmm h = ph[w];
    const bool ancestor = (h.flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB) != 0;
    int64_t cells = 0, merge = 0, acells = 0, amerge = 0;
    int tf = 0, tg = 0, mc = 1, mm = 1;
    const bool units = (xflags & MRP_XF_UNITS) != 0;
    for (int k = lane; k < h.n_cols; k += WAVE) {
        const PlanCol c = plan[h.col0 + k];
        /* Every count is kept within the bound the HOST assumes for the column (mrp_side_bound: a pruned column has at most S cells
         * and never more than the bipartitions of its reads; rphmm_host.c r_cross_build sums exactly these products): a valid parent
         * never exceeds it, a discarded one may hold anything -- and a level launched without waiting for its totals (mrp_engine.cpp,
         * deferred launch) has arrays of the bounds' size. */
        const int S1 = (int) mrp_side_bound(c.d1, S), S2 = (int) mrp_side_bound(c.d2, S);
        const int C1 = layout_count(c.a_ncells, S1), C2 = layout_count(c.b_ncells, S2);
        int Ma = 0, Mb = 0;
        if (!c.last) {
            Ma = c.out_a == MRP_CONN_REAL ? layout_count(c.a_nmerge, S1) : (c.out_a == MRP_CONN_IDENT ? C1 : 1);
            Mb = c.out_b == MRP_CONN_REAL ? layout_count(c.b_nmerge, S2) : (c.out_b == MRP_CONN_IDENT ? C2 : 1);
        }
        uint16_t *dm = o.dims + 4 * (h.col0 + k);
        dm[0] = (uint16_t) C1; dm[1] = (uint16_t) C2; dm[2] = (uint16_t) Ma; dm[3] = (uint16_t) Mb;
        const int Cf = C1 * C2, Mf = Ma * Mb;
        /* MRP_XF_UNITS: a column some side of which has reads holds its cells in complement pairs, a merge column some side of
         * which is paired likewise: one array entry per pair */
        const int C = units && ((c.a_part && c.d1 > 0) || (c.b_part && c.d2 > 0)) ? Cf >> 1 : Cf;
        const int M = units && !c.last && (c.out_a_paired || c.out_b_paired) ? Mf >> 1 : Mf;
        cells += C; merge += M; acells += Cf; amerge += Mf;
        const int nt = (C + MRP_EMIT_TILE - 1) / MRP_EMIT_TILE;
        if (c.uniform_alleles != 0 && !ancestor) tf += nt; else tg += nt;
        mc = C > mc ? C : mc;
        mm = M > mm ? M : mm;
    }
    /* (an hmm has at most 2^31 cells: checked on the host against the static bounds) */
    const int lo = wave_sum_i32((int) (cells & 0xFFFF)), hi = wave_sum_i32((int) (cells >> 16));
    const int mlo = wave_sum_i32((int) (merge & 0xFFFF)), mhi = wave_sum_i32((int) (merge >> 16));
    const int alo = wave_sum_i32((int) (acells & 0xFFFF)), ahi = wave_sum_i32((int) (acells >> 16));
    const int amlo = wave_sum_i32((int) (amerge & 0xFFFF)), amhi = wave_sum_i32((int) (amerge >> 16));
    tf = wave_sum_i32(tf); tg = wave_sum_i32(tg); mc = wave_max_i32(mc); mm = wave_max_i32(mm);
    if (lane == 0) {
        LayoutTot t;
        t.cells = ((int64_t) hi << 16) + lo; t.merge = ((int64_t) mhi << 16) + mlo;
        t.acells = ((int64_t) ahi << 16) + alo; t.amerge = ((int64_t) amhi << 16) + amlo;
        t.tiles_fast = tf; t.tiles_gen = tg; t.max_cells = mc; t.max_merge = mm;
        o.tot[w] = t;
    }
}

/* pass 2: where every hmm starts (cells padded to a multiple of 4 per hmm), the totals, the DevHmm records -- an exclusive scan over the
 * hmms' sums in two small kernels of 256-thread workgroups, a tile of 256 hmms each:
 *   mrp_layout_tiles_kernel   the six sums of every tile (coalesced: thread i reads hmm 256 t + i);
 *   mrp_layout_scan_kernel    tile t adds up the tiles before it (at most a few hundred: 37 000 hmms are 145 tiles), scans its own 256
 *                             hmms in LDS and writes their bases and DevHmm records; the last tile writes the totals.
 * Through round 4 this was ONE workgroup of 1 024 threads walking the hmms in runs (two passes of strided 48-byte reads, 128 registers
 * and 48 spilled): 20-240 us alone -- and, needing a CU's whole register file to start, 1 ms on average once the device was full of
 * other batches' chain workgroups, on the critical path of every level (62 ms of summed kernel time per 1 152-chunk step). */
#define LAYOUT_TILE 256
static __device__ __forceinline__ void layout_sums_of(const LayoutTot &x, int64_t (&v)[6]) {
    v[0] = (x.cells + 3) & ~3ll; v[1] = x.merge; v[2] = x.tiles_fast; v[3] = x.tiles_gen; v[4] = x.acells; v[5] = x.amerge;
}
__global__ void __launch_bounds__(LAYOUT_TILE) mrp_layout_tiles_kernel(int64_t n_hmms, LayoutOut o, int64_t *__restrict__ tile_sums) {
    __shared__ int64_t wsum[LAYOUT_TILE / WAVE][6];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int64_t i = (int64_t) blockIdx.x * LAYOUT_TILE + t;
    int64_t v[6] = {0, 0, 0, 0, 0, 0};
    if (i < n_hmms) layout_sums_of(o.tot[i], v);
#pragma unroll
    for (int q = 0; q < 6; q++) {
        int64_t x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
        if (lane == 0) wsum[wave][q] = x;
    }
    __syncthreads();
    if (t < 6) {
        int64_t x = 0;
#pragma unroll
        for (int w = 0; w < LAYOUT_TILE / WAVE; w++) x += wsum[w][t];
        tile_sums[(int64_t) blockIdx.x * 6 + t] = x;
    }
}
__global__ void __launch_bounds__(LAYOUT_TILE) mrp_layout_scan_kernel(const PlanHmm *__restrict__ ph, int64_t n_hmms, LayoutOut o,
                                                                      const int64_t *__restrict__ tile_sums) {
    __shared__ int64_t wsum[LAYOUT_TILE / WAVE][6];
    __shared__ int64_t before[6];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int64_t tile = blockIdx.x, i = tile * LAYOUT_TILE + t;
    /* the tiles before this one */
    int64_t pre[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t j = t; j < tile; j += LAYOUT_TILE)
#pragma unroll
        for (int q = 0; q < 6; q++) pre[q] += tile_sums[j * 6 + q];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        int64_t x = pre[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
        if (lane == 0) wsum[wave][q] = x;
    }
    __syncthreads();
    if (t < 6) {
        int64_t x = 0;
#pragma unroll
        for (int w = 0; w < LAYOUT_TILE / WAVE; w++) x += wsum[w][t];
        before[t] = x;
    }
    __syncthreads();
    /* this tile's hmms */
    LayoutTot x{};
    int64_t v[6] = {0, 0, 0, 0, 0, 0}, incl[6];
    if (i < n_hmms) { x = o.tot[i]; layout_sums_of(x, v); }
#pragma unroll
    for (int q = 0; q < 6; q++) { incl[q] = wave_incl_scan_i64(v[q], lane); if (lane == WAVE - 1) wsum[wave][q] = incl[q]; }
    __syncthreads();
    int64_t excl[6];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        int64_t bw = before[q], all = before[q];
#pragma unroll
        for (int w = 0; w < LAYOUT_TILE / WAVE; w++) { const int64_t y = wsum[w][q]; if (w < wave) bw += y; all += y; }
        excl[q] = bw + incl[q] - v[q];
        if (tile == (int64_t) gridDim.x - 1 && t == 0) o.totals[q] = all;
    }
    if (i < n_hmms) {
        const PlanHmm h = ph[i];
        LayoutBase b;
        b.cell0 = excl[0]; b.mcell0 = excl[1]; b.tile_fast0 = excl[2]; b.tile_gen0 = excl[3];
        o.base[i] = b;
        DevHmm d;
        d.col0 = h.col0; d.n_cols = h.n_cols; d.flags = h.flags; d.max_merge = x.max_merge; d.max_cells = x.max_cells;
        d.wide_idx = 0; d.pad = 0; d.n_cells = x.cells; d.n_merge = x.merge; d.cost_bound = h.cost_bound;
        o.hmms[i] = d;
    }
}

/* pass 3, one wave per hmm: the offsets of its columns and every per-column descriptor of the level's kernels */
__global__ void __launch_bounds__(256) mrp_layout_fill_kernel(const PlanCol *__restrict__ plan, const PlanHmm *__restrict__ ph, int64_t n_hmms,
                                                              const DevChunk *__restrict__ chunks, uint32_t xflags, LayoutOut o) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t w = (int64_t) blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (w >= n_hmms) return;
    const PlanHmm h = ph[w];
    const LayoutBase base = o.base[w];
    const bool ancestor = (h.flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB) != 0;
    int64_t c_off = base.cell0, m_off = base.mcell0, t_fast = base.tile_fast0, t_gen = o.totals[2] + base.tile_gen0;
    for (int k0 = 0; k0 < h.n_cols; k0 += WAVE) {
        const int k = k0 + lane;
        const bool in = k < h.n_cols;
        const int64_t col = h.col0 + (in ? k : 0);
        const PlanCol c = plan[col];
        const uint16_t *dm = o.dims + 4 * col;
        const int C1 = in ? dm[0] : 0, C2 = in ? dm[1] : 0, Ma = in ? dm[2] : 0, Mb = in ? dm[3] : 0;
        const bool units = (xflags & MRP_XF_UNITS) != 0; /* array entries per column: see mrp_layout_count_kernel */
        const int C = units && ((c.a_part && c.d1 > 0) || (c.b_part && c.d2 > 0)) ? (C1 * C2) >> 1 : C1 * C2;
        const int M = units && !c.last && (c.out_a_paired || c.out_b_paired) ? (Ma * Mb) >> 1 : Ma * Mb;
        const int nt = (C + MRP_EMIT_TILE - 1) / MRP_EMIT_TILE;
        const bool fast = c.uniform_alleles != 0 && !ancestor;
        int tc, tm, tf, tg;
        const int xc = wave_excl_scan_shfl(C, lane, &tc), xm = wave_excl_scan_shfl(M, lane, &tm);
        const int xf = wave_excl_scan_shfl(in && fast ? nt : 0, lane, &tf), xg = wave_excl_scan_shfl(in && !fast ? nt : 0, lane, &tg);
        if (in) {
            DevCol dc;
            dc.cell_off = c_off + xc; dc.mcell_off = c.last ? 0 : m_off + xm; dc.slot_off = c.slot_off; dc.read_off = c.read_off;
            dc.n_cells = C; dc.n_merge = M; dc.site_start = c.site_start; dc.n_sites = c.n_sites; dc.depth = c.depth; dc.n_slots = c.n_slots;
            dc.chunk = c.chunk; dc.flags = h.flags | ((uint32_t) (c.uniform_alleles > 255 ? 0 : c.uniform_alleles) << 8); /* bits 8..15: allele count shared by the column's sites (0: they differ) */
            o.cols[col] = dc;
            SweepCol sc;
            sc.cell_off = dc.cell_off; sc.mcell_off = dc.mcell_off; sc.n_cells = C; sc.n_merge = M; sc.pad[0] = 0; sc.pad[1] = 0;
            o.scols[col] = sc;
            PlaneCol pc;
            pc.pool = chunks[c.chunk].pool; pc.read_off = c.read_off; pc.slot_off = c.slot_off; pc.depth = c.depth; pc.n_slots = c.n_slots;
            pc.need_planes = c.need_planes; pc.pad = 0;
            o.pcols[col] = pc;
            TileCol tcl;
            tcl.first = fast ? t_fast + xf : t_gen + xg; tcl.uniform_alleles = c.uniform_alleles; tcl.pad = 0;
            o.tilecols[col] = tcl;
            CrossCol x;
            x.a_part = c.a_part; x.b_part = c.b_part; x.a_np = c.a_np; x.b_np = c.b_np;
            x.x_cell_off = dc.cell_off;
            x.C1 = (uint16_t) C1; x.C2 = (uint16_t) C2; x.Ma = (uint16_t) Ma; x.Mb = (uint16_t) Mb;
            x.d1 = c.d1; x.d2 = c.d2;
            uint8_t fl = (uint8_t) xflags;
            x.out_a = c.last ? 0 : c.out_a; x.out_b = c.last ? 0 : c.out_b;
            if (!c.last) { if (c.out_a_paired) fl |= MRP_XF_OUT_A_PAIRED; if (c.out_b_paired) fl |= MRP_XF_OUT_B_PAIRED; }
            x.Pa = 0; x.Pb = 0; x.in_a = 0; x.in_b = 0;
            if (k > 0) { /* the connector that enters the column is the one that leaves the column before */
                const PlanCol q = plan[col - 1];
                const uint16_t *qm = o.dims + 4 * (col - 1);
                x.Pa = qm[2]; x.Pb = qm[3]; x.in_a = q.out_a; x.in_b = q.out_b;
                if (q.out_a_paired) fl |= MRP_XF_IN_A_PAIRED;
                if (q.out_b_paired) fl |= MRP_XF_IN_B_PAIRED;
            }
            x.flags = fl; x.pad = 0;
            o.ccols[col] = x;
        }
        c_off += tc; m_off += tm; t_fast += tf; t_gen += tg;
    }
}

hipError_t mrp_launch_layout(const PlanCol *plan_dev, const PlanHmm *hmms_dev, int64_t n_hmms, int64_t n_cols, const DevChunk *chunks_dev,
                             int32_t S, uint32_t xflags, LayoutOut out, hipStream_t stream) {
    if (n_hmms <= 0) return hipSuccess;
    (void) n_cols;
    const unsigned g = (unsigned) ((n_hmms + 3) / 4);
    hipLaunchKernelGGL(mrp_layout_count_kernel, dim3(g), dim3(256), 0, stream, plan_dev, hmms_dev, n_hmms, S, xflags, out);
    const unsigned tiles = (unsigned) ((n_hmms + LAYOUT_TILE - 1) / LAYOUT_TILE);
    hipLaunchKernelGGL(mrp_layout_tiles_kernel, dim3(tiles), dim3(LAYOUT_TILE), 0, stream, n_hmms, out, out.tile_sums);
    hipLaunchKernelGGL(mrp_layout_scan_kernel, dim3(tiles), dim3(LAYOUT_TILE), 0, stream, hmms_dev, n_hmms, out, out.tile_sums);
    hipLaunchKernelGGL(mrp_layout_fill_kernel, dim3(g), dim3(256), 0, stream, plan_dev, hmms_dev, n_hmms, chunks_dev, xflags, out);
    return hipGetLastError();
}
