/*
 * mrp_wave.h -- cross-lane and scalar-path primitives of the gfx950 kernels (wave64), each defined here once.
 * Device inline functions only, integer only: no kernel, no state, nothing a floating-point compile flag can touch.
 */
#ifndef MRP_WAVE_H
#define MRP_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define WAVE 64
/* Read-only data that is uniform across a wave (column descriptors, bit planes, site tables) is
 * loaded through the constant address space so that hipcc emits s_load (scalar cache, SGPR
 * operands) instead of 64 identical vector loads.  None of it is written by the kernel reading it. */
#define K_AS(T) const __attribute__((address_space(4))) T *
#define K_PTR(T, p) ((K_AS(T)) (p))
/* whole-struct load through the scalar path (dword copies; SROA turns them into s_load_dwordxN) */
template <typename T>
static __device__ __forceinline__ T k_load(const T *p) {
    static_assert(sizeof(T) % 4 == 0, "dword sized");
    T v;
    K_AS(uint32_t) s = K_PTR(uint32_t, p);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&v);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; i++) dst[i] = s[i];
    return v;
}

/* Workgroup barrier that orders LDS traffic only (__syncthreads() also waits for every global load in
 * flight, which would serialize the prefetch of the next column with the work on the current one, and
 * for every store). */
static __device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
/* LDS traffic of ONE wave is in order once its counter has drained: what lanes wrote is visible to the other lanes */
static __device__ __forceinline__ void wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
/* Number of set bits of m below this lane, twice on purpose -- they compile differently: lanemask_lt_count takes ANY lane
 * index it is given (a 64-bit shift, mask and popcount), mbcnt64 counts below the executing lane itself with the two
 * v_mbcnt instructions. */
static __device__ __forceinline__ uint32_t lanemask_lt_count(uint64_t m, int lane) {
    return (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
}
static __device__ __forceinline__ int mbcnt64(uint64_t m) {
    return (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
}
/* reductions over the wave, the result in every lane (__shfl_xor butterfly) */
static __device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
static __device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, WAVE); v = t > v ? t : v; }
    return v;
}
/* prefix sums over the wave, on shuffles: 64-bit values, and an exclusive one that also returns the total */
static __device__ __forceinline__ int64_t wave_incl_scan_i64(int64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) { const int64_t t = __shfl_up(v, o, WAVE); if (lane >= o) v += t; }
    return v;
}
static __device__ __forceinline__ int wave_excl_scan_shfl(int v, int lane, int *total) {
    int x = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) { const int t = __shfl_up(x, o, WAVE); if (lane >= o) x += t; }
    *total = __shfl(x, WAVE - 1, WAVE);
    return x - v;
}

/* Cross-lane primitives of the single-wave sections, on the DPP path where gfx950 has one (tools/ubench/dpp_prims.hip
 * checks them against the __shfl versions and times them: bitonic128 0.58 us vs 1.10 us, scan 0.07 vs 0.20 us). */
template <int CTRL, int ROWMASK = 0xf>
static __device__ __forceinline__ uint32_t dpp_mov(uint32_t x) {
    return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) x, CTRL, ROWMASK, 0xf, false);
}
static __device__ __forceinline__ int wave_incl_scan(int v, int lane) {
    int t;
    t = (int) dpp_mov<0x111>((uint32_t) v) + v; if ((lane & 15) >= 1) v = t;       /* row_shr:1 */
    t = (int) dpp_mov<0x112>((uint32_t) v) + v; if ((lane & 15) >= 2) v = t;
    t = (int) dpp_mov<0x114>((uint32_t) v) + v; if ((lane & 15) >= 4) v = t;
    t = (int) dpp_mov<0x118>((uint32_t) v) + v; if ((lane & 15) >= 8) v = t;
    t = (int) dpp_mov<0x142, 0xa>((uint32_t) v) + v; if ((lane & 31) >= 16) v = t; /* row_bcast:15 */
    t = (int) dpp_mov<0x143, 0xc>((uint32_t) v) + v; if (lane >= 32) v = t;        /* row_bcast:31 */
    return v;
}
/* the same with the shifted-in lanes read as zero by the DPP unit itself (bound_ctrl, row masks): an add per step */
static __device__ __forceinline__ int wave_incl_scan_bc(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  /* row_shr:1 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); /* row_bcast:15 into rows 1 and 3 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); /* row_bcast:31 into rows 2 and 3 */
    return v;
}
template <int J>
static __device__ __forceinline__ uint32_t lane_xor(uint32_t x, int lane) {
    if (J == 1) return dpp_mov<0xB1>(x); /* quad_perm [1,0,3,2] */
    if (J == 2) return dpp_mov<0x4E>(x); /* quad_perm [2,3,0,1] */
    if (J == 4) { const uint32_t a = dpp_mov<0x104>(x), b = dpp_mov<0x114>(x); return (lane & 4) ? b : a; } /* row_shl:4 / row_shr:4 */
    if (J == 8) { const uint32_t a = dpp_mov<0x108>(x), b = dpp_mov<0x118>(x); return (lane & 8) ? b : a; }
    return (uint32_t) __shfl_xor((int) x, J, WAVE);
}
/* Ascending bitonic sort of 128 distinct keys held two per lane (index lane and lane + 64) by one wave. */
template <int K, int J>
static __device__ __forceinline__ void bitonic_step(uint32_t &k0, uint32_t &k1, int lane) {
    if (J == 64) { /* K == 128: the partner is the lane's other key */
        const uint32_t lo = k0 < k1 ? k0 : k1, hi = k0 < k1 ? k1 : k0;
        k0 = lo; k1 = hi;
    } else {
        const uint32_t p0 = lane_xor<J>(k0, lane), p1 = lane_xor<J>(k1, lane);
        const bool lower = (lane & J) == 0;
        const bool asc0 = (lane & K) == 0, asc1 = ((lane + 64) & K) == 0;
        const uint32_t mn0 = k0 < p0 ? k0 : p0, mx0 = k0 < p0 ? p0 : k0;
        const uint32_t mn1 = k1 < p1 ? k1 : p1, mx1 = k1 < p1 ? p1 : k1;
        k0 = (lower == asc0) ? mn0 : mx0;
        k1 = (lower == asc1) ? mn1 : mx1;
    }
}
template <int K>
static __device__ __forceinline__ void bitonic_merge(uint32_t &k0, uint32_t &k1, int lane) {
    if (K >= 128) bitonic_step<K, 64>(k0, k1, lane);
    if (K >= 64) bitonic_step<K, 32>(k0, k1, lane);
    if (K >= 32) bitonic_step<K, 16>(k0, k1, lane);
    if (K >= 16) bitonic_step<K, 8>(k0, k1, lane);
    if (K >= 8) bitonic_step<K, 4>(k0, k1, lane);
    if (K >= 4) bitonic_step<K, 2>(k0, k1, lane);
    bitonic_step<K, 1>(k0, k1, lane);
}
static __device__ __forceinline__ void wave_bitonic_sort128(uint32_t &k0, uint32_t &k1, int lane) {
    bitonic_merge<2>(k0, k1, lane);
    bitonic_merge<4>(k0, k1, lane);
    bitonic_merge<8>(k0, k1, lane);
    bitonic_merge<16>(k0, k1, lane);
    bitonic_merge<32>(k0, k1, lane);
    bitonic_merge<64>(k0, k1, lane);
    bitonic_merge<128>(k0, k1, lane);
}
/* the same for 64 NR keys, NR per lane (index lane + 64 u in register u): ascending */
template <int NR, int K, int J>
static __device__ __forceinline__ void bitonic_step_n(uint32_t (&k)[NR], int lane) {
    if (J >= 64) { /* the partner sits in another register of the same lane; K > J >= 64: the direction depends on u alone */
        constexpr int dj = J / 64;
#pragma unroll
        for (int u = 0; u < NR; u++)
            if ((u & dj) == 0) {
                const bool asc = ((u * 64) & K) == 0;
                const uint32_t a = k[u], b = k[u | dj], lo = a < b ? a : b, hi = a < b ? b : a;
                k[u] = asc ? lo : hi;
                k[u | dj] = asc ? hi : lo;
            }
    } else {
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const uint32_t pv = lane_xor<J>(k[u], lane);
            const bool lower = (lane & J) == 0, asc = ((lane + 64 * u) & K) == 0;
            const uint32_t mn = k[u] < pv ? k[u] : pv, mx = k[u] < pv ? pv : k[u];
            k[u] = (lower == asc) ? mn : mx;
        }
    }
}
template <int NR, int K>
static __device__ __forceinline__ void bitonic_merge_n(uint32_t (&k)[NR], int lane) {
    if (K >= 512) bitonic_step_n<NR, K, 256>(k, lane);
    if (K >= 256) bitonic_step_n<NR, K, 128>(k, lane);
    if (K >= 128) bitonic_step_n<NR, K, 64>(k, lane);
    if (K >= 64) bitonic_step_n<NR, K, 32>(k, lane);
    if (K >= 32) bitonic_step_n<NR, K, 16>(k, lane);
    if (K >= 16) bitonic_step_n<NR, K, 8>(k, lane);
    if (K >= 8) bitonic_step_n<NR, K, 4>(k, lane);
    if (K >= 4) bitonic_step_n<NR, K, 2>(k, lane);
    bitonic_step_n<NR, K, 1>(k, lane);
}
template <int NR>
static __device__ __forceinline__ void wave_bitonic_sort_n(uint32_t (&k)[NR], int lane) {
    bitonic_merge_n<NR, 2>(k, lane); bitonic_merge_n<NR, 4>(k, lane); bitonic_merge_n<NR, 8>(k, lane); bitonic_merge_n<NR, 16>(k, lane);
    bitonic_merge_n<NR, 32>(k, lane); bitonic_merge_n<NR, 64>(k, lane);
    if (NR >= 2) bitonic_merge_n<NR, 128>(k, lane);
    if (NR >= 4) bitonic_merge_n<NR, 256>(k, lane);
    if (NR >= 8) bitonic_merge_n<NR, 512>(k, lane);
}

#endif
