/*
 * mrp_pairhmm_dev.h -- the device arithmetic the pair-HMM kernels share: logAdd, the forward cell, the dot product of a cell.  It began
 * as text taken out of mrp_pairhmm.hip when mrp_posterior.hip needed the very same expressions; the walk over the diagonals and the
 * cells of a traceback, built on it, are in mrp_pairhmm_walk.h.  Device code only; every unit that includes it is compiled with
 * -ffp-contract=off.
 */
#ifndef MRP_PAIRHMM_DEV_H_
#define MRP_PAIRHMM_DEV_H_

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

struct St {
    double m, x, y;
};

#define PHM_NEG (-__builtin_inf())

/* lookup(), pairwiseAligner.c:282-293: the float literals are rounded to float first, as the C compiler does */
static __device__ __forceinline__ double phm_lookup(double x) {
    const bool a = x <= 1.0, b = x <= 2.5, c = x <= 4.5;
    const double c3 = a ? (double) -0.009350833524763f : b ? (double) -0.014532321752540f : c ? (double) -0.004605031767994f : (double) -0.000458661602210f;
    const double c2 = a ? (double) 0.130659527668286f : b ? (double) 0.139942324101744f : c ? (double) 0.063427417320019f : (double) 0.009695946122598f;
    const double c1 = a ? (double) 0.498799810682272f : b ? (double) 0.495635523139337f : c ? (double) 0.695956496475118f : (double) 0.930734667215156f;
    const double c0 = a ? (double) 0.693203116424741f : b ? (double) 0.692140569840976f : c ? (double) 0.514272634594009f : (double) 0.168037164329057f;
    return ((c3 * x + c2) * x + c1) * x + c0;
}
/* logAdd(), pairwiseAligner.c:295-299 */
static __device__ __forceinline__ double phm_log_add(double x, double y) {
    const bool lt = x < y;
    const double hi = lt ? y : x, lo = lt ? x : y;
    const double d = hi - lo; /* NaN for two LOG_ZEROs: not used, lo == LOG_ZERO decides first */
    return (lo == PHM_NEG || d >= 7.5) ? hi : phm_lookup(d) + lo;
}

/* toCells[to] = logAdd(toCells[to], from + (eP + tP)) three times, starting from LOG_ZERO (logAdd(LOG_ZERO, a) == a) */
static __device__ __forceinline__ double phm_chain(double a, double b, double c) { return phm_log_add(phm_log_add(a, b), c); }

struct PhmRowT { /* eP + tP of the gap-y transitions of a row (y fixed) */
    double open, extend, sw;
};
static __device__ __forceinline__ St phm_cell(const St &lower, const St &middle, const St &upper, const double *t, double eX, double eM,
                                              const PhmRowT &ty) {
    St cur;
    cur.x = phm_chain(lower.m + (eX + t[3]), lower.x + (eX + t[5]), lower.y + (eX + t[7]));
    cur.m = phm_chain(middle.m + (eM + t[0]), middle.x + (eM + t[1]), middle.y + (eM + t[2]));
    cur.y = phm_chain(upper.m + ty.open, upper.y + ty.extend, upper.x + ty.sw);
    return cur;
}
/* cell_dotProduct, pairwiseAligner.c:333-339 */
static __device__ __forceinline__ double phm_dot(const St &f, const double *e) {
    double tot = f.m + e[0];
    tot = phm_log_add(tot, f.x + e[1]);
    return phm_log_add(tot, f.y + e[2]);
}

}  // namespace

#endif /* MRP_PAIRHMM_DEV_H_ */
