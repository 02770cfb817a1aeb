/*
 * mrp_posterior_plan.h -- what mrp_posterior_aligned_pairs decides by host arithmetic alone: whether its options are the ones
 * getPosteriorProbsWithBanding asserts (impl/pairwiseAligner.c:714-718), and at which diagonals of a band the reference traces back
 * (:746-749, :768, :819).  No HIP call: mrp_posterior_tracebacks hands the list out, the device entry launches a wave per element.
 */
#ifndef MRP_POSTERIOR_PLAN_H_
#define MRP_POSTERIOR_PLAN_H_

#include <cstdint>
#include <vector>

#include "../../include/margin_rphmm.h"

/* One traceback: started at diagonal d, it takes the posteriors of the diagonals (to, from] */
struct PstTraceback {
    int64_t d, to, from;
};

/* NULL, or what is wrong with the options (the text after "who: ") */
static inline const char *pst_options_error(const mrp_posterior_options *o) {
    if (o->reserved != 0) return "options.reserved must be 0";
    if (!(o->threshold > 0.0)) /* NaN included */
        return "threshold must lie in (0, 1]: a threshold of 0 would return every cell of the band";
    if (!(o->threshold <= 1.0)) return "threshold must lie in (0, 1] (pairwiseAligner.c:615-616)";
    if (o->expansion < 0 || o->expansion % 2 != 0) return "diagonalExpansion must be even and >= 0 (pairwiseAligner.c:715-716)";
    if (o->traceback_diagonals < 1) return "traceBackDiagonals must be >= 1 (pairwiseAligner.c:714)";
    if (o->min_diags_between_traceback < 2) return "minDiagsBetweenTraceBack must be >= 2 (pairwiseAligner.c:717)";
    if (!(o->traceback_diagonals + 1 < o->min_diags_between_traceback))
        return "traceBackDiagonals + 1 must be < minDiagsBetweenTraceBack (pairwiseAligner.c:718)";
    return nullptr;
}

/* The reference's loop over the diagonals 1..n of a band (xmy_l / xmy_r as mrp_band_diagonals gives them), pairwiseAligner.c:739-834:
 * a traceback at d when d == n, or when d >= tracedBackTo + minDiagsBetweenTraceBack and the diagonal has at most
 * 2 * diagonalExpansion + 1 cells; it ends at d - (traceBackDiagonals + 1), at d itself when d == n.  Appends to out. */
static inline void pst_plan_tracebacks(const int32_t *xmy_l, const int32_t *xmy_r, int64_t n, int64_t expansion, int64_t min_diags,
                                       int64_t traceback_diagonals, std::vector<PstTraceback> &out) {
    int64_t to = 0;
    for (int64_t d = 1; d <= n; d++) {
        const bool at_end = d == n;
        const int64_t width = ((int64_t) xmy_r[d] - xmy_l[d]) / 2 + 1;
        if (!(at_end || (d >= to + min_diags && width <= expansion * 2 + 1))) continue;
        const int64_t from = d - (at_end ? 0 : traceback_diagonals + 1);
        out.push_back(PstTraceback{d, to, from});
        to = from;
    }
}

#endif /* MRP_POSTERIOR_PLAN_H_ */
