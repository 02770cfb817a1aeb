/*
 * mrp_band_dynamic.cpp -- the host entries over the dynamic anchor band (band_constructDynamic, impl/pairwiseAligner.c:120-173, what
 * getPosteriorProbsWithBanding builds when dynamicAnchorExpansion is set, :726): the band, its width and cells, the tracebacks it
 * decides.  Plain C++, no HIP; the band itself is mrp_band.h's, the traceback rule mrp_posterior_plan.h's.
 */
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_band.h"
#include "mrp_posterior_plan.h"
#include "rphmm_host.h" /* mrp_set_error */

extern "C" {

int mrp_band_diagonals_dynamic(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, const int64_t *anchor_expansion, int32_t *xmy_l,
                               int32_t *xmy_r) {
    static const char *who = "mrp_band_diagonals_dynamic";
    if (!xmy_l || !xmy_r || (n_anchors > 0 && (!anchors || !anchor_expansion)) || n_anchors < 0) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who);
    const int rc = band_closed_form_any(anchors, anchor_expansion, true, n_anchors, lx, ly, 0, xmy_l, xmy_r, nullptr, nullptr);
    return rc == MRP_OK ? rc : mrp_set_error(rc, "%s: invalid anchors or an odd or negative expansion (pairwiseAligner.c:151-158)", who);
}

int mrp_pair_diagonal_width_dynamic(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, const int64_t *anchor_expansion, int32_t *width_out,
                                    int64_t *cells_out) {
    static const char *who = "mrp_pair_diagonal_width_dynamic";
    if ((n_anchors > 0 && (!anchors || !anchor_expansion)) || n_anchors < 0) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (lx < 0 || ly < 0) return mrp_set_error(MRP_ERR_ARG, "%s: invalid anchors or an odd or negative expansion (pairwiseAligner.c:151-158)", who);
    if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who);
    std::vector<int32_t> Lb((size_t) (lx + ly + 1)), Rb((size_t) (lx + ly + 1));
    int width = 1;
    int64_t cells = 1;
    const int rc = band_closed_form_any(anchors, anchor_expansion, true, n_anchors, lx, ly, 0, Lb.data(), Rb.data(), &cells, &width);
    if (rc != MRP_OK) return mrp_set_error(rc, "%s: invalid anchors or an odd or negative expansion (pairwiseAligner.c:151-158)", who);
    if (width_out) *width_out = width;
    if (cells_out) *cells_out = cells;
    return MRP_OK;
}

int mrp_posterior_tracebacks_dynamic(const int64_t *anchors, const int64_t *anchor_expansion, int64_t n_anchors, int64_t lx, int64_t ly,
                                     const mrp_posterior_options *opt, int64_t *triples_out, int64_t capacity, int64_t *n_out) {
    static const char *who = "mrp_posterior_tracebacks_dynamic";
    if (!opt || !n_out || (n_anchors > 0 && (!anchors || !anchor_expansion)) || n_anchors < 0 || capacity < 0 || (capacity > 0 && !triples_out))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or negative count", who);
    if (const char *msg = pst_options_error(opt)) return mrp_set_error(MRP_ERR_ARG, "%s: %s", who, msg);
    if (lx < 0 || ly < 0 || lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: bad string lengths", who);
    const int64_t n = lx + ly;
    std::vector<int32_t> L((size_t) n + 1), R((size_t) n + 1);
    if (band_closed_form_any(anchors, anchor_expansion, true, n_anchors, lx, ly, 0, L.data(), R.data(), nullptr, nullptr) != MRP_OK)
        return mrp_set_error(MRP_ERR_ARG, "%s: invalid anchors or an odd or negative expansion (pairwiseAligner.c:151-158)", who);
    std::vector<PstTraceback> plan;
    pst_plan_tracebacks(L.data(), R.data(), n, opt->expansion, opt->min_diags_between_traceback, opt->traceback_diagonals, plan);
    *n_out = (int64_t) plan.size();
    for (int64_t k = 0; k < (int64_t) plan.size() && k < capacity; k++) {
        triples_out[3 * k] = plan[(size_t) k].d;
        triples_out[3 * k + 1] = plan[(size_t) k].to;
        triples_out[3 * k + 2] = plan[(size_t) k].from;
    }
    return MRP_OK;
}

}  // extern "C"
