/*
 * mrp_band.h -- the band of the banded pairwise aligner in closed form, for band_construct (impl/pairwiseAligner.c:175-226, one
 * expansion for the whole band) and band_constructDynamic (:120-173, an expansion per anchor).  Host arithmetic only, no HIP call.
 */
#ifndef MRP_BAND_H_
#define MRP_BAND_H_

#include <algorithm>
#include <cstdint>

#include "../../include/margin_rphmm.h"

/* Between two consecutive anchor points P = (px, py) and N = (nx, ny) (matrix coordinates; the first P is (0, 0), the last N is
 * (lx, ly)) the reference bounds the diagonals xay in (px + py, nx + ny] by xL = px - e/2, yL = ny + e/2, xU = nx + e/2,
 * yU = py - e/2 (clamped to the matrix), :218-221 / :165-168; on such a diagonal band_setCurrentDiagonal (:96-114) yields the smallest
 * xmy of the right parity with xmy >= xL - yL, x >= xL, y <= yL and the largest with xmy <= (xU - yU rounded UP to the parity),
 * x <= xU, y >= yU.
 *   anchor_expansion == NULL: band_construct, e = expansion everywhere.
 *   dynamic: band_constructDynamic.  e is read with the anchor N (:148), so the stretch that ends at anchor i is bounded with anchor
 * i's expansion; no further anchor leaves e as it is, so the stretch behind the last anchor keeps the last anchor's, and a pair
 * without anchors has e = 0 (:134), which still bounds nothing: the clamps give the whole matrix.  `expansion` is not read. */
static inline int band_closed_form_any(const int64_t *anchors, const int64_t *anchor_expansion, bool dynamic, int64_t n_anchors, int64_t lx, int64_t ly,
                                       int64_t expansion, int32_t *L, int32_t *R, int64_t *cells, int *max_width) {
    if (lx < 0 || ly < 0) return MRP_ERR_ARG;
    if (!dynamic && (expansion < 0 || expansion % 2 != 0)) return MRP_ERR_ARG;
    int64_t e2 = dynamic ? 0 : expansion / 2;
    auto clamp = [](int64_t z, int64_t hi) { return z < 0 ? (int64_t) 0 : (z > hi ? hi : z); };
    L[0] = 0;
    R[0] = 0;
    int64_t total = 1;
    int mw = 1;
    int64_t px = 0, py = 0, ai = 0;
    while (px + py < lx + ly) {
        int64_t nx = lx, ny = ly;
        if (ai < n_anchors) {
            nx = anchors[2 * ai] + 1;
            ny = anchors[2 * ai + 1] + 1;
            if (!(nx > px && ny > py && nx <= lx && ny <= ly)) return MRP_ERR_ARG; /* asserts :206-211 / :151-156 */
            if (dynamic) {
                const int64_t e = anchor_expansion[ai];
                if (e < 0 || e % 2 != 0) return MRP_ERR_ARG; /* asserts :157-158 */
                e2 = e / 2;
            }
            ai++;
        }
        const int64_t xL = clamp(px - e2, lx), yL = clamp(ny + e2, ly), xU = clamp(nx + e2, lx), yU = clamp(py - e2, ly);
        for (int64_t d = px + py + 1; d <= nx + ny; d++) {
            int64_t l = xL - yL, r = xU - yU;
            if ((d + l) % 2 != 0) l++;
            if ((d + r) % 2 != 0) r++;
            l = std::max(l, std::max(2 * xL - d, d - 2 * yL));
            r = std::min(r, std::min(2 * xU - d, d - 2 * yU));
            if (l > r) return MRP_ERR_ARG; /* diagonal_construct :22-27 throws */
            L[d] = (int32_t) l;
            R[d] = (int32_t) r;
            const int64_t w = (r - l) / 2 + 1;
            total += w;
            if (w > mw) mw = (int) w;
        }
        px = nx;
        py = ny;
    }
    /* the reference ignores anchors left over once (lx, ly) has been reached only if there are none: an anchor list that
     * runs past the end fails its asserts, an anchor exactly at (lx - 1, ly - 1) followed by nothing is fine */
    if (ai < n_anchors) return MRP_ERR_ARG;
    if (cells) *cells = total;
    if (max_width) *max_width = mw;
    return MRP_OK;
}

#endif /* MRP_BAND_H_ */
