/*
 * repeat_counts_host_check.cpp -- two programs in one file.
 *
 * (1) The host half of mrp_ml_repeat_counts under the sanitizers, on a machine without a device: every argument error
 * (rc_check_and_build) with nothing written, the per-read array it builds, the sequence numbers of both walk orders
 * (rc_sequence_number), the transposed table (rc_transpose_table), mrp_rle_expand, and the NULL context.  A stand-alone program: the host
 * code of mrp_repeat_counts.hip is compiled into it with the sanitizers, everything else comes from the library as built.
 *
 *   cd margin_amd/csrc
 *   F="-std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I."
 *   hipcc $F -x hip -c ../../tools/hostcheck/repeat_counts_host_check.cpp -o check_main.o
 *   hipcc $F -c mrp_repeat_counts.hip -o check_repeat_counts.o
 *   $ROCM/lib/llvm/bin/clang++ -fsanitize=address,undefined check_main.o check_repeat_counts.o -L../lib -lmargin_rphmm -L$ROCM/lib -lamdhip64 \
 *         -Wl,-rpath,$PWD/../lib -Wl,-rpath,$ROCM/lib -o repeat_counts_host_check
 *   ./repeat_counts_host_check      (prints "ok" and returns 0)
 *
 * (2) With -DRC_TIMING_ONLY, no sanitizer, no HIP and no library: the estimate as a plain sequential C restatement on one host thread,
 * the yardstick of tools/repeat_count_probe.py.
 *
 *   g++ -O2 -std=c++17 -ffp-contract=off -DRC_TIMING_ONLY tools/hostcheck/repeat_counts_host_check.cpp -o tools/hostcheck/repeat_counts_host_time
 *   ./repeat_counts_host_time FILE   (FILE as the probe writes it; prints one line: milliseconds, the sum of the counts, a hash of the log probabilities)
 */
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

/* ---- the sequential restatement: repeatSubMatrix.c:65-238 and poa.c:324-340, 1715-1756, in the reference's own shape -- a list of
 * observations per node, appended read by read, and a loop over the candidates per node ---- */
namespace seq {

struct Observation { int32_t read, y, weight; };

struct Input {
    int32_t R = 0, walk_backwards = 0, phased = 0;
    double s = 0.0;
    std::vector<double> table; /* [4][R][R] */
    std::vector<uint8_t> symbols, counts, strand, in_hap;
    std::vector<int64_t> y_off, first;
    std::vector<int32_t> x_shift, x, y, weight;
};

static double log_prob_for(const Input &in, int base, const std::vector<Observation> &obs, int side, int64_t u) {
    double lp = 0.0;
    for (const Observation &o : obs) {
        if (side >= 0 && (in.in_hap[(size_t) o.read] != 0) != (side == 1)) continue;
        int64_t c = in.counts[(size_t) (in.y_off[(size_t) o.read] + o.y)];
        if (c >= in.R) c = in.R - 1;
        const int b = in.strand[(size_t) o.read] ? base : 3 - base;
        lp += in.table[((size_t) b * in.R + (size_t) u) * in.R + (size_t) c] * o.weight;
    }
    return lp / 10000000.0;
}

static int64_t get_max(const double *v, int64_t n, double *best) {
    double m = v[0];
    int64_t at = 0;
    for (int64_t i = 1; i < n; i++)
        if (v[i] > m) { m = v[i]; at = i; }
    *best = m;
    return at;
}

static void estimate(const Input &in, std::vector<int32_t> &count, std::vector<double> &lp_out) {
    const size_t n_nodes = in.symbols.size(), n_reads = in.y_off.size();
    std::vector<std::vector<Observation>> obs(n_nodes);
    for (size_t r = 0; r < n_reads; r++) /* poa_augment, read by read */
        for (int64_t k = in.first[r]; k < in.first[r + 1]; k++) {
            const int64_t i = in.walk_backwards ? in.first[r] + (in.first[r + 1] - 1 - k) : k;
            obs[(size_t) (in.x[(size_t) i] + in.x_shift[r])].push_back(Observation{(int32_t) r, in.y[(size_t) i], in.weight[(size_t) i]});
        }
    count.assign(n_nodes, 0);
    lp_out.assign(n_nodes, 0.0);
    std::vector<double> lp1((size_t) in.R), lp2((size_t) in.R);
    for (size_t k = 0; k < n_nodes; k++) {
        int64_t mn = in.R, mx = 0;
        for (const Observation &o : obs[k]) {
            const int64_t c = in.counts[(size_t) (in.y_off[(size_t) o.read] + o.y)];
            if (c < mn) mn = c;
            if (c > mx) mx = c;
        }
        if (mx >= in.R) mx = in.R - 1;
        int64_t ml = 0;
        double best = -INFINITY;
        if (mn != in.R) {
            const int base = in.symbols[k] > 3 ? 0 : in.symbols[k];
            if (!in.phased) {
                for (int64_t u = mn; u <= mx; u++) lp1[(size_t) (u - mn)] = log_prob_for(in, base, obs[k], -1, u);
                ml = get_max(lp1.data(), mx - mn + 1, &best) + mn;
            } else {
                for (int64_t u = mn; u <= mx; u++) {
                    lp1[(size_t) (u - mn)] = log_prob_for(in, base, obs[k], 1, u);
                    lp2[(size_t) (u - mn)] = log_prob_for(in, base, obs[k], 0, u);
                }
                double ml2;
                get_max(lp2.data(), mx - mn + 1, &ml2);
                auto p = [&](int64_t i) { return lp1[(size_t) i] + ((lp2[(size_t) i] > ml2 + in.s) ? lp2[(size_t) i] : ml2 + in.s); };
                best = p(0);
                ml = mn;
                for (int64_t u = mn + 1; u <= mx; u++) {
                    const double v = p(u - mn);
                    if (v >= best) { best = v; ml = u; }
                }
            }
        }
        count[k] = ml == 0 ? 1 : (int32_t) ml;
        lp_out[k] = best;
    }
}

}  // namespace seq

#ifdef RC_TIMING_ONLY

template <class T> static bool read_vec(FILE *f, std::vector<T> &v) {
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0) return false;
    v.resize((size_t) n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t) n, f) == (size_t) n;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    seq::Input in;
    int32_t head[3];
    bool ok = fread(head, 4, 3, f) == 3 && fread(&in.s, 8, 1, f) == 1;
    in.R = head[0]; in.walk_backwards = head[1]; in.phased = head[2];
    ok = ok && read_vec(f, in.table) && read_vec(f, in.symbols) && read_vec(f, in.counts) && read_vec(f, in.strand) && read_vec(f, in.in_hap) &&
         read_vec(f, in.y_off) && read_vec(f, in.first) && read_vec(f, in.x_shift) && read_vec(f, in.x) && read_vec(f, in.y) && read_vec(f, in.weight);
    fclose(f);
    if (!ok || in.table.size() != (size_t) 4 * in.R * in.R || in.first.size() != in.y_off.size() + 1) { fprintf(stderr, "bad file\n"); return 2; }
    std::vector<int32_t> count;
    std::vector<double> lp;
    double best_ms = 0.0;
    for (int rep = 0; rep < 3; rep++) { /* the fastest of three */
        const auto t0 = std::chrono::steady_clock::now();
        seq::estimate(in, count, lp);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rep == 0 || ms < best_ms) best_ms = ms;
    }
    int64_t total = 0;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < count.size(); k++) {
        total += count[k];
        uint64_t bits;
        memcpy(&bits, &lp[k], 8);
        h = (h ^ bits) * 1099511628211ull;
    }
    printf("%.3f %lld %016llx\n", best_ms, (long long) total, (unsigned long long) h);
    return 0;
}

#else

#include "../../include/margin_rphmm.h"
#include "../../margin_amd/csrc/mrp_repeat_counts.h"

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main() {
    const int R = 7;
    std::vector<double> table((size_t) 4 * R * R);
    for (size_t i = 0; i < table.size(); i++) table[i] = -0.01 * (double) (i % 23) - 0.001 * (double) i;
    table[5] = -INFINITY;

    /* the transposed table */
    HostVec<double> tt;
    rc_transpose_table(table.data(), R, tt);
    REQUIRE(tt.size() == table.size());
    for (int b = 0; b < 4; b++)
        for (int u = 0; u < R; u++)
            for (int o = 0; o < R; o++) {
                const double a = tt[((size_t) b * R + o) * R + u], w = table[((size_t) b * R + u) * R + o];
                REQUIRE(memcmp(&a, &w, 8) == 0);
            }

    /* both walk orders number a call's matches 0 .. n - 1, each once; backwards mirrors inside a read */
    {
        const int64_t first[5] = {0, 3, 3, 4, 9};
        for (int backwards = 0; backwards < 2; backwards++) {
            std::vector<int> seen(9, 0);
            for (int r = 0; r < 4; r++)
                for (int64_t i = first[r]; i < first[r + 1]; i++) {
                    const int64_t q = rc_sequence_number(first[r], first[r + 1], i, backwards);
                    REQUIRE(q >= first[r] && q < first[r + 1]);
                    REQUIRE(q == (backwards ? first[r] + first[r + 1] - 1 - i : i));
                    seen[(size_t) q]++;
                }
            for (int v : seen) REQUIRE(v == 1);
        }
    }

    /* two consensus strings: 3 nodes under 2 reads, 2 nodes under 1 read; every array exactly as long as it must be */
    std::vector<int64_t> node_first{0, 3, 5}, read_first{0, 2, 3}, y_off{0, 3, 5}, first{0, 3, 5, 7};
    std::vector<uint8_t> symbols{0, 1, 4, 2, 3}, counts{1, 2, 3, 2, 9, 1, 255}, strand{1, 0, 1}, hap{1, 0, 0};
    std::vector<int32_t> y_len{3, 2, 2}, shift{0, 1, 0}, x{0, 1, 2, 0, 1, 0, 1}, y{0, 1, 2, 0, 1, 0, 1}, w{5, 7, 1, 3, 4, 9, 9};
    std::vector<double> lp_none;
    mrp_posterior_pairs m{first.data(), x.data(), y.data(), w.data(), nullptr};
    mrp_repeat_count_options opt{1, 0, -9.210340371976182, 0};
    std::vector<int32_t> out(5, -7);
    std::vector<double> lp(5, -7.0);
    std::vector<int64_t> len(2, -7);
    mrp_repeat_count_stats st;
    memset(&st, 0x55, sizeof(st));
    const mrp_repeat_count_stats st0 = st;
    auto call = [&](const mrp_posterior_pairs *mm, const mrp_repeat_count_options *oo, int32_t max_repeat, const uint8_t *h) {
        return mrp_ml_repeat_counts(nullptr, table.data(), max_repeat, 2, node_first.data(), symbols.data(), read_first.data(), counts.data(),
                                    (int64_t) counts.size(), y_off.data(), y_len.data(), strand.data(), shift.data(), h, mm, oo, out.data(), lp.data(), len.data(), &st);
    };
    REQUIRE(call(&m, &opt, R, hap.data()) == MRP_ERR_NO_DEVICE && call(&m, &opt, R, nullptr) == MRP_ERR_NO_DEVICE);
    REQUIRE(call(nullptr, &opt, R, nullptr) == MRP_ERR_ARG && call(&m, nullptr, R, nullptr) == MRP_ERR_ARG);
    REQUIRE(call(&m, &opt, 1, nullptr) == MRP_ERR_ARG && call(&m, &opt, 256, nullptr) == MRP_ERR_ARG);
    {
        std::vector<double> t8((size_t) 4 * 8 * 8, 0.0); /* a table for R = 8 is read to its end and no further */
        t8.back() = NAN;
        REQUIRE(mrp_ml_repeat_counts(nullptr, t8.data(), 8, 2, node_first.data(), symbols.data(), read_first.data(), counts.data(), (int64_t) counts.size(), y_off.data(),
                                     y_len.data(), strand.data(), shift.data(), nullptr, &m, &opt, out.data(), lp.data(), len.data(), &st) == MRP_ERR_ARG);
        REQUIRE(strstr(mrp_last_error(), "log_prob[3][7][7] is NaN") != nullptr);
    }
    {
        mrp_repeat_count_options bad = opt;
        bad.reserved = 1;
        REQUIRE(call(&m, &bad, R, nullptr) == MRP_ERR_ARG);
        bad = opt;
        bad.walk_backwards = 2;
        REQUIRE(call(&m, &bad, R, nullptr) == MRP_ERR_ARG);
        bad = opt;
        bad.log_het_substitution = NAN;
        REQUIRE(call(&m, &bad, R, hap.data()) == MRP_ERR_ARG && call(&m, &bad, R, nullptr) == MRP_ERR_NO_DEVICE);
    }
    {
        std::vector<int32_t> bx(x), by(y), bw(w);
        mrp_posterior_pairs b{first.data(), bx.data(), by.data(), bw.data(), nullptr};
        by[4] = 2; /* read 1 has two counts */
        REQUIRE(call(&b, &opt, R, nullptr) == MRP_ERR_ARG && strstr(mrp_last_error(), "consensus 0, read 1, match 4") != nullptr);
        by = y;
        bx[6] = 2; /* consensus 1 has two nodes */
        REQUIRE(call(&b, &opt, R, nullptr) == MRP_ERR_ARG && strstr(mrp_last_error(), "consensus 1, read 2, match 6") != nullptr);
        bx = x;
        bx[3] = -2; /* read 1: -2 + x_shift 1 */
        REQUIRE(call(&b, &opt, R, nullptr) == MRP_ERR_ARG && strstr(mrp_last_error(), "read 1, match 3") != nullptr);
        bx = x;
        bw[0] = -1;
        REQUIRE(call(&b, &opt, R, nullptr) == MRP_ERR_ARG && strstr(mrp_last_error(), "negative weight") != nullptr);
        std::vector<int64_t> bf{0, 3, 2, 7};
        mrp_posterior_pairs c{bf.data(), x.data(), y.data(), w.data(), nullptr};
        REQUIRE(call(&c, &opt, R, nullptr) == MRP_ERR_ARG);
        std::vector<int64_t> beyond(y_off);
        beyond[2] = 6; /* the last read ends one byte behind the pool */
        REQUIRE(mrp_ml_repeat_counts(nullptr, table.data(), R, 2, node_first.data(), symbols.data(), read_first.data(), counts.data(), (int64_t) counts.size(),
                                     beyond.data(), y_len.data(), strand.data(), shift.data(), nullptr, &m, &opt, out.data(), lp.data(), len.data(), &st) == MRP_ERR_ARG);
    }
    for (int32_t v : out) REQUIRE(v == -7);
    for (double v : lp) REQUIRE(v == -7.0);
    for (int64_t v : len) REQUIRE(v == -7);
    REQUIRE(memcmp(&st, &st0, sizeof(st)) == 0);
    /* no consensus: no array but the offsets is read */
    {
        const int64_t zero = 0;
        mrp_posterior_pairs none{const_cast<int64_t *>(&zero), nullptr, nullptr, nullptr, nullptr};
        REQUIRE(mrp_ml_repeat_counts(nullptr, table.data(), R, 0, &zero, nullptr, &zero, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &none, &opt, nullptr,
                                     nullptr, nullptr, nullptr) == MRP_ERR_NO_DEVICE);
    }

    /* the per-read array */
    {
        HostVec<RcRead> reads;
        REQUIRE(rc_check_and_build("check", table.data(), R, 2, node_first.data(), symbols.data(), read_first.data(), counts.data(), (int64_t) counts.size(),
                                   y_off.data(), y_len.data(), strand.data(), shift.data(), hap.data(), &m, &opt, out.data(), len.data(), reads) == MRP_OK);
        REQUIRE(reads.size() == 3 && reads[0].node_base == 0 && reads[1].node_base == 1 && reads[2].node_base == 3);
        REQUIRE(reads[0].flags == (RC_STRAND | RC_IN_HAP) && reads[1].flags == 0u && reads[2].flags == RC_STRAND && reads[2].y_off == 5);
        REQUIRE(rc_check_and_build("check", table.data(), R, 2, node_first.data(), symbols.data(), read_first.data(), counts.data(), (int64_t) counts.size(),
                                   y_off.data(), y_len.data(), strand.data(), nullptr, nullptr, &m, &opt, out.data(), len.data(), reads) == MRP_OK);
        REQUIRE(reads[1].node_base == 0 && reads[0].flags == RC_STRAND); /* no x_shift: 0; no read_in_hap: nobody in the haplotype */
    }

    /* the sequential restatement on the same input: 255 is overlong, the -inf entry is reachable */
    {
        seq::Input in;
        in.R = R; in.walk_backwards = 1; in.phased = 1; in.s = opt.log_het_substitution;
        in.table = table; in.symbols = symbols; in.counts = counts; in.strand = strand; in.in_hap = hap;
        in.y_off = y_off; in.first = first; in.x_shift = {0, 1, 3}; /* (global node = x + shift: consensus 1 begins at node 3) */
        in.x = x; in.y = y; in.weight = w;
        std::vector<int32_t> c;
        std::vector<double> l;
        seq::estimate(in, c, l);
        REQUIRE(c.size() == 5 && c[0] >= 1 && c[4] == 1 && l[4] == -INFINITY); /* node 4: its only observation is overlong */
    }

    /* mrp_rle_expand */
    {
        const char *s = "AAACGGGGGGGGTNN";
        std::vector<uint8_t> sym(15), cnt(15);
        const int64_t n = mrp_rle_compress(s, 15, 256, sym.data(), cnt.data());
        REQUIRE(n == 5);
        sym.resize((size_t) n); cnt.resize((size_t) n);
        sym.shrink_to_fit(); cnt.shrink_to_fit();
        std::vector<char> back(15);
        REQUIRE(mrp_rle_expand(sym.data(), cnt.data(), nullptr, n, nullptr, 0) == 15);
        REQUIRE(mrp_rle_expand(sym.data(), cnt.data(), nullptr, n, back.data(), 15) == 15 && memcmp(back.data(), s, 15) == 0);
        REQUIRE(mrp_rle_expand(sym.data(), cnt.data(), nullptr, n, back.data(), 14) == -1);
        std::vector<int32_t> c32(cnt.begin(), cnt.end());
        REQUIRE(mrp_rle_expand(sym.data(), nullptr, c32.data(), n, back.data(), 15) == 15 && memcmp(back.data(), s, 15) == 0);
        REQUIRE(mrp_rle_expand(sym.data(), cnt.data(), c32.data(), n, back.data(), 15) == -1 && mrp_rle_expand(sym.data(), nullptr, nullptr, n, back.data(), 15) == -1);
        c32[2] = -1;
        REQUIRE(mrp_rle_expand(sym.data(), nullptr, c32.data(), n, back.data(), 15) == -1 && mrp_rle_expand(nullptr, nullptr, nullptr, 0, nullptr, 0) == 0);
    }
    printf("ok\n");
    return 0;
}

#endif
