/*
 * poa_host_check.cpp -- two programs in one file.
 *
 * (1) The host halves of mrp_poa_augment and mrp_poa_consensus under the sanitizers, on a machine without a device: every argument error
 * (poa_check_and_build) with nothing written, the per-read array and the table sizing it leaves, the keys, mrp_poa_consensus against
 * constants taken from tests/poa_oracle.py, and the NULL context.  A stand-alone program: the host code of mrp_poa.hip and
 * mrp_poa_consensus.cpp is compiled into it with the sanitizers, everything else comes from the library as built.
 *
 *   cd margin_amd/csrc
 *   F="-std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I."
 *   hipcc $F -x hip -c ../../tools/hostcheck/poa_host_check.cpp -o check_main.o
 *   hipcc $F -c mrp_poa.hip -o check_poa.o
 *   $ROCM/lib/llvm/bin/clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c mrp_poa_consensus.cpp -o check_poa_consensus.o
 *   $ROCM/lib/llvm/bin/clang++ -fsanitize=address,undefined check_main.o check_poa.o check_poa_consensus.o -L../lib -lmargin_rphmm -L$ROCM/lib -lamdhip64 \
 *         -Wl,-rpath,$PWD/../lib -Wl,-rpath,$ROCM/lib -o poa_host_check
 *   ./poa_host_check      (prints "ok" and returns 0; tests/test_poa_host.py does exactly this)
 *
 * (2) With -DPOA_TIMING_ONLY, no sanitizer, no HIP and no library: poa_augment, getMaxWeight and the totals as a plain sequential C
 * restatement on one host thread, the yardstick of tools/poa_probe.py.
 *
 *   g++ -O2 -std=c++17 -ffp-contract=off -DPOA_TIMING_ONLY tools/hostcheck/poa_host_check.cpp -o tools/hostcheck/poa_host_time
 *   ./poa_host_time IN OUT   (IN as the probe writes it; writes the outputs to OUT in the probe's order and prints the milliseconds)
 */
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifdef POA_TIMING_ONLY

#include <algorithm>
#include <unordered_set>

/* ---- the sequential restatement: poa.c:176-543, 794-839, 1335-1348 and rle.c:157-176 in the reference's own shape -- a list of inserts
 * and of deletes per node, searched linearly, a set of the read's matches, the two sorts and the (k, l) loops ---- */
namespace seq {

struct Str { std::vector<uint8_t> s; std::vector<int64_t> c; };
struct Insert { Str str; double wf = 0, wr = 0; int64_t n = 0; };
struct Delete { int64_t length = 0; double wf = 0, wr = 0; int64_t n = 0; };
struct Node { double bw[5] = {0, 0, 0, 0, 0}; std::vector<double> rcw; std::vector<Insert> ins; std::vector<Delete> del; };
struct Entry { int64_t w, x, y; };

static bool eq(const uint8_t *sa, const int64_t *ca, int64_t i, const uint8_t *sb, const int64_t *cb, int64_t j, bool cmp) {
    return sa[i] == sb[j] && (!cmp || ca[i] == cb[j]);
}
static bool has_internal_repeat(const Str &s, int64_t n, bool cmp) {
    const int64_t len = (int64_t) s.s.size();
    if (len % n != 0) return false;
    for (int64_t i = n; i < len; i += n)
        for (int64_t j = 0; j < n; j++)
            if (!eq(s.s.data(), s.c.data(), j, s.s.data(), s.c.data(), j + i, cmp)) return false;
    return true;
}
static int64_t get_shift(const Str &ref, int64_t start, const Str &s, bool cmp) {
    const int64_t len = (int64_t) s.s.size();
    int64_t n = 0;
    while (n++ < len)
        if (has_internal_repeat(s, n, cmp)) break;
    for (int64_t k = start - n; k >= 0; k -= n) {
        bool ok = true;
        for (int64_t l = 0; l < n && ok; l++) ok = eq(ref.s.data(), ref.c.data(), k + l, s.s.data(), s.c.data(), l, cmp);
        if (!ok) break;
        start = k;
    }
    if (len == 1 && cmp && start > 0 && ref.s[(size_t) start - 1] == s.s[0]) start--;
    return start;
}
static int64_t common_suffix(const Str &ref, int64_t length1, const Str &s, bool cmp) {
    const int64_t len = (int64_t) s.s.size();
    int64_t i = 0;
    while (length1 - i - 1 >= 0 && len - i - 1 >= 0 && eq(ref.s.data(), ref.c.data(), length1 - 1 - i, s.s.data(), s.c.data(), len - 1 - i, cmp)) i++;
    return i;
}
static void rotate(Str &s, int64_t rotation, bool merge) {
    const int64_t n = (int64_t) s.s.size();
    std::vector<uint8_t> rs((size_t) n);
    std::vector<int64_t> rc((size_t) n);
    for (int64_t i = 0; i < n; i++) {
        rs[(size_t) ((i + rotation) % n)] = s.s[(size_t) i];
        rc[(size_t) ((i + rotation) % n)] = s.c[(size_t) i];
    }
    int64_t j = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!merge || i == 0 || rs[(size_t) i] != rs[(size_t) i - 1]) {
            s.s[(size_t) j] = rs[(size_t) i];
            s.c[(size_t) j++] = rc[(size_t) i];
        } else {
            s.c[(size_t) j - 1] += rc[(size_t) i];
        }
    }
    s.s.resize((size_t) j);
    s.c.resize((size_t) j);
}
static uint64_t key(int64_t x, int64_t y) { return ((uint64_t) (x + 1) << 32) | (uint64_t) (uint32_t) (y + 1); }

static void augment(std::vector<Node> &nodes, const Str &ref, const Str &read, bool strand, int R, std::vector<Entry> &matches, std::vector<Entry> &inserts,
                    std::vector<Entry> &deletes, bool cmp, bool merge) {
    const int64_t L = (int64_t) ref.s.size(), M = (int64_t) read.s.size();
    for (const Entry &m : matches) {
        Node &node = nodes[(size_t) m.x + 1];
        node.bw[read.s[(size_t) m.y]] += (double) m.w;
        const int64_t rc = read.c[(size_t) m.y] < R ? read.c[(size_t) m.y] : R - 1;
        node.rcw[(size_t) rc] += (double) m.w;
    }
    std::unordered_set<uint64_t> set;
    set.reserve(matches.size() * 2);
    for (const Entry &m : matches) set.insert(key(m.x, m.y));
    auto is_match = [&](int64_t x, int64_t y) { return set.count(key(x, y)) != 0; };
    std::sort(inserts.begin(), inserts.end(), [](const Entry &a, const Entry &b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
    for (size_t i = 0; i < inserts.size();) {
        size_t j = i + 1;
        for (; j < inserts.size(); j++)
            if (inserts[i].x != inserts[j].x || inserts[i].y + (int64_t) (j - i) != inserts[j].y) break;
        for (size_t k = i; k < j; k++) {
            const int64_t yk = inserts[i].y + (int64_t) (k - i);
            if (!is_match(inserts[i].x, yk - 1) && yk - 1 > -1) continue;
            for (size_t l = k; l < j; l++) {
                const int64_t yl = inserts[i].y + (int64_t) (l - i);
                if (!is_match(inserts[i].x + 1, yl + 1) && yl + 1 < M) continue;
                Str s;
                s.s.assign(read.s.begin() + yk, read.s.begin() + yl + 1);
                s.c.assign(read.c.begin() + yk, read.c.begin() + yl + 1);
                double w = 4294967295.0;
                for (size_t m = k; m <= l; m++) w = w < (double) inserts[m].w ? w : (double) inserts[m].w;
                int64_t pos = get_shift(ref, inserts[i].x + 1, s, cmp);
                const int64_t suffix = common_suffix(ref, pos, s, cmp);
                if (suffix > 0) {
                    rotate(s, suffix, merge);
                    pos -= suffix;
                }
                Node &node = nodes[(size_t) pos];
                Insert *at = nullptr;
                for (Insert &e : node.ins)
                    if (e.str.s == s.s && e.str.c == s.c) { at = &e; break; }
                if (!at) {
                    node.ins.emplace_back();
                    at = &node.ins.back();
                    at->str = s;
                }
                (strand ? at->wf : at->wr) += w;
                at->n++;
            }
        }
        i = j;
    }
    std::sort(deletes.begin(), deletes.end(), [](const Entry &a, const Entry &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
    for (size_t i = 0; i < deletes.size();) {
        size_t j = i + 1;
        for (; j < deletes.size(); j++)
            if (deletes[i].y != deletes[j].y || deletes[i].x + (int64_t) (j - i) != deletes[j].x) break;
        for (size_t k = i; k < j; k++) {
            const int64_t xk = deletes[i].x + (int64_t) (k - i);
            if (!is_match(xk - 1, deletes[i].y) && xk - 1 > -1) continue;
            for (size_t l = k; l < j; l++) {
                const int64_t xl = deletes[i].x + (int64_t) (l - i);
                if (!is_match(xl + 1, deletes[i].y + 1) && xl + 1 < L) continue;
                const int64_t length = (int64_t) (l - k) + 1;
                double w = 4294967295.0;
                for (size_t m = k; m <= l; m++) w = w < (double) deletes[m].w ? w : (double) deletes[m].w;
                Str s;
                s.s.assign(ref.s.begin() + xk, ref.s.begin() + xk + length);
                s.c.assign(ref.c.begin() + xk, ref.c.begin() + xk + length);
                int64_t pos = get_shift(ref, xk, s, cmp);
                pos -= common_suffix(ref, pos, s, cmp);
                Node &node = nodes[(size_t) pos];
                Delete *at = nullptr;
                for (Delete &e : node.del)
                    if (e.length == length) { at = &e; break; }
                if (!at) {
                    node.del.emplace_back();
                    at = &node.del.back();
                    at->length = length;
                }
                (strand ? at->wf : at->wr) += w;
                at->n++;
            }
        }
        i = j;
    }
}

static int32_t get_max_weight(const double *w, int64_t n, int64_t ref, double penalty) {
    double mx = 0;
    int64_t at = -1;
    for (int64_t j = 0; j < n; j++)
        if (j != ref && w[j] >= mx) { mx = w[j]; at = j; }
    return (int32_t) (w[ref] * penalty >= mx ? ref : at);
}

}  // namespace seq

template <class T>
static void get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> h, node_first, read_first, y_off, first[3];
    std::vector<double> pen;
    std::vector<uint8_t> symbols, ref_counts, read_s, read_c, strand;
    std::vector<int32_t> y_len, x_shift, lx[3], ly[3], lw[3];
    get(f, h, 6); /* R, n_consensus, pool_bytes, compare, merge, n_reads */
    get(f, pen, 1);
    const int R = (int) h[0];
    const int64_t n_consensus = h[1], n_reads = h[5];
    get(f, node_first, (size_t) n_consensus + 1);
    get(f, symbols, (size_t) node_first.back());
    get(f, ref_counts, (size_t) node_first.back());
    get(f, read_first, (size_t) n_consensus + 1);
    get(f, read_s, (size_t) h[2]);
    get(f, read_c, (size_t) h[2]);
    get(f, y_off, (size_t) n_reads);
    get(f, y_len, (size_t) n_reads);
    get(f, strand, (size_t) n_reads);
    get(f, x_shift, (size_t) n_reads);
    for (int q = 0; q < 3; q++) { /* matches, deletes, inserts */
        get(f, first[q], (size_t) n_reads + 1);
        get(f, lx[q], (size_t) first[q].back());
        get(f, ly[q], (size_t) first[q].back());
        get(f, lw[q], (size_t) first[q].back());
    }
    fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> base_weight, wf, wr, dwf, dwr, totals;
    std::vector<int32_t> base_pick, count_pick, str_len, pool_c, del_len;
    std::vector<int64_t> ins_first{0}, str_off, nobs, del_first{0}, dnobs;
    std::vector<uint8_t> pool_s;
    for (int64_t c = 0; c < n_consensus; c++) {
        seq::Str ref;
        ref.s.assign(symbols.begin() + node_first[(size_t) c], symbols.begin() + node_first[(size_t) c + 1]);
        for (int64_t k = node_first[(size_t) c]; k < node_first[(size_t) c + 1]; k++) ref.c.push_back(ref_counts[(size_t) k]);
        std::vector<seq::Node> nodes(ref.s.size() + 1);
        for (seq::Node &n : nodes) n.rcw.assign((size_t) R, 0.0);
        for (int64_t r = read_first[(size_t) c]; r < read_first[(size_t) c + 1]; r++) {
            seq::Str read;
            read.s.assign(read_s.begin() + y_off[(size_t) r], read_s.begin() + y_off[(size_t) r] + y_len[(size_t) r]);
            for (int64_t k = 0; k < y_len[(size_t) r]; k++) read.c.push_back(read_c[(size_t) (y_off[(size_t) r] + k)]);
            std::vector<seq::Entry> l[3];
            for (int q = 0; q < 3; q++)
                for (int64_t i = first[q][(size_t) r]; i < first[q][(size_t) r + 1]; i++)
                    l[q].push_back({lw[q][(size_t) i], (int64_t) lx[q][(size_t) i] + x_shift[(size_t) r], ly[q][(size_t) i]});
            seq::augment(nodes, ref, read, strand[(size_t) r] != 0, R, l[0], l[2], l[1], h[3] != 0, h[4] != 0);
        }
        double t[4] = {0, 0, 0, 0};
        for (size_t k = 0; k < nodes.size(); k++) {
            const seq::Node &n = nodes[k];
            const int sym = k == 0 ? 4 : ref.s[k - 1];
            const int64_t cnt = k == 0 ? 1 : ref.c[k - 1];
            base_weight.insert(base_weight.end(), n.bw, n.bw + 5);
            base_pick.push_back(seq::get_max_weight(n.bw, 5, sym, pen[0]));
            count_pick.push_back(seq::get_max_weight(n.rcw.data(), R, cnt, pen[0]));
            t[0] += n.bw[sym];
            for (int j = 0; j < 5; j++)
                if (j != sym) t[1] += n.bw[j];
            for (const seq::Insert &e : n.ins) {
                t[2] += (e.wf + e.wr) * (double) e.str.s.size();
                str_off.push_back((int64_t) pool_s.size());
                str_len.push_back((int32_t) e.str.s.size());
                pool_s.insert(pool_s.end(), e.str.s.begin(), e.str.s.end());
                for (int64_t v : e.str.c) pool_c.push_back((int32_t) v);
                wf.push_back(e.wf);
                wr.push_back(e.wr);
                nobs.push_back(e.n);
            }
            for (const seq::Delete &e : n.del) {
                t[3] += (e.wf + e.wr) * (double) e.length;
                del_len.push_back((int32_t) e.length);
                dwf.push_back(e.wf);
                dwr.push_back(e.wr);
                dnobs.push_back(e.n);
            }
            ins_first.push_back((int64_t) str_len.size());
            del_first.push_back((int64_t) del_len.size());
        }
        totals.insert(totals.end(), t, t + 4);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    put(o, base_weight); put(o, base_pick); put(o, count_pick); put(o, ins_first); put(o, str_off); put(o, str_len); put(o, wf); put(o, wr); put(o, nobs);
    put(o, pool_s); put(o, pool_c); put(o, del_first); put(o, del_len); put(o, dwf); put(o, dwr); put(o, dnobs); put(o, totals);
    fclose(o);
    printf("%.3f\n", ms);
    return 0;
}

#else /* ---- the sanitized host check ---- */

#include "mrp_poa.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

struct Call { /* two consensus strings: 3 positions under 2 reads (the second cropped by 1), 2 positions under 1 read */
    int32_t R = 12;
    std::vector<int64_t> node_first{0, 3, 5}, read_first{0, 2, 3}, y_off{0, 3, 5};
    std::vector<uint8_t> symbols{0, 1, 4, 2, 3}, ref_counts{1, 2, 3, 1, 1}, read_s{0, 1, 2, 1, 3, 2, 3}, read_c{1, 2, 3, 2, 9, 1, 1}, strand{1, 0, 1};
    std::vector<int32_t> y_len{3, 2, 2}, x_shift{0, 1, 0};
    std::vector<int64_t> mf{0, 3, 5, 7}, df{0, 1, 2, 2}, inf{0, 2, 3, 3};
    std::vector<int32_t> mx{0, 1, 2, 0, 1, 0, 1}, my{0, 1, 2, 0, 1, 0, 1}, mw{5, 7, 1, 3, 4, 9, 9};
    std::vector<int32_t> dx{1, 0}, dy{0, -1}, dw{4, 6}, ix{0, -1, 1}, iy{1, 0, 1}, iw{3, 2, 2};
    mrp_posterior_pairs m, d, i;
    mrp_poa_options opt{1, 1, 0.5, 0, 0, 0};
    mrp_poa out;
    HostVec<PoaRead> reads;
    int64_t slots = -7;
    Call() { memset(&out, 0x5a, sizeof(out)); bind(); }
    void bind() {
        m = {mf.data(), mx.data(), my.data(), mw.data(), nullptr};
        d = {df.data(), dx.data(), dy.data(), dw.data(), nullptr};
        i = {inf.data(), ix.data(), iy.data(), iw.data(), nullptr};
    }
    int check() {
        bind();
        return poa_check_and_build("check", R, 2, node_first.data(), symbols.data(), ref_counts.data(), read_first.data(), read_s.data(), read_c.data(),
                                   (int64_t) read_s.size(), y_off.data(), y_len.data(), strand.data(), x_shift.data(), &m, &d, &i, &opt, &out, reads, &slots);
    }
    bool untouched() const {
        const unsigned char *p = (const unsigned char *) &out;
        for (size_t k = 0; k < sizeof(out); k++)
            if (p[k] != 0x5a) return false;
        return slots == -7;
    }
};

template <class F>
static void refused(F change) {
    Call c;
    change(c);
    CHECK(c.check() == MRP_ERR_ARG);
    CHECK(c.untouched());
}

int main() {
    /* the table sizing and the keys */
    CHECK(poa_table_lg(0) == -1 && poa_table_lg(1) == 1 && poa_table_lg(2) == 2 && poa_table_lg(3) == 3 && poa_table_lg(4) == 3 && poa_table_lg(5) == 4);
    for (int64_t n : {1ll, 7ll, 64ll, 65ll, 1000ll, (1ll << 31) - 1}) {
        const int lg = poa_table_lg(n);
        CHECK((1ll << lg) >= 2 * n && (1ll << (lg - 1)) < 2 * n && lg <= 32);
        for (int64_t x : {-1ll, 0ll, 5ll, (1ll << 31) - 2})
            for (int64_t y : {-1ll, 0ll, 9ll, (1ll << 31) - 2}) {
                if (x == -1 && y == -1) continue;
                CHECK(poa_key(x, y) != 0 && (uint64_t) poa_slot(poa_key(x, y), lg) < (1ull << lg));
            }
    }
    CHECK(poa_key(-1, 0) == 1 && poa_key(0, -1) == (1ull << 32) && poa_key(3, 4) == ((4ull << 32) | 5));
    PoaRecord a{}, b{};
    a.key_hi = 1; a.key_lo = 9; b.key_hi = 2; b.key_lo = 0;
    CHECK(poa_key_less(a, b) && !poa_key_less(b, a) && !poa_key_less(a, a));
    b.key_hi = 1;
    CHECK(poa_key_less(b, a));
    CHECK(sizeof(PoaRecord) == 40 && sizeof(PoaRead) == 80);
    /* the well-formed call: the per-read array */
    {
        Call c;
        CHECK(c.check() == MRP_OK);
        CHECK(c.reads.size() == 3 && c.slots == (8 + 2 + 4) + (4 + 2 + 2) + (4 + 0 + 0));
        CHECK(c.reads[0].node_base == 0 && c.reads[1].node_base == 0 && c.reads[2].node_base == 4 && c.reads[2].ref_base == 3);
        CHECK(c.reads[1].shift == 1 && c.reads[1].strand == 0 && c.reads[1].L == 3 && c.reads[2].L == 2 && c.reads[2].cons == 1 && c.reads[1].y_off == 3);
        CHECK(c.reads[0].lg[0] == 3 && c.reads[0].lg[1] == 1 && c.reads[0].lg[2] == 2 && c.reads[2].lg[1] == -1 && c.reads[2].lg[2] == -1);
        CHECK(c.reads[0].table[0] == 0 && c.reads[0].table[1] == 8 && c.reads[0].table[2] == 10 && c.reads[1].table[0] == 14 && c.reads[2].table[0] == 22);
        c.slots = -7;
        CHECK(c.untouched());
        /* the NULL context comes after the checks, with nothing written */
        mrp_poa_stats st;
        memset(&st, 0x5a, sizeof(st));
        CHECK(mrp_poa_augment(nullptr, c.R, 2, c.node_first.data(), c.symbols.data(), c.ref_counts.data(), c.read_first.data(), c.read_s.data(), c.read_c.data(),
                              (int64_t) c.read_s.size(), c.y_off.data(), c.y_len.data(), c.strand.data(), c.x_shift.data(), &c.m, &c.d, &c.i, &c.opt, &c.out,
                              &st) == MRP_ERR_NO_DEVICE);
        CHECK(c.untouched() && ((const unsigned char *) &st)[0] == 0x5a && strstr(mrp_last_error(), "no context"));
        c.R = 1;
        CHECK(mrp_poa_augment(nullptr, c.R, 2, c.node_first.data(), c.symbols.data(), c.ref_counts.data(), c.read_first.data(), c.read_s.data(), c.read_c.data(),
                              (int64_t) c.read_s.size(), c.y_off.data(), c.y_len.data(), c.strand.data(), c.x_shift.data(), &c.m, &c.d, &c.i, &c.opt, &c.out,
                              &st) == MRP_ERR_ARG);
    }
    /* every argument error, with nothing written */
    refused([](Call &c) { c.R = 1; });
    refused([](Call &c) { c.R = 256; });
    refused([](Call &c) { c.opt.compare_repeat_counts = 2; });
    refused([](Call &c) { c.opt.merge_ends = -1; });
    refused([](Call &c) { c.opt.want_repeat_count_weight = 3; });
    refused([](Call &c) { c.opt.reference_base_penalty = NAN; });
    refused([](Call &c) { c.opt.reference_base_penalty = -1.0; });
    refused([](Call &c) { c.opt.reserved = 1; });
    refused([](Call &c) { c.opt.reserved2 = 1; });
    refused([](Call &c) { c.node_first[0] = 1; });
    refused([](Call &c) { c.node_first[2] = 2; });
    refused([](Call &c) { c.read_first[1] = -1; });
    refused([](Call &c) { c.symbols[1] = 5; });
    refused([](Call &c) { c.ref_counts[3] = 0; });
    refused([](Call &c) { c.ref_counts[2] = 12; });
    refused([](Call &c) { c.y_off[2] = 6; });
    refused([](Call &c) { c.y_len[1] = -1; });
    refused([](Call &c) { c.read_s[4] = 7; });
    refused([](Call &c) { c.mf[0] = 1; });
    refused([](Call &c) { c.df[2] = 0; });
    refused([](Call &c) { c.inf[1] = 4; c.inf[2] = 3; });
    refused([](Call &c) { c.my[4] = 2; });
    refused([](Call &c) { c.my[5] = -1; });
    refused([](Call &c) { c.mx[4] = 2; });
    refused([](Call &c) { c.mx[0] = -1; });
    refused([](Call &c) { c.dx[0] = -1; });
    refused([](Call &c) { c.dx[0] = 3; });
    refused([](Call &c) { c.dy[1] = -2; });
    refused([](Call &c) { c.dy[1] = 2; });
    refused([](Call &c) { c.ix[1] = -2; });
    refused([](Call &c) { c.ix[2] = 2; });
    refused([](Call &c) { c.iy[0] = -1; });
    refused([](Call &c) { c.iy[0] = 3; });
    refused([](Call &c) { c.mw[1] = -7; });
    refused([](Call &c) { c.dw[1] = -7; });
    refused([](Call &c) { c.iw[2] = -7; });
    refused([](Call &c) { c.x_shift[0] = 1; });
    {
        Call c;
        c.bind();
        CHECK(poa_check_and_build("check", c.R, 2, nullptr, c.symbols.data(), c.ref_counts.data(), c.read_first.data(), c.read_s.data(), c.read_c.data(), 7,
                                  c.y_off.data(), c.y_len.data(), c.strand.data(), nullptr, &c.m, &c.d, &c.i, &c.opt, &c.out, c.reads, &c.slots) == MRP_ERR_ARG);
        CHECK(poa_check_and_build("check", c.R, 2, c.node_first.data(), c.symbols.data(), c.ref_counts.data(), c.read_first.data(), c.read_s.data(), c.read_c.data(), 7,
                                  c.y_off.data(), c.y_len.data(), c.strand.data(), nullptr, &c.m, nullptr, &c.i, &c.opt, &c.out, c.reads, &c.slots) == MRP_ERR_ARG);
        c.m.x = nullptr;
        CHECK(poa_check_and_build("check", c.R, 2, c.node_first.data(), c.symbols.data(), c.ref_counts.data(), c.read_first.data(), c.read_s.data(), c.read_c.data(), 7,
                                  c.y_off.data(), c.y_len.data(), c.strand.data(), nullptr, &c.m, &c.d, &c.i, &c.opt, &c.out, c.reads, &c.slots) == MRP_ERR_ARG);
        CHECK(c.untouched());
    }
    /* mrp_poa_consensus on the graph of the reference's vector (tests/golden/poa/augment_example.json); the expected values are
     * tests/poa_oracle.py's consensus() */
    {
        const double bw[8 * 5] = {0, 0, 0, 0, 0, 0, 0, 100, 0, 0, 100, 0, 0, 0, 0, 0, 0, 0, 50, 0, 0, 0, 0, 50, 0, 100, 0, 0, 0, 0, 0, 100, 0, 0, 0, 0, 0, 75, 25, 0};
        const int32_t base_pick[8] = {4, 2, 0, 3, 3, 0, 1, 2}, count_pick[8] = {1, 1, 1, 1, 1, 1, 1, 0 /* the 0 -> 1 rule */};
        const int64_t ins_first[9] = {0, 0, 0, 0, 0, 0, 0, 2, 4}, str_off[4] = {0, 1, 3, 5}, del_first[9] = {0, 0, 0, 1, 1, 1, 1, 1, 1};
        const int32_t str_len[4] = {1, 2, 2, 1}, pool_c[6] = {1, 1, 1, 1, 1, 1}, del_len[1] = {1};
        const uint8_t pool_s[6] = {2, 2, 2, 2, 3, 3};
        const double wf[4] = {50, 25, 50, 75}, wr[4] = {0, 0, 0, 0}, dwf[1] = {100}, dwr[1] = {0};
        for (int rle = 1; rle >= 0; rle--) {
            uint8_t *s = nullptr;
            int32_t *c = nullptr;
            int64_t n = -7, *map = nullptr;
            CHECK(mrp_poa_consensus(7, bw, base_pick, count_pick, ins_first, str_off, str_len, wf, wr, pool_s, pool_c, 6, del_first, del_len, dwf, dwr, rle, &s, &c, &n,
                                    &map) == MRP_OK);
            const uint8_t want_rle[7] = {2, 0, 3, 0, 1, 2, 3}, want_plain[8] = {2, 0, 3, 0, 1, 2, 2, 3};
            const int32_t counts_rle[7] = {1, 1, 1, 1, 1, 2, 1};
            const int64_t map_rle[7] = {0, 1, -1, 2, 3, 4, 5}, map_plain[7] = {0, 1, -1, 2, 3, 4, 6};
            CHECK(n == (rle ? 7 : 8));
            if (s && c && map && n == (rle ? 7 : 8)) {
                CHECK(memcmp(s, rle ? want_rle : want_plain, (size_t) n) == 0);
                for (int64_t k = 0; k < n; k++) CHECK(c[k] == (rle ? counts_rle[k] : 1));
                CHECK(memcmp(map, rle ? map_rle : map_plain, sizeof(map_rle)) == 0);
            }
            mrp_free(s);
            mrp_free(c);
            mrp_free(map);
        }
        /* a zero-length reference; refusals with nothing written */
        uint8_t *s = nullptr;
        int32_t *c = nullptr;
        int64_t n = -7, *map = nullptr;
        const int64_t zero[2] = {0, 0};
        CHECK(mrp_poa_consensus(0, bw, base_pick, count_pick, zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, zero, nullptr, nullptr, nullptr, 1, &s, &c, &n,
                                &map) == MRP_OK);
        CHECK(n == 0 && s && c && map);
        mrp_free(s);
        mrp_free(c);
        mrp_free(map);
        s = nullptr; c = nullptr; map = nullptr; n = -7;
        const double nan_wf[4] = {50, 25, NAN, 75};
        CHECK(mrp_poa_consensus(7, bw, base_pick, count_pick, ins_first, str_off, str_len, nan_wf, wr, pool_s, pool_c, 6, del_first, del_len, dwf, dwr, 1, &s, &c, &n,
                                &map) == MRP_ERR_ARG);
        CHECK(strstr(mrp_last_error(), "the reference dereferences NULL") != nullptr);
        const int32_t long_del[1] = {7};
        CHECK(mrp_poa_consensus(7, bw, base_pick, count_pick, ins_first, str_off, str_len, wf, wr, pool_s, pool_c, 6, del_first, long_del, dwf, dwr, 1, &s, &c, &n,
                                &map) == MRP_ERR_ARG);
        CHECK(mrp_poa_consensus(7, bw, base_pick, count_pick, ins_first, str_off, str_len, wf, wr, pool_s, pool_c, 5, del_first, del_len, dwf, dwr, 1, &s, &c, &n,
                                &map) == MRP_ERR_ARG);
        CHECK(mrp_poa_consensus(7, nullptr, base_pick, count_pick, ins_first, str_off, str_len, wf, wr, pool_s, pool_c, 6, del_first, del_len, dwf, dwr, 1, &s, &c, &n,
                                &map) == MRP_ERR_ARG);
        CHECK(!s && !c && !map && n == -7);
    }
    mrp_poa zeroed;
    memset(&zeroed, 0, sizeof(zeroed));
    mrp_poa_free(&zeroed);
    mrp_poa_free(nullptr);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}

#endif
