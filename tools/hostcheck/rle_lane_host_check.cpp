/*
 * rle_lane_host_check.cpp -- the host half of the run-length lane pairs under the sanitizers, on a machine without a device: the owner
 * search over symbols and counts (substring_owners), the caps (mrp_rle_lane_caps), the eligibility scan and the launch classes
 * (phm_classify with PhmLaunch::rle_lane), the compact repeat table (phm_rle_check_and_build), and the argument errors and the NULL
 * context of mrp_allele_read_supports_rle.  A stand-alone program: the host code of mrp_pairhmm.hip is compiled into it with the
 * sanitizers, everything else comes from the library as built.
 *
 *   cd margin_amd/csrc
 *   F="-std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I."
 *   hipcc $F -x hip -c ../../tools/hostcheck/rle_lane_host_check.cpp -o check_main.o
 *   hipcc $F -c mrp_pairhmm.hip -o check_pairhmm.o
 *   $ROCM/lib/llvm/bin/clang++ -fsanitize=address,undefined check_main.o check_pairhmm.o -L../lib -lmargin_rphmm -L$ROCM/lib -lamdhip64 \
 *         -Wl,-rpath,$PWD/../lib -Wl,-rpath,$ROCM/lib -o rle_lane_host_check
 *   ./rle_lane_host_check      (prints "ok" and returns 0)
 * -Xarch_host: the host code alone is instrumented; the kernels are compiled as ever and never run here.  The program's own objects
 * come first at the link, so their definitions stand in for the library's.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "../../margin_amd/csrc/mrp_pairhmm.h"

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main() {
    /* the caps */
    int32_t cap[4], bound = 0;
    REQUIRE(mrp_rle_lane_caps(2, cap, &bound) == MRP_OK && bound >= 2 && cap[0] <= cap[1] && cap[1] <= cap[2] && cap[2] <= cap[3] && cap[3] <= 100);
    REQUIRE(mrp_rle_lane_caps(0, cap, &bound) == MRP_ERR_ARG && mrp_rle_lane_caps(1, nullptr, nullptr) == MRP_OK);
    for (int32_t n = 1; n <= 300; n++) {
        int32_t c[4];
        REQUIRE(mrp_rle_lane_caps(n, c, nullptr) == MRP_OK);
        for (int k = 0; k < 4; k++) REQUIRE(c[k] >= -1 && c[k] <= 100 && (k == 0 || c[k] >= c[k - 1]) && (c[3] >= 0 || c[k] == -1));
    }
    REQUIRE(mrp_rle_lane_caps(2, cap, &bound) == MRP_OK);

    /* a pool of strings with counts: exactly as long as its last string, so that a read beyond it is seen */
    const int R = 51;
    std::vector<double> table((size_t) 4 * R * R);
    for (size_t i = 0; i < table.size(); i++) table[i] = -0.01 * (double) (i % 97);
    const mrp_repeat_model repeat[2] = {{R, 1, table.data()}, {R, 0, table.data()}};
    mrp_pair_hmm model;
    memset(&model, 0, sizeof(model));
    std::vector<uint8_t> pool, counts;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    auto add = [&](int n, int count_of, int special_at, int special) {
        off.push_back((int64_t) pool.size());
        len.push_back(n);
        for (int i = 0; i < n; i++) {
            pool.push_back((uint8_t) ((i * 7 + n) % 5));
            counts.push_back((uint8_t) (i == special_at ? special : (i * 3 + count_of) % bound));
        }
    };
    /* strings 0..3: alleles (one beyond the last cap); 4..9: reads -- 4 and 6 equal, 5 as 4 with another count, 7 empty, 8 with a count
     * at the bound, 9 with the largest count */
    add(7, 1, -1, 0); add(cap[3], 2, -1, 0); add(cap[3] + 5, 3, -1, 0); add(cap[0] + 1, 4, -1, 0);
    add(9, 1, -1, 0); add(9, 1, 4, (1 * 3 + 1 + 1) % bound); add(9, 1, -1, 0); add(0, 0, -1, 0); add(9, 1, 8, bound); add(9, 1, 0, R - 1);
    pool.shrink_to_fit();
    counts.shrink_to_fit();
    const int64_t pool_bytes = (int64_t) pool.size();

    /* the owner search over symbols and counts */
    {
        const int64_t first[2] = {0, 6};
        std::vector<int64_t> owner;
        substring_owners(1, first, pool.data(), off.data() + 4, len.data() + 4, nullptr, false, owner, counts.data());
        REQUIRE(owner.size() == 6 && owner[0] == 0 && owner[1] == 1 && owner[2] == 0 && owner[3] == 3 && owner[4] == 4 && owner[5] == 5);
        substring_owners(1, first, pool.data(), off.data() + 4, len.data() + 4, nullptr, false, owner); /* symbols alone: 5, 8 and 9 equal 4 too */
        REQUIRE(owner[1] == 0 && owner[2] == 0 && owner[4] == 0 && owner[5] == 0 && owner[3] == 3);
        substring_owners(1, first, pool.data(), off.data() + 4, len.data() + 4, nullptr, true, owner, counts.data());
        REQUIRE(owner[0] == 2 && owner[2] == 2 && owner[1] == 1);
    }

    /* the entry without a context: the argument errors write nothing, a valid call has no device */
    const int64_t allele_first[2] = {0, 4}, read_first[2] = {0, 6};
    const uint8_t strand[6] = {1, 0, 0, 1, 0, 1};
    std::vector<float> support(24, 7.0f);
    auto call = [&](const uint8_t *cnt, const int64_t *rf, int64_t expansion) {
        return mrp_allele_read_supports_rle(nullptr, &model, &model, &repeat[0], &repeat[1], 1, allele_first, rf, pool.data(), cnt, pool_bytes, off.data(), len.data(),
                                            off.data() + 4, len.data() + 4, strand, expansion, support.data(), nullptr);
    };
    REQUIRE(call(counts.data(), read_first, 20) == MRP_ERR_NO_DEVICE);
    REQUIRE(mrp_allele_read_supports_rle(nullptr, &model, &model, &repeat[0], &repeat[1], 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, 20, nullptr, nullptr) == MRP_ERR_NO_DEVICE); /* no bubbles: no array is read */
    REQUIRE(call(nullptr, read_first, 20) == MRP_ERR_ARG && call(counts.data(), read_first, 3) == MRP_ERR_ARG);
    const int64_t descending[2] = {0, -2};
    REQUIRE(call(counts.data(), descending, 20) == MRP_ERR_ARG);
    {
        std::vector<uint8_t> bad(counts);
        bad[(size_t) off[9]] = (uint8_t) R; /* read 5's first count */
        REQUIRE(call(bad.data(), read_first, 20) == MRP_ERR_ARG && strstr(mrp_last_error(), "read 5") != nullptr);
        bad = counts;
        bad[(size_t) off[2] + (size_t) len[2] - 1] = 255; /* the last count of allele 2 */
        REQUIRE(call(bad.data(), read_first, 20) == MRP_ERR_ARG && strstr(mrp_last_error(), "allele 2") != nullptr);
        std::vector<int64_t> beyond(off.begin() + 4, off.end());
        beyond[5] += 1; /* the last read ends one byte behind the pool */
        REQUIRE(mrp_allele_read_supports_rle(nullptr, &model, &model, &repeat[0], &repeat[1], 1, allele_first, read_first, pool.data(), counts.data(), pool_bytes,
                                             off.data(), len.data(), beyond.data(), len.data() + 4, strand, 20, support.data(), nullptr) == MRP_ERR_ARG);
        const mrp_repeat_model wrong = {257, 1, table.data()};
        REQUIRE(mrp_allele_read_supports_rle(nullptr, &model, &model, &repeat[0], &wrong, 1, allele_first, read_first, pool.data(), counts.data(), pool_bytes,
                                             off.data(), len.data(), off.data() + 4, len.data() + 4, strand, 20, support.data(), nullptr) == MRP_ERR_ARG);
        REQUIRE(mrp_allele_read_supports_rle(nullptr, &model, nullptr, &repeat[0], &repeat[1], 1, allele_first, read_first, pool.data(), counts.data(), pool_bytes,
                                             off.data(), len.data(), off.data() + 4, len.data() + 4, strand, 20, support.data(), nullptr) == MRP_ERR_ARG);
    }
    for (float v : support) REQUIRE(v == 7.0f);

    /* the eligibility scan and the launch classes: every allele against every read, lane pairs on and off */
    PhmPairList pairs;
    for (int j = 0; j < 4; j++)
        for (int k = 4; k < 10; k++) pairs.add(off[(size_t) j], len[(size_t) j], off[(size_t) k], len[(size_t) k], (j + k) % 2, nullptr);
    const PhmPairs P = pairs.view();
    PhmRle rle;
    REQUIRE(phm_rle_check_and_build("check", repeat, 2, counts.data(), P, rle) == MRP_OK);
    REQUIRE(rle.rep_lane.size() == (size_t) 2 * 5 * bound * bound);
    for (int m = 0; m < 2; m++)
        for (int cx = 0; cx < 5; cx++)
            for (int u = 0; u < bound; u++)
                for (int o = 0; o < bound; o++)
                    REQUIRE(rle.rep_lane[(((size_t) m * 5 + cx) * bound + u) * bound + o] == rle.rep[(size_t) rle.rep_first[m] + ((size_t) cx * R + u) * R + o]);
    for (int on = 0; on < 2; on++) {
        PhmLaunch L;
        L.rle = &rle;
        L.rle_lane = on != 0;
        const mrp_pair_hmm both[2] = {model, model};
        REQUIRE(phm_classify("check", both, 2, pool_bytes, P, 20, 0, 0, 0, L) == MRP_OK);
        size_t lane = 0, wave = 0;
        for (int c = 0; c < 4; c++) {
            lane += L.lane_pairs[c].size();
            wave += L.wave_pairs[c].size();
            for (const PhmLanePair &p : L.lane_pairs[c]) REQUIRE(p.lx <= cap[c] && (c == 0 || p.lx > cap[c - 1]));
        }
        /* eligible: alleles 0, 1, 3 against reads 4..7 */
        REQUIRE(lane == (on ? 12u : 0u) && lane + wave == 24u);
        if (on) REQUIRE(L.lane_pairs[0].size() == 4 && L.lane_pairs[1].size() == 4 && L.lane_pairs[2].empty() && L.lane_pairs[3].size() == 4);
    }
    {
        /* a small max_repeat: the compact table keeps zeros beyond it */
        std::vector<double> small((size_t) 4 * 3 * 3, -0.5);
        const mrp_repeat_model r3 = {3, 1, small.data()};
        const int64_t o0 = 0;
        const int32_t l2 = 2;
        const uint8_t sym[2] = {0, 4}, cnt[2] = {2, 0};
        const PhmPairs one{1, &o0, &l2, &o0, &l2, nullptr, nullptr, nullptr};
        PhmRle r;
        REQUIRE(phm_rle_check_and_build("check", &r3, 1, cnt, one, r) == MRP_OK && r.rep_lane.size() == (size_t) 5 * bound * bound);
        REQUIRE(r.rep_lane[(size_t) (0 * bound + 2) * bound + 2] == 2.3025 * -0.5 && r.rep_lane[(size_t) (0 * bound + 3) * bound + 0] == 0.0);
        (void) sym;
    }
    printf("ok\n");
    return 0;
}
