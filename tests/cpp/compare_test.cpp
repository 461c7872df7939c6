// Exercises infur::Compare of include/infur_processor.hpp (the confusion matrix and the best partner per value of two planes).
//   compare_test cpu   -- the surface that needs no GPU: feature bits, constants, argument checks
//   compare_test gpu   -- the worked example of include/infur_hip.h word for word (the dense form), and a u32 plane against a u8
//                         plane with 70 x 66 values (the table form) against a double loop over the pixels written out here
#include <cstdio>
#include <cstring>
#include <vector>

#include "infur_processor.hpp"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int cpu_tests() {
    CHECK(infur_abi_version() == INFUR_ABI_VERSION && INFUR_ABI_VERSION == 7);
    CHECK(infur_features() & INFUR_FEATURE_COMPARE);
    CHECK(INFUR_FEATURE_COMPARE == 512 && (infur_features() & 511u) == 511u);  // the nine older bits stay set
    CHECK(INFUR_COMPARE_IGNORE_A == 1 && INFUR_COMPARE_IGNORE_B == 2 && INFUR_COMPARE_WORDS == 4 && INFUR_COMPARE_COUNT_WORDS == 8);
    CHECK(INFUR_COMPARE_PIXELS == 0 && INFUR_COMPARE_PARTNER == 1 && INFUR_COMPARE_INTER == 2 && INFUR_COMPARE_UNION == 3);
    CHECK(INFUR_COMPARE_COMPARED == 0 && INFUR_COMPARE_EQUAL == 1 && INFUR_COMPARE_IGNORED == 2 && INFUR_COMPARE_OUTSIDE == 3 && INFUR_COMPARE_PAIRS == 4 &&
          INFUR_COMPARE_MATCHED == 5 && INFUR_COMPARE_RUNS == 6 && INFUR_COMPARE_STATUS == 7);
    CHECK(INFUR_COMPARE_OVERFLOW == 1 && INFUR_COMPARE_TABLE == 2 && INFUR_COMPARE_NONE == 0xFFFFFFFFu);
    uint32_t b[16], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    const uint8_t* f = (const uint8_t*)b;
    // every rejected call, and a good one: without a context each is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_compare(nullptr, b, 2, b, 1, 2, 2, 0, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);         // elem_a
    CHECK(infur_compare(nullptr, b, 1, b, 1, 2, 2, 4, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);         // an unknown flag bit
    CHECK(infur_compare(nullptr, b, 1, b, 1, 2, 2, 0, 0, 256, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);       // no byte holds 256
    CHECK(infur_compare(nullptr, b, 1, b, 1, 65536, 1, 0, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);     // a side above 65535
    CHECK(infur_compare(nullptr, b, 1, b, 1, 2, 2, 0, 0, 0, b, 1, 1, b, b, b, 48) == INFUR_E_INVALID_ARG);        // slots: no power of two
    CHECK(infur_compare(nullptr, b, 1, b, 1, 2, 2, 0, 0, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, 0) == INFUR_E_INVALID_ARG);  // nothing wanted
    CHECK(infur_compare(nullptr, nullptr, 1, b, 1, 2, 2, 0, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);   // no plane
    CHECK(infur_compare(nullptr, b, 1, b, 1, 2, 2, 0, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);
    CHECK(infur_compare_dev(nullptr, b, 1, b, 1, 2, 2, 0, 0, 0, b, 1, 1, b, b, b, 0) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_compare(nullptr, f, 2, 2, 1.0f, 0, 0, 0, 0, f, 4, nullptr, nullptr, 0, b, 1, 1, b, b, b, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_compare_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 0, 0, b, 4, nullptr, nullptr, 0, b, 1, 1, b, b, b, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Compare compare(c);
    CHECK(compare.is_dirty());
    using Cmd = infur::Compare::Cmd;
    const uint32_t N = INFUR_COMPARE_NONE;
    infur::CompareOut o;
    // the worked example of the header
    const std::vector<uint8_t> a = {0, 0, 1, 1, 0, 1, 1, 2}, b = {0, 0, 0, 1, 0, 1, 1, 1};
    o.rows_a = o.rows_b = 3;
    CHECK(compare.advance(a, b, 2, 4, o) == INFUR_OK && !compare.is_dirty());
    CHECK(o.matrix == (std::vector<uint32_t>{3, 0, 0, 1, 3, 0, 0, 1, 0}) && o.at(1, 0) == 1);
    CHECK(o.a == (std::vector<uint32_t>{3, 0, 3, 4, 4, 1, 3, 5, 1, 1, 1, 4}));
    CHECK(o.b == (std::vector<uint32_t>{4, 0, 3, 4, 4, 1, 3, 5, 0, N, 0, 0}));
    CHECK(o.counts == (std::vector<uint32_t>{8, 6, 0, 0, 4, 2, 6, 0}));
    CHECK(o.matched_a(0) && o.matched_a(1) && !o.matched_a(2) && o.pixel_accuracy() == 0.75);
    // with two values on a's side the pixel with a == 2 is outside
    o.rows_a = 2;
    CHECK(compare.advance(a, b, 2, 4, o) == INFUR_OK && o.count(INFUR_COMPARE_OUTSIDE) == 1 && o.matrix.size() == 6 && o.b[4] == 3);
    // b's 1 ignored: five pixels are compared
    CHECK(compare.control({Cmd::IgnoreB, 1}) == INFUR_OK && compare.is_dirty());
    o.rows_a = 3;
    CHECK(compare.advance(a, b, 2, 4, o) == INFUR_OK && o.count(INFUR_COMPARE_IGNORED) == 4 && o.count(INFUR_COMPARE_COMPARED) == 4);
    CHECK(o.matrix == (std::vector<uint32_t>{3, 0, 0, 1, 0, 0, 0, 0, 0}));
    CHECK(compare.control({Cmd::IgnoreNone, 0}) == INFUR_OK);

    // the table form: 70 x 66 values on a 37 x 70 plane, a as u32 and b as u8, against a double loop over the pixels
    const uint32_t H = 37, W = 70, RA = 70, RB = 66;
    std::vector<uint32_t> pa(H * W);
    std::vector<uint8_t> pb(H * W);
    for (uint32_t i = 0; i < H * W; i++) {
        pa[i] = (i / 3 * 7 + i / W) % 73;  // runs of three; 70, 71, 72 are outside
        pb[i] = (uint8_t)((i / 5 * 11 + i / W) % 66);
    }
    std::vector<uint32_t> m(RA * RB, 0), pix_a(RA, 0), pix_b(RB, 0);
    uint32_t outside = 0, equal = 0, runs = 0, pairs = 0;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t i = y * W + x, va = pa[i], vb = pb[i];
            if (va >= RA) {
                outside++;
                continue;
            }
            m[va * RB + vb]++, pix_a[va]++, pix_b[vb]++;
            equal += va == vb;
            const bool cont = x % 64 != 0 && pa[i - 1] == va && pb[i - 1] == vb;
            runs += !cont;
        }
    o.rows_a = RA, o.rows_b = RB;
    CHECK(compare.advance(pa, pb, H, W, o) == INFUR_OK);
    CHECK(o.matrix == m && o.count(INFUR_COMPARE_STATUS) == INFUR_COMPARE_TABLE && o.count(INFUR_COMPARE_OUTSIDE) == outside && outside > 0);
    CHECK(o.count(INFUR_COMPARE_COMPARED) == H * W && o.count(INFUR_COMPARE_EQUAL) == equal && o.count(INFUR_COMPARE_RUNS) == runs);
    uint32_t matched = 0;
    for (uint32_t i = 0; i < RA; i++) {
        uint32_t best = 0, at = N;
        for (uint32_t j = 0; j < RB; j++) {
            pairs += m[i * RB + j] != 0;
            if (m[i * RB + j] > best) best = m[i * RB + j], at = j;
        }
        const uint32_t uni = best ? pix_a[i] + pix_b[at] - best : 0;
        CHECK(o.a[i * 4] == pix_a[i] && o.a[i * 4 + 1] == at && o.a[i * 4 + 2] == best && o.a[i * 4 + 3] == uni);
        matched += 2ull * best > uni;
    }
    for (uint32_t j = 0; j < RB; j++) {
        uint32_t best = 0, at = N;
        for (uint32_t i = 0; i < RA; i++)
            if (m[i * RB + j] > best) best = m[i * RB + j], at = i;
        CHECK(o.b[j * 4] == pix_b[j] && o.b[j * 4 + 1] == at && o.b[j * 4 + 2] == best && o.b[j * 4 + 3] == (best ? pix_b[j] + pix_a[at] - best : 0));
    }
    CHECK(o.count(INFUR_COMPARE_PAIRS) == pairs && o.count(INFUR_COMPARE_MATCHED) == matched);
    // a table too small for the runs: the overflow is visible, PIXELS and the matrix are still exact
    CHECK(compare.control({Cmd::PairSlots, 64}) == INFUR_OK && compare.is_dirty() && compare.advance(pa, pb, H, W, o) == INFUR_OK);
    CHECK(o.count(INFUR_COMPARE_STATUS) == (INFUR_COMPARE_TABLE | INFUR_COMPARE_OVERFLOW) && o.matrix == m && o.count(INFUR_COMPARE_PAIRS) == 0);
    for (uint32_t i = 0; i < RA; i++) CHECK(o.a[i * 4] == pix_a[i] && o.a[i * 4 + 1] == N && o.a[i * 4 + 2] == 0 && o.a[i * 4 + 3] == 0);
    CHECK(compare.control({Cmd::PairSlots, 48}) == INFUR_OK && compare.advance(pa, pb, H, W, o) == INFUR_E_INVALID_ARG);
    CHECK(compare.control({Cmd::PairSlots, 0}) == INFUR_OK);
    // one output at a time, the empty plane, planes that are not h * w elements
    o.want_matrix = false;
    CHECK(compare.advance(pa, pb, H, W, o) == INFUR_OK && o.matrix.empty() && o.count(INFUR_COMPARE_PAIRS) == pairs);
    o.rows_a = o.rows_b = 2;
    o.want_matrix = true;
    CHECK(compare.advance(std::vector<uint8_t>(), std::vector<uint8_t>(), 3, 0, o) == INFUR_OK);
    CHECK(o.matrix == (std::vector<uint32_t>{0, 0, 0, 0}) && o.a == (std::vector<uint32_t>{0, N, 0, 0, 0, N, 0, 0}) && o.a == o.b);
    CHECK(o.counts == std::vector<uint32_t>(8, 0));
    CHECK(compare.advance(a, b, 3, 5, o) == INFUR_E_SHAPE && compare.advance(a, pb, 2, 4, o) == INFUR_E_SHAPE);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
