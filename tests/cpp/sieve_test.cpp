// Exercises infur::Adjacency and infur::Sieve of include/infur_processor.hpp (the region adjacency graph, and speckle regions
// merged into their neighbours).
//   sieve_test cpu   -- the surface that needs no GPU: feature bits, constants, argument checks
//   sieve_test gpu   -- the worked example of include/infur_hip.h word for word through Regions -> Adjacency and Regions -> Sieve, a
//                       striped plane against counts written out here, the overflow and the rounds rules
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
    CHECK(infur_features() & INFUR_FEATURE_SIEVE);
    CHECK(INFUR_FEATURE_SIEVE == 1024 && (infur_features() & 1023u) == 1023u);  // the ten older bits stay set
    CHECK(INFUR_ADJ_SKIP == 1 && INFUR_ADJ_PAIR_WORDS == 4 && INFUR_ADJ_ROW_WORDS == 4 && INFUR_ADJ_COUNT_WORDS == 8);
    CHECK(INFUR_ADJ_A == 0 && INFUR_ADJ_B == 1 && INFUR_ADJ_BORDER == 2 && INFUR_ADJ_FIRST == 3);
    CHECK(INFUR_ADJ_DEGREE == 0 && INFUR_ADJ_LONGEST == 1 && INFUR_ADJ_ROW_BORDER == 2 && INFUR_ADJ_PERIMETER == 3);
    CHECK(INFUR_ADJ_PAIRS == 0 && INFUR_ADJ_EDGES == 1 && INFUR_ADJ_SKIPPED == 2 && INFUR_ADJ_OUTSIDE == 3 && INFUR_ADJ_RUNS == 4 && INFUR_ADJ_WRITTEN == 5 &&
          INFUR_ADJ_STATUS == 7);
    CHECK(INFUR_ADJ_OVERFLOW == 1 && INFUR_ADJ_TRUNCATED == 2 && INFUR_ADJ_NONE == 0xFFFFFFFFu);
    CHECK(INFUR_SIEVE_CLASS == 0 && INFUR_SIEVE_INTO == 1 && INFUR_SIEVE_ROUND == 2 && INFUR_SIEVE_BORDER == 3 && INFUR_SIEVE_ROW_WORDS == 4);
    CHECK(INFUR_SIEVE_REGIONS == 0 && INFUR_SIEVE_SMALL == 1 && INFUR_SIEVE_ABSORBED == 2 && INFUR_SIEVE_STRANDED == 3 && INFUR_SIEVE_ROUNDS == 4 &&
          INFUR_SIEVE_PIXELS_CHANGED == 5 && INFUR_SIEVE_PAIRS == 6 && INFUR_SIEVE_STATUS == 7 && INFUR_SIEVE_COUNT_WORDS == 8);
    CHECK(INFUR_SIEVE_OVERFLOW == 1 && INFUR_SIEVE_ROUNDS_EXHAUSTED == 2 && INFUR_SIEVE_TABLE_SHORT == 4 && INFUR_SIEVE_NONE == 0xFFFFFFFFu);
    uint32_t b[32], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    const uint8_t* f = (const uint8_t*)b;
    uint8_t* g = (uint8_t*)b;
    const uint64_t* t = (const uint64_t*)b;
    uint64_t* u = (uint64_t*)b;
    // every rejected call, and a good one: without a context each is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_adjacency(nullptr, b, 2, 2, 2, 0, 0, 4, b, 4, b, b, 0) == INFUR_E_INVALID_ARG);    // elem
    CHECK(infur_adjacency(nullptr, b, 1, 2, 2, 2, 0, 4, b, 4, b, b, 0) == INFUR_E_INVALID_ARG);    // an unknown flag bit
    CHECK(infur_adjacency(nullptr, b, 1, 2, 2, 1, 256, 4, b, 4, b, b, 0) == INFUR_E_INVALID_ARG);  // no byte holds 256
    CHECK(infur_adjacency(nullptr, b, 1, 2, 2, 0, 0, 4, b, 4, b, b, 48) == INFUR_E_INVALID_ARG);   // slots: no power of two
    CHECK(infur_adjacency(nullptr, b, 1, 2, 2, 0, 0, 4, b, 4, b, b, 0) == INFUR_E_INVALID_ARG);
    CHECK(infur_adjacency_dev(nullptr, b, 1, 2, 2, 0, 0, 4, b, 4, b, b, 0) == INFUR_E_INVALID_ARG);
    CHECK(infur_sieve(nullptr, f, b, t, 1, 1, 2, 2, 2, 65, 0, g, b, b) == INFUR_E_INVALID_ARG);  // max_rounds
    CHECK(infur_sieve(nullptr, f, b, t, 1, 1, 2, 2, 2, 0, 100, g, b, b) == INFUR_E_INVALID_ARG);  // slots
    CHECK(infur_sieve(nullptr, f, b, t, 1, 1, 2, 2, 2, 0, 0, g, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_sieve_dev(nullptr, b, b, b, 1, b, 2, 2, 2, 0, 0, b, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_sieve(nullptr, f, 2, 2, 1.0f, 0, 0, 8, 2, 0, g, g, 4, b, 16, u, 1, b, nullptr, &ow, &oh, 0, 0, g, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_sieve_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 8, 2, 0, b, b, 4, b, 16, b, 1, b, nullptr, &ow, &oh, 0, 0, b, b) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 32; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    const uint32_t N = INFUR_ADJ_NONE;
    using V = std::vector<uint32_t>;
    // the worked example of the header: a 4 x 6 plane of two classes with two speckles, one of which needs two rounds
    infur::Planes p;
    p.width = 6, p.height = 4;
    p.klass = {1, 1, 1, 2, 2, 2, 1, 3, 1, 2, 2, 2, 1, 1, 1, 2, 4, 4, 1, 1, 1, 2, 4, 5};
    infur::Regions regions(c, INFUR_CONNECT_4);
    infur::RegionsOut r;
    r.table_rows = 8;
    CHECK(regions.advance(p, r) == INFUR_OK && r.n == 5);
    CHECK(r.labels == (V{0, 0, 0, 1, 1, 1, 0, 2, 0, 1, 1, 1, 0, 0, 0, 1, 3, 3, 0, 0, 0, 1, 3, 4}));

    infur::Adjacency adjacency(c);
    CHECK(adjacency.is_dirty());
    infur::AdjacencyOut a;
    a.rows = 5, a.pair_rows = 8;
    CHECK(adjacency.advance(r.labels, 4, 6, a) == INFUR_OK && !adjacency.is_dirty());
    CHECK(a.pairs == (V{0, 2, 4, 3, 0, 1, 4, 4, 1, 3, 4, 21, 3, 4, 2, 35}) && a.n_pairs() == 4);
    CHECK(a.table == (V{2, 1, 4, 18, 2, 0, 4, 14, 1, 0, 4, 4, 2, 1, 4, 8, 1, 3, 2, 4}));
    CHECK(a.counts == (V{4, 14, 0, 0, 9, 4, 0, 0}));
    CHECK(a.border(3, 1) == 4 && a.border(4, 3) == 2 && a.border(0, 4) == 0);
    // two records fit: truncated, and the first two in order of FIRST
    a.pair_rows = 2;
    CHECK(adjacency.advance(r.labels, 4, 6, a) == INFUR_OK && a.pairs == (V{0, 2, 4, 3, 0, 1, 4, 4}));
    CHECK(a.count(INFUR_ADJ_WRITTEN) == 2 && a.count(INFUR_ADJ_STATUS) == INFUR_ADJ_TRUNCATED && a.count(INFUR_ADJ_PAIRS) == 4);
    // the class plane itself, class 1 skipped: 3 touches nothing any more
    using ACmd = infur::Adjacency::Cmd;
    CHECK(adjacency.control({ACmd::Skip, 1}) == INFUR_OK && adjacency.is_dirty());
    a.rows = 6, a.pair_rows = 8;
    CHECK(adjacency.advance(p.klass, 4, 6, a) == INFUR_OK);
    CHECK(a.pairs == (V{2, 4, 4, 21, 4, 5, 2, 35}) && a.count(INFUR_ADJ_SKIPPED) == 11 && a.table[3 * 4 + 1] == N && a.table[3 * 4 + 3] == 4);
    CHECK(adjacency.control({ACmd::SkipNone, 0}) == INFUR_OK);

    // vertical stripes one pixel wide, 5 x 64, as a u8 plane of 64 values: 63 pairs of border 5, R = 63
    const uint32_t H = 5, W = 64;
    std::vector<uint8_t> stripes(H * W);
    for (uint32_t i = 0; i < H * W; i++) stripes[i] = (uint8_t)(i % W);
    a.rows = 64, a.pair_rows = 64;
    CHECK(adjacency.advance(stripes, H, W, a) == INFUR_OK && a.n_pairs() == 63 && a.count(INFUR_ADJ_RUNS) == 63 && a.count(INFUR_ADJ_EDGES) == 315);
    for (uint32_t i = 0; i < 63; i++) CHECK(a.pairs[i * 4] == i && a.pairs[i * 4 + 1] == i + 1 && a.pairs[i * 4 + 2] == 5 && a.pairs[i * 4 + 3] == 2 * i);
    for (uint32_t v = 0; v < 64; v++) {
        const uint32_t deg = v == 0 || v == 63 ? 1 : 2;
        CHECK(a.table[v * 4] == deg && a.table[v * 4 + 1] == (v == 0 ? 1 : v - 1) && a.table[v * 4 + 2] == 5 && a.table[v * 4 + 3] == 2 * H + 2);
    }
    // 2 R = 126 > 64 slots: the overflow is visible, the perimeters are still exact
    CHECK(adjacency.control({ACmd::PairSlots, 64}) == INFUR_OK && adjacency.advance(stripes, H, W, a) == INFUR_OK);
    CHECK(a.count(INFUR_ADJ_STATUS) == INFUR_ADJ_OVERFLOW && a.n_pairs() == 0 && a.count(INFUR_ADJ_PAIRS) == 0 && a.count(INFUR_ADJ_RUNS) == 63);
    for (uint32_t v = 0; v < 64; v++) CHECK(a.table[v * 4] == 0 && a.table[v * 4 + 1] == N && a.table[v * 4 + 2] == 0 && a.table[v * 4 + 3] == 2 * H + 2);
    CHECK(adjacency.control({ACmd::PairSlots, 48}) == INFUR_OK && adjacency.advance(stripes, H, W, a) == INFUR_E_INVALID_ARG);
    CHECK(adjacency.advance(stripes, H, W + 1, a) == INFUR_E_SHAPE);

    // Sieve of the worked example
    infur::Sieve sieve(c, 4);
    infur::SieveOut s;
    CHECK(sieve.is_dirty() && sieve.advance(p.klass, r, s) == INFUR_OK && !sieve.is_dirty());
    CHECK(s.rows == (V{1, 0, 0, 0, 2, 1, 0, 0, 1, 0, 1, 4, 2, 1, 1, 4, 2, 1, 2, 2}));
    CHECK(s.counts == (V{5, 3, 3, 0, 2, 5, 4, 0}));
    for (uint32_t i = 0; i < 24; i++) CHECK(s.klass[i] == (i % 6 < 3 ? 1 : 2));
    // one round leaves region 4 stranded, and says so
    using SCmd = infur::Sieve::Cmd;
    CHECK(sieve.control({SCmd::MaxRounds, 65}) == INFUR_E_INVALID_ARG && !sieve.is_dirty());
    CHECK(sieve.control({SCmd::MaxRounds, 1}) == INFUR_OK && sieve.is_dirty() && sieve.advance(p.klass, r, s) == INFUR_OK);
    CHECK(s.counts == (V{5, 3, 2, 1, 1, 4, 4, INFUR_SIEVE_ROUNDS_EXHAUSTED}) && s.word(4, INFUR_SIEVE_ROUND) == INFUR_SIEVE_NONE && s.klass[23] == 5);
    // a table too small for the runs: nothing merges, the plane is copied
    CHECK(sieve.control({SCmd::MaxRounds, 0}) == INFUR_OK && sieve.control({SCmd::PairSlots, 64}) == INFUR_OK);
    p.width = W, p.height = H, p.klass = stripes;
    r.table_rows = 64;
    CHECK(regions.advance(p, r) == INFUR_OK && r.n == 64);
    CHECK(sieve.control({SCmd::MinPixels, 6}) == INFUR_OK && sieve.advance(stripes, r, s) == INFUR_OK);
    CHECK(s.counts == (V{64, 64, 0, 64, 0, 0, 0, INFUR_SIEVE_OVERFLOW}) && s.klass == stripes);
    // with room, every stripe is small and none is kept: all stranded, ROUNDS 0
    CHECK(sieve.control({SCmd::PairSlots, 0}) == INFUR_OK && sieve.advance(stripes, r, s) == INFUR_OK);
    CHECK(s.counts == (V{64, 64, 0, 64, 0, 0, 63, 0}) && s.klass == stripes);
    // a threshold of 5 keeps them all
    CHECK(sieve.control({SCmd::MinPixels, 5}) == INFUR_OK && sieve.advance(stripes, r, s) == INFUR_OK && s.counts == (V{64, 0, 0, 0, 0, 0, 63, 0}));
    r.want_labels = false;
    CHECK(regions.advance(p, r) == INFUR_OK && sieve.advance(stripes, r, s) == INFUR_E_SHAPE);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
