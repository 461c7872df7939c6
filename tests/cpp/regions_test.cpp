// Exercises infur::Regions of include/infur_processor.hpp (connected components of the class plane: labels, table, count).
//   regions_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   regions_test gpu   -- hand-written known answers: a 3 x 3 checkerboard, two rectangles across tile borders with the
//                         min_pixels / skip-background / truncation rules, and the command validation
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
    CHECK(infur_abi_version() == INFUR_ABI_VERSION);
    CHECK(infur_features() & INFUR_FEATURE_REGIONS);
    CHECK(INFUR_REGION_WORDS == 10 && INFUR_REGION_CLASS == 8 && INFUR_REGION_FIRST == 9 && INFUR_REGION_NONE == 0xFFFFFFFFu);
    CHECK(INFUR_CONNECT_4 == 4 && INFUR_CONNECT_8 == 8 && INFUR_REGIONS_SKIP_BACKGROUND == 1);
    uint8_t b[16] = {0};
    uint32_t n = 7;
    CHECK(infur_regions(nullptr, b, nullptr, 4, 4, INFUR_CONNECT_4, 0, 0, nullptr, nullptr, 0, &n) == INFUR_E_INVALID_ARG);
    CHECK(infur_regions_dev(nullptr, b, nullptr, 4, 4, INFUR_CONNECT_4, 0, 0, nullptr, nullptr, 0, &n) == INFUR_E_INVALID_ARG);
    CHECK(n == 7);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Regions reg(c);
    using Cmd = infur::Regions::Cmd;
    CHECK(reg.is_dirty());
    CHECK(reg.control({Cmd::Connectivity, 6}) == INFUR_E_INVALID_ARG);
    CHECK(reg.control({Cmd::Flags, 2}) == INFUR_E_INVALID_ARG);
    // 3 x 3 checkerboard: nine regions at connectivity 4, two at connectivity 8
    {
        infur::Planes p;
        p.width = 3; p.height = 3;
        p.klass = {0, 1, 0, 1, 0, 1, 0, 1, 0};
        infur::RegionsOut out;
        CHECK(reg.control({Cmd::Connectivity, INFUR_CONNECT_4}) == INFUR_OK);
        CHECK(reg.advance(p, out) == INFUR_OK && !reg.is_dirty());
        CHECK(out.n == 9 && out.rows() == 9);
        for (uint32_t i = 0; i < 9; i++) {
            CHECK(out.labels[i] == i && out.word(i, INFUR_REGION_FIRST) == i && out.word(i, INFUR_REGION_CLASS) == (i & 1));
            CHECK(out.word(i, INFUR_STAT_PIXELS) == 1 && out.word(i, INFUR_STAT_SUM_X) == i % 3 && out.word(i, INFUR_STAT_SUM_Y) == i / 3);
            CHECK(out.word(i, INFUR_STAT_SUM_CONF) == 0);
        }
        CHECK(reg.control({Cmd::Connectivity, INFUR_CONNECT_8}) == INFUR_OK && reg.is_dirty());
        CHECK(reg.advance(p, out) == INFUR_OK);
        CHECK(out.n == 2);
        for (uint32_t i = 0; i < 9; i++) CHECK(out.labels[i] == (i & 1));
        CHECK(out.word(0, INFUR_STAT_PIXELS) == 5 && out.word(1, INFUR_STAT_PIXELS) == 4);
        CHECK(out.word(0, INFUR_STAT_MAX_X) == 2 && out.word(1, INFUR_STAT_MIN_X) == 0 && out.word(1, INFUR_STAT_MIN_Y) == 0);
        CHECK(out.word(1, INFUR_REGION_FIRST) == 1 && out.word(1, INFUR_REGION_CLASS) == 1);
    }
    // 150 x 70 (three tiles wide, three high): class 2 in x 60..69, y 30..39 (100 pixels, over a tile corner), class 5 in the
    // single pixel (149, 69), class 0 elsewhere; confidence 3 everywhere
    {
        infur::Planes p;
        p.width = 150; p.height = 70;
        const size_t hw = (size_t)150 * 70;
        p.klass.assign(hw, 0);
        p.conf.assign(hw, 3);
        uint64_t sx = 0, sy = 0;
        for (uint32_t y = 30; y <= 39; y++)
            for (uint32_t x = 60; x <= 69; x++) {
                p.klass[(size_t)y * 150 + x] = 2;
                sx += x;
                sy += y;
            }
        p.klass[hw - 1] = 5;
        infur::RegionsOut out;
        CHECK(reg.advance(p, out) == INFUR_OK);
        CHECK(out.n == 3 && out.labels[0] == 0 && out.labels[(size_t)30 * 150 + 60] == 1 && out.labels[hw - 1] == 2);
        CHECK(out.word(0, INFUR_STAT_PIXELS) == hw - 101 && out.word(0, INFUR_STAT_SUM_CONF) == 3 * (hw - 101));
        CHECK(out.word(1, INFUR_STAT_PIXELS) == 100 && out.word(1, INFUR_STAT_SUM_X) == sx && out.word(1, INFUR_STAT_SUM_Y) == sy);
        CHECK(out.word(1, INFUR_STAT_MIN_X) == 60 && out.word(1, INFUR_STAT_MAX_X) == 69 && out.word(1, INFUR_STAT_MIN_Y) == 30 &&
              out.word(1, INFUR_STAT_MAX_Y) == 39);
        CHECK(out.word(1, INFUR_REGION_CLASS) == 2 && out.word(1, INFUR_REGION_FIRST) == (uint64_t)30 * 150 + 60);
        CHECK(out.word(2, INFUR_REGION_CLASS) == 5 && out.word(2, INFUR_STAT_PIXELS) == 1 && out.word(2, INFUR_STAT_MIN_X) == 149);
        // speckle removal and no background: only the rectangle is left, as region 0
        CHECK(reg.control({Cmd::MinPixels, 2}) == INFUR_OK && reg.control({Cmd::Flags, INFUR_REGIONS_SKIP_BACKGROUND}) == INFUR_OK);
        CHECK(reg.advance(p, out) == INFUR_OK);
        CHECK(out.n == 1 && out.labels[0] == INFUR_REGION_NONE && out.labels[hw - 1] == INFUR_REGION_NONE);
        CHECK(out.labels[(size_t)39 * 150 + 69] == 0 && out.word(0, INFUR_STAT_PIXELS) == 100 && out.word(0, INFUR_STAT_SUM_CONF) == 300);
        // truncation: two of three rows, the count and the label plane are complete
        CHECK(reg.control({Cmd::MinPixels, 0}) == INFUR_OK && reg.control({Cmd::Flags, 0}) == INFUR_OK);
        out.table_rows = 2;
        CHECK(reg.advance(p, out) == INFUR_OK);
        CHECK(out.n == 3 && out.rows() == 2 && out.labels[hw - 1] == 2 && out.word(1, INFUR_STAT_PIXELS) == 100);
    }
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
