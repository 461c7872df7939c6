// Exercises infur::Raster of include/infur_processor.hpp (polygon loops and run-length records filled back into a plane).
//   raster_test cpu   -- the surface that needs no GPU: feature bits, constants, argument checks
//   raster_test gpu   -- the worked example of include/infur_hip.h through hand-made loops, the round trips through Outlines and
//                        Runs, an overlap, a u32 plane and truncated input
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
    CHECK(infur_features() & INFUR_FEATURE_RASTER);
    CHECK(INFUR_FEATURE_RASTER == 4096 && (infur_features() & 4095u) == 4095u);  // the twelve older bits stay set
    CHECK(INFUR_RASTER_LOOPS == 0 && INFUR_RASTER_PAINTED == 1 && INFUR_RASTER_CONFLICT == 2 && INFUR_RASTER_STATUS == 3 && INFUR_RASTER_COUNT_WORDS == 4);
    CHECK(INFUR_RASTER_TRUNCATED == 1 && INFUR_RASTER_MALFORMED == 2 && INFUR_RASTER_OUTSIDE == 4);
    uint32_t b[32];
    std::memset(b, 0x5A, sizeof b);
    // every rejected call, and a good one: without a context each is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 2, 0, 1, 0, b, b) == INFUR_E_INVALID_ARG);     // width 0
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 8192, 2, 1, 0, b, b) == INFUR_E_INVALID_ARG);  // too high
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 2, 2, 2, 0, b, b) == INFUR_E_INVALID_ARG);     // elem_bytes
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 2, 2, 1, 256, b, b) == INFUR_E_INVALID_ARG);   // fill on bytes
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 2, 2, 1, 0, nullptr, nullptr) == INFUR_E_INVALID_ARG);
    CHECK(infur_raster(nullptr, b, 1, b, 4, b, 2, 2, 1, 0, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_raster_dev(nullptr, b, 1, b, 4, b, 2, 2, 1, 0, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_raster_runs(nullptr, b, 1, 1, 2, 2, 1, 0, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_raster_runs_dev(nullptr, b, 1, b, 2, 2, 1, 0, b, b) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 32; i++) CHECK(b[i] == 0x5A5A5A5Au);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Raster raster(c);
    CHECK(raster.is_dirty());
    CHECK(raster.control({infur::Raster::Cmd::Fill, 2, 0}) == INFUR_E_INVALID_ARG && raster.control({infur::Raster::Cmd::Fill, 1, 256}) == INFUR_E_INVALID_ARG);
    infur::RasterOut r;

    // the worked example: the diamond (4,0) (8,4) (4,8) (0,4) of value 7 on an 8 x 8 plane
    infur::OutlinesOut o;
    o.width = o.height = 8;
    o.loops = {0, 4, 7, 0};
    o.vertices = {0 * 9 + 4, 4 * 9 + 8, 8 * 9 + 4, 4 * 9 + 0};
    o.n_loops = 1, o.n_vertices = 4;
    CHECK(raster.advance(o, r) == INFUR_OK && !raster.is_dirty());
    CHECK(r.n == 1 && r.painted == 32 && r.conflict == 0 && r.status == 0 && r.plane.size() == 64);
    const uint32_t from[8] = {3, 2, 1, 0, 0, 1, 2, 3}, to[8] = {4, 5, 6, 7, 7, 6, 5, 4};
    for (uint32_t y = 0; y < 8; y++)
        for (uint32_t x = 0; x < 8; x++) CHECK(r.at(x, y) == (x >= from[y] && x < to[y] ? 7u : 0u));

    // the round trips: a plane with a hole and an island, through Outlines and through Runs
    std::vector<uint8_t> plane(9 * 13, 0);
    for (int y = 1; y <= 7; y++)
        for (int x = 1; x <= 10; x++) plane[y * 13 + x] = (y >= 3 && y <= 5 && x >= 3 && x <= 7) ? (y == 4 && x == 5 ? 2 : 0) : 1;
    infur::Outlines outlines(c);
    CHECK(outlines.control({infur::Outlines::Cmd::Skip, 0}) == INFUR_OK);
    CHECK(outlines.advance(plane, 9, 13, o) == INFUR_OK && o.n_loops == 3);
    CHECK(raster.advance(o, r) == INFUR_OK && r.plane == plane && r.conflict == 0 && r.painted == 70 - 15 + 1);
    infur::Runs runs(c);
    CHECK(runs.control({infur::Runs::Cmd::Skip, 0}) == INFUR_OK);
    infur::RunsOut ro;
    CHECK(runs.advance(plane, 9, 13, ro) == INFUR_OK && ro.n > 0);
    CHECK(raster.advance(ro, r) == INFUR_OK && r.plane == plane && r.n == ro.n && r.conflict == 0 && r.painted == 70 - 15 + 1);

    // a u32 plane, and the fill value where nothing is painted
    CHECK(raster.control({infur::Raster::Cmd::Fill, 4, INFUR_REGION_NONE}) == INFUR_OK && raster.is_dirty());
    CHECK(raster.advance(o, r) == INFUR_OK && r.elem_bytes == 4 && r.plane.size() == plane.size() * 4);
    CHECK(r.at(0, 0) == INFUR_REGION_NONE && r.at(1, 1) == 1 && r.at(5, 4) == 2 && r.at(4, 4) == INFUR_REGION_NONE);

    // two squares that overlap in 2 x 2 pixels: those are refused
    CHECK(raster.control({infur::Raster::Cmd::Fill, 1, 9}) == INFUR_OK);
    infur::OutlinesOut two;
    two.width = 6, two.height = 5;
    two.loops = {0, 4, 1, 0, 4, 4, 2, 0};
    two.vertices = {0 * 7 + 0, 0 * 7 + 3, 3 * 7 + 3, 3 * 7 + 0, 1 * 7 + 1, 1 * 7 + 5, 4 * 7 + 5, 4 * 7 + 1};
    two.n_loops = 2, two.n_vertices = 8;
    CHECK(raster.advance(two, r) == INFUR_OK && r.conflict == 4 && r.painted == 9 + 12 - 8 && r.at(1, 1) == 9 && r.at(0, 0) == 1 && r.at(4, 3) == 2);

    // truncated input: the counts say so and there is no plane
    two.n_loops = 3;
    CHECK(raster.advance(two, r) == INFUR_OK && r.n == 3 && r.painted == 0 && r.status == INFUR_RASTER_TRUNCATED && r.plane.empty());
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
