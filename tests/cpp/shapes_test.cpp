// Exercises infur::Shapes of include/infur_processor.hpp (area, moments, convex hull and minimum rectangle per outline loop).
//   shapes_test cpu   -- the surface that needs no GPU: feature bits, constants, argument checks
//   shapes_test gpu   -- the two worked examples of include/infur_hip.h word for word through Outlines -> Shapes, a plane with a
//                        hole, short rows and truncated input
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
    CHECK(infur_features() & INFUR_FEATURE_SHAPES);
    CHECK(INFUR_FEATURE_SHAPES == 2048 && (infur_features() & 2047u) == 2047u);  // the eleven older bits stay set
    CHECK(INFUR_SHAPE_AREA2 == 0 && INFUR_SHAPE_PERIMETER == 1 && INFUR_SHAPE_M10_6 == 2 && INFUR_SHAPE_M01_6 == 3 && INFUR_SHAPE_M20_12 == 4 &&
          INFUR_SHAPE_M02_12 == 5 && INFUR_SHAPE_M11_24 == 6 && INFUR_SHAPE_HULL_AREA2 == 7);
    CHECK(INFUR_SHAPE_RECT_EDGE == 8 && INFUR_SHAPE_RECT_W == 9 && INFUR_SHAPE_RECT_H == 10 && INFUR_SHAPE_RECT_L == 11 && INFUR_SHAPE_WORDS == 12);
    CHECK(INFUR_SHAPE_OUTER == 8 && INFUR_SHAPE_HOLES == 9 && INFUR_SHAPE_LOOP == 10);
    CHECK(INFUR_SHAPES_LOOPS == 0 && INFUR_SHAPES_VERTICES == 1 && INFUR_SHAPES_STATUS == 2 && INFUR_SHAPES_LARGEST == 3 && INFUR_SHAPES_COUNT_WORDS == 4);
    CHECK(INFUR_SHAPES_TRUNCATED == 1 && INFUR_SHAPES_MALFORMED == 2);
    uint32_t b[32], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    const uint8_t* f = (const uint8_t*)b;
    uint8_t* g = (uint8_t*)b;
    uint64_t* u = (uint64_t*)b;
    // every rejected call, and a good one: without a context each is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_shapes(nullptr, b, 1, b, 4, b, 2, 0, b, 1, b, 4, u, 1, u, 1, b) == INFUR_E_INVALID_ARG);     // width 0
    CHECK(infur_shapes(nullptr, b, 1, b, 4, b, 8192, 2, b, 1, b, 4, u, 1, u, 1, b) == INFUR_E_INVALID_ARG);  // too high
    CHECK(infur_shapes(nullptr, b, 1, b, 4, b, 2, 2, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == INFUR_E_INVALID_ARG);
    CHECK(infur_shapes(nullptr, b, 1, b, 4, b, 2, 2, b, 1, b, 4, u, 1, u, 1, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_shapes_dev(nullptr, b, 1, b, 4, b, 2, 2, b, 1, b, 4, b, 1, b, 1, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_shapes(nullptr, f, 2, 2, 1.0f, 0, 0, 8, 0, 0, g, g, 4, b, 16, u, 1, b, nullptr, &ow, &oh, 0, b, 1, b, 4, u, 1, u, b) ==
          INFUR_E_INVALID_ARG);
    CHECK(infur_frame_shapes_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 8, 0, 0, b, b, 4, b, 16, b, 1, b, nullptr, &ow, &oh, 0, b, 1, b, 4, b, 1, b, b) ==
          INFUR_E_INVALID_ARG);
    for (int i = 0; i < 32; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    using V = std::vector<uint32_t>;
    using S = std::vector<int64_t>;
    infur::Outlines outlines(c);
    CHECK(outlines.control({infur::Outlines::Cmd::Skip, 0}) == INFUR_OK);
    infur::Shapes shapes(c);
    CHECK(shapes.is_dirty());
    infur::OutlinesOut o;
    infur::ShapesOut s;

    // worked example 1, the "C": 24 x 24, class 1 = [2:22, 2:22] minus [7:17, 7:22]
    std::vector<uint8_t> plane(24 * 24, 0);
    for (int y = 2; y < 22; y++)
        for (int x = 2; x < 22; x++) plane[y * 24 + x] = !(y >= 7 && y < 17 && x >= 7) ? 1 : 0;
    CHECK(outlines.advance(plane, 24, 24, o) == INFUR_OK && o.n_loops == 1 && o.n_vertices == 8);
    s.value_rows = 2;
    CHECK(shapes.advance(o, s) == INFUR_OK && !shapes.is_dirty());
    CHECK(s.n_loops == 1 && s.n_vertices == 4 && s.status == 0 && s.largest == 4);
    CHECK(s.shapes == (S{500, 110, 15750, 18000, 439000, 577000, 756000, 800, 0, 400, 400, 400}));
    CHECK(s.values == (S{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, 500, 110, 15750, 18000, 439000, 577000, 756000, 800, 1, 0, 0, 0}));
    CHECK(s.word(0, INFUR_LOOP_OFFSET) == 0 && s.word(0, INFUR_LOOP_COUNT) == 4 && s.word(0, INFUR_LOOP_VALUE) == 1);
    const uint32_t cx[4] = {2, 22, 22, 2}, cy[4] = {2, 2, 22, 22};
    for (uint32_t i = 0; i < 4; i++) CHECK(s.x(i) == cx[i] && s.y(i) == cy[i]);

    // worked example 2, the slanted bar: 12 x 16, value 2 where |(x - 8) - (y - 6)| <= 1, 1 <= y <= 10, 1 <= x <= 14
    plane.assign(12 * 16, 0);
    for (int y = 1; y <= 10; y++)
        for (int x = 1; x <= 14; x++) {
            const int d = (x - 8) - (y - 6);
            if (d >= -1 && d <= 1) plane[y * 16 + x] = 2;
        }
    CHECK(outlines.advance(plane, 12, 16, o) == INFUR_OK && o.n_loops == 1 && o.n_vertices == 40);
    s.value_rows = 3;
    CHECK(shapes.advance(o, s) == INFUR_OK && s.n_vertices == 6 && s.status == 0 && s.largest == 6);
    CHECK(s.shapes == (S{60, 44, 1440, 1080, 26280, 15960, 40500, 78, 1, 198, 36, 162}));
    const uint32_t bx[6] = {2, 5, 14, 14, 11, 2}, by[6] = {1, 1, 10, 11, 11, 2};
    for (uint32_t i = 0; i < 6; i++) CHECK(s.x(i) == bx[i] && s.y(i) == by[i]);
    CHECK(s.value(2, INFUR_SHAPE_AREA2) == 60 && s.value(2, INFUR_SHAPE_HULL_AREA2) == 78 && s.value(2, INFUR_SHAPE_LOOP) == 0 &&
          s.value(1, INFUR_SHAPE_LOOP) == -1);

    // a 5 x 5 ring of value 1 around one pixel of value 0, on a 7 x 7 plane: an outer loop and a hole
    plane.assign(7 * 7, 0);
    for (int y = 1; y <= 5; y++)
        for (int x = 1; x <= 5; x++) plane[y * 7 + x] = !(x == 3 && y == 3);
    CHECK(outlines.advance(plane, 7, 7, o) == INFUR_OK && o.n_loops == 2);
    s.value_rows = 2;
    CHECK(shapes.advance(o, s) == INFUR_OK && s.n_loops == 2 && s.n_vertices == 8 && s.largest == 4);
    CHECK(s.shape(0, INFUR_SHAPE_AREA2) == 50 && s.shape(1, INFUR_SHAPE_AREA2) == -2 && s.shape(1, INFUR_SHAPE_HULL_AREA2) == -2);
    CHECK(s.value(1, INFUR_SHAPE_AREA2) == 48 && s.value(1, INFUR_SHAPE_OUTER) == 1 && s.value(1, INFUR_SHAPE_HOLES) == 1 &&
          s.value(1, INFUR_SHAPE_HULL_AREA2) == 50 && s.value(1, INFUR_SHAPE_PERIMETER) == 24);
    // the ring is symmetric about (3.5, 3.5): M10_6 = 6 * 24 * 3.5
    CHECK(s.value(1, INFUR_SHAPE_M10_6) == 504 && s.value(1, INFUR_SHAPE_M01_6) == 504);
    // short rows: the counts stay complete
    s.loops_rows = 1, s.vertex_rows = 3, s.shape_rows = 1;
    CHECK(shapes.advance(o, s) == INFUR_OK && s.n_loops == 2 && s.n_vertices == 8 && s.loops.size() == 4 && s.vertices.size() == 3 &&
          s.shapes.size() == 12 && s.shape(0, INFUR_SHAPE_AREA2) == 50);
    // truncated input: the counts say so, the per-value table is that of a plane without loops
    o.n_loops = 3;
    s = infur::ShapesOut();
    s.value_rows = 2;
    CHECK(shapes.advance(o, s) == INFUR_OK && s.n_loops == 3 && s.n_vertices == 0 && s.status == INFUR_SHAPES_TRUNCATED && s.largest == 0);
    CHECK(s.loops.empty() && s.vertices.empty() && s.shapes.empty() && s.value(1, INFUR_SHAPE_LOOP) == -1 && s.value(1, INFUR_SHAPE_AREA2) == 0);
    (void)V{};
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
