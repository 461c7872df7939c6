// Exercises infur::Simplify of include/infur_processor.hpp (Douglas-Peucker on Outlines' loops).
//   simplify_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   simplify_test gpu   -- hand-written known answers: a staircase of three steps at the tolerances where it changes, a ring with an
//                          island that collapses, the saddle loop, truncated rows, truncated input, the empty plane
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

using V = std::vector<uint32_t>;

static int cpu_tests() {
    CHECK(infur_abi_version() == INFUR_ABI_VERSION && INFUR_ABI_VERSION == 7);
    CHECK(infur_features() & INFUR_FEATURE_SIMPLIFY);
    CHECK((infur_features() & 31u) == 31u);  // Segments, Regions, Tracks, Runs and Outlines are still announced
    CHECK(INFUR_FEATURE_SIMPLIFY == 32 && INFUR_SIMPLIFY_TRUNCATED == 1 && INFUR_SIMPLIFY_MALFORMED == 2);
    CHECK(INFUR_SIMPLIFY_LOOPS == 0 && INFUR_SIMPLIFY_VERTICES == 1 && INFUR_SIMPLIFY_DEGENERATE == 2 && INFUR_SIMPLIFY_STATUS == 3 &&
          INFUR_SIMPLIFY_COUNT_WORDS == 4);
    uint32_t b[16], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    CHECK(infur_simplify(nullptr, b, 1, b, 4, b, 2, 2, 16, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_simplify_dev(nullptr, b, 1, b, 4, b, 2, 2, 16, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_polygons(nullptr, (const uint8_t*)b, 2, 2, 1.0f, 0, 0, 0, 0, 0, 16, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_polygons_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 0, 0, 0, 16, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Outlines outl(c);
    infur::Simplify simp(c);
    CHECK(simp.is_dirty());
    using OCmd = infur::Outlines::Cmd;
    using Cmd = infur::Simplify::Cmd;
    infur::OutlinesOut o;
    infur::SimplifyOut s;
    CHECK(outl.control({OCmd::Skip, 0}) == INFUR_OK);
    // three unit steps: (0,0) (1,0) (1,1) (2,1) (2,2) (3,2) (3,3) (0,3).  The far anchor is (3,3).  The outer corners of the staircase
    // are 0.707 px off the chord and tie: the first is examined.  11/16 px keeps it and nothing behind it; 12/16 px keeps none;
    // the corner (0,3) is 2.12 px off its chord and goes at 34/16
    const std::vector<uint8_t> stairs = {1, 0, 0, 1, 1, 0, 1, 1, 1};
    CHECK(outl.advance(stairs, 3, 3, o) == INFUR_OK && o.vertices == (V{0, 1, 5, 6, 10, 11, 15, 12}));
    CHECK(simp.control({Cmd::Tol16, 0}) == INFUR_OK && simp.advance(o, s) == INFUR_OK && !simp.is_dirty());
    CHECK(s.loops == (V{0, 8, 1, 0}) && s.vertices == o.vertices && s.n_loops == 1 && s.n_vertices == 8 && s.n_degenerate == 0 && s.status == 0);
    CHECK(simp.control({Cmd::Tol16, 11}) == INFUR_OK && simp.is_dirty() && simp.advance(o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 4, 1, 0}) && s.vertices == (V{0, 1, 15, 12}) && s.n_degenerate == 0);
    CHECK(simp.control({Cmd::Tol16, 12}) == INFUR_OK && simp.advance(o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 3, 1, 0}) && s.vertices == (V{0, 15, 12}) && s.x(1) == 3 && s.y(1) == 3 && !s.is_degenerate(0));
    CHECK(simp.control({Cmd::Tol16, 33}) == INFUR_OK && simp.advance(o, s) == INFUR_OK && s.vertices == (V{0, 15, 12}));
    CHECK(simp.control({Cmd::Tol16, 34}) == INFUR_OK && simp.advance(o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 2, 1, 0}) && s.vertices == (V{0, 15}) && s.n_degenerate == 1 && s.is_degenerate(0) && s.status == 0);
    CHECK(simp.control({Cmd::Tol16, 65536}) == INFUR_E_INVALID_ARG);
    // a 7 x 9 ring with an island of 2 x 1 pixels in its hole: the island's other corners are 0.894 px off its diagonal
    std::vector<uint8_t> ring(7 * 9, 0);
    for (int y = 0; y < 7; y++)
        for (int x = 0; x < 9; x++) ring[y * 9 + x] = (y == 0 || y == 6 || x == 0 || x == 8 || (y == 3 && (x == 3 || x == 4))) ? 1 : 0;
    CHECK(outl.advance(ring, 7, 9, o) == INFUR_OK && o.n_loops == 3 && o.n_vertices == 12);
    CHECK(simp.control({Cmd::Tol16, 14}) == INFUR_OK && simp.advance(o, s) == INFUR_OK && s.loops == o.loops && s.vertices == o.vertices);
    CHECK(simp.control({Cmd::Tol16, 15}) == INFUR_OK && simp.advance(o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 4, 1, 0, 4, 4, 1, 30, 8, 2, 1, 120}) && s.vertices == (V{0, 9, 79, 70, 18, 11, 61, 68, 33, 45}));
    CHECK(s.n_loops == 3 && s.n_vertices == 10 && s.n_degenerate == 1 && s.status == 0 && s.is_hole(1) && !s.is_hole(2) && s.is_degenerate(2));
    // room for two records and five vertices: the counts are complete, OFFSET' does not depend on the truncation
    s.loops_rows = 2;
    s.vertex_rows = 5;
    CHECK(simp.advance(o, s) == INFUR_OK && s.n_loops == 3 && s.n_vertices == 10 && s.n_degenerate == 1 && s.rows() == 2);
    CHECK(s.loops == (V{0, 4, 1, 0, 4, 4, 1, 30}) && s.vertices == (V{0, 9, 79, 70, 18}));
    s.loops_rows = 1u << 16;
    s.vertex_rows = 1u << 20;
    // Outlines with room for two of the three records: the input is truncated, and Simplify says so and produces nothing
    o.loops_rows = 2;
    CHECK(outl.advance(ring, 7, 9, o) == INFUR_OK && o.n_loops == 3 && o.rows() == 2);
    CHECK(simp.advance(o, s) == INFUR_OK && s.n_loops == 3 && s.n_vertices == 0 && s.n_degenerate == 0 && s.status == INFUR_SIMPLIFY_TRUNCATED);
    CHECK(s.loops.empty() && s.vertices.empty() && s.rows() == 0);
    o.loops_rows = 1u << 16;
    // the saddle under 8-connectivity: one loop that passes vertex (1, 1) twice
    const std::vector<uint8_t> saddle = {1, 0, 0, 1};
    CHECK(outl.control({OCmd::Connectivity, 8}) == INFUR_OK && outl.advance(saddle, 2, 2, o) == INFUR_OK && o.n_vertices == 8);
    CHECK(simp.control({Cmd::Tol16, 11}) == INFUR_OK && simp.advance(o, s) == INFUR_OK && s.loops == (V{0, 4, 1, 0}) && s.vertices == (V{0, 1, 8, 7}));
    CHECK(simp.control({Cmd::Tol16, 12}) == INFUR_OK && simp.advance(o, s) == INFUR_OK && s.loops == (V{0, 2, 1, 0}) && s.vertices == (V{0, 8}));
    // the empty plane: no loops, and a width of 0 is refused
    CHECK(outl.advance(std::vector<uint8_t>(), 0, 3, o) == INFUR_OK && o.n_loops == 0);
    CHECK(simp.advance(o, s) == INFUR_OK && s.n_loops == 0 && s.n_vertices == 0 && s.status == 0 && s.loops.empty() && s.vertices.empty());
    CHECK(outl.advance(std::vector<uint8_t>(), 3, 0, o) == INFUR_OK && simp.advance(o, s) == INFUR_E_INVALID_ARG);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
