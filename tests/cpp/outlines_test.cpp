// Exercises infur::Outlines of include/infur_processor.hpp (region boundaries as polygon loops).
//   outlines_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   outlines_test gpu   -- hand-written known answers: a ring with an island in its hole, the saddle under both connectivities,
//                          a 1 x 1 plane, an edge capacity one below the edges, truncation, a label plane with 0xFFFFFFFF, a
//                          cycle longer than a workgroup, the empty plane
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
    CHECK(infur_features() & INFUR_FEATURE_OUTLINES);
    CHECK((infur_features() & 15u) == 15u);  // Segments, Regions, Tracks and Runs are still announced
    CHECK(INFUR_FEATURE_OUTLINES == 16 && INFUR_OUTLINES_SKIP == 1 && INFUR_OUTLINES_CONN8 == 2);
    CHECK(INFUR_LOOP_OFFSET == 0 && INFUR_LOOP_COUNT == 1 && INFUR_LOOP_VALUE == 2 && INFUR_LOOP_START == 3 && INFUR_LOOP_WORDS == 4);
    uint32_t b[16], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    CHECK(infur_outlines(nullptr, b, 1, 2, 2, 0, 0, 0, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_outlines_dev(nullptr, b, 4, 2, 2, 0, 0, 0, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_outlines(nullptr, (const uint8_t*)b, 2, 2, 1.0f, 0, 0, 0, 0, 0, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_outlines_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 0, 0, 0, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Outlines outl(c);
    CHECK(outl.is_dirty());
    using Cmd = infur::Outlines::Cmd;
    infur::OutlinesOut o;
    // a 7 x 9 ring of class 1 with an island in its hole, class 0 skipped: outer loop, hole, island
    std::vector<uint8_t> ring(7 * 9, 0);
    for (int y = 0; y < 7; y++)
        for (int x = 0; x < 9; x++) ring[y * 9 + x] = (y == 0 || y == 6 || x == 0 || x == 8 || (y == 3 && (x == 3 || x == 4))) ? 1 : 0;
    CHECK(outl.control({Cmd::Skip, 0}) == INFUR_OK);
    CHECK(outl.advance(ring, 7, 9, o) == INFUR_OK && !outl.is_dirty());
    CHECK(o.n_loops == 3 && o.n_vertices == 12 && o.n_edges == 62 && o.rows() == 3);
    CHECK(o.loops == (V{0, 4, 1, 0, 4, 4, 1, 30, 8, 4, 1, 120}));
    CHECK(o.vertices == (V{0, 9, 79, 70, 18, 11, 61, 68, 33, 35, 45, 43}));
    CHECK(!o.is_hole(0) && o.is_hole(1) && !o.is_hole(2) && o.x(4) == 8 && o.y(4) == 1);
    // the saddle: two loops under 4-connectivity, one loop that passes vertex (1, 1) twice under 8-connectivity
    const std::vector<uint8_t> saddle = {1, 0, 0, 1};
    CHECK(outl.advance(saddle, 2, 2, o) == INFUR_OK && o.n_loops == 2 && o.n_edges == 8);
    CHECK(o.loops == (V{0, 4, 1, 0, 4, 4, 1, 12}) && o.vertices == (V{0, 1, 4, 3, 4, 5, 8, 7}));
    CHECK(outl.control({Cmd::Connectivity, 8}) == INFUR_OK && outl.is_dirty() && outl.control({Cmd::Connectivity, 6}) == INFUR_E_INVALID_ARG);
    CHECK(outl.advance(saddle, 2, 2, o) == INFUR_OK && o.n_loops == 1 && o.n_vertices == 8 && o.n_edges == 8);
    CHECK(o.loops == (V{0, 8, 1, 0}) && o.vertices == (V{0, 1, 4, 5, 8, 7, 4, 3}));
    CHECK(outl.control({Cmd::Connectivity, 4}) == INFUR_OK && outl.control({Cmd::NoSkip, 0}) == INFUR_OK);
    // 1 x 1
    CHECK(outl.advance(std::vector<uint8_t>{5}, 1, 1, o) == INFUR_OK && o.loops == (V{0, 4, 5, 0}) && o.vertices == (V{0, 1, 3, 2}) && o.n_edges == 4);
    // an edge capacity one below the edges: the edge count alone
    CHECK(outl.control({Cmd::Skip, 0}) == INFUR_OK && outl.control({Cmd::MaxEdges, 61}) == INFUR_OK);
    CHECK(outl.advance(ring, 7, 9, o) == INFUR_OK && o.n_loops == 0 && o.n_vertices == 0 && o.n_edges == 62 && o.loops.empty() && o.vertices.empty());
    CHECK(outl.control({Cmd::MaxEdges, 62}) == INFUR_OK && outl.advance(ring, 7, 9, o) == INFUR_OK && o.n_loops == 3);
    CHECK(outl.control({Cmd::MaxEdges, 0}) == INFUR_OK);
    // room for two records and five vertices: the counts are complete, OFFSET does not depend on the truncation
    o.loops_rows = 2;
    o.vertex_rows = 5;
    CHECK(outl.advance(ring, 7, 9, o) == INFUR_OK && o.n_loops == 3 && o.n_vertices == 12 && o.rows() == 2);
    CHECK(o.loops == (V{0, 4, 1, 0, 4, 4, 1, 30}) && o.vertices == (V{0, 9, 79, 70, 18}));
    o.loops_rows = 1u << 16;
    o.vertex_rows = 1u << 20;
    CHECK(outl.control({Cmd::Skip, 256}) == INFUR_OK && outl.advance(ring, 7, 9, o) == INFUR_E_INVALID_ARG);  // no byte holds 256
    // a label plane: INFUR_REGION_NONE is skipped, ids above 2^24 survive
    const uint32_t N = INFUR_REGION_NONE, big = (1u << 24) + 1;
    const V q = {N, big, big, 7, N, N};
    CHECK(outl.control({Cmd::Skip, N}) == INFUR_OK);
    CHECK(outl.advance(q, 2, 3, o) == INFUR_OK && o.n_loops == 2 && o.n_edges == 10);
    CHECK(o.loops == (V{0, 4, big, 4, 4, 4, 7, 12}) && o.vertices == (V{1, 3, 7, 5, 4, 5, 9, 8}));
    // one cycle across many workgroups
    CHECK(outl.control({Cmd::NoSkip, 0}) == INFUR_OK);
    const std::vector<uint8_t> line(3000, 9);
    CHECK(outl.advance(line, 1, 3000, o) == INFUR_OK && o.n_edges == 6002 && o.loops == (V{0, 4, 9, 0}) && o.vertices == (V{0, 3000, 6001, 3001}));
    CHECK(outl.advance(line, 3000, 1, o) == INFUR_OK && o.n_edges == 6002 && o.loops == (V{0, 4, 9, 0}) && o.vertices == (V{0, 1, 6001, 6000}));
    // the empty plane, and a plane that is not h * w elements
    CHECK(outl.advance(std::vector<uint8_t>(), 3, 0, o) == INFUR_OK && o.n_loops == 0 && o.n_edges == 0 && o.loops.empty() && o.vertices.empty());
    CHECK(outl.advance(ring, 8, 9, o) == INFUR_E_SHAPE);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
