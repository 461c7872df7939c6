// Exercises infur::Coverage of include/infur_processor.hpp (shared borders simplified once).
//   coverage_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   coverage_test gpu   -- known answers: a T of three regions at the tolerances where it changes, with and without a skipped
//                          region; four values around one point; the capacity in augmented vertices; truncated rows and input
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
    CHECK(infur_features() & INFUR_FEATURE_COVERAGE);
    CHECK((infur_features() & 63u) == 63u);  // Segments, Regions, Tracks, Runs, Outlines and Simplify are still announced
    CHECK(INFUR_FEATURE_COVERAGE == 64 && INFUR_COVERAGE_SKIP == 1);
    CHECK(INFUR_COVERAGE_TRUNCATED == 1 && INFUR_COVERAGE_MALFORMED == 2 && INFUR_COVERAGE_OVERFLOW == 4);
    CHECK(INFUR_COVERAGE_LOOPS == 0 && INFUR_COVERAGE_VERTICES == 1 && INFUR_COVERAGE_DEGENERATE == 2 && INFUR_COVERAGE_STATUS == 3 &&
          INFUR_COVERAGE_AUG == 4 && INFUR_COVERAGE_ARCS == 5 && INFUR_COVERAGE_COUNT_WORDS == 6);
    uint32_t b[16], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    CHECK(infur_coverage(nullptr, b, 1, 2, 2, 0, 0, b, 1, b, 4, b, 16, 0, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_coverage_dev(nullptr, b, 1, 2, 2, 0, 0, b, 1, b, 4, b, 16, 0, b, 1, b, 4, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_coverage(nullptr, (const uint8_t*)b, 2, 2, 1.0f, 0, 0, 0, 0, 0, 16, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_coverage_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 0, 0, 0, 16, b, 1, b, 4, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Outlines outl(c);
    infur::Coverage cov(c);
    CHECK(cov.is_dirty());
    using OCmd = infur::Outlines::Cmd;
    using Cmd = infur::Coverage::Cmd;
    infur::OutlinesOut o;
    infur::CoverageOut s;
    // a bar of 1 over a 2-wide region of 2 and a 1-wide region of 3.  (2,1), id 6, is a T-junction: a corner of regions 2 and 3
    // and a point inside the bar's lower edge, where it is inserted
    const std::vector<uint8_t> tee = {1, 1, 1, 2, 2, 3, 2, 2, 3};
    CHECK(outl.advance(tee, 3, 3, o) == INFUR_OK && o.vertices == (V{0, 3, 7, 4, 4, 6, 14, 12, 6, 7, 15, 14}));
    CHECK(cov.control({Cmd::Tol16, 0}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK && !cov.is_dirty());
    CHECK(s.loops == (V{0, 5, 1, 0, 5, 4, 2, 12, 9, 4, 3, 20}) && s.vertices == (V{0, 3, 7, 6, 4, 4, 6, 14, 12, 6, 7, 15, 14}));
    CHECK(s.n_loops == 3 && s.n_vertices == 13 && s.n_degenerate == 0 && s.status == 0 && s.n_aug == 13 && s.n_arcs == 9);
    CHECK(cov.control({Cmd::Tol16, 12}) == INFUR_OK && cov.is_dirty() && cov.advance(tee, o, s) == INFUR_OK && s.n_vertices == 13);
    // at one pixel the plane's corners go: every loop begins at its first kept vertex, and the bar keeps the junction (2,1)
    CHECK(cov.control({Cmd::Tol16, 16}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 3, 1, 0, 3, 4, 2, 12, 7, 3, 3, 20}) && s.vertices == (V{7, 6, 4, 4, 6, 14, 12, 6, 7, 14}) && s.n_aug == 13 && s.n_arcs == 9);
    CHECK(s.x(1) == 2 && s.y(1) == 1 && !s.is_degenerate(0) && !s.is_hole(0));
    CHECK(cov.control({Cmd::Tol16, 65535}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 3, 1, 0, 3, 3, 2, 12, 6, 3, 3, 20}) && s.vertices == (V{7, 6, 4, 4, 6, 14, 6, 7, 14}) && s.n_degenerate == 0);
    CHECK(cov.control({Cmd::Tol16, 65536}) == INFUR_E_INVALID_ARG);
    // room for two records and five vertices: the counts are complete, OFFSET' does not depend on the truncation
    s.loops_rows = 2;
    s.vertex_rows = 5;
    CHECK(cov.control({Cmd::Tol16, 16}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK && s.n_loops == 3 && s.n_vertices == 10 && s.rows() == 2);
    CHECK(s.loops == (V{0, 3, 1, 0, 3, 4, 2, 12}) && s.vertices == (V{7, 6, 4, 4, 6}));
    s.loops_rows = 1u << 16;
    s.vertex_rows = 1u << 20;
    // thirteen augmented vertices: a capacity of twelve overflows, visibly, and produces nothing
    CHECK(cov.control({Cmd::AugRows, 13}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK && s.n_vertices == 10 && s.status == 0);
    CHECK(cov.control({Cmd::AugRows, 12}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK);
    CHECK(s.n_loops == 3 && s.n_vertices == 0 && s.n_degenerate == 0 && s.status == INFUR_COVERAGE_OVERFLOW && s.n_aug == 13 && s.n_arcs == 0);
    CHECK(s.loops.empty() && s.vertices.empty() && s.rows() == 0);
    CHECK(cov.control({Cmd::AugRows, 0}) == INFUR_OK);
    // region 3 skipped, for Outlines and for Coverage alike: (2,1) is still a junction, now of 1, 2 and none
    CHECK(outl.control({OCmd::Skip, 3}) == INFUR_OK && outl.advance(tee, 3, 3, o) == INFUR_OK && o.n_loops == 2 && o.n_vertices == 8);
    CHECK(cov.control({Cmd::Skip, 3}) == INFUR_OK && cov.control({Cmd::Tol16, 12}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 4, 1, 0, 4, 4, 2, 12}) && s.vertices == (V{0, 3, 6, 4, 4, 6, 14, 12}) && s.n_aug == 9 && s.n_arcs == 4);
    CHECK(cov.control({Cmd::Tol16, 16}) == INFUR_OK && cov.advance(tee, o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 2, 1, 0, 2, 4, 2, 12}) && s.vertices == (V{6, 4, 4, 6, 14, 12}) && s.n_degenerate == 1 && s.is_degenerate(0));
    CHECK(outl.control({OCmd::NoSkip, 0}) == INFUR_OK && cov.control({Cmd::NoSkip, 0}) == INFUR_OK);
    // four values around one point: every border is an arc of two vertices, the plane's corners go at 12/16 px
    const std::vector<uint8_t> four = {1, 2, 3, 4};
    CHECK(outl.advance(four, 2, 2, o) == INFUR_OK && o.n_loops == 4 && o.n_vertices == 16);
    CHECK(cov.control({Cmd::Tol16, 11}) == INFUR_OK && cov.advance(four, o, s) == INFUR_OK && s.vertices == o.vertices && s.n_arcs == 12);
    CHECK(cov.control({Cmd::Tol16, 12}) == INFUR_OK && cov.advance(four, o, s) == INFUR_OK);
    CHECK(s.loops == (V{0, 3, 1, 0, 3, 3, 2, 4, 6, 3, 3, 8, 9, 3, 4, 12}) && s.vertices == (V{1, 4, 3, 1, 5, 4, 3, 4, 7, 4, 5, 7}));
    // Outlines with room for three of the four records: the input is truncated, and Coverage says so and produces nothing
    o.loops_rows = 3;
    CHECK(outl.advance(four, 2, 2, o) == INFUR_OK && o.n_loops == 4 && o.rows() == 3);
    CHECK(cov.advance(four, o, s) == INFUR_OK && s.n_loops == 4 && s.n_vertices == 0 && s.status == INFUR_COVERAGE_TRUNCATED && s.n_aug == 0);
    CHECK(s.loops.empty() && s.vertices.empty() && s.rows() == 0);
    o.loops_rows = 1u << 16;
    // a plane that does not match the outlines' shape, and an empty plane, are refused
    CHECK(cov.advance(tee, o, s) == INFUR_E_SHAPE);
    CHECK(outl.advance(std::vector<uint8_t>(), 0, 3, o) == INFUR_OK && cov.advance(std::vector<uint8_t>(), o, s) == INFUR_E_INVALID_ARG);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
