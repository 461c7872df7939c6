// Exercises infur::Runs of include/infur_processor.hpp (a plane as run-length records).
//   runs_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   runs_test gpu   -- hand-written known answers: runs that stop at the end of a row, skip, truncation, a u32 plane with
//                      0xFFFFFFFF, a run longer than a workgroup, the empty plane
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
    CHECK(infur_features() & INFUR_FEATURE_RUNS);
    CHECK(INFUR_FEATURE_RUNS == 8 && INFUR_RUNS_SKIP == 1);
    CHECK(INFUR_RUN_START == 0 && INFUR_RUN_END == 1 && INFUR_RUN_VALUE == 2 && INFUR_RUN_WORDS == 3);
    uint32_t b[16], ow = 0, oh = 0;
    std::memset(b, 0x5A, sizeof b);
    CHECK(infur_runs(nullptr, b, 1, 2, 2, 0, 0, b, 1, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_runs_dev(nullptr, b, 4, 2, 2, 0, 0, b, 1, b, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_runs(nullptr, (const uint8_t*)b, 2, 2, 1.0f, 0, 0, 0, 0, b, 1, b, 3, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_runs_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 0, 0, b, 1, b, 3, b, nullptr, 0, nullptr, &ow, &oh) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Runs runs(c);
    CHECK(runs.is_dirty());
    using Cmd = infur::Runs::Cmd;
    infur::RunsOut o;
    // 2 x 5: the 2 that ends row 0 and the 2 that begins row 1 are two runs
    const std::vector<uint8_t> p = {1, 1, 2, 2, 2, 2, 0, 0, 3, 3};
    CHECK(runs.advance(p, 2, 5, o) == INFUR_OK && !runs.is_dirty());
    CHECK(o.n == 5 && o.rows() == 5 && o.runs.size() == 15 && o.row_start == (std::vector<uint32_t>{0, 2, 5}));
    CHECK(o.runs == (std::vector<uint32_t>{0, 2, 1, 2, 5, 2, 5, 6, 2, 6, 8, 0, 8, 10, 3}));
    CHECK(o.word(3, INFUR_RUN_START) == 6 && o.word(3, INFUR_RUN_END) == 8 && o.word(3, INFUR_RUN_VALUE) == 0);
    // without the runs of value 2
    CHECK(runs.control({Cmd::Skip, 2}) == INFUR_OK && runs.is_dirty());
    CHECK(runs.advance(p, 2, 5, o) == INFUR_OK && o.n == 3 && o.row_start == (std::vector<uint32_t>{0, 1, 3}));
    CHECK(o.runs == (std::vector<uint32_t>{0, 2, 1, 6, 8, 0, 8, 10, 3}));
    CHECK(runs.control({Cmd::Skip, 256}) == INFUR_OK && runs.advance(p, 2, 5, o) == INFUR_E_INVALID_ARG);  // no byte holds 256
    // room for two records: the count is complete, the row index too
    CHECK(runs.control({Cmd::NoSkip, 0}) == INFUR_OK);
    o.runs_rows = 2;
    CHECK(runs.advance(p, 2, 5, o) == INFUR_OK && o.n == 5 && o.rows() == 2 && o.row_start == (std::vector<uint32_t>{0, 2, 5}));
    CHECK(o.runs == (std::vector<uint32_t>{0, 2, 1, 2, 5, 2}));
    o.runs_rows = 1u << 16;
    // a label plane: INFUR_REGION_NONE is skipped, ids above 2^24 survive
    const uint32_t N = INFUR_REGION_NONE, big = (1u << 24) + 1;
    const std::vector<uint32_t> q = {N, N, big, big, 7, N};
    CHECK(runs.control({Cmd::Skip, N}) == INFUR_OK);
    CHECK(runs.advance(q, 2, 3, o) == INFUR_OK && o.n == 3 && o.row_start == (std::vector<uint32_t>{0, 1, 3}));
    CHECK(o.runs == (std::vector<uint32_t>{2, 3, big, 3, 4, big, 4, 5, 7}));
    // one run across three workgroups, then one run per pixel
    CHECK(runs.control({Cmd::NoSkip, 0}) == INFUR_OK);
    const std::vector<uint8_t> line(3000, 9);
    CHECK(runs.advance(line, 1, 3000, o) == INFUR_OK && o.n == 1 && o.runs == (std::vector<uint32_t>{0, 3000, 9}));
    CHECK(runs.advance(line, 3000, 1, o) == INFUR_OK && o.n == 3000 && o.row_start.size() == 3001 && o.row_start[3000] == 3000);
    CHECK(o.word(2999, INFUR_RUN_START) == 2999 && o.word(2999, INFUR_RUN_END) == 3000 && o.row_start[1234] == 1234);
    // the empty plane, and a plane that is not h * w elements
    CHECK(runs.advance(std::vector<uint8_t>(), 3, 0, o) == INFUR_OK && o.n == 0 && o.runs.empty() && o.row_start == (std::vector<uint32_t>{0, 0, 0, 0}));
    CHECK(runs.advance(p, 3, 5, o) == INFUR_E_SHAPE);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
