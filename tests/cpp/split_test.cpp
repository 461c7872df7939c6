// Exercises infur::Split of include/infur_processor.hpp (touching objects of one value separated at their necks).
// cpu: feature bits and argument checks, no GPU; gpu: the worked example of include/infur_hip.h word for word, and a skipped value
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
    CHECK(INFUR_FEATURE_SPLIT == 8192 && (infur_features() & 16383u) == 16383u);  // the thirteen older bits stay set
    uint32_t b[32];
    std::memset(b, 0x5A, sizeof b);
    // without a context every call is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_split(nullptr, b, 4, b, 2, 2, 0, 0, 1, 0, b, b, 1, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_split_dev(nullptr, b, 4, b, 2, 2, 0, 0, 1, 0, b, b, 1, b) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 32; i++) CHECK(b[i] == 0x5A5A5A5Au);
    std::printf("cpu ok\n");
    return 0;
}

static bool same(const uint32_t* got, std::initializer_list<uint32_t> want) {
    size_t i = 0;
    for (uint32_t v : want)
        if (got[i++] != v) return false;
    return true;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Split split(c);
    CHECK(split.is_dirty() && split.control({infur::Split::Cmd::Core, 4, false, 0, 100}) == INFUR_E_INVALID_ARG);
    // the header's example: h = 1, w = 9, one value, heights 1 4 9 4 1 4 9 4 1
    const std::vector<uint8_t> plane(9, 1);
    const std::vector<uint32_t> height = {1, 4, 9, 4, 1, 4, 9, 4, 1};
    infur::SplitOut out;
    CHECK(split.control({infur::Split::Cmd::Core, 4, false, 0, 0}) == INFUR_OK);
    CHECK(split.advance(plane.data(), 1, height.data(), 1, 9, out) == INFUR_OK && !split.is_dirty());
    CHECK(same(out.labels.data(), {0, 0, 0, 0, 0, 1, 1, 1, 1}) && out.table.size() == 12);
    CHECK(same(out.row(0), {1, 5, 0, 2, 9, 1}) && same(out.row(1), {1, 4, 5, 6, 9, 1}) && same(out.counts, {2, 2, 1, 1, 2, 1, 0, 0}));
    CHECK(split.control({infur::Split::Cmd::Core, 1, false, 0, 0}) == INFUR_OK && split.advance(plane.data(), 1, height.data(), 1, 9, out) == INFUR_OK);
    CHECK(out.segments() == 1 && same(out.row(0), {1, 9, 0, 2, 9, 0}) && same(out.counts, {1, 2, 1, 1, 2, 0, 0, 0}));
    CHECK(split.control({infur::Split::Cmd::Core, 10, false, 0, 0}) == INFUR_OK && split.advance(plane.data(), 1, height.data(), 1, 9, out) == INFUR_OK);
    CHECK(out.segments() == 1 && same(out.row(0), {1, 9, 0, 2, 9, 0}) && same(out.counts, {1, 2, 1, 1, 0, 0, 1, 0}));
    // pixel 4 skipped: two segments of value 1 that never touch, no pair
    std::vector<uint32_t> wide(plane.begin(), plane.end());
    wide[4] = 7;
    CHECK(split.control({infur::Split::Cmd::Core, 1, true, 7, 0}) == INFUR_OK && split.advance(wide.data(), 4, height.data(), 1, 9, out) == INFUR_OK);
    CHECK(same(out.labels.data(), {0, 0, 0, 0, INFUR_SPLIT_NONE, 1, 1, 1, 1}) && same(out.counts, {2, 2, 0, 0, 2, 1, 0, 0}));
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    return argc >= 2 && !std::strcmp(argv[1], "gpu") ? gpu_tests() : cpu_tests();
}
