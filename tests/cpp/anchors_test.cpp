// Exercises infur::Anchors of include/infur_processor.hpp (a distance transform by value, one interior point per value).
//   anchors_test cpu   -- the surface that needs no GPU: feature bits, constants, argument checks
//   anchors_test gpu   -- known answers printed by tests/anchors_ref.py: the "C" whose centroid lies off it, and a 16 x 24
//                         plane of blobs (regions_ref.smooth(16, 24, seed=1, classes=5, cell=6)) with and without a skip
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
    CHECK(infur_features() & INFUR_FEATURE_ANCHORS);
    CHECK(INFUR_FEATURE_ANCHORS == 256 && (infur_features() & 255u) == 255u);  // the eight older bits stay set
    CHECK(INFUR_ANCHORS_SKIP == 1 && INFUR_ANCHOR_PIXEL == 0 && INFUR_ANCHOR_DIST2 == 1 && INFUR_ANCHOR_WORDS == 2 && INFUR_ANCHOR_NONE == 0xFFFFFFFFu);
    uint32_t b[16], ow = 0, oh = 0;
    uint64_t t[4];
    std::memset(b, 0x5A, sizeof b);
    std::memset(t, 0x5A, sizeof t);
    // every rejected call, and a good one: without a context each is INFUR_E_INVALID_ARG and nothing is written
    CHECK(infur_anchors(nullptr, b, 1, 2, 2, 2, 0, b, b, 1) == INFUR_E_INVALID_ARG);         // an unknown flag bit
    CHECK(infur_anchors(nullptr, b, 1, 2, 2, 1, 256, b, b, 1) == INFUR_E_INVALID_ARG);       // no byte holds 256
    CHECK(infur_anchors(nullptr, b, 2, 2, 2, 0, 0, b, b, 1) == INFUR_E_INVALID_ARG);         // elem_bytes
    CHECK(infur_anchors(nullptr, b, 4, 65536, 1, 0, 0, b, b, 1) == INFUR_E_INVALID_ARG);     // a side above 65535
    CHECK(infur_anchors(nullptr, nullptr, 4, 2, 2, 0, 0, b, b, 1) == INFUR_E_INVALID_ARG);   // no plane
    CHECK(infur_anchors(nullptr, b, 4, 2, 2, 0, 0, nullptr, b, 0) == INFUR_E_INVALID_ARG);   // nothing wanted
    CHECK(infur_anchors(nullptr, b, 1, 2, 2, 0, 0, b, b, 1) == INFUR_E_INVALID_ARG);
    CHECK(infur_anchors_dev(nullptr, b, 4, 2, 2, 0, 0, b, b, 1) == INFUR_E_INVALID_ARG);
    CHECK(infur_frame_anchors(nullptr, (const uint8_t*)b, 2, 2, 1.0f, 0, 0, 8, 0, 0, nullptr, nullptr, 0, b, 16, t, 1, b, nullptr, &ow, &oh, b, 16, b) ==
          INFUR_E_INVALID_ARG);
    CHECK(infur_frame_anchors_dev(nullptr, b, 2, 2, 1.0f, 0, 0, 8, 0, 0, nullptr, nullptr, 0, b, 16, t, 1, b, nullptr, &ow, &oh, b, 16, b) ==
          INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au);
    for (int i = 0; i < 4; i++) CHECK(t[i] == 0x5A5A5A5A5A5A5A5Aull);
    CHECK(ow == 0 && oh == 0);
    std::printf("cpu ok\n");
    return 0;
}

// regions_ref.smooth(16, 24, seed=1, classes=5, cell=6)
static const std::vector<uint8_t> kSmooth = {
    2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 0,
    2, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 0,
    2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 0,
    2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1,
    2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 4, 4, 0, 0, 4, 4, 4, 4, 4, 2, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0,
    4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0,
    4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
    4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 3, 3,
    4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 3, 3,
    4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 3,
    4, 3, 3, 3, 3, 3, 2, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 4, 4, 0, 0, 0, 0, 3};
// anchors_ref.distance(plane, SKIP, 0)
static const std::vector<uint32_t> kSmoothDist2 = {
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0,
    1, 4, 4, 2, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 4, 4, 4, 4, 2, 1, 1, 1, 0,
    1, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 5, 2, 1, 1, 1, 1, 2, 1, 0,
    1, 4, 2, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 2, 1, 1, 1, 1, 2, 5, 2, 1,
    1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 4, 4, 5, 8, 4, 1,
    1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 5, 8, 9, 10, 9, 4, 1,
    1, 4, 2, 1, 1, 1, 1, 2, 4, 4, 4, 2, 1, 2, 1, 1, 4, 8, 13, 16, 13, 9, 4, 1,
    1, 2, 1, 1, 2, 4, 4, 5, 8, 9, 8, 5, 4, 4, 1, 1, 4, 9, 13, 10, 8, 5, 4, 1,
    1, 1, 1, 2, 5, 4, 4, 4, 4, 4, 5, 5, 4, 2, 1, 1, 4, 9, 8, 5, 4, 2, 1, 1,
    1, 1, 2, 5, 2, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 2, 5, 4, 4, 2, 1, 1, 0, 0,
    1, 4, 5, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 5, 2, 1, 1, 1, 0, 0, 0, 0,
    1, 4, 4, 1, 1, 2, 4, 4, 4, 2, 1, 1, 2, 4, 5, 2, 1, 0, 0, 0, 0, 0, 0, 0,
    1, 4, 2, 1, 1, 4, 8, 9, 8, 4, 1, 1, 4, 8, 4, 1, 0, 0, 0, 0, 0, 0, 1, 1,
    1, 2, 1, 1, 2, 5, 4, 5, 8, 4, 1, 1, 4, 9, 4, 1, 0, 0, 0, 0, 0, 0, 1, 1,
    1, 1, 1, 2, 4, 2, 1, 2, 4, 4, 1, 1, 4, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1};

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Anchors anchors(c);
    CHECK(anchors.is_dirty());
    using Cmd = infur::Anchors::Cmd;
    const uint32_t N = INFUR_ANCHOR_NONE;
    infur::AnchorsOut o;
    // the "C": the square [2:22, 2:22] of class 1 with [7:17, 7:22] cut out of its right side, class 0 skipped
    std::vector<uint8_t> cee(24 * 24, 0);
    for (int y = 2; y < 22; y++)
        for (int x = 2; x < 22; x++) cee[y * 24 + x] = (y >= 7 && y < 17 && x >= 7) ? 0 : 1;
    uint64_t sx = 0, sy = 0, n1 = 0;
    for (int i = 0; i < 24 * 24; i++)
        if (cee[i]) sx += i % 24, sy += i / 24, n1++;
    CHECK(sx == 10 * n1 && 2 * sy == 23 * n1 && cee[11 * 24 + 10] == 0);  // its centroid (10.0, 11.5) is a pixel of class 0
    o.rows = 3;
    CHECK(anchors.control({Cmd::Skip, 0}) == INFUR_OK && anchors.advance(cee, 24, 24, o) == INFUR_OK && !anchors.is_dirty());
    CHECK(o.anchors == (std::vector<uint32_t>{N, 0, 100, 9, N, 0}) && !o.has(0) && o.has(1) && o.x(1) == 4 && o.y(1) == 4 && cee[100] == 1);
    uint64_t sum = 0;
    for (uint32_t d : o.dist2) sum += d;
    CHECK(o.dist2.size() == 576 && sum == 926);
    CHECK(std::vector<uint32_t>(o.dist2.begin() + 96, o.dist2.begin() + 120) ==
          (std::vector<uint32_t>{0, 0, 1, 4, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 4, 1, 0, 0}));  // row 4: the upper arm's centre line
    // the plane of blobs
    o.rows = 6;
    CHECK(anchors.advance(kSmooth, 16, 24, o) == INFUR_OK && o.dist2 == kSmoothDist2);
    CHECK(o.anchors == (std::vector<uint32_t>{N, 0, 163, 16, 25, 4, 295, 9, 177, 9, N, 0}));
    // without the skip class 0 is a region too, and nothing else moves
    CHECK(anchors.control({Cmd::NoSkip, 0}) == INFUR_OK && anchors.is_dirty() && anchors.advance(kSmooth, 16, 24, o) == INFUR_OK);
    CHECK(o.anchors == (std::vector<uint32_t>{78, 5, 163, 16, 25, 4, 295, 9, 177, 9, N, 0}));
    sum = 0;
    for (size_t i = 0; i < o.dist2.size(); i++) {
        sum += o.dist2[i];
        CHECK(kSmooth[i] == 0 ? o.dist2[i] >= 1 : o.dist2[i] == kSmoothDist2[i]);
    }
    CHECK(sum == 946);
    // the same plane as u32 labels, INFUR_REGION_NONE where class 0 was: the same distances, the rows of the labels
    std::vector<uint32_t> labels(kSmooth.size());
    for (size_t i = 0; i < labels.size(); i++) labels[i] = kSmooth[i] ? kSmooth[i] : INFUR_REGION_NONE;
    CHECK(anchors.control({Cmd::Skip, INFUR_REGION_NONE}) == INFUR_OK && anchors.advance(labels, 16, 24, o) == INFUR_OK && o.dist2 == kSmoothDist2);
    CHECK(o.anchors == (std::vector<uint32_t>{N, 0, 163, 16, 25, 4, 295, 9, 177, 9, N, 0}));
    // one output at a time, a byte plane cannot skip 256, the empty plane, a plane that is not h * w elements
    o.want_dist2 = false;
    o.rows = 2;
    CHECK(anchors.advance(labels, 16, 24, o) == INFUR_OK && o.dist2.empty() && o.anchors == (std::vector<uint32_t>{N, 0, 163, 16}));
    o.rows = 0;
    CHECK(anchors.advance(labels, 16, 24, o) == INFUR_E_INVALID_ARG);  // nothing wanted
    o.want_dist2 = true;
    CHECK(anchors.advance(labels, 16, 24, o) == INFUR_OK && o.anchors.empty() && o.dist2 == kSmoothDist2);
    o.rows = 2;
    CHECK(anchors.control({Cmd::Skip, 256}) == INFUR_OK && anchors.advance(kSmooth, 16, 24, o) == INFUR_E_INVALID_ARG);
    CHECK(anchors.control({Cmd::NoSkip, 0}) == INFUR_OK);
    CHECK(anchors.advance(std::vector<uint8_t>(), 3, 0, o) == INFUR_OK && o.dist2.empty() && o.anchors == (std::vector<uint32_t>{N, 0, N, 0}));
    CHECK(anchors.advance(kSmooth, 3, 5, o) == INFUR_E_SHAPE);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
