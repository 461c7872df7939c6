// Exercises infur::Tracks of include/infur_processor.hpp (region identities carried from frame to frame).
//   tracks_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   tracks_test gpu   -- hand-written known answers: a rectangle that moves keeps its track and reports its predecessor, a
//                        rectangle that appears in front of it in raster order gets the next id, reset, truncation
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
    CHECK(infur_features() & INFUR_FEATURE_TRACKS);
    CHECK(INFUR_FEATURE_TRACKS == 4 && INFUR_TRACK_WORDS == 8 && INFUR_TRACK_NONE == 0xFFFFFFFFu && INFUR_TRACKS_SUMMARY_WORDS == 4);
    CHECK(INFUR_TRACK_ID == 0 && INFUR_TRACK_AGE == 1 && INFUR_TRACK_BORN == 2 && INFUR_TRACK_PREV_REGION == 3 && INFUR_TRACK_OVERLAP == 4);
    CHECK(INFUR_TRACK_PREV_PIXELS == 5 && INFUR_TRACK_PREV_SUM_X == 6 && INFUR_TRACK_PREV_SUM_Y == 7);
    CHECK(INFUR_TRACKS_TRUNCATED == 1 && INFUR_TRACKS_OVERFLOW == 2 && INFUR_TRACKS_IDS_EXHAUSTED == 4);
    uint32_t b[16];
    uint64_t t[16];
    std::memset(b, 0x5A, sizeof b);
    std::memset(t, 0x5A, sizeof t);
    void* trk = b;
    CHECK(infur_tracker_create(nullptr, 0, 0, &trk) == INFUR_E_INVALID_ARG && trk == b);
    CHECK(infur_tracker_reset(nullptr, 1) == INFUR_E_INVALID_ARG);
    infur_tracker_destroy(nullptr);
    CHECK(infur_tracks(nullptr, b, t, 1, 1, 2, 2, 1, b, b, t, b) == INFUR_E_INVALID_ARG);
    CHECK(infur_tracks_dev(nullptr, b, t, 1, b, 2, 2, 1, b, b, t, b) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au && t[i] == 0x5A5A5A5A5A5A5A5Aull);
    std::printf("cpu ok\n");
    return 0;
}

// 150 x 70 (three tiles wide, three high), class 0 with class-2 rectangles [x0, x0 + w) x [y0, y0 + h)
struct Rect {
    uint32_t x0, y0, w, h;
};
static infur::Planes plane_of(const std::vector<Rect>& rects) {
    infur::Planes p;
    p.width = 150;
    p.height = 70;
    p.klass.assign((size_t)150 * 70, 0);
    for (const Rect& r : rects)
        for (uint32_t y = r.y0; y < r.y0 + r.h; y++)
            for (uint32_t x = r.x0; x < r.x0 + r.w; x++) p.klass[(size_t)y * 150 + x] = 2;
    return p;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Regions reg(c);
    infur::Tracks trk(c);
    CHECK(trk.ok() && trk.is_dirty());
    using Cmd = infur::Tracks::Cmd;
    infur::RegionsOut r;
    infur::TracksOut t;
    t.want_plane = true;
    const size_t hw = (size_t)150 * 70;
    // frame 0: one rectangle over a tile corner -- background is track 0, the rectangle track 1
    CHECK(reg.advance(plane_of({{60, 30, 10, 10}}), r) == INFUR_OK && r.n == 2);
    CHECK(trk.advance(r, t) == INFUR_OK && !trk.is_dirty());
    CHECK(t.rows == 2 && t.track_of_region.size() == 2 && t.track_of_region[0] == 0 && t.track_of_region[1] == 1);
    CHECK(t.status() == 0 && t.summary[INFUR_TRACKS_SUMMARY_CONTINUED] == 0 && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 2 &&
          t.summary[INFUR_TRACKS_SUMMARY_ENDED] == 0);
    CHECK(t.word(1, INFUR_TRACK_AGE) == 1 && t.word(1, INFUR_TRACK_BORN) == 0 && t.word(1, INFUR_TRACK_PREV_REGION) == INFUR_REGION_NONE &&
          t.word(1, INFUR_TRACK_PREV_PIXELS) == 0);
    CHECK(t.plane.size() == hw && t.plane[0] == 0 && t.plane[(size_t)30 * 150 + 60] == 1);
    const uint64_t sx0 = r.word(1, INFUR_STAT_SUM_X), sy0 = r.word(1, INFUR_STAT_SUM_Y);
    // frame 1: moved by (3, 1) -- same track, age 2, 7 x 9 pixels in common, the predecessor's sums for the centroid step
    CHECK(reg.advance(plane_of({{63, 31, 10, 10}}), r) == INFUR_OK && r.n == 2);
    CHECK(trk.advance(r, t) == INFUR_OK);
    CHECK(t.track_of_region[0] == 0 && t.track_of_region[1] == 1 && t.summary[INFUR_TRACKS_SUMMARY_CONTINUED] == 2);
    CHECK(t.word(1, INFUR_TRACK_ID) == 1 && t.word(1, INFUR_TRACK_AGE) == 2 && t.word(1, INFUR_TRACK_BORN) == 0);
    CHECK(t.word(1, INFUR_TRACK_PREV_REGION) == 1 && t.word(1, INFUR_TRACK_OVERLAP) == 63 && t.word(1, INFUR_TRACK_PREV_PIXELS) == 100);
    CHECK(t.word(1, INFUR_TRACK_PREV_SUM_X) == sx0 && t.word(1, INFUR_TRACK_PREV_SUM_Y) == sy0);
    CHECK(r.word(1, INFUR_STAT_SUM_X) - sx0 == 300 && r.word(1, INFUR_STAT_SUM_Y) - sy0 == 100);  // 100 pixels moved by (3, 1)
    // frame 2: a second rectangle in front of it in raster order is region 1 and gets the next id; the first keeps track 1
    CHECK(reg.advance(plane_of({{63, 31, 10, 10}, {5, 2, 5, 3}}), r) == INFUR_OK && r.n == 3);
    CHECK(trk.advance(r, t) == INFUR_OK);
    CHECK(t.track_of_region[0] == 0 && t.track_of_region[1] == 2 && t.track_of_region[2] == 1);
    CHECK(t.word(2, INFUR_TRACK_AGE) == 3 && t.word(1, INFUR_TRACK_AGE) == 1 && t.word(1, INFUR_TRACK_BORN) == 2);
    CHECK(t.summary[INFUR_TRACKS_SUMMARY_CONTINUED] == 2 && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 1 && t.summary[INFUR_TRACKS_SUMMARY_ENDED] == 0);
    CHECK(t.plane[(size_t)2 * 150 + 5] == 2 && t.plane[(size_t)40 * 150 + 72] == 1 && t.plane[hw - 1] == 0);
    // frame 3: the first rectangle is gone -- its track ends
    CHECK(reg.advance(plane_of({{5, 2, 5, 3}}), r) == INFUR_OK && r.n == 2);
    CHECK(trk.advance(r, t) == INFUR_OK);
    CHECK(t.track_of_region[1] == 2 && t.summary[INFUR_TRACKS_SUMMARY_ENDED] == 1 && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 0);
    // min_overlap above what the regions share: everything is new; then reset
    CHECK(trk.control({Cmd::MinOverlap, 1u << 30}) == INFUR_OK && trk.is_dirty());
    CHECK(trk.advance(r, t) == INFUR_OK && t.track_of_region[0] == 3 && t.track_of_region[1] == 4 && t.summary[INFUR_TRACKS_SUMMARY_ENDED] == 2);
    CHECK(trk.control({Cmd::MinOverlap, 1}) == INFUR_OK && trk.control({Cmd::Reset, 100}) == INFUR_OK);
    CHECK(trk.advance(r, t) == INFUR_OK && t.track_of_region[0] == 100 && t.track_of_region[1] == 101 && t.word(1, INFUR_TRACK_BORN) == 5);
    // a one-row table: the second region is not tracked
    r.table.resize(INFUR_REGION_WORDS);
    CHECK(trk.advance(r, t) == INFUR_OK && t.rows == 1 && t.status() == INFUR_TRACKS_TRUNCATED && t.track_of_region[0] == 100);
    CHECK(t.plane[0] == 100 && t.plane[(size_t)2 * 150 + 5] == INFUR_TRACK_NONE);
    // a tracker with too few slots for this plane (70 rows of three runs) says so
    infur::Tracks tiny(c, 0, 64);
    CHECK(tiny.ok() && tiny.advance(r, t) == INFUR_OK && t.status() == INFUR_TRACKS_TRUNCATED);
    CHECK(tiny.advance(r, t) == INFUR_OK && t.status() == (INFUR_TRACKS_TRUNCATED | INFUR_TRACKS_OVERFLOW) && t.track_of_region[0] == 1);
    infur::Tracks bad(c, 0, 100);
    CHECK(!bad.ok());
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
