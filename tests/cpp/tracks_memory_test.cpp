// Exercises the memory of infur::Tracks (include/infur_processor.hpp): a lost track is kept for a few frames.
//   tracks_memory_test cpu   -- the surface that needs no GPU: feature bit, constants, argument checks
//   tracks_memory_test gpu   -- the gap sequence by hand: a rectangle, an empty frame, the rectangle again keeps its id
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
    CHECK((infur_features() & 255) == 255 && INFUR_FEATURE_TRACK_MEMORY == 128 && INFUR_TRACKS_GALLERY_FULL == 8);
    CHECK(INFUR_LOST_ID == 0 && INFUR_LOST_AGE == 1 && INFUR_LOST_BORN == 2 && INFUR_LOST_CLASS == 3 && INFUR_LOST_PIXELS == 4);
    CHECK(INFUR_LOST_SUM_X == 5 && INFUR_LOST_SUM_Y == 6 && INFUR_LOST_MIN_X == 7 && INFUR_LOST_MIN_Y == 8 && INFUR_LOST_MAX_X == 9);
    CHECK(INFUR_LOST_MAX_Y == 10 && INFUR_LOST_SEEN == 11 && INFUR_LOST_WORDS == 12);
    CHECK(INFUR_TRACK_MEMORY_REVIVED == 0 && INFUR_TRACK_MEMORY_LOST == 1 && INFUR_TRACK_MEMORY_EXPIRED == 2 && INFUR_TRACK_MEMORY_HELD == 3 &&
          INFUR_TRACK_MEMORY_WORDS == 4);
    uint32_t b[16];
    uint64_t t[16];
    std::memset(b, 0x5A, sizeof b);
    std::memset(t, 0x5A, sizeof t);
    CHECK(infur_tracker_set_memory(nullptr, 1, 0, 0) == INFUR_E_INVALID_ARG);
    CHECK(infur_tracker_memory(nullptr, b, 4, b, t, 1) == INFUR_E_INVALID_ARG);
    CHECK(infur_tracker_memory_dev(nullptr, b, 4, b, t, 1) == INFUR_E_INVALID_ARG);
    for (int i = 0; i < 16; i++) CHECK(b[i] == 0x5A5A5A5Au && t[i] == 0x5A5A5A5A5A5A5A5Aull);
    std::printf("cpu ok\n");
    return 0;
}

// 150 x 70, class 0 with one class-2 rectangle [60, 70) x [30, 40), or none
static infur::Planes plane_of(bool rect) {
    infur::Planes p;
    p.width = 150;
    p.height = 70;
    p.klass.assign((size_t)150 * 70, 0);
    if (rect)
        for (uint32_t y = 30; y < 40; y++)
            for (uint32_t x = 60; x < 70; x++) p.klass[(size_t)y * 150 + x] = 2;
    return p;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Regions reg(c);
    infur::Tracks trk(c);
    infur::RegionsOut r;
    infur::TracksOut t;
    infur::TracksMemory m;
    CHECK(trk.ok() && trk.memory(m, 2, 2) == INFUR_E_INVALID_ARG);  // no memory yet
    CHECK(trk.set_memory(1, 0, 65537) == INFUR_E_INVALID_ARG && trk.set_memory(1) == INFUR_OK && trk.is_dirty());
    // frame 0: background is track 0, the rectangle track 1
    CHECK(reg.advance(plane_of(true), r) == INFUR_OK && r.n == 2 && trk.advance(r, t) == INFUR_OK);
    CHECK(t.track_of_region[0] == 0 && t.track_of_region[1] == 1 && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 2);
    CHECK(trk.memory(m, 3, 2) == INFUR_OK && m.held() == 0 && m.lost.empty() && m.gap_of_region.size() == 3);
    const uint64_t sx = r.word(1, INFUR_STAT_SUM_X), sy = r.word(1, INFUR_STAT_SUM_Y);
    // frame 1: the rectangle is gone -- its track ends and waits in the gallery, SEEN = 0
    CHECK(reg.advance(plane_of(false), r) == INFUR_OK && r.n == 1 && trk.advance(r, t) == INFUR_OK);
    CHECK(t.summary[INFUR_TRACKS_SUMMARY_CONTINUED] == 1 && t.summary[INFUR_TRACKS_SUMMARY_ENDED] == 1);
    CHECK(trk.memory(m, 1, 4) == INFUR_OK && m.summary[INFUR_TRACK_MEMORY_LOST] == 1 && m.held() == 1 && m.lost.size() == INFUR_LOST_WORDS);
    CHECK(m.word(0, INFUR_LOST_ID) == 1 && m.word(0, INFUR_LOST_AGE) == 1 && m.word(0, INFUR_LOST_BORN) == 0 && m.word(0, INFUR_LOST_CLASS) == 2);
    CHECK(m.word(0, INFUR_LOST_PIXELS) == 100 && m.word(0, INFUR_LOST_SUM_X) == sx && m.word(0, INFUR_LOST_SUM_Y) == sy);
    CHECK(m.word(0, INFUR_LOST_MIN_X) == 60 && m.word(0, INFUR_LOST_MIN_Y) == 30 && m.word(0, INFUR_LOST_MAX_X) == 69 &&
          m.word(0, INFUR_LOST_MAX_Y) == 39 && m.word(0, INFUR_LOST_SEEN) == 0);
    // frame 2: it returns with its id, age 2, born 0, the entry's sums in the PREV words, gap 1
    CHECK(reg.advance(plane_of(true), r) == INFUR_OK && r.n == 2 && trk.advance(r, t) == INFUR_OK);
    CHECK(t.status() == 0 && t.track_of_region[0] == 0 && t.track_of_region[1] == 1 && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 0);
    CHECK(t.summary[INFUR_TRACKS_SUMMARY_CONTINUED] == 1 && t.word(1, INFUR_TRACK_AGE) == 2 && t.word(1, INFUR_TRACK_BORN) == 0);
    CHECK(t.word(1, INFUR_TRACK_PREV_REGION) == INFUR_REGION_NONE && t.word(1, INFUR_TRACK_OVERLAP) == 0 && t.word(1, INFUR_TRACK_PREV_PIXELS) == 100 &&
          t.word(1, INFUR_TRACK_PREV_SUM_X) == sx && t.word(1, INFUR_TRACK_PREV_SUM_Y) == sy);
    CHECK(trk.memory(m, 4, 1) == INFUR_OK && m.summary[INFUR_TRACK_MEMORY_REVIVED] == 1 && m.held() == 0 && m.lost.empty());
    CHECK(m.gap_of_region[0] == 0 && m.gap_of_region[1] == 1 && m.gap_of_region[2] == 0 && m.gap_of_region[3] == 0);
    // two empty frames are one too many for max_lost = 1: the entry expires and the rectangle is new
    for (int i = 0; i < 2; i++) CHECK(reg.advance(plane_of(false), r) == INFUR_OK && trk.advance(r, t) == INFUR_OK);
    CHECK(trk.memory(m, 0, 0) == INFUR_OK && m.held() == 1);
    CHECK(reg.advance(plane_of(true), r) == INFUR_OK && trk.advance(r, t) == INFUR_OK && t.track_of_region[1] == 2);
    CHECK(trk.memory(m, 2, 0) == INFUR_OK && m.summary[INFUR_TRACK_MEMORY_EXPIRED] == 1 && m.held() == 0 && m.gap_of_region[1] == 0);
    // memory off again: the calls refuse, the tracker tracks on
    CHECK(trk.set_memory(0) == INFUR_OK && trk.memory(m, 2, 0) == INFUR_E_INVALID_ARG);
    CHECK(trk.advance(r, t) == INFUR_OK && t.summary[INFUR_TRACKS_SUMMARY_NEW] == 2 && t.track_of_region[0] == 3);
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
