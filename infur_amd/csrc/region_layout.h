// region_layout.h -- the staging arithmetic the frame calls behind Regions share (infur_regions.cpp, infur_tracks.cpp,
// infur_anchors.cpp, infur_sieve.cpp, infur_shapes.cpp, infur_split.cpp, infur_skeleton.cpp, infur_centrelines.cpp,
// infur_expand.cpp, infur_appearance.cpp): where Regions' products lie in a stage's staging buffer, and Anchors' behind them.  No HIP and no project
// header but egress_layout.h: plain g++ compiles it (tests/cpp/region_layout_test.cpp sweeps it under the sanitizers).
// infur_region_frames.h ties the row constants to the public header's.
#pragma once
#include "egress_layout.h"

namespace infur {

constexpr size_t kRegionRowBytes = 80, kAnchorRowBytes = 8;  // a row of the region table, {pixel, dist2} of a region

// Regions' staged products from `at` on: [n_regions][region table, at most one row per pixel][label plane][class plane]
// [confidence plane], each slot on a 256-byte boundary.  `at` is on such a boundary; the stage's own slots lie before it or
// from `end` on.
struct RegLayout {
    size_t rows, n, table, labels, klass, conf, end;
    RegLayout(size_t at, size_t npix, uint32_t table_rows) {
        rows = min_rows(table_rows, npix);
        n = at;
        table = n + kSlotAlign;
        labels = table + align_up(rows * kRegionRowBytes, kSlotAlign);
        klass = labels + align_up(npix * 4, kSlotAlign);
        conf = klass + align_up(npix, kSlotAlign);
        end = conf + align_up(npix, kSlotAlign);
    }
};

// ... and Anchors' behind them: [dist2][anchors, anchor_rows x 2 words].  `end` is the end of both.
struct RegAnchLayout : RegLayout {
    size_t dist2, anchors;
    RegAnchLayout(size_t at, size_t npix, uint32_t table_rows, uint32_t anchor_rows) : RegLayout(at, npix, table_rows) {
        dist2 = end;
        anchors = dist2 + align_up(npix * 4, kSlotAlign);
        end = anchors + align_up((size_t)anchor_rows * kAnchorRowBytes, kSlotAlign);
    }
};

}  // namespace infur
