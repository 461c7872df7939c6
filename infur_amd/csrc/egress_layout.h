// egress_layout.h -- the arithmetic the egress stages' host sides share (infur_runs.cpp, infur_outlines.cpp, infur_simplify.cpp,
// infur_coverage.cpp): the staging layout of the polygon stages, what Outlines leaves for the stage behind it, and the row rules
// that decide how many bytes a copy moves into a caller's array.  No HIP and no project header: plain g++ compiles it
// (tests/cpp/egress_layout_test.cpp sweeps it under the sanitizers).  infur_egress.h ties the constants to the public header's.
#pragma once
#include <cstddef>
#include <cstdint>

namespace infur {

inline constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline constexpr size_t min_rows(size_t a, size_t b) { return a < b ? a : b; }

constexpr size_t kSlotAlign = 256;                                 // every staging slot starts on such a boundary
constexpr size_t kLoopBytes = 16, kVertexBytes = 4, kStatRowBytes = 64;  // a loop record, a vertex id, one class of the statistics
constexpr size_t kCountsOutBytes = 24, kCountsInBytes = 8;         // Coverage's six count words; Outlines' {n_loops, n_vertices}
constexpr uint32_t kStatsMaxClasses = 256;                         // the class byte holds no more (kernels.h: kSegMaxClasses)
constexpr uint32_t kMaxSide = 8191;  // Simplify, Coverage: every coordinate difference stays below 2^13: 256 * cross^2 < 2^62

// the classes a host-pointer frame call stages statistics for
inline uint32_t staged_classes(bool wanted, uint32_t capacity) { return wanted ? (capacity < kStatsMaxClasses ? capacity : kStatsMaxClasses) : 0; }

// the capacity of Outlines in edges: 0 and anything above the worst case are the worst case
inline size_t edge_capacity(size_t hw, uint32_t max_edges) { return max_edges && max_edges < hw * 4 ? max_edges : hw * 4; }

// the most a frame of npix = w x h pixels can produce: one loop per pixel; four vertices per pixel, and behind Coverage the
// lattice's junctions as well
inline size_t frame_max_loops(size_t npix) { return npix; }
inline size_t frame_max_vertices(size_t npix) { return npix * 4; }
inline size_t frame_max_vertices_coverage(size_t npix, size_t w, size_t h) { return npix * 4 + (w + 1) * (h + 1); }

// rows to stage for an output: none where the caller has no array, never more than there can be
inline size_t stage_rows(bool wanted, uint32_t rows, size_t most) { return wanted ? min_rows(rows, most) : 0; }
// rows to copy back: what the count says, within what was staged; `nothing`: the status says that no record was written
inline size_t copy_rows(uint32_t n, size_t rows, bool nothing = false) { return nothing ? 0 : min_rows(n, rows); }

// The staging of a polygon stage's host-pointer calls (st_outl_io, st_simp_io, st_cov_io):
// [counts out][counts in][statistics table k x 8 u64][records out][vertices out][records in][vertices in][plane], each slot on
// a 256-byte boundary; a slot of size zero costs nothing.  The rows are what stage_rows left of the caller's.
struct PolyStage {
    size_t loops_rows, vertex_rows;
    size_t counts_out, counts_in, stats, loops, vertices, loops_in, vertices_in, plane, bytes;
    PolyStage(size_t loops_rows_, size_t vertex_rows_, uint32_t k, size_t loops_rows_in, size_t vertex_rows_in, size_t plane_bytes)
        : loops_rows(loops_rows_), vertex_rows(vertex_rows_) {
        counts_out = 0;
        counts_in = counts_out + align_up(kCountsOutBytes, kSlotAlign);
        stats = counts_in + align_up(kCountsInBytes, kSlotAlign);
        loops = stats + align_up((size_t)k * kStatRowBytes, kSlotAlign);
        vertices = loops + align_up(loops_rows * kLoopBytes, kSlotAlign);
        loops_in = vertices + align_up(vertex_rows * kVertexBytes, kSlotAlign);
        vertices_in = loops_in + align_up(loops_rows_in * kLoopBytes, kSlotAlign);
        plane = vertices_in + align_up(vertex_rows_in * kVertexBytes, kSlotAlign);
        bytes = plane + align_up(plane_bytes, kSlotAlign);
    }
};

// st_poly, what Outlines leaves for Simplify or Coverage inside the polygon frame calls: [counts][records][vertices].  `cap` is
// edge_capacity(): a loop has at least four edges and a vertex is the tail of one
struct PolyScratch {
    size_t loops_rows, vertex_rows, loops, vertices, bytes;
    explicit PolyScratch(size_t cap) {
        loops_rows = cap / 4 ? cap / 4 : 1;
        vertex_rows = cap;
        loops = kSlotAlign;
        vertices = loops + align_up(loops_rows * kLoopBytes, kSlotAlign);
        bytes = vertices + align_up(vertex_rows * kVertexBytes, kSlotAlign);
    }
};

}  // namespace infur
