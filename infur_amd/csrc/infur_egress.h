// infur_egress.h -- the host side the egress stages share (Runs, Outlines, Simplify, Coverage; internal, beside infur_rt.h): the
// argument checks with their messages, the read-back of a polygon stage, the host-pointer frame wrapper of the three polygon
// frame calls, and the two front halves of their _dev forms.  The sizes and row rules are egress_layout.h's.  Every frame path
// here enqueues eagerly on the context's stream, and every buffer is private scratch no captured graph of the library can point
// into: growing it leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#pragma once
#include <cstring>

#include "infur_rt.h"

namespace infur {

static_assert(kLoopBytes == INFUR_LOOP_WORDS * 4 && kStatRowBytes == INFUR_STAT_WORDS * 8 && kStatsMaxClasses == (uint32_t)kSegMaxClasses &&
                  kCountsOutBytes == INFUR_COVERAGE_COUNT_WORDS * 4,
              "egress_layout.h and the public header disagree");

// ---- argument checks, in the words the stages have always used ----
// a plane's element size, the stage's flags (`noun`: "runs", "outlines", "coverage") and the skip value
inline int32_t elem_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t known_flags, const char* noun, uint32_t skip_value) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_bytes %u: 1 or 4", elem_bytes);
    if (flags & ~known_flags) return fail(c, INFUR_E_INVALID_ARG, "unknown %s flags 0x%x", noun, flags);
    if (elem_bytes == 1 && skip_value > 255) return fail(c, INFUR_E_INVALID_ARG, "skip_value %u: a byte plane holds at most 255", skip_value);
    return INFUR_OK;
}
inline int32_t tol_check(infur_ctx* c, uint32_t tol16) {
    if (tol16 > 65535) return fail(c, INFUR_E_INVALID_ARG, "tol16 %u: at most 65535 (4095.9 pixels)", tol16);
    return INFUR_OK;
}
// sides of at most kMaxSide; Simplify, which reads no plane, lets a height of 0 pass
inline int32_t side_check(infur_ctx* c, uint32_t h, uint32_t w, bool empty_ok) {
    if (w != 0 && w <= kMaxSide && h <= kMaxSide && (h != 0 || empty_ok)) return INFUR_OK;
    if (empty_ok) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a plane of width 1 to %u and height up to %u", w, h, kMaxSide, kMaxSide);
    return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a plane of width and height 1 to %u", w, h, kMaxSide);
}
// `sfx`: "" where the arguments are loops, vertices, counts (Outlines), "_out" behind Outlines
inline int32_t wanted_check(infur_ctx* c, const void* loops, uint32_t loops_rows, const void* vertices, uint32_t vertex_rows, const void* counts,
                            const char* sfx) {
    if ((loops && loops_rows) || (vertices && vertex_rows) || counts) return INFUR_OK;
    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: loops%s (with rows), vertices%s (with rows) or counts%s", sfx, sfx, sfx);
}
inline int32_t no_plane(infur_ctx* c, uint32_t h, uint32_t w) { return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no plane pointer", w, h); }
// Outlines' output as the input of the stage behind it: the counts, and a pointer for whatever rows are declared
inline int32_t input_check(infur_ctx* c, const void* loops, uint32_t loops_rows_in, const void* vertices, uint32_t vertex_rows_in, const void* counts) {
    if (!counts) return fail(c, INFUR_E_INVALID_ARG, "no counts: Outlines' {n_loops, n_vertices, ..} say how much of the input there is");
    if ((!loops && loops_rows_in) || (!vertices && vertex_rows_in))
        return fail(c, INFUR_E_INVALID_ARG, "%u records and %u vertices declared and no pointer to them", loops_rows_in, vertex_rows_in);
    return INFUR_OK;
}

// ---- read-back ----
// the statistics table of a host-pointer frame call, enqueued behind its _dev sibling
inline int32_t stats_read_back(infur_ctx* c, uint64_t* stats, const void* d_stats) {
    if (stats) HIPCHK(c, hipMemcpyAsync(stats, d_stats, (size_t)c->num_classes * kStatRowBytes, hipMemcpyDeviceToHost, c->stream));
    return INFUR_OK;
}
// The counts first: they decide how many records and vertices there are to copy.  `nothing_mask`: the status bits (counts[3])
// under which nothing but the counts was written.
inline int32_t poly_read_back(infur_ctx* c, const uint8_t* base, const PolyStage& st, size_t count_words, uint32_t nothing_mask, uint32_t* loops,
                              uint32_t* vertices, uint32_t* counts) {
    uint32_t n[kCountsOutBytes / 4] = {};
    HIPCHK(c, hipMemcpyAsync(n, base + st.counts_out, count_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t nl = copy_rows(n[0], st.loops_rows, (n[3] & nothing_mask) != 0), nv = copy_rows(n[1], st.vertex_rows);
    if (loops && nl) HIPCHK(c, hipMemcpy(loops, base + st.loops, nl * kLoopBytes, hipMemcpyDeviceToHost));
    if (vertices && nv) HIPCHK(c, hipMemcpy(vertices, base + st.vertices, nv * kVertexBytes, hipMemcpyDeviceToHost));
    if (counts) std::memcpy(counts, n, count_words * 4);
    return INFUR_OK;
}

// ---- the host-pointer form of a polygon frame call (frame_host, infur_rt.h) ----
struct PolyHostOut {  // the caller's arrays
    uint32_t* loops;
    uint32_t loops_rows;
    uint32_t* vertices;
    uint32_t vertex_rows;
    uint32_t* counts;
    uint64_t* stats;
    uint32_t stats_capacity;
};
struct PolyDevOut {  // their staging, as the _dev sibling takes it: null where the caller wants nothing
    void *loops, *vertices, *counts, *stats;
    uint32_t loops_rows, vertex_rows;
};
//   io                     the stage's staging buffer
//   lattice                the vertices may include the lattice's junctions (Coverage)
//   dev(d_bgr, d_sc, out)  the _dev sibling on the staged frame and outputs
template <class Dev>
int32_t poly_frame_host(infur_ctx* c, Buf& io, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint8_t* scaled, uint32_t* ow, uint32_t* oh,
                        const PolyHostOut& o, size_t count_words, uint32_t nothing_mask, bool lattice, Dev&& dev) {
    PolyStage st(0, 0, 0, 0, 0, 0);
    uint8_t* base = nullptr;
    const bool any = (o.loops && o.loops_rows) || (o.vertices && o.vertex_rows) || o.counts;
    return frame_host(
        c, bgr, w, h, factor, scaled, ow, oh,
        [&](size_t npix) -> int32_t {
            const size_t most = lattice ? frame_max_vertices_coverage(npix, *ow, *oh) : frame_max_vertices(npix);
            st = PolyStage(stage_rows(o.loops, o.loops_rows, frame_max_loops(npix)), stage_rows(o.vertices, o.vertex_rows, most),
                           staged_classes(o.stats, o.stats_capacity), 0, 0, 0);
            RETIF(ensure_private(c, io, st.bytes));
            base = (uint8_t*)io.p;
            return INFUR_OK;
        },
        [&](void* d_bgr, void* d_scaled) {
            return dev(d_bgr, d_scaled,
                       PolyDevOut{st.loops_rows ? base + st.loops : nullptr, st.vertex_rows ? base + st.vertices : nullptr, any ? base : nullptr,
                                  o.stats ? base + st.stats : nullptr, (uint32_t)st.loops_rows, (uint32_t)st.vertex_rows});
        },
        [&](size_t) -> int32_t {
            RETIF(stats_read_back(c, o.stats, base + st.stats));
            return poly_read_back(c, base, st, count_words, nothing_mask, o.loops, o.vertices, o.counts);
        });
}

// ---- the front halves of the _dev frame calls ----
// Scale -> model -> Segments decode of the class plane into the private scratch `plane`, with that call's own checks, errors and
// MODEL_NOT_LOADED rule.  check(rows of the scaled frame): the stage's own output checks, made only where a model is loaded
// and the frame scales, so that without one Scale still runs.  -> *klass: the class plane on the device
template <class Check>
int32_t frame_class_plane(infur_ctx* c, Buf& plane, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                          void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh, void** klass, Check&& check) {
    uint32_t rows = 0;
    const size_t npix = scale_npix(w, h, factor, &rows);
    *klass = nullptr;
    if (c->loaded && npix) {
        RETIF(check(rows));
        RETIF(ensure_private(c, plane, npix));
        *klass = plane.p;
    }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
    return infur_frame_segments_dev(c, d_bgr, w, h, factor, mode, decode, *klass, nullptr, npix, d_stats, stats_capacity, nullptr, 0, d_scaled, ow, oh);
}

// infur_frame_outlines_dev, which also hands out the class plane it outlined (infur_outlines.cpp)
int32_t frame_outlines_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                           uint32_t skip_value, uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows,
                           void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh, void** klass);

// What infur_frame_polygons_dev and infur_frame_coverage_dev do before their last call: the tolerance first, the scaled size
// before the model runs, then Outlines into st_poly.  On OK `at` and `base` say where the loops lie and `klass` where the class
// plane does.
struct PolyFront {
    PolyScratch at{1};
    uint8_t* base = nullptr;
    void* klass = nullptr;
};
inline int32_t poly_frame_front(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                uint32_t skip_value, uint32_t max_edges, uint32_t tol16, bool empty_ok, const void* d_loops, uint32_t loops_rows,
                                const void* d_vertices, uint32_t vertex_rows, const void* d_counts, void* d_stats, uint32_t stats_capacity,
                                void* d_scaled, uint32_t* ow, uint32_t* oh, PolyFront* f) {
    RETIF(tol_check(c, tol16));
    const size_t npix = scale_npix(w, h, factor);
    uint32_t sw = 0, sh = 0;
    if (npix && infur_scale_out_dims(w, h, factor, &sw, &sh) == INFUR_OK) RETIF(side_check(c, sh, sw, empty_ok));
    if (c->loaded && npix) {
        RETIF(wanted_check(c, d_loops, loops_rows, d_vertices, vertex_rows, d_counts, "_out"));
        f->at = PolyScratch(edge_capacity(npix, max_edges));
        RETIF(ensure_private(c, c->st_poly, f->at.bytes));
        f->base = (uint8_t*)c->st_poly.p;
    }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
    uint8_t* b = f->base;
    return frame_outlines_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, b ? b + f->at.loops : nullptr,
                              (uint32_t)f->at.loops_rows, b ? b + f->at.vertices : nullptr, (uint32_t)f->at.vertex_rows, b, d_stats, stats_capacity,
                              d_scaled, ow, oh, &f->klass);
}

}  // namespace infur
