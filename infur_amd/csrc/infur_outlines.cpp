// infur_outlines.cpp -- Outlines, the polygon stage behind the four decodes (include/infur_hip.h): the boundaries of the regions
// of a byte or u32 plane as closed loops of lattice vertices, so that a host copies out polygons and not the dense plane.
// Kernels: outlines.hip.  Everything is enqueued on the context's stream; the layout, checks, read-back and frame wrapper it
// shares with the other egress stages are infur_egress.h's, and so is the rule that its buffers are private scratch.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kLoopWords == INFUR_LOOP_WORDS, "outlines.hip and the header disagree about the record");

int32_t outlines_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value) {
    return elem_check(c, elem_bytes, flags, INFUR_OUTLINES_SKIP | INFUR_OUTLINES_CONN8, "outlines", skip_value);
}

// an edge id is 4 * i + s in a u32, and 0xFFFFFFFF stands for none
int32_t outlines_plane_check(infur_ctx* c, uint32_t h, uint32_t w) {
    if ((size_t)h * w * 4 >= 0xFFFFFFFFull) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: an edge indexes at most 2^30 - 1 pixels", w, h);
    return INFUR_OK;
}

}  // namespace

// infur_frame_outlines_dev; *klass: the class plane it decoded into st_outl_plane and outlined, for the stage behind it
int32_t infur::frame_outlines_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                  uint32_t skip_value, uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows,
                                  void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh, void** klass) {
    if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
    RETIF(outlines_check(c, 1, flags, skip_value));
    RETIF(frame_class_plane(c, c->st_outl_plane, d_bgr, w, h, factor, mode, decode, d_stats, stats_capacity, d_scaled, ow, oh, klass,
                            [&](uint32_t) { return wanted_check(c, d_loops, loops_rows, d_vertices, vertex_rows, d_counts, ""); }));
    return infur_outlines_dev(c, *klass, 1, *oh, *ow, flags, skip_value, max_edges, d_loops, loops_rows, d_vertices, vertex_rows, d_counts);
}

extern "C" {

int32_t infur_outlines_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                           uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, elem_bytes, flags, skip_value));
        RETIF(outlines_plane_check(c, h, w));
        const size_t hw = (size_t)h * w;
        RETIF(wanted_check(c, d_loops, loops_rows, d_vertices, vertex_rows, d_counts, ""));
        if (hw == 0) {  // empty plane: no edge
            if (d_counts) HIPCHK(c, hipMemsetAsync(d_counts, 0, 12, c->stream));
            return INFUR_OK;
        }
        if (!d_plane) return no_plane(c, h, w);
        const size_t cap = edge_capacity(hw, max_edges);
        RETIF(ensure_private(c, c->st_outl, outlines_scratch_bytes(hw, cap)));
        ProfScope ps(c, "outlines", "outlines", 0, (double)hw * elem_bytes * 4);
        // (d_loops goes to the kernel as given, also with no rows: Simplify and Coverage null such a pointer)
        HIPCHK(c, launch_outlines(d_plane, (int)elem_bytes, h, w, (flags & INFUR_OUTLINES_SKIP) != 0, (flags & INFUR_OUTLINES_CONN8) != 0, skip_value, cap,
                                  c->st_outl.p, (unsigned*)d_loops, d_loops ? loops_rows : 0, (unsigned*)d_vertices, d_vertices ? vertex_rows : 0,
                                  (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_outlines(infur_ctx* c, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                       uint32_t max_edges, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, elem_bytes, flags, skip_value));
        RETIF(outlines_plane_check(c, h, w));
        const size_t hw = (size_t)h * w;
        RETIF(wanted_check(c, loops, loops_rows, vertices, vertex_rows, counts, ""));
        if (hw == 0) {
            if (counts) std::memset(counts, 0, 12);
            return INFUR_OK;
        }
        if (!plane) return no_plane(c, h, w);
        const PolyStage st(stage_rows(loops, loops_rows, frame_max_loops(hw)), stage_rows(vertices, vertex_rows, frame_max_vertices(hw)), 0, 0, 0,
                           hw * elem_bytes);
        RETIF(ensure_private(c, c->st_outl_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_outl_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_outlines_dev(c, base + st.plane, elem_bytes, h, w, flags, skip_value, max_edges, st.loops_rows ? base + st.loops : nullptr,
                                 (uint32_t)st.loops_rows, st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows, base));
        return poly_read_back(c, base, st, 3, 0, loops, vertices, counts);
    });
}

int32_t infur_frame_outlines_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                 uint32_t skip_value, uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows,
                                 void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        void* klass = nullptr;
        return frame_outlines_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, d_loops, loops_rows, d_vertices, vertex_rows, d_counts,
                                  d_stats, stats_capacity, d_scaled, ow, oh, &klass);
    });
}

int32_t infur_frame_outlines(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, uint32_t max_edges, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows,
                             uint32_t* counts, uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, 1, flags, skip_value));
        return poly_frame_host(c, c->st_outl_io, bgr, w, h, factor, scaled, ow, oh, {loops, loops_rows, vertices, vertex_rows, counts, stats, stats_capacity},
                               3, 0, false, [&](void* d_bgr, void* d_scaled, const PolyDevOut& d) {
                                   return infur_frame_outlines_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, d.loops, d.loops_rows,
                                                                   d.vertices, d.vertex_rows, d.counts, d.stats, stats_capacity, d_scaled, ow, oh);
                               });
    });
}

}  // extern "C"
