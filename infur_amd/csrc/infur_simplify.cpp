// infur_simplify.cpp -- Simplify, the stage behind Outlines (include/infur_hip.h): Douglas-Peucker on the loops Outlines left in
// device memory, so that a host copies out polygons with a tolerance and not the pixel staircase.  Kernels: simplify.hip.
// Everything is enqueued on the context's stream; the layout, checks, read-back, frame wrapper and the front half of the frame
// call it shares with the other egress stages are infur_egress.h's, and so is the rule that its buffers are private scratch.
#include "infur_egress.h"

using namespace infur;

namespace {

int32_t simplify_check(infur_ctx* c, uint32_t h, uint32_t w, uint32_t tol16) {
    RETIF(side_check(c, h, w, true));
    return tol_check(c, tol16);
}

}  // namespace

extern "C" {

int32_t infur_simplify_dev(infur_ctx* c, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in,
                           const void* d_counts, uint32_t h, uint32_t w, uint32_t tol16, void* d_loops_out, uint32_t loops_rows_out,
                           void* d_vertices_out, uint32_t vertex_rows_out, void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(simplify_check(c, h, w, tol16));
        RETIF(wanted_check(c, d_loops_out, loops_rows_out, d_vertices_out, vertex_rows_out, d_counts_out, "_out"));
        RETIF(input_check(c, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts));
        if (vertex_rows_in == 0xFFFFFFFFu) return fail(c, INFUR_E_INVALID_ARG, "vertex_rows_in: at most 2^32 - 2");
        RETIF(ensure_private(c, c->st_simp, simplify_scratch_bytes(loops_rows_in, vertex_rows_in)));
        ProfScope ps(c, "simplify", "simplify", 0, (double)vertex_rows_in * 4 + (double)loops_rows_in * 16);
        HIPCHK(c, launch_simplify((const unsigned*)d_loops, loops_rows_in, (const unsigned*)d_vertices, vertex_rows_in, (const unsigned*)d_counts, w, tol16,
                                  c->st_simp.p, loops_rows_out ? (unsigned*)d_loops_out : nullptr, d_loops_out ? loops_rows_out : 0,
                                  vertex_rows_out ? (unsigned*)d_vertices_out : nullptr, d_vertices_out ? vertex_rows_out : 0, (unsigned*)d_counts_out,
                                  c->stream));
        return INFUR_OK;
    });
}

int32_t infur_simplify(infur_ctx* c, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices, uint32_t vertex_rows_in,
                       const uint32_t* counts, uint32_t h, uint32_t w, uint32_t tol16, uint32_t* loops_out, uint32_t loops_rows_out,
                       uint32_t* vertices_out, uint32_t vertex_rows_out, uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(simplify_check(c, h, w, tol16));
        RETIF(wanted_check(c, loops_out, loops_rows_out, vertices_out, vertex_rows_out, counts_out, "_out"));
        RETIF(input_check(c, loops, loops_rows_in, vertices, vertex_rows_in, counts));
        // only what the counts say there is travels; an output is never longer than its input
        const size_t nl = copy_rows(counts[0], loops_rows_in), nv = copy_rows(counts[1], vertex_rows_in);
        const PolyStage st(stage_rows(loops_out, loops_rows_out, nl), stage_rows(vertices_out, vertex_rows_out, nv), 0, nl, nv, 0);
        RETIF(ensure_private(c, c->st_simp_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_simp_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.counts_in, counts, 8, hipMemcpyHostToDevice, c->stream));
        if (nl) HIPCHK(c, hipMemcpyAsync(base + st.loops_in, loops, nl * INFUR_LOOP_WORDS * 4, hipMemcpyHostToDevice, c->stream));
        if (nv) HIPCHK(c, hipMemcpyAsync(base + st.vertices_in, vertices, nv * 4, hipMemcpyHostToDevice, c->stream));
        // (the rows declared to the device are what was copied: truncated input stays truncated, counts[k] > rows)
        RETIF(infur_simplify_dev(c, base + st.loops_in, (uint32_t)nl, base + st.vertices_in, (uint32_t)nv, base + st.counts_in, h, w, tol16,
                                 st.loops_rows ? base + st.loops : nullptr, (uint32_t)st.loops_rows, st.vertex_rows ? base + st.vertices : nullptr,
                                 (uint32_t)st.vertex_rows, base));
        return poly_read_back(c, base, st, INFUR_SIMPLIFY_COUNT_WORDS, INFUR_SIMPLIFY_TRUNCATED, loops_out, vertices_out, counts_out);
    });
}

int32_t infur_frame_polygons_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                 uint32_t skip_value, uint32_t max_edges, uint32_t tol16, void* d_loops, uint32_t loops_rows, void* d_vertices,
                                 uint32_t vertex_rows, void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        PolyFront f;  // scale -> model -> Segments decode -> Outlines
        RETIF(poly_frame_front(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, tol16, true, d_loops, loops_rows, d_vertices, vertex_rows,
                               d_counts, d_stats, stats_capacity, d_scaled, ow, oh, &f));
        return infur_simplify_dev(c, f.base + f.at.loops, (uint32_t)f.at.loops_rows, f.base + f.at.vertices, (uint32_t)f.at.vertex_rows, f.base, *oh, *ow,
                                  tol16, d_loops, loops_rows, d_vertices, vertex_rows, d_counts);
    });
}

int32_t infur_frame_polygons(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, uint32_t max_edges, uint32_t tol16, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices,
                             uint32_t vertex_rows, uint32_t* counts, uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        return poly_frame_host(c, c->st_simp_io, bgr, w, h, factor, scaled, ow, oh, {loops, loops_rows, vertices, vertex_rows, counts, stats, stats_capacity},
                               INFUR_SIMPLIFY_COUNT_WORDS, INFUR_SIMPLIFY_TRUNCATED, false, [&](void* d_bgr, void* d_scaled, const PolyDevOut& d) {
                                   return infur_frame_polygons_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, tol16, d.loops,
                                                                   d.loops_rows, d.vertices, d.vertex_rows, d.counts, d.stats, stats_capacity, d_scaled, ow,
                                                                   oh);
                               });
    });
}

}  // extern "C"
