// infur_coverage.cpp -- Coverage, Simplify's sibling behind Outlines (include/infur_hip.h): the loops Outlines left in device
// memory simplified arc by arc, so that the polygons of neighbouring regions still share their borders.  Kernels: coverage.hip.
// Everything is enqueued on the context's stream; the layout, checks, read-back, frame wrapper and the front half of the frame
// call it shares with the other egress stages are infur_egress.h's, and so is the rule that its buffers are private scratch.
#include "infur_egress.h"

using namespace infur;

namespace {

constexpr uint32_t kNothing = INFUR_COVERAGE_TRUNCATED | INFUR_COVERAGE_OVERFLOW;  // nothing but the counts was written

int32_t coverage_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value, uint32_t tol16, uint32_t h, uint32_t w) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_COVERAGE_SKIP, "coverage", skip_value));
    RETIF(tol_check(c, tol16));
    return side_check(c, h, w, false);
}

}  // namespace

extern "C" {

int32_t infur_coverage_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                           const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in, const void* d_counts,
                           uint32_t tol16, uint32_t aug_rows, void* d_loops_out, uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out,
                           void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(coverage_check(c, elem_bytes, flags, skip_value, tol16, h, w));
        RETIF(wanted_check(c, d_loops_out, loops_rows_out, d_vertices_out, vertex_rows_out, d_counts_out, "_out"));
        if (!d_plane) return no_plane(c, h, w);
        RETIF(input_check(c, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts));
        const uint64_t all = (uint64_t)vertex_rows_in + (uint64_t)(h + 1) * (w + 1);  // every vertex and every junction: cannot overflow
        if (all > 0xFFFFFFFEull) return fail(c, INFUR_E_INVALID_ARG, "vertex_rows_in %u: with the lattice at most 2^32 - 2", vertex_rows_in);
        if (aug_rows == 0xFFFFFFFFu) return fail(c, INFUR_E_INVALID_ARG, "aug_rows: at most 2^32 - 2");
        const uint32_t rows = aug_rows ? aug_rows : (uint32_t)all;
        RETIF(ensure_private(c, c->st_cov, coverage_scratch_bytes(h, w, loops_rows_in, rows)));
        ProfScope ps(c, "coverage", "coverage", 0, (double)vertex_rows_in * 4 + (double)loops_rows_in * 16 + (double)h * w * elem_bytes * 8);
        HIPCHK(c, launch_coverage(d_plane, (int)elem_bytes, h, w, (flags & INFUR_COVERAGE_SKIP) != 0, skip_value, (const unsigned*)d_loops, loops_rows_in,
                                  (const unsigned*)d_vertices, vertex_rows_in, (const unsigned*)d_counts, tol16, rows, c->st_cov.p,
                                  loops_rows_out ? (unsigned*)d_loops_out : nullptr, d_loops_out ? loops_rows_out : 0,
                                  vertex_rows_out ? (unsigned*)d_vertices_out : nullptr, d_vertices_out ? vertex_rows_out : 0, (unsigned*)d_counts_out,
                                  c->stream));
        return INFUR_OK;
    });
}

int32_t infur_coverage(infur_ctx* c, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                       const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices, uint32_t vertex_rows_in, const uint32_t* counts,
                       uint32_t tol16, uint32_t aug_rows, uint32_t* loops_out, uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out,
                       uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(coverage_check(c, elem_bytes, flags, skip_value, tol16, h, w));
        RETIF(wanted_check(c, loops_out, loops_rows_out, vertices_out, vertex_rows_out, counts_out, "_out"));
        if (!plane) return no_plane(c, h, w);
        RETIF(input_check(c, loops, loops_rows_in, vertices, vertex_rows_in, counts));
        // only what the counts say there is travels; the output holds at most every input vertex and every lattice vertex
        const size_t nl = copy_rows(counts[0], loops_rows_in), nv = copy_rows(counts[1], vertex_rows_in);
        const size_t most = nv + (size_t)(h + 1) * (w + 1), plane_bytes = (size_t)h * w * elem_bytes;
        const PolyStage st(stage_rows(loops_out, loops_rows_out, nl), stage_rows(vertices_out, vertex_rows_out, most), 0, nl, nv, plane_bytes);
        RETIF(ensure_private(c, c->st_cov_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_cov_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.counts_in, counts, 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, plane_bytes, hipMemcpyHostToDevice, c->stream));
        if (nl) HIPCHK(c, hipMemcpyAsync(base + st.loops_in, loops, nl * INFUR_LOOP_WORDS * 4, hipMemcpyHostToDevice, c->stream));
        if (nv) HIPCHK(c, hipMemcpyAsync(base + st.vertices_in, vertices, nv * 4, hipMemcpyHostToDevice, c->stream));
        // (the rows declared to the device are what was copied: truncated input stays truncated, counts[k] > rows)
        RETIF(infur_coverage_dev(c, base + st.plane, elem_bytes, h, w, flags, skip_value, base + st.loops_in, (uint32_t)nl, base + st.vertices_in, (uint32_t)nv,
                                 base + st.counts_in, tol16, aug_rows, st.loops_rows ? base + st.loops : nullptr, (uint32_t)st.loops_rows,
                                 st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows, base));
        return poly_read_back(c, base, st, INFUR_COVERAGE_COUNT_WORDS, kNothing, loops_out, vertices_out, counts_out);
    });
}

int32_t infur_frame_coverage_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                 uint32_t skip_value, uint32_t max_edges, uint32_t tol16, void* d_loops, uint32_t loops_rows, void* d_vertices,
                                 uint32_t vertex_rows, void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        PolyFront f;  // scale -> model -> Segments decode -> Outlines, which also hands out the class plane it outlined
        RETIF(poly_frame_front(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, tol16, false, d_loops, loops_rows, d_vertices, vertex_rows,
                               d_counts, d_stats, stats_capacity, d_scaled, ow, oh, &f));
        return infur_coverage_dev(c, f.klass, 1, *oh, *ow, flags & INFUR_OUTLINES_SKIP ? INFUR_COVERAGE_SKIP : 0, skip_value, f.base + f.at.loops,
                                  (uint32_t)f.at.loops_rows, f.base + f.at.vertices, (uint32_t)f.at.vertex_rows, f.base, tol16, 0, d_loops, loops_rows,
                                  d_vertices, vertex_rows, d_counts);
    });
}

int32_t infur_frame_coverage(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, uint32_t max_edges, uint32_t tol16, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices,
                             uint32_t vertex_rows, uint32_t* counts, uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        return poly_frame_host(c, c->st_cov_io, bgr, w, h, factor, scaled, ow, oh, {loops, loops_rows, vertices, vertex_rows, counts, stats, stats_capacity},
                               INFUR_COVERAGE_COUNT_WORDS, kNothing, true, [&](void* d_bgr, void* d_scaled, const PolyDevOut& d) {
                                   return infur_frame_coverage_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, tol16, d.loops,
                                                                   d.loops_rows, d.vertices, d.vertex_rows, d.counts, d.stats, stats_capacity, d_scaled, ow,
                                                                   oh);
                               });
    });
}

}  // extern "C"
