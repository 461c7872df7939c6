// infur_coverage.cpp -- Coverage, Simplify's sibling behind Outlines (include/infur_hip.h): the loops Outlines left in device
// memory simplified arc by arc, so that the polygons of neighbouring regions still share their borders.  Kernels: coverage.hip.
// Everything is enqueued on the context's stream.  Like infur_simplify.cpp the frame path here always enqueues eagerly, and every
// buffer of this file is private scratch no captured graph of the library can point into: growing it leaves mem_gen -- and with
// it the graphs infur_frame_advance_dev has cached -- alone.
#include <cstring>
#include <new>

#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"

using namespace infur;

namespace {

constexpr uint32_t kMaxSide = 8191;  // every coordinate difference stays below 2^13: 256 * cross^2 < 2^62

int32_t coverage_size_check(infur_ctx* c, uint32_t h, uint32_t w) {
    if (w == 0 || w > kMaxSide || h == 0 || h > kMaxSide) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a plane of width and height 1 to %u", w, h, kMaxSide);
    return INFUR_OK;
}

int32_t coverage_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value, uint32_t tol16) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_bytes %u: 1 or 4", elem_bytes);
    if (flags & ~(uint32_t)INFUR_COVERAGE_SKIP) return fail(c, INFUR_E_INVALID_ARG, "unknown coverage flags 0x%x", flags);
    if (elem_bytes == 1 && skip_value > 255) return fail(c, INFUR_E_INVALID_ARG, "skip_value %u: a byte plane holds at most 255", skip_value);
    if (tol16 > 65535) return fail(c, INFUR_E_INVALID_ARG, "tol16 %u: at most 65535 (4095.9 pixels)", tol16);
    return INFUR_OK;
}

const char* const kNothingWanted = "no output wanted: loops_out (with rows), vertices_out (with rows) or counts_out";
const char* const kNoCounts = "no counts: Outlines' {n_loops, n_vertices, ..} say how much of the input there is";

// st_cov_io: [counts_out][counts][statistics table k x 8 u64][records out][vertices out][records in][vertices in][plane], on
// 256-byte boundaries
struct CovStage {
    size_t loops_rows, vertex_rows, counts_in, stats, loops, vertices, loops_in, vertices_in, plane, bytes;
    CovStage(size_t loops_rows_, size_t vertex_rows_, uint32_t k, size_t loops_rows_in, size_t vertex_rows_in, size_t plane_bytes) {
        loops_rows = loops_rows_;
        vertex_rows = vertex_rows_;
        counts_in = 256;
        stats = 512;
        loops = stats + align_up((size_t)k * INFUR_STAT_WORDS * 8, 256);
        vertices = loops + align_up(loops_rows * INFUR_LOOP_WORDS * 4, 256);
        loops_in = vertices + align_up(vertex_rows * 4, 256);
        vertices_in = loops_in + align_up(loops_rows_in * INFUR_LOOP_WORDS * 4, 256);
        plane = vertices_in + align_up(vertex_rows_in * 4, 256);
        bytes = plane + align_up(plane_bytes, 256);
    }
};

// the counts first: they decide how many records and vertices there are to copy
int32_t coverage_read_back(infur_ctx* c, const uint8_t* base, const CovStage& st, uint32_t* loops, uint32_t* vertices, uint32_t* counts) {
    uint32_t n[INFUR_COVERAGE_COUNT_WORDS] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(n, base, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool nothing = (n[3] & (INFUR_COVERAGE_TRUNCATED | INFUR_COVERAGE_OVERFLOW)) != 0;  // nothing but the counts was written
    const size_t nl = nothing ? 0 : (n[0] < st.loops_rows ? n[0] : st.loops_rows), nv = n[1] < st.vertex_rows ? n[1] : st.vertex_rows;
    if (loops && nl) HIPCHK(c, hipMemcpy(loops, base + st.loops, nl * INFUR_LOOP_WORDS * 4, hipMemcpyDeviceToHost));
    if (vertices && nv) HIPCHK(c, hipMemcpy(vertices, base + st.vertices, nv * 4, hipMemcpyDeviceToHost));
    if (counts) std::memcpy(counts, n, sizeof n);
    return INFUR_OK;
}

// the capacity of Outlines in edges (infur_outlines.cpp): 0 and anything above the worst case are the worst case
size_t edge_capacity(size_t hw, uint32_t max_edges) { return max_edges && max_edges < hw * 4 ? max_edges : hw * 4; }

// st_cov_poly, what Outlines leaves for Coverage inside infur_frame_coverage_dev: [counts][records][vertices].  A loop has at
// least four edges and a vertex is the tail of one
struct PolyScratch {
    size_t loops_rows, vertex_rows, loops, vertices, bytes;
    explicit PolyScratch(size_t cap) {
        loops_rows = cap / 4 ? cap / 4 : 1;
        vertex_rows = cap;
        loops = 256;
        vertices = loops + align_up(loops_rows * INFUR_LOOP_WORDS * 4, 256);
        bytes = vertices + align_up(vertex_rows * 4, 256);
    }
};

}  // namespace

extern "C" {

int32_t infur_coverage_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                           const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in, const void* d_counts,
                           uint32_t tol16, uint32_t aug_rows, void* d_loops_out, uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out,
                           void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(coverage_check(c, elem_bytes, flags, skip_value, tol16));
        RETIF(coverage_size_check(c, h, w));
        if (!(d_loops_out && loops_rows_out) && !(d_vertices_out && vertex_rows_out) && !d_counts_out)
            return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
        if (!d_plane) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no plane pointer", w, h);
        if (!d_counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNoCounts);
        if ((!d_loops && loops_rows_in) || (!d_vertices && vertex_rows_in))
            return fail(c, INFUR_E_INVALID_ARG, "%u records and %u vertices declared and no pointer to them", loops_rows_in, vertex_rows_in);
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
        RETIF(coverage_check(c, elem_bytes, flags, skip_value, tol16));
        RETIF(coverage_size_check(c, h, w));
        if (!(loops_out && loops_rows_out) && !(vertices_out && vertex_rows_out) && !counts_out) return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
        if (!plane) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no plane pointer", w, h);
        if (!counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNoCounts);
        if ((!loops && loops_rows_in) || (!vertices && vertex_rows_in))
            return fail(c, INFUR_E_INVALID_ARG, "%u records and %u vertices declared and no pointer to them", loops_rows_in, vertex_rows_in);
        // only what the counts say there is travels; the output holds at most every input vertex and every lattice vertex
        const size_t nl = counts[0] < loops_rows_in ? counts[0] : loops_rows_in, nv = counts[1] < vertex_rows_in ? counts[1] : vertex_rows_in;
        const size_t most = nv + (size_t)(h + 1) * (w + 1);
        const size_t lrows = loops_out ? (loops_rows_out < nl ? loops_rows_out : nl) : 0, vrows = vertices_out ? (vertex_rows_out < most ? vertex_rows_out : most) : 0;
        const size_t plane_bytes = (size_t)h * w * elem_bytes;
        const CovStage st(lrows, vrows, 0, nl, nv, plane_bytes);
        RETIF(ensure_private(c, c->st_cov_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_cov_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.counts_in, counts, 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, plane_bytes, hipMemcpyHostToDevice, c->stream));
        if (nl) HIPCHK(c, hipMemcpyAsync(base + st.loops_in, loops, nl * INFUR_LOOP_WORDS * 4, hipMemcpyHostToDevice, c->stream));
        if (nv) HIPCHK(c, hipMemcpyAsync(base + st.vertices_in, vertices, nv * 4, hipMemcpyHostToDevice, c->stream));
        // (the rows declared to the device are what was copied: truncated input stays truncated, counts[k] > rows)
        RETIF(infur_coverage_dev(c, base + st.plane, elem_bytes, h, w, flags, skip_value, base + st.loops_in, (uint32_t)nl, base + st.vertices_in, (uint32_t)nv,
                                 base + st.counts_in, tol16, aug_rows, lrows ? base + st.loops : nullptr, (uint32_t)lrows, vrows ? base + st.vertices : nullptr,
                                 (uint32_t)vrows, base));
        return coverage_read_back(c, base, st, loops_out, vertices_out, counts_out);
    });
}

int32_t infur_frame_coverage_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                 uint32_t skip_value, uint32_t max_edges, uint32_t tol16, void* d_loops, uint32_t loops_rows, void* d_vertices,
                                 uint32_t vertex_rows, void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(coverage_check(c, 1, 0, 0, tol16));
        const size_t npix = scale_npix(w, h, factor);
        PolyScratch at(1);
        uint8_t* base = nullptr;
        uint32_t sw = 0, sh = 0;
        if (npix && infur_scale_out_dims(w, h, factor, &sw, &sh) == INFUR_OK) RETIF(coverage_size_check(c, sh, sw));  // before the model runs
        if (c->loaded && npix) {
            if (!(d_loops && loops_rows) && !(d_vertices && vertex_rows) && !d_counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
            at = PolyScratch(edge_capacity(npix, max_edges));
            RETIF(ensure_private(c, c->st_cov_poly, at.bytes));
            base = (uint8_t*)c->st_cov_poly.p;
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Outlines, with that call's own checks, errors and MODEL_NOT_LOADED rule; the class
        // plane it outlined stays in st_outl_plane
        RETIF(infur_frame_outlines_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, base ? base + at.loops : nullptr,
                                       (uint32_t)at.loops_rows, base ? base + at.vertices : nullptr, (uint32_t)at.vertex_rows, base, d_stats,
                                       stats_capacity, d_scaled, ow, oh));
        return infur_coverage_dev(c, c->st_outl_plane.p, 1, *oh, *ow, flags & INFUR_OUTLINES_SKIP ? INFUR_COVERAGE_SKIP : 0, skip_value, base + at.loops,
                                  (uint32_t)at.loops_rows, base + at.vertices, (uint32_t)at.vertex_rows, base, tol16, 0, d_loops, loops_rows, d_vertices,
                                  vertex_rows, d_counts);
    });
}

int32_t infur_frame_coverage(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, uint32_t max_edges, uint32_t tol16, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices,
                             uint32_t vertex_rows, uint32_t* counts, uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        CovStage st(0, 0, 0, 0, 0, 0);
        uint8_t* base = nullptr;
        const bool any = (loops && loops_rows) || (vertices && vertex_rows) || counts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                // at most one loop per pixel; four vertices per pixel and the lattice's junctions
                const size_t most = npix * 4 + ((size_t)*ow + 1) * ((size_t)*oh + 1);
                const size_t lr = loops ? (loops_rows < npix ? loops_rows : npix) : 0, vr = vertices ? (vertex_rows < most ? vertex_rows : most) : 0;
                st = CovStage(lr, vr, stats ? (stats_capacity < (uint32_t)kSegMaxClasses ? stats_capacity : (uint32_t)kSegMaxClasses) : 0, 0, 0, 0);
                RETIF(ensure_private(c, c->st_cov_io, st.bytes));
                base = (uint8_t*)c->st_cov_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                return infur_frame_coverage_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, tol16, st.loops_rows ? base + st.loops : nullptr,
                                                (uint32_t)st.loops_rows, st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows,
                                                any ? base : nullptr, stats ? base + st.stats : nullptr, stats_capacity, d_scaled, ow, oh);
            },
            [&](size_t) -> int32_t {
                if (stats) HIPCHK(c, hipMemcpyAsync(stats, base + st.stats, (size_t)c->num_classes * INFUR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
                return coverage_read_back(c, base, st, loops, vertices, counts);
            });
    });
}

}  // extern "C"
