// infur_outlines.cpp -- Outlines, the polygon stage behind the four decodes (include/infur_hip.h): the boundaries of the regions
// of a byte or u32 plane as closed loops of lattice vertices, so that a host copies out polygons and not the dense plane.
// Kernels: outlines.hip.  Everything is enqueued on the context's stream.  Like infur_runs.cpp the frame path here always
// enqueues eagerly, and every buffer of this file is private scratch no captured graph of the library can point into: growing
// it leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include <cstring>
#include <new>

#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"

using namespace infur;

namespace {

static_assert(kLoopWords == INFUR_LOOP_WORDS, "outlines.hip and the header disagree about the record");

int32_t outlines_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_bytes %u: 1 or 4", elem_bytes);
    if (flags & ~(uint32_t)(INFUR_OUTLINES_SKIP | INFUR_OUTLINES_CONN8)) return fail(c, INFUR_E_INVALID_ARG, "unknown outlines flags 0x%x", flags);
    if (elem_bytes == 1 && skip_value > 255) return fail(c, INFUR_E_INVALID_ARG, "skip_value %u: a byte plane holds at most 255", skip_value);
    return INFUR_OK;
}

// an edge id is 4 * i + s in a u32, and 0xFFFFFFFF stands for none
int32_t outlines_plane_check(infur_ctx* c, uint32_t h, uint32_t w) {
    if ((size_t)h * w * 4 >= 0xFFFFFFFFull) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: an edge indexes at most 2^30 - 1 pixels", w, h);
    return INFUR_OK;
}

// the capacity in edges: 0 and anything above the worst case are the worst case
size_t edge_capacity(size_t hw, uint32_t max_edges) { return max_edges && max_edges < hw * 4 ? max_edges : hw * 4; }

// st_outl_io: [counts][statistics table k x 8 u64][loop records, at most one per pixel][vertices, at most four per pixel][plane],
// on 256-byte boundaries
struct OutlStage {
    size_t loops_rows, vertex_rows, stats, loops, vertices, plane, bytes;
    OutlStage(size_t npix, uint32_t loops_rows_, uint32_t vertex_rows_, uint32_t k, size_t plane_bytes) {
        loops_rows = loops_rows_ < npix ? loops_rows_ : npix;
        vertex_rows = vertex_rows_ < npix * 4 ? vertex_rows_ : npix * 4;
        stats = 256;
        loops = stats + align_up((size_t)k * INFUR_STAT_WORDS * 8, 256);
        vertices = loops + align_up(loops_rows * INFUR_LOOP_WORDS * 4, 256);
        plane = vertices + align_up(vertex_rows * 4, 256);
        bytes = plane + align_up(plane_bytes, 256);
    }
};

// the counts first: they decide how many records and vertices there are to copy
int32_t outlines_read_back(infur_ctx* c, const uint8_t* base, const OutlStage& st, uint32_t* loops, uint32_t* vertices, uint32_t* counts) {
    uint32_t n[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(n, base, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t nl = n[0] < st.loops_rows ? n[0] : st.loops_rows, nv = n[1] < st.vertex_rows ? n[1] : st.vertex_rows;
    if (loops && nl) HIPCHK(c, hipMemcpy(loops, base + st.loops, nl * INFUR_LOOP_WORDS * 4, hipMemcpyDeviceToHost));
    if (vertices && nv) HIPCHK(c, hipMemcpy(vertices, base + st.vertices, nv * 4, hipMemcpyDeviceToHost));
    if (counts) std::memcpy(counts, n, sizeof n);
    return INFUR_OK;
}

const char* const kNothingWanted = "no output wanted: loops (with rows), vertices (with rows) or counts";

}  // namespace

extern "C" {

int32_t infur_outlines_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                           uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, elem_bytes, flags, skip_value));
        RETIF(outlines_plane_check(c, h, w));
        const size_t hw = (size_t)h * w;
        if (!(d_loops && loops_rows) && !(d_vertices && vertex_rows) && !d_counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
        if (hw == 0) {  // empty plane: no edge
            if (d_counts) HIPCHK(c, hipMemsetAsync(d_counts, 0, 12, c->stream));
            return INFUR_OK;
        }
        if (!d_plane) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no plane pointer", w, h);
        const size_t cap = edge_capacity(hw, max_edges);
        RETIF(ensure_private(c, c->st_outl, outlines_scratch_bytes(hw, cap)));
        ProfScope ps(c, "outlines", "outlines", 0, (double)hw * elem_bytes * 4);
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
        if (!(loops && loops_rows) && !(vertices && vertex_rows) && !counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
        if (hw == 0) {
            if (counts) std::memset(counts, 0, 12);
            return INFUR_OK;
        }
        if (!plane) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no plane pointer", w, h);
        const OutlStage st(hw, loops ? loops_rows : 0, vertices ? vertex_rows : 0, 0, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_outl_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_outl_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_outlines_dev(c, base + st.plane, elem_bytes, h, w, flags, skip_value, max_edges, st.loops_rows ? base + st.loops : nullptr,
                                 (uint32_t)st.loops_rows, st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows, base));
        return outlines_read_back(c, base, st, loops, vertices, counts);
    });
}

int32_t infur_frame_outlines_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                 uint32_t skip_value, uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows,
                                 void* d_counts, void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, 1, flags, skip_value));
        const size_t npix = scale_npix(w, h, factor);
        void* kl = nullptr;
        if (c->loaded && npix) {
            if (!(d_loops && loops_rows) && !(d_vertices && vertex_rows) && !d_counts) return fail(c, INFUR_E_INVALID_ARG, "%s", kNothingWanted);
            RETIF(ensure_private(c, c->st_outl_plane, npix));  // the class plane is decoded into scratch
            kl = c->st_outl_plane.p;
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_segments_dev(c, d_bgr, w, h, factor, mode, decode, kl, nullptr, npix, d_stats, stats_capacity, nullptr, 0, d_scaled, ow, oh));
        return infur_outlines_dev(c, kl, 1, *oh, *ow, flags, skip_value, max_edges, d_loops, loops_rows, d_vertices, vertex_rows, d_counts);
    });
}

int32_t infur_frame_outlines(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, uint32_t max_edges, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows,
                             uint32_t* counts, uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(outlines_check(c, 1, flags, skip_value));
        OutlStage st(0, 0, 0, 0, 0);
        uint8_t* base = nullptr;
        const bool any = (loops && loops_rows) || (vertices && vertex_rows) || counts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                st = OutlStage(npix, loops ? loops_rows : 0, vertices ? vertex_rows : 0,
                               stats ? (stats_capacity < (uint32_t)kSegMaxClasses ? stats_capacity : (uint32_t)kSegMaxClasses) : 0, 0);
                RETIF(ensure_private(c, c->st_outl_io, st.bytes));
                base = (uint8_t*)c->st_outl_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                return infur_frame_outlines_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, max_edges, st.loops_rows ? base + st.loops : nullptr,
                                                (uint32_t)st.loops_rows, st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows,
                                                any ? base : nullptr, stats ? base + st.stats : nullptr, stats_capacity, d_scaled, ow, oh);
            },
            [&](size_t) -> int32_t {
                if (stats) HIPCHK(c, hipMemcpyAsync(stats, base + st.stats, (size_t)c->num_classes * INFUR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
                return outlines_read_back(c, base, st, loops, vertices, counts);
            });
    });
}

}  // extern "C"
