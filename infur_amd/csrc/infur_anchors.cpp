// infur_anchors.cpp -- Anchors, the stage behind Regions and Tracks that measures how thick a region is (include/infur_hip.h): the
// exact squared distance transform of a byte or u32 plane by value, and per value its most interior pixel, so that a host places a
// caption on the object and not at a centroid beside it.  Kernels: anchors.hip.  Everything is enqueued on the context's stream;
// the element checks and the frame wrapper are the egress stages' (infur_egress.h, infur_rt.h), and so is the rule that its
// buffers are private scratch: growing them leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kAnchorWords == INFUR_ANCHOR_WORDS, "anchors.hip and the header disagree about the row");

constexpr uint32_t kAnchMaxSide = 65535;  // the row distance is a u16, a pixel index a u32

int32_t anchors_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value) {
    return elem_check(c, elem_bytes, flags, INFUR_ANCHORS_SKIP, "anchors", skip_value);
}
int32_t anchors_side_check(infur_ctx* c, uint32_t h, uint32_t w) {
    if (h > kAnchMaxSide || w > kAnchMaxSide) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a plane of width and height up to %u", w, h, kAnchMaxSide);
    return INFUR_OK;
}
int32_t anchors_wanted(infur_ctx* c, const void* dist2, const void* anchors, uint32_t rows) {
    if (dist2 || (anchors && rows)) return INFUR_OK;
    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: dist2 or anchors (with rows)");
}

// st_anch_io of infur_anchors: [anchors, rows x 2 words][dist2][plane], on 256-byte boundaries
struct AnchStage {
    size_t dist2, plane, bytes;
    AnchStage(size_t npix, size_t rows, size_t plane_bytes) {
        dist2 = align_up(rows * INFUR_ANCHOR_WORDS * 4, 256);
        plane = dist2 + align_up(npix * 4, 256);
        bytes = plane + align_up(plane_bytes, 256) + 256;
    }
};

// st_anch_io of infur_frame_anchors: [count][table, at most one row per pixel][label plane][class plane][confidence plane][dist2]
// [anchors, table_rows x 2 words], on 256-byte boundaries
struct AnchFrameStage {
    size_t rows, table, labels, klass, conf, dist2, anchors, bytes;
    AnchFrameStage(size_t npix, uint32_t table_rows, uint32_t anchor_rows) {
        rows = table_rows < npix ? table_rows : npix;
        table = 256;
        labels = table + align_up(rows * INFUR_REGION_WORDS * 8, 256);
        klass = labels + align_up(npix * 4, 256);
        conf = klass + align_up(npix, 256);
        dist2 = conf + align_up(npix, 256);
        anchors = dist2 + align_up(npix * 4, 256);
        bytes = anchors + align_up((size_t)anchor_rows * INFUR_ANCHOR_WORDS * 4, 256);
    }
};

}  // namespace

extern "C" {

int32_t infur_anchors_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                          void* d_dist2, void* d_anchors, uint32_t rows) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(anchors_check(c, elem_bytes, flags, skip_value));
        RETIF(anchors_side_check(c, h, w));
        const size_t hw = (size_t)h * w;
        RETIF(anchors_wanted(c, d_dist2, d_anchors, rows));
        if (hw && !d_plane) return no_plane(c, h, w);
        if (hw) RETIF(ensure_private(c, c->st_anch, anchors_scratch_bytes(hw, d_anchors ? rows : 0)));
        ProfScope ps(c, "anchors", "anchors", 0, (double)hw * (2.0 * elem_bytes + 4 + (d_dist2 ? 4 : 0)));
        // (an empty plane: the NONE rows and nothing else)
        HIPCHK(c, launch_anchors(d_plane, (int)elem_bytes, h, w, (flags & INFUR_ANCHORS_SKIP) != 0, skip_value, c->st_anch.p, (unsigned*)d_dist2,
                                 (unsigned*)d_anchors, rows, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_anchors(infur_ctx* c, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                      uint32_t* dist2, uint32_t* anchors, uint32_t rows) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(anchors_check(c, elem_bytes, flags, skip_value));
        RETIF(anchors_side_check(c, h, w));
        const size_t hw = (size_t)h * w;
        RETIF(anchors_wanted(c, dist2, anchors, rows));
        if (hw && !plane) return no_plane(c, h, w);
        if (!anchors) rows = 0;
        if (!hw && !rows) return INFUR_OK;  // an empty plane and no table: nothing to write
        const AnchStage st(dist2 ? hw : 0, rows, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_anch_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_anch_io.p;
        if (hw) HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_anchors_dev(c, hw ? base + st.plane : nullptr, elem_bytes, h, w, flags, skip_value, (dist2 && hw) ? base + st.dist2 : nullptr,
                                rows ? base : nullptr, rows));
        if (dist2 && hw) HIPCHK(c, hipMemcpyAsync(dist2, base + st.dist2, hw * 4, hipMemcpyDeviceToHost, c->stream));
        if (rows) HIPCHK(c, hipMemcpyAsync(anchors, base, (size_t)rows * INFUR_ANCHOR_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_anchors_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                                uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap,
                                void* d_labels, size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow,
                                uint32_t* oh, void* d_dist2, size_t dist2_cap, void* d_anchors) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        const bool anch = d_dist2 || (d_anchors && table_rows);
        void* lb = d_labels;
        size_t lb_cap = labels_cap;
        if (c->loaded && npix) {
            if (!d_labels && !d_table && !d_n && !anch) return INFUR_E_INVALID_ARG;
            if (d_labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
            if (d_dist2 && dist2_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the distance plane needs %zu bytes, buffer has %zu", npix * 4, dist2_cap);
            if (!lb && anch) {  // the label plane Anchors reads, when the caller does not want it
                RETIF(ensure_private(c, c->st_anch_plane, npix * 4));
                lb = c->st_anch_plane.p;
                lb_cap = npix * 4;
            }
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap,
                                      d_table, table_rows, d_n, d_scaled, ow, oh));
        if (!anch) return INFUR_OK;
        return infur_anchors_dev(c, lb, 4, *oh, *ow, INFUR_ANCHORS_SKIP, INFUR_REGION_NONE, d_dist2, d_anchors, table_rows);
    });
}

int32_t infur_frame_anchors(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                            uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap,
                            uint32_t* labels, size_t labels_cap, uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled,
                            uint32_t* ow, uint32_t* oh, uint32_t* dist2, size_t dist2_cap, uint32_t* anchors) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        AnchFrameStage st(0, 0, 0);
        uint8_t* base = nullptr;
        const uint32_t arows = anchors ? table_rows : 0;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
                if (c->loaded && dist2 && dist2_cap < npix * 4)
                    return fail(c, INFUR_E_CAPACITY, "the distance plane needs %zu bytes, buffer has %zu", npix * 4, dist2_cap);
                st = AnchFrameStage(npix, table ? table_rows : 0, arows);
                RETIF(ensure_private(c, c->st_anch_io, st.bytes));
                base = (uint8_t*)c->st_anch_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                // (table_rows reaches the device call as given when anchors are wanted: its rows are all written)
                return infur_frame_anchors_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, base + st.klass,
                                               (conf || table) ? base + st.conf : nullptr, npix, (labels || dist2 || arows) ? base + st.labels : nullptr,
                                               npix * 4, (table && st.rows) ? base + st.table : nullptr, arows ? table_rows : (uint32_t)st.rows,
                                               (labels || table || n_regions) ? base : nullptr, d_scaled, ow, oh, dist2 ? base + st.dist2 : nullptr,
                                               npix * 4, arows ? base + st.anchors : nullptr);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (dist2) HIPCHK(c, hipMemcpyAsync(dist2, base + st.dist2, npix * 4, hipMemcpyDeviceToHost, c->stream));
                if (arows) HIPCHK(c, hipMemcpyAsync(anchors, base + st.anchors, (size_t)arows * INFUR_ANCHOR_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                uint32_t n = 0;
                HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
                if (labels) HIPCHK(c, hipMemcpyAsync(labels, base + st.labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const size_t rows = n < st.rows ? n : st.rows;
                if (table && rows) HIPCHK(c, hipMemcpy(table, base + st.table, rows * INFUR_REGION_WORDS * 8, hipMemcpyDeviceToHost));
                if (n_regions) *n_regions = n;
                return INFUR_OK;
            });
    });
}

}  // extern "C"
