// infur_centrelines.cpp -- Centrelines, the stage behind Skeleton that traces the one-pixel centrelines into polyline branches
// (include/infur_hip.h): a record per branch and the vertex lists in Outlines' layout, and eight counts.  Kernels: centrelines.hip.
// Everything is enqueued on the context's stream; the element checks are the egress stages' (infur_egress.h), the host-pointer frame
// call's staging of Regions' and Anchors' products, their capacity checks and read-back the ones the stages behind Regions share
// (infur_region_frames.h), and so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs
// infur_frame_advance_dev has cached -- alone.
#include "infur_region_frames.h"

using namespace infur;

namespace {

static_assert(kCentrelineWords == INFUR_CENTRELINE_WORDS && kCentrelinesCountWords == INFUR_CENTRELINES_COUNT_WORDS &&
                  kCentrelinesOverflow == INFUR_CENTRELINES_OVERFLOW && INFUR_CENTRELINE_OFFSET == 0 && INFUR_CENTRELINE_MIN_H == 7 &&
                  INFUR_CENTRELINES_STATUS == 7,
              "centrelines.hip and the header disagree");

constexpr uint32_t kCentrelinesMaxSide = 65535;

int32_t centrelines_check(infur_ctx* c, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, const void* records, uint32_t rows,
                          const void* vertices, uint32_t vertex_rows, const void* counts) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_CENTRELINES_SKIP | INFUR_CENTRELINES_CORNERS, "centrelines", skip_value));
    if (h > kCentrelinesMaxSide || w > kCentrelinesMaxSide)
        return fail(c, INFUR_E_INVALID_ARG, "%ux%u: planes of width and height up to %u", w, h, kCentrelinesMaxSide);
    if ((size_t)h * w >= ((size_t)1 << 30)) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a dart indexes at most 2^30 - 1 pixels", w, h);
    if (!(records && rows) && !(vertices && vertex_rows) && !counts)
        return fail(c, INFUR_E_INVALID_ARG, "no output wanted: records (with rows), vertices (with rows) or counts");
    return INFUR_OK;
}

// the capacity in links: max_links, or the most a plane can hold for 0 (and never more than that)
size_t link_capacity(size_t npix, uint32_t max_links) { return max_links && max_links < 2 * npix ? max_links : 2 * npix; }

// st_cl_io of infur_centrelines: [counts][records][vertices][kind][height][plane], on 256-byte boundaries
struct CentrelinesStage {
    size_t rows, vertex_rows, records, vertices, kind, height, plane, bytes;
    CentrelinesStage(size_t npix, size_t record_rows, size_t vrows, bool have_kind, bool have_height, size_t plane_bytes) {
        rows = record_rows < 4 * npix + 1 ? record_rows : 4 * npix + 1;  // (no plane has more branches than darts and pixels)
        vertex_rows = vrows < 8 * npix + 1 ? vrows : 8 * npix + 1;
        records = 256;
        vertices = records + align_up(rows * INFUR_CENTRELINE_WORDS * 4, 256);
        kind = vertices + align_up(vertex_rows * 4, 256);
        height = kind + align_up(have_kind ? npix : 0, 256);
        plane = height + align_up(have_height ? npix * 4 : 0, 256);
        bytes = plane + align_up(plane_bytes, 256) + 256;
    }
};

// the counts first: they say how many records and vertices there are to copy
int32_t centrelines_read_back(infur_ctx* c, const uint8_t* base, const CentrelinesStage& st, uint32_t* records, uint32_t* vertices, uint32_t* counts) {
    uint32_t n[INFUR_CENTRELINES_COUNT_WORDS] = {};
    HIPCHK(c, hipMemcpyAsync(n, base, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t nr = n[INFUR_CENTRELINES_BRANCHES] < st.rows ? n[INFUR_CENTRELINES_BRANCHES] : st.rows;
    const size_t nv = n[INFUR_CENTRELINES_VERTICES] < st.vertex_rows ? n[INFUR_CENTRELINES_VERTICES] : st.vertex_rows;
    if (records && nr) HIPCHK(c, hipMemcpy(records, base + st.records, nr * INFUR_CENTRELINE_WORDS * 4, hipMemcpyDeviceToHost));
    if (vertices && nv) HIPCHK(c, hipMemcpy(vertices, base + st.vertices, nv * 4, hipMemcpyDeviceToHost));
    if (counts) std::memcpy(counts, n, sizeof n);
    return INFUR_OK;
}

// st_cl_io of infur_frame_centrelines: Centrelines' own staging as above, then Regions' and Anchors' products from its kind slot on
// (no kind, height or plane travels: the slots behind the vertices are free), then Skeleton's: [kind][skeleton table][skeleton counts]
struct CentrelinesFrameStage {
    CentrelinesStage cl;
    RegAnchLayout r;
    size_t srows, kind, stable, scounts, bytes;
    CentrelinesFrameStage(size_t npix, const RegHostOut& o, size_t skel_rows, size_t record_rows, size_t vrows)
        : cl(npix, record_rows, vrows, false, false, 0), r(cl.kind, npix, o.staged_rows(), o.anchor_rows()) {
        srows = skel_rows;
        kind = r.end;
        stable = kind + align_up(npix, 256);
        scounts = stable + align_up(srows * INFUR_SKELETON_WORDS * 4, 256);
        bytes = scounts + 256;
    }
};

}  // namespace

extern "C" {

int32_t infur_centrelines_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, const void* d_kind, const void* d_height, uint32_t h, uint32_t w,
                              uint32_t flags, uint32_t skip_value, uint32_t max_links, void* d_records, uint32_t rows, void* d_vertices, uint32_t vertex_rows,
                              void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(centrelines_check(c, elem_bytes, h, w, flags, skip_value, d_records, rows, d_vertices, vertex_rows, d_counts));
        const size_t hw = (size_t)h * w;
        if (hw && !d_plane) return no_plane(c, h, w);
        const size_t cap = link_capacity(hw, max_links);
        if (hw) RETIF(ensure_private(c, c->st_cl, centrelines_scratch_bytes(hw, cap)));
        ProfScope ps(c, "centrelines", "centrelines", 0, (double)hw * (elem_bytes + (d_kind ? 1.0 : 0.0) + 6.0));
        // (an empty plane: zero counts and nothing else)
        HIPCHK(c, launch_centrelines(d_plane, (int)elem_bytes, (const uint8_t*)d_kind, (const unsigned*)d_height, h, w, (flags & INFUR_CENTRELINES_SKIP) != 0,
                                     (flags & INFUR_CENTRELINES_CORNERS) != 0, skip_value, cap, c->st_cl.p, rows ? (unsigned*)d_records : nullptr, rows,
                                     vertex_rows ? (unsigned*)d_vertices : nullptr, vertex_rows, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_centrelines(infur_ctx* c, const void* plane, uint32_t elem_bytes, const uint8_t* kind, const uint32_t* height, uint32_t h, uint32_t w,
                          uint32_t flags, uint32_t skip_value, uint32_t max_links, uint32_t* records, uint32_t rows, uint32_t* vertices, uint32_t vertex_rows,
                          uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(centrelines_check(c, elem_bytes, h, w, flags, skip_value, records, rows, vertices, vertex_rows, counts));
        const size_t hw = (size_t)h * w;
        if (hw && !plane) return no_plane(c, h, w);
        const CentrelinesStage st(hw, records ? rows : 0, vertices ? vertex_rows : 0, kind != nullptr, height != nullptr, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_cl_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_cl_io.p;
        if (hw) HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        if (hw && kind) HIPCHK(c, hipMemcpyAsync(base + st.kind, kind, hw, hipMemcpyHostToDevice, c->stream));
        if (hw && height) HIPCHK(c, hipMemcpyAsync(base + st.height, height, hw * 4, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_centrelines_dev(c, hw ? base + st.plane : nullptr, elem_bytes, (hw && kind) ? base + st.kind : nullptr,
                                    (hw && height) ? base + st.height : nullptr, h, w, flags, skip_value, max_links, st.rows ? base + st.records : nullptr,
                                    (uint32_t)st.rows, st.vertex_rows ? base + st.vertices : nullptr, (uint32_t)st.vertex_rows, base));
        return centrelines_read_back(c, base, st, records, vertices, counts);
    });
}

int32_t infur_frame_centrelines_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                                    uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels,
                                    size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh, void* d_dist2,
                                    size_t dist2_cap, void* d_anchors, uint32_t max_rounds, void* d_kind, size_t kind_cap, void* d_skel_table, uint32_t skel_rows,
                                    void* d_skel_counts, uint32_t cl_flags, uint32_t max_links, void* d_records, uint32_t record_rows, void* d_vertices,
                                    uint32_t vertex_rows, void* d_cl_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        const size_t npix = scale_npix(w, h, factor);
        const bool cl = (d_records && record_rows) || (d_vertices && vertex_rows) || d_cl_counts;
        void *lb = d_labels, *d2 = d_dist2, *kd = d_kind;
        size_t lb_cap = labels_cap, d2_cap = dist2_cap, kd_cap = kind_cap;
        if (c->loaded && npix && cl) {
            RETIF(centrelines_check(c, 4, 1, 1, cl_flags | INFUR_CENTRELINES_SKIP, INFUR_REGION_NONE, d_records, record_rows, d_vertices, vertex_rows, d_cl_counts));
            if (cl_flags & INFUR_CENTRELINES_SKIP) return fail(c, INFUR_E_INVALID_ARG, "the frame call skips INFUR_REGION_NONE itself: CORNERS or 0");
            if (!lb || !d2 || !kd) {  // the planes Centrelines reads, when the caller does not want them: [labels][dist2][kind]
                const size_t one = align_up(npix * 4, 256);
                RETIF(ensure_private(c, c->st_cl_plane, 3 * one));
                if (!lb) lb = c->st_cl_plane.p, lb_cap = npix * 4;
                if (!d2) d2 = (uint8_t*)c->st_cl_plane.p + one, d2_cap = npix * 4;
                if (!kd) kd = (uint8_t*)c->st_cl_plane.p + 2 * one, kd_cap = npix;
            }
        }  // (otherwise the call below fails before it decodes, or runs without Centrelines)
        // scale -> model -> Segments decode -> Regions -> Anchors -> Skeleton, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_skeleton_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap, d_table,
                                       table_rows, d_n, d_scaled, ow, oh, d2, d2_cap, d_anchors, max_rounds, kd, kd_cap, d_skel_table, skel_rows,
                                       d_skel_counts));
        if (!cl) return INFUR_OK;
        return infur_centrelines_dev(c, lb, 4, kd, d2, *oh, *ow, cl_flags | INFUR_CENTRELINES_SKIP, INFUR_REGION_NONE, max_links, d_records, record_rows,
                                     d_vertices, vertex_rows, d_cl_counts);
    });
}

int32_t infur_frame_centrelines(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                                uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels, size_t labels_cap,
                                uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh, uint32_t* dist2,
                                size_t dist2_cap, uint32_t* anchors, uint32_t max_rounds, uint8_t* kind, size_t kind_cap, uint32_t* skel_table,
                                uint32_t skel_rows, uint32_t* skel_counts, uint32_t cl_flags, uint32_t max_links, uint32_t* records, uint32_t record_rows,
                                uint32_t* vertices, uint32_t vertex_rows, uint32_t* cl_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        const RegHostOut o{klass, conf, plane_cap, labels, labels_cap, table, table_rows, n_regions, dist2, dist2_cap, anchors};
        CentrelinesFrameStage st(0, o, 0, 0, 0);
        uint8_t* base = nullptr;
        const bool cl = (records && record_rows) || (vertices && vertex_rows) || cl_counts;
        const bool skel = kind || (skel_table && skel_rows) || skel_counts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(reg_caps_check(c, o, npix));
                RETIF(cap_check(c, "kind", c->loaded, kind, kind_cap, npix));
                st = CentrelinesFrameStage(npix, o, skel_table ? skel_rows : 0, records ? record_rows : 0, vertices ? vertex_rows : 0);
                RETIF(ensure_private(c, c->st_cl_io, st.bytes));
                base = (uint8_t*)c->st_cl_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                const RegDevArgs a = reg_dev_args(o, base, st.r, npix, skel || cl);
                return infur_frame_centrelines_dev(
                    c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, a.klass, a.conf, a.plane_cap, a.labels, a.labels_cap, a.table,
                    a.table_rows, a.n, d_scaled, ow, oh, a.dist2, a.dist2_cap, a.anchors, max_rounds, (kind || cl) ? base + st.kind : nullptr, npix, st.srows ? base + st.stable : nullptr, (uint32_t)st.srows,
                    skel_counts ? base + st.scounts : nullptr, cl_flags, max_links, st.cl.rows ? base + st.cl.records : nullptr, (uint32_t)st.cl.rows,
                    st.cl.vertex_rows ? base + st.cl.vertices : nullptr, (uint32_t)st.cl.vertex_rows, cl ? base : nullptr);
            },
            [&](size_t npix) -> int32_t {
                if (kind) HIPCHK(c, hipMemcpyAsync(kind, base + st.kind, npix, hipMemcpyDeviceToHost, c->stream));
                if (st.srows) HIPCHK(c, hipMemcpyAsync(skel_table, base + st.stable, st.srows * INFUR_SKELETON_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                if (skel_counts) HIPCHK(c, hipMemcpyAsync(skel_counts, base + st.scounts, INFUR_SKELETON_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                RETIF(reg_read_back(c, base, st.r, npix, o));
                if (!cl) return INFUR_OK;
                return centrelines_read_back(c, base, st.cl, records, vertices, cl_counts);
            });
    });
}

}  // extern "C"
