// infur_skeleton.cpp -- Skeleton, the stage behind Regions and Anchors that thins every value of a plane to one-pixel centrelines
// (include/infur_hip.h): Guo and Hall's two-sub-iteration rule on device bitmaps, then kind_out, a row per value and eight counts.
// Kernels: skeleton.hip.  Everything is enqueued on the context's stream; the element checks are the egress stages' (infur_egress.h),
// the frame calls' staging of Regions' and Anchors' products, their capacity checks and read-back the ones the stages behind Regions
// share (infur_region_frames.h), and so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and
// with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_region_frames.h"

using namespace infur;

namespace {

static_assert(kSkeletonWords == INFUR_SKELETON_WORDS && kSkeletonCountWords == INFUR_SKELETON_COUNT_WORDS && kSkeletonUnfinished == INFUR_SKELETON_UNFINISHED &&
                  kSkeletonMaxRounds == INFUR_SKELETON_MAX_ROUNDS && INFUR_SKELETON_PIXELS == 0 && INFUR_SKELETON_FIRST == 5 && INFUR_SKELETON_MAX_H == 7,
              "skeleton.hip and the header disagree");

constexpr uint32_t kSkeletonMaxSide = 65535;

// -> *rounds: the sub-iterations the call may run (max_rounds, or min(h, w) + 2 for 0)
int32_t skeleton_check(infur_ctx* c, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t max_rounds, const void* kind,
                       const void* table, uint32_t rows, const void* counts, uint32_t* rounds) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_SKELETON_SKIP, "skeleton", skip_value));
    if (h > kSkeletonMaxSide || w > kSkeletonMaxSide)
        return fail(c, INFUR_E_INVALID_ARG, "%ux%u: planes of width and height up to %u", w, h, kSkeletonMaxSide);
    if (max_rounds > INFUR_SKELETON_MAX_ROUNDS) return fail(c, INFUR_E_INVALID_ARG, "max_rounds %u: at most %u, or 0", max_rounds, (unsigned)INFUR_SKELETON_MAX_ROUNDS);
    if (!kind && !(table && rows) && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: kind_out, table (with rows) or counts");
    *rounds = max_rounds ? max_rounds : (h < w ? h : w) + 2;
    return INFUR_OK;
}

// st_skel_io of infur_skeleton: [counts][table][kind][height][plane], on 256-byte boundaries
struct SkeletonStage {
    size_t rows, table, kind, height, plane, bytes;
    SkeletonStage(size_t npix, size_t table_rows, bool want_kind, bool have_height, size_t plane_bytes) {
        rows = table_rows;
        table = 256;
        kind = table + align_up(rows * INFUR_SKELETON_WORDS * 4, 256);
        height = kind + align_up(want_kind ? npix : 0, 256);
        plane = height + align_up(have_height ? npix * 4 : 0, 256);
        bytes = plane + align_up(plane_bytes, 256) + 256;
    }
};

int32_t skeleton_read_back(infur_ctx* c, const uint8_t* base, const SkeletonStage& st, size_t npix, uint8_t* kind, uint32_t* table, uint32_t* counts) {
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_SKELETON_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if (kind && npix) HIPCHK(c, hipMemcpyAsync(kind, base + st.kind, npix, hipMemcpyDeviceToHost, c->stream));
    if (table && st.rows) HIPCHK(c, hipMemcpyAsync(table, base + st.table, st.rows * INFUR_SKELETON_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return INFUR_OK;
}

// st_skel_io of infur_frame_skeleton: Skeleton's own staging as above, then Regions' and Anchors' products from its height slot on
// (no height or plane travels: the slots behind kind are free)
struct SkeletonFrameStage {
    SkeletonStage sk;
    RegAnchLayout r;
    SkeletonFrameStage(size_t npix, const RegHostOut& o, size_t skel_rows, bool want_kind)
        : sk(npix, skel_rows, want_kind, false, 0), r(sk.height, npix, o.staged_rows(), o.anchor_rows()) {}
};

}  // namespace

extern "C" {

int32_t infur_skeleton_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, const void* d_height, uint32_t h, uint32_t w, uint32_t flags,
                           uint32_t skip_value, uint32_t max_rounds, void* d_kind_out, void* d_table, uint32_t rows, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t rounds = 0;
        RETIF(skeleton_check(c, elem_bytes, h, w, flags, skip_value, max_rounds, d_kind_out, d_table, rows, d_counts, &rounds));
        const size_t hw = (size_t)h * w;
        if (hw && !d_plane) return no_plane(c, h, w);
        if (hw) RETIF(ensure_private(c, c->st_skel, skeleton_scratch_bytes(h, w)));
        ProfScope ps(c, "skeleton", "skeleton", 0, (double)hw * (elem_bytes + (d_height ? 4.0 : 0.0) + (d_kind_out ? 1 : 0)));
        // (an empty plane: the empty rows, zero counts and nothing else)
        HIPCHK(c, launch_skeleton(d_plane, (int)elem_bytes, (const unsigned*)d_height, h, w, (flags & INFUR_SKELETON_SKIP) != 0, skip_value, rounds,
                                  c->st_skel.p, (uint8_t*)d_kind_out, rows ? (unsigned*)d_table : nullptr, rows, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_skeleton(infur_ctx* c, const void* plane, uint32_t elem_bytes, const uint32_t* height, uint32_t h, uint32_t w, uint32_t flags,
                       uint32_t skip_value, uint32_t max_rounds, uint8_t* kind_out, uint32_t* table, uint32_t rows, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t rounds = 0;
        RETIF(skeleton_check(c, elem_bytes, h, w, flags, skip_value, max_rounds, kind_out, table, rows, counts, &rounds));
        const size_t hw = (size_t)h * w;
        if (hw && !plane) return no_plane(c, h, w);
        const SkeletonStage st(hw, table ? rows : 0, kind_out != nullptr, height != nullptr, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_skel_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_skel_io.p;
        if (hw) HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        if (hw && height) HIPCHK(c, hipMemcpyAsync(base + st.height, height, hw * 4, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_skeleton_dev(c, hw ? base + st.plane : nullptr, elem_bytes, (hw && height) ? base + st.height : nullptr, h, w, flags, skip_value, max_rounds,
                                 kind_out ? base + st.kind : nullptr, st.rows ? base + st.table : nullptr, (uint32_t)st.rows, base));
        return skeleton_read_back(c, base, st, hw, kind_out, table, counts);
    });
}

int32_t infur_frame_skeleton_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                                 uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels, size_t labels_cap,
                                 void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh, void* d_dist2, size_t dist2_cap,
                                 void* d_anchors, uint32_t max_rounds, void* d_kind, size_t kind_cap, void* d_skel_table, uint32_t skel_rows,
                                 void* d_skel_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        const bool skel = d_kind || (d_skel_table && skel_rows) || d_skel_counts;
        void *lb = d_labels, *d2 = d_dist2;
        size_t lb_cap = labels_cap, d2_cap = dist2_cap;
        if (c->loaded && npix) {
            uint32_t rounds = 0;
            if (skel) RETIF(skeleton_check(c, 4, 1, 1, INFUR_SKELETON_SKIP, INFUR_REGION_NONE, max_rounds, d_kind, d_skel_table, skel_rows, d_skel_counts, &rounds));
            RETIF(cap_check(c, "kind", true, d_kind, kind_cap, npix));
            RETIF(cap_check(c, "label", true, d_labels, labels_cap, npix * 4));
            RETIF(cap_check(c, "distance", true, d_dist2, dist2_cap, npix * 4));
            if (skel) RETIF(borrow_planes(c, c->st_skel_plane, npix, &lb, &lb_cap, &d2, &d2_cap));  // the planes Skeleton reads
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions -> Anchors, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_anchors_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap, d_table,
                                      table_rows, d_n, d_scaled, ow, oh, d2, d2_cap, d_anchors));
        if (!skel) return INFUR_OK;
        return infur_skeleton_dev(c, lb, 4, d2, *oh, *ow, INFUR_SKELETON_SKIP, INFUR_REGION_NONE, max_rounds, d_kind, d_skel_table, skel_rows, d_skel_counts);
    });
}

int32_t infur_frame_skeleton(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                             uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels, size_t labels_cap,
                             uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh, uint32_t* dist2,
                             size_t dist2_cap, uint32_t* anchors, uint32_t max_rounds, uint8_t* kind, size_t kind_cap, uint32_t* skel_table, uint32_t skel_rows,
                             uint32_t* skel_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const RegHostOut o{klass, conf, plane_cap, labels, labels_cap, table, table_rows, n_regions, dist2, dist2_cap, anchors};
        SkeletonFrameStage st(0, o, 0, false);
        uint8_t* base = nullptr;
        const bool skel = kind || (skel_table && skel_rows) || skel_counts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(reg_caps_check(c, o, npix));
                RETIF(cap_check(c, "kind", c->loaded, kind, kind_cap, npix));
                st = SkeletonFrameStage(npix, o, skel_table ? skel_rows : 0, kind != nullptr);
                RETIF(ensure_private(c, c->st_skel_io, st.r.end));
                base = (uint8_t*)c->st_skel_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                const RegDevArgs a = reg_dev_args(o, base, st.r, npix, skel);
                return infur_frame_skeleton_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, a.klass, a.conf, a.plane_cap,
                                                a.labels, a.labels_cap, a.table, a.table_rows, a.n, d_scaled, ow, oh, a.dist2, a.dist2_cap, a.anchors,
                                                max_rounds, kind ? base + st.sk.kind : nullptr, npix, st.sk.rows ? base + st.sk.table : nullptr,
                                                (uint32_t)st.sk.rows, skel ? base : nullptr);
            },
            [&](size_t npix) -> int32_t {
                RETIF(reg_read_back(c, base, st.r, npix, o));
                if (!skel) return INFUR_OK;
                return skeleton_read_back(c, base, st.sk, npix, kind, skel_table, skel_counts);
            });
    });
}

}  // extern "C"
