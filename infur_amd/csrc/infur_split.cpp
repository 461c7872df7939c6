// infur_split.cpp -- Split, the stage behind Regions and Anchors that separates touching objects of one value at their necks
// (include/infur_hip.h): a marker watershed of a u32 height plane, typically Anchors' dist2, whose output is a label plane again.
// Kernels: split.hip.  Everything is enqueued on the context's stream; the element checks are the egress stages' (infur_egress.h),
// the frame calls' staging of Regions' and Anchors' products, their capacity checks and read-back the ones the stages behind Regions
// share (infur_region_frames.h), and so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and
// with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_region_frames.h"

using namespace infur;

namespace {

static_assert(kSplitWords == INFUR_SPLIT_WORDS && kSplitCountWords == INFUR_SPLIT_COUNT_WORDS && kSplitOverflow == INFUR_SPLIT_OVERFLOW,
              "split.hip and the header disagree");

constexpr uint32_t kSplitMaxSide = 65535;
constexpr uint64_t kSplitMaxPixels = 1ull << 31;  // an edge id is a u32
constexpr uint32_t kSplitDefaultSlots = 1u << 20;

int32_t split_check(infur_ctx* c, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t pair_slots, const void* labels,
                    const void* table, uint32_t rows, const void* counts, uint32_t* slots) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_SPLIT_SKIP, "split", skip_value));
    if (h > kSplitMaxSide || w > kSplitMaxSide || (uint64_t)h * w >= kSplitMaxPixels)
        return fail(c, INFUR_E_INVALID_ARG, "%ux%u: planes of width and height up to %u and fewer than 2^31 pixels", w, h, kSplitMaxSide);
    *slots = pair_slots ? pair_slots : kSplitDefaultSlots;
    if (*slots < 64 || (*slots & (*slots - 1))) return fail(c, INFUR_E_INVALID_ARG, "pair_slots %u: a power of two of at least 64, or 0", pair_slots);
    if (!labels && !(table && rows) && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: labels_out, table (with rows) or counts");
    return INFUR_OK;
}

// st_split_io of infur_split: [counts][table][labels][height][plane], on 256-byte boundaries
struct SplitStage {
    size_t rows, table, labels, height, plane, bytes;
    SplitStage(size_t npix, size_t table_rows, bool want_labels, size_t plane_bytes) {
        rows = table_rows < npix ? table_rows : npix;
        table = 256;
        labels = table + align_up(rows * INFUR_SPLIT_WORDS * 4, 256);
        height = labels + align_up(want_labels ? npix * 4 : 0, 256);
        plane = height + align_up(npix * 4, 256);
        bytes = plane + align_up(plane_bytes, 256) + 256;
    }
};

// the counts first: they say how many rows there are to copy
int32_t split_read_back(infur_ctx* c, const uint8_t* base, const SplitStage& st, size_t npix, uint32_t* labels, uint32_t* table, uint32_t* counts) {
    uint32_t n[INFUR_SPLIT_COUNT_WORDS] = {};
    HIPCHK(c, hipMemcpyAsync(n, base, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!(n[INFUR_SPLIT_STATUS] & INFUR_SPLIT_OVERFLOW)) {
        const size_t got = n[INFUR_SPLIT_SEGMENTS] < st.rows ? n[INFUR_SPLIT_SEGMENTS] : st.rows;
        if (labels && npix) HIPCHK(c, hipMemcpy(labels, base + st.labels, npix * 4, hipMemcpyDeviceToHost));
        if (table && got) HIPCHK(c, hipMemcpy(table, base + st.table, got * INFUR_SPLIT_WORDS * 4, hipMemcpyDeviceToHost));
    }
    if (counts) std::memcpy(counts, n, sizeof n);
    return INFUR_OK;
}

// st_split_io of infur_frame_split: Split's own staging as above, then Regions' and Anchors' products from its height slot on
// (no height or plane travels: the slots behind Split's labels are free)
struct SplitFrameStage {
    SplitStage sp;
    RegAnchLayout r;
    SplitFrameStage(size_t npix, const RegHostOut& o, size_t split_rows, bool want_labels)
        : sp(npix, split_rows, want_labels, 0), r(sp.height, npix, o.staged_rows(), o.anchor_rows()) {}
};

}  // namespace

extern "C" {

int32_t infur_split_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, const void* d_height, uint32_t h, uint32_t w, uint32_t flags,
                        uint32_t skip_value, uint32_t core, uint32_t pair_slots, void* d_labels_out, void* d_table, uint32_t rows, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        RETIF(split_check(c, elem_bytes, h, w, flags, skip_value, pair_slots, d_labels_out, d_table, rows, d_counts, &slots));
        const size_t hw = (size_t)h * w;
        if (hw && !d_plane) return no_plane(c, h, w);
        if (hw && !d_height) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no height plane", w, h);
        if (hw) RETIF(ensure_private(c, c->st_split, split_scratch_bytes(hw, slots, (int)elem_bytes)));
        ProfScope ps(c, "split", "split", 0, (double)hw * (elem_bytes + 4.0 + (d_labels_out ? 4 : 0)));
        // (an empty plane: zero counts and nothing else)
        HIPCHK(c, launch_split(d_plane, (int)elem_bytes, (const unsigned*)d_height, h, w, (flags & INFUR_SPLIT_SKIP) != 0, skip_value, core, c->st_split.p,
                               slots, (unsigned*)d_labels_out, rows ? (unsigned*)d_table : nullptr, rows, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_split(infur_ctx* c, const void* plane, uint32_t elem_bytes, const uint32_t* height, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                    uint32_t core, uint32_t pair_slots, uint32_t* labels_out, uint32_t* table, uint32_t rows, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        RETIF(split_check(c, elem_bytes, h, w, flags, skip_value, pair_slots, labels_out, table, rows, counts, &slots));
        const size_t hw = (size_t)h * w;
        if (hw && !plane) return no_plane(c, h, w);
        if (hw && !height) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no height plane", w, h);
        if (!hw) {  // no pixel, no segment
            if (counts) std::memset(counts, 0, INFUR_SPLIT_COUNT_WORDS * 4);
            return INFUR_OK;
        }
        const SplitStage st(hw, table ? rows : 0, labels_out != nullptr, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_split_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_split_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.height, height, hw * 4, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_split_dev(c, base + st.plane, elem_bytes, base + st.height, h, w, flags, skip_value, core, pair_slots,
                              labels_out ? base + st.labels : nullptr, st.rows ? base + st.table : nullptr, (uint32_t)st.rows, base));
        return split_read_back(c, base, st, hw, labels_out, table, counts);
    });
}

int32_t infur_frame_split_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                              uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels, size_t labels_cap,
                              void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh, void* d_dist2, size_t dist2_cap,
                              void* d_anchors, uint32_t core, uint32_t pair_slots, void* d_split_labels, size_t split_labels_cap, void* d_split_table,
                              uint32_t split_rows, void* d_split_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        const bool split = d_split_labels || (d_split_table && split_rows) || d_split_counts;
        void *lb = d_labels, *d2 = d_dist2;
        size_t lb_cap = labels_cap, d2_cap = dist2_cap;
        if (c->loaded && npix) {
            uint32_t slots = 0;
            if (split)
                RETIF(split_check(c, 4, 1, 1, INFUR_SPLIT_SKIP, INFUR_REGION_NONE, pair_slots, d_split_labels, d_split_table, split_rows, d_split_counts,
                                  &slots));
            RETIF(cap_check(c, "segment", true, d_split_labels, split_labels_cap, npix * 4));
            RETIF(cap_check(c, "label", true, d_labels, labels_cap, npix * 4));
            RETIF(cap_check(c, "distance", true, d_dist2, dist2_cap, npix * 4));
            if (split) RETIF(borrow_planes(c, c->st_split_plane, npix, &lb, &lb_cap, &d2, &d2_cap));  // the planes Split reads
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions -> Anchors, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_anchors_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap, d_table,
                                      table_rows, d_n, d_scaled, ow, oh, d2, d2_cap, d_anchors));
        if (!split) return INFUR_OK;
        return infur_split_dev(c, lb, 4, d2, *oh, *ow, INFUR_SPLIT_SKIP, INFUR_REGION_NONE, core, pair_slots, d_split_labels, d_split_table, split_rows,
                               d_split_counts);
    });
}

int32_t infur_frame_split(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                          uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels, size_t labels_cap,
                          uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh, uint32_t* dist2,
                          size_t dist2_cap, uint32_t* anchors, uint32_t core, uint32_t pair_slots, uint32_t* split_labels, size_t split_labels_cap,
                          uint32_t* split_table, uint32_t split_rows, uint32_t* split_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const RegHostOut o{klass, conf, plane_cap, labels, labels_cap, table, table_rows, n_regions, dist2, dist2_cap, anchors};
        SplitFrameStage st(0, o, 0, false);
        uint8_t* base = nullptr;
        const bool split = split_labels || (split_table && split_rows) || split_counts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(reg_caps_check(c, o, npix));
                RETIF(cap_check(c, "segment", c->loaded, split_labels, split_labels_cap, npix * 4));
                st = SplitFrameStage(npix, o, split_table ? split_rows : 0, split_labels != nullptr);
                RETIF(ensure_private(c, c->st_split_io, st.r.end));
                base = (uint8_t*)c->st_split_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                const RegDevArgs a = reg_dev_args(o, base, st.r, npix, split);
                return infur_frame_split_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, a.klass, a.conf, a.plane_cap, a.labels,
                                             a.labels_cap, a.table, a.table_rows, a.n, d_scaled, ow, oh, a.dist2, a.dist2_cap, a.anchors, core, pair_slots,
                                             split_labels ? base + st.sp.labels : nullptr, npix * 4, st.sp.rows ? base + st.sp.table : nullptr,
                                             (uint32_t)st.sp.rows, split ? base : nullptr);
            },
            [&](size_t npix) -> int32_t {
                RETIF(reg_read_back(c, base, st.r, npix, o));
                if (!split) return INFUR_OK;
                return split_read_back(c, base, st.sp, npix, split_labels, split_table, split_counts);
            });
    });
}

}  // extern "C"
