// infur_expand.cpp -- Expand, the stage that gives a value to the pixels that have none (include/infur_hip.h): every open pixel of a
// byte or u32 plane takes the value of its exact nearest seed, within a reach, with the squared distance, the seed's index, a row per
// value and eight counts.  Kernels: expand.hip.  Everything is enqueued on the context's stream; the frame calls' staging of Regions'
// products, their capacity checks and read-back are the ones the stages behind Regions share (infur_region_frames.h), and so is
// the rule that its buffers are private scratch: growing them leaves mem_gen -- and with it the
// graphs infur_frame_advance_dev has cached -- alone.
#include "infur_region_frames.h"

using namespace infur;

namespace {

static_assert(kExpandWords == INFUR_EXPAND_WORDS && kExpandCountWords == INFUR_EXPAND_COUNT_WORDS && kExpandNoSeed == INFUR_EXPAND_NO_SEED &&
                  kExpandMaxSide == INFUR_EXPAND_MAX_SIDE,
              "expand.hip and the header disagree");

// the checks that need no pointer, in Anchors' order: element size, flag bits, open_value against the element size, sides
int32_t expand_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t open_value, uint32_t h, uint32_t w) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_bytes %u: 1 or 4", elem_bytes);
    if (flags) return fail(c, INFUR_E_INVALID_ARG, "unknown expand flags 0x%x", flags);
    if (elem_bytes == 1 && open_value > 255) return fail(c, INFUR_E_INVALID_ARG, "open_value %u: a byte plane holds at most 255", open_value);
    if (h > kExpandMaxSide || w > kExpandMaxSide) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: a plane of width and height up to %u", w, h, kExpandMaxSide);
    return INFUR_OK;
}
int32_t expand_wanted(infur_ctx* c, const void* out, const void* dist2, const void* source, const void* table, uint32_t rows, const void* counts) {
    if (out || dist2 || source || (table && rows) || counts) return INFUR_OK;
    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: out, dist2, source, table (with rows) or counts");
}
int32_t expand_pointers(infur_ctx* c, const void* plane, const void* out, uint32_t h, uint32_t w) {
    if ((size_t)h * w && !plane) return no_plane(c, h, w);
    if ((size_t)h * w && out == plane) return fail(c, INFUR_E_INVALID_ARG, "out is the plane: Expand does not work in place");
    return INFUR_OK;
}

// st_exp_io of infur_expand: [counts][table, rows x 4 words][out][dist2][source][plane], on 256-byte boundaries
struct ExpStage {
    size_t table, out, dist2, source, plane, bytes;
    ExpStage(size_t rows, size_t out_bytes, size_t dist2_pix, size_t source_pix, size_t plane_bytes) {
        table = 256;
        out = table + align_up(rows * INFUR_EXPAND_WORDS * 4, 256);
        dist2 = out + align_up(out_bytes, 256);
        source = dist2 + align_up(dist2_pix * 4, 256);
        plane = source + align_up(source_pix * 4, 256);
        bytes = plane + align_up(plane_bytes, 256) + 256;
    }
};

// st_exp_io of infur_frame_expand: [counts], Regions' products, then [grown][dist2][source][expand table], on 256-byte boundaries
struct ExpFrameStage {
    size_t counts;
    RegLayout r;
    size_t grown, dist2, source, etable, bytes;
    ExpFrameStage(size_t npix, uint32_t table_rows, uint32_t expand_rows) : counts(0), r(256, npix, table_rows) {
        grown = r.end;
        dist2 = grown + align_up(npix * 4, 256);
        source = dist2 + align_up(npix * 4, 256);
        etable = source + align_up(npix * 4, 256);
        bytes = etable + align_up((size_t)expand_rows * INFUR_EXPAND_WORDS * 4, 256);
    }
};

}  // namespace

extern "C" {

int32_t infur_expand_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t open_value,
                         uint32_t reach, void* d_out, void* d_dist2, void* d_source, void* d_table, uint32_t rows, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(expand_check(c, elem_bytes, flags, open_value, h, w));
        RETIF(expand_wanted(c, d_out, d_dist2, d_source, d_table, rows, d_counts));
        RETIF(expand_pointers(c, d_plane, d_out, h, w));
        const size_t hw = (size_t)h * w;
        if (hw) RETIF(ensure_private(c, c->st_exp, expand_scratch_bytes(hw, d_table ? rows : 0)));
        ProfScope ps(c, "expand", "expand", 0, (double)hw * (2.0 * elem_bytes + 8 + (d_dist2 ? 4 : 0) + (d_source ? 4 : 0)));
        // (an empty plane: zero rows, zero counts and nothing else)
        HIPCHK(c, launch_expand(d_plane, (int)elem_bytes, h, w, open_value, reach, c->st_exp.p, d_out, (unsigned*)d_dist2, (unsigned*)d_source,
                                (unsigned*)d_table, rows, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_expand(infur_ctx* c, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t open_value, uint32_t reach,
                     void* out, uint32_t* dist2, uint32_t* source, uint32_t* table, uint32_t rows, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(expand_check(c, elem_bytes, flags, open_value, h, w));
        RETIF(expand_wanted(c, out, dist2, source, table, rows, counts));
        RETIF(expand_pointers(c, plane, out, h, w));
        const size_t hw = (size_t)h * w;
        if (!table) rows = 0;
        if (!hw && !rows && !counts) return INFUR_OK;  // an empty plane, no table and no counts: nothing to write
        const ExpStage st(rows, out ? hw * elem_bytes : 0, dist2 ? hw : 0, source ? hw : 0, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_exp_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_exp_io.p;
        if (hw) HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_expand_dev(c, hw ? base + st.plane : nullptr, elem_bytes, h, w, flags, open_value, reach, (out && hw) ? base + st.out : nullptr,
                               (dist2 && hw) ? base + st.dist2 : nullptr, (source && hw) ? base + st.source : nullptr, rows ? base + st.table : nullptr,
                               rows, counts ? base : nullptr));
        if (out && hw) HIPCHK(c, hipMemcpyAsync(out, base + st.out, hw * elem_bytes, hipMemcpyDeviceToHost, c->stream));
        if (dist2 && hw) HIPCHK(c, hipMemcpyAsync(dist2, base + st.dist2, hw * 4, hipMemcpyDeviceToHost, c->stream));
        if (source && hw) HIPCHK(c, hipMemcpyAsync(source, base + st.source, hw * 4, hipMemcpyDeviceToHost, c->stream));
        if (rows) HIPCHK(c, hipMemcpyAsync(table, base + st.table, (size_t)rows * INFUR_EXPAND_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_EXPAND_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_expand_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                               uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels,
                               size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh, uint32_t reach,
                               void* d_grown, size_t grown_cap, void* d_dist2, size_t dist2_cap, void* d_source, size_t source_cap, void* d_etable,
                               uint32_t expand_rows, void* d_ecounts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        const bool exp = d_grown || d_dist2 || d_source || (d_etable && expand_rows) || d_ecounts;
        void* lb = d_labels;
        size_t lb_cap = labels_cap;
        if (c->loaded && npix) {
            if (!d_labels && !d_table && !d_n && !exp) return INFUR_E_INVALID_ARG;
            RETIF(cap_check(c, "label", true, d_labels, labels_cap, npix * 4));
            RETIF(cap_check(c, "grown", true, d_grown, grown_cap, npix * 4));
            RETIF(cap_check(c, "distance", true, d_dist2, dist2_cap, npix * 4));
            RETIF(cap_check(c, "source", true, d_source, source_cap, npix * 4));
            if (exp) RETIF(borrow_planes(c, c->st_exp_plane, npix, &lb, &lb_cap));  // the label plane Expand reads
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap,
                                      d_table, table_rows, d_n, d_scaled, ow, oh));
        if (!exp) return INFUR_OK;
        return infur_expand_dev(c, lb, 4, *oh, *ow, 0, INFUR_REGION_NONE, reach, d_grown, d_dist2, d_source, d_etable, expand_rows, d_ecounts);
    });
}

int32_t infur_frame_expand(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                           uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels, size_t labels_cap,
                           uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh, uint32_t reach,
                           uint32_t* grown, size_t grown_cap, uint32_t* dist2, size_t dist2_cap, uint32_t* source, size_t source_cap, uint32_t* etable,
                           uint32_t expand_rows, uint32_t* ecounts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const RegHostOut o{klass, conf, plane_cap, labels, labels_cap, table, table_rows, n_regions};  // (dist2 here is Expand's own)
        ExpFrameStage st(0, 0, 0);
        uint8_t* base = nullptr;
        const uint32_t erows = etable ? expand_rows : 0;
        const bool exp = grown || dist2 || source || erows || ecounts;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(reg_caps_check(c, o, npix));
                RETIF(cap_check(c, "grown", c->loaded, grown, grown_cap, npix * 4));
                RETIF(cap_check(c, "distance", c->loaded, dist2, dist2_cap, npix * 4));
                RETIF(cap_check(c, "source", c->loaded, source, source_cap, npix * 4));
                st = ExpFrameStage(npix, o.staged_rows(), erows);
                RETIF(ensure_private(c, c->st_exp_io, st.bytes));
                base = (uint8_t*)c->st_exp_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                const RegDevArgs a = reg_dev_args(o, base, st.r, npix, exp);
                return infur_frame_expand_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, a.klass, a.conf, a.plane_cap, a.labels,
                                              a.labels_cap, a.table, a.table_rows, a.n, d_scaled, ow, oh, reach, grown ? base + st.grown : nullptr,
                                              npix * 4, dist2 ? base + st.dist2 : nullptr, npix * 4, source ? base + st.source : nullptr, npix * 4,
                                              erows ? base + st.etable : nullptr, erows, ecounts ? base + st.counts : nullptr);
            },
            [&](size_t npix) -> int32_t {
                if (grown) HIPCHK(c, hipMemcpyAsync(grown, base + st.grown, npix * 4, hipMemcpyDeviceToHost, c->stream));
                if (dist2) HIPCHK(c, hipMemcpyAsync(dist2, base + st.dist2, npix * 4, hipMemcpyDeviceToHost, c->stream));
                if (source) HIPCHK(c, hipMemcpyAsync(source, base + st.source, npix * 4, hipMemcpyDeviceToHost, c->stream));
                if (erows) HIPCHK(c, hipMemcpyAsync(etable, base + st.etable, (size_t)erows * INFUR_EXPAND_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                if (ecounts) HIPCHK(c, hipMemcpyAsync(ecounts, base + st.counts, INFUR_EXPAND_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                return reg_read_back(c, base, st.r, npix, o);
            });
    });
}

}  // extern "C"
