// infur_appearance.cpp -- Appearance, the stage that says what an object looks like (include/infur_hip.h): per value of a byte or u32
// plane the pixel count, the colour sums, the six second moments and the joint 64-bin histogram of the packed BGR frame, with eight
// counts.  Kernels: appearance.hip.  Everything is enqueued on the context's stream; the frame calls' staging of Regions' products,
// their capacity checks and read-back are the ones the stages behind Regions share (infur_region_frames.h), and so is the rule that
// its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_region_frames.h"

using namespace infur;

namespace {

static_assert(kAppearanceWords == INFUR_APPEARANCE_WORDS && kAppearanceBins == INFUR_APPEARANCE_BINS &&
                  kAppearanceCountWords == INFUR_APPEARANCE_COUNT_WORDS && kAppearanceNothing == INFUR_APPEARANCE_NOTHING &&
                  kAppearanceMaxSide == INFUR_APPEARANCE_MAX_SIDE,
              "appearance.hip and the header disagree");

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && p < q + b_bytes && q < p + a_bytes;
}

// in the siblings' order: element size, flags (and the skip value against the element size), sides, nothing wanted, a NULL plane or
// frame, an output that overlaps an input
int32_t appearance_check(infur_ctx* c, const void* frame, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                         uint32_t skip_value, const void* table, uint32_t rows, const void* hist, const void* counts) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_APPEARANCE_SKIP, "appearance", (flags & INFUR_APPEARANCE_SKIP) ? skip_value : 0));
    RETIF(side_check(c, h, w, false, kAppearanceMaxSide));
    if (!table && !hist && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: table, hist or counts");
    if (!plane) return no_plane(c, h, w);
    if (!frame) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u frame and no frame pointer", w, h);
    const size_t hw = (size_t)h * w;
    const void* out[3] = {table, hist, counts};
    const size_t bytes[3] = {(size_t)rows * INFUR_APPEARANCE_WORDS * 8, (size_t)rows * INFUR_APPEARANCE_BINS * 4, INFUR_APPEARANCE_COUNT_WORDS * 4};
    const char* name[3] = {"table", "hist", "counts"};
    for (int k = 0; k < 3; k++) {
        if (overlaps(out[k], bytes[k], frame, hw * 3)) return fail(c, INFUR_E_INVALID_ARG, "%s overlaps the frame", name[k]);
        if (overlaps(out[k], bytes[k], plane, hw * elem_bytes)) return fail(c, INFUR_E_INVALID_ARG, "%s overlaps the plane", name[k]);
    }
    return INFUR_OK;
}

// st_app_io of infur_appearance: [counts][table][hist][plane][frame], on 256-byte boundaries
struct AppStage {
    size_t table, hist, plane, frame, bytes;
    AppStage(size_t table_rows, size_t hist_rows, size_t plane_bytes, size_t frame_bytes) {
        table = 256;
        hist = table + align_up(table_rows * INFUR_APPEARANCE_WORDS * 8, 256);
        plane = hist + align_up(hist_rows * INFUR_APPEARANCE_BINS * 4, 256);
        frame = plane + align_up(plane_bytes, 256);
        bytes = frame + align_up(frame_bytes, 256);
    }
};

// st_app_io of infur_frame_appearance: [counts], Regions' products, then [appearance table][hist], on 256-byte boundaries
struct AppFrameStage {
    size_t counts;
    RegLayout r;
    size_t atable, ahist, bytes;
    AppFrameStage(size_t npix, uint32_t table_rows, size_t atable_rows, size_t ahist_rows) : counts(0), r(256, npix, table_rows) {
        atable = r.end;
        ahist = atable + align_up(atable_rows * INFUR_APPEARANCE_WORDS * 8, 256);
        bytes = ahist + align_up(ahist_rows * INFUR_APPEARANCE_BINS * 4, 256);
    }
};

}  // namespace

extern "C" {

int32_t infur_appearance_dev(infur_ctx* c, const void* d_frame, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                             uint32_t skip_value, void* d_table, uint32_t table_rows, void* d_hist, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(appearance_check(c, d_frame, d_plane, elem_bytes, h, w, flags, skip_value, d_table, table_rows, d_hist, d_counts));
        RETIF(ensure_private(c, c->st_app, appearance_scratch_bytes(table_rows, d_hist != nullptr)));
        const size_t hw = (size_t)h * w;
        ProfScope ps(c, "appearance", "appearance", 0, (double)hw * (3.0 + elem_bytes) + (double)table_rows * (d_table ? 96.0 + 512.0 : 512.0));
        HIPCHK(c, launch_appearance((const uint8_t*)d_frame, d_plane, (int)elem_bytes, h, w, (flags & INFUR_APPEARANCE_SKIP) != 0, skip_value, c->st_app.p,
                                    (unsigned long long*)d_table, table_rows, (unsigned*)d_hist, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_appearance(infur_ctx* c, const uint8_t* frame, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                         uint32_t skip_value, uint64_t* table, uint32_t table_rows, uint32_t* hist, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(appearance_check(c, frame, plane, elem_bytes, h, w, flags, skip_value, table, table_rows, hist, counts));
        const size_t hw = (size_t)h * w;
        const AppStage st(table ? table_rows : 0, hist ? table_rows : 0, hw * elem_bytes, hw * 3);
        RETIF(ensure_private(c, c->st_app_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_app_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.frame, frame, hw * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_appearance_dev(c, base + st.frame, base + st.plane, elem_bytes, h, w, flags, skip_value, table ? base + st.table : nullptr, table_rows,
                                   hist ? base + st.hist : nullptr, counts ? base : nullptr));
        if (table && table_rows)
            HIPCHK(c, hipMemcpyAsync(table, base + st.table, (size_t)table_rows * INFUR_APPEARANCE_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
        if (hist && table_rows)
            HIPCHK(c, hipMemcpyAsync(hist, base + st.hist, (size_t)table_rows * INFUR_APPEARANCE_BINS * 4, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_APPEARANCE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_appearance_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                                   uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap,
                                   void* d_labels, size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow,
                                   uint32_t* oh, void* d_atable, uint32_t appearance_rows, void* d_ahist, void* d_acounts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        const bool app = d_atable || d_ahist || d_acounts;
        void* lb = d_labels;
        size_t lb_cap = labels_cap;
        if (c->loaded && npix) {
            if (!d_labels && !d_table && !d_n && !app) return INFUR_E_INVALID_ARG;
            RETIF(cap_check(c, "label", true, d_labels, labels_cap, npix * 4));
            if (app) RETIF(borrow_planes(c, c->st_app_plane, npix, &lb, &lb_cap));  // the label plane Appearance reads
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap,
                                      d_table, table_rows, d_n, d_scaled, ow, oh));
        if (!app) return INFUR_OK;
        const void* frame = d_scaled ? d_scaled : (factor != 1.0f ? c->st_scaled.p : d_bgr);  // where scale_forward left the scaled frame
        return infur_appearance_dev(c, frame, lb, 4, *oh, *ow, INFUR_APPEARANCE_SKIP, INFUR_REGION_NONE, d_atable, appearance_rows, d_ahist, d_acounts);
    });
}

int32_t infur_frame_appearance(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                               uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap,
                               uint32_t* labels, size_t labels_cap, uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled,
                               uint32_t* ow, uint32_t* oh, uint64_t* atable, uint32_t appearance_rows, uint32_t* ahist, uint32_t* acounts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const RegHostOut o{klass, conf, plane_cap, labels, labels_cap, table, table_rows, n_regions};
        AppFrameStage st(0, 0, 0, 0);
        uint8_t* base = nullptr;
        const bool app = atable || ahist || acounts;
        const size_t trows = atable ? appearance_rows : 0, hrows = ahist ? appearance_rows : 0;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(reg_caps_check(c, o, npix));
                st = AppFrameStage(npix, o.staged_rows(), trows, hrows);
                RETIF(ensure_private(c, c->st_app_io, st.bytes));
                base = (uint8_t*)c->st_app_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const RegDevArgs a = reg_dev_args(o, base, st.r, (size_t)*ow * *oh, app);
                return infur_frame_appearance_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, a.klass, a.conf, a.plane_cap,
                                                  a.labels, a.labels_cap, a.table, a.table_rows, a.n, d_scaled, ow, oh,
                                                  atable ? base + st.atable : nullptr, appearance_rows, ahist ? base + st.ahist : nullptr,
                                                  acounts ? base + st.counts : nullptr);
            },
            [&](size_t npix) -> int32_t {
                if (trows) HIPCHK(c, hipMemcpyAsync(atable, base + st.atable, trows * INFUR_APPEARANCE_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
                if (hrows) HIPCHK(c, hipMemcpyAsync(ahist, base + st.ahist, hrows * INFUR_APPEARANCE_BINS * 4, hipMemcpyDeviceToHost, c->stream));
                if (acounts) HIPCHK(c, hipMemcpyAsync(acounts, base + st.counts, INFUR_APPEARANCE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                return reg_read_back(c, base, st.r, npix, o);
            });
    });
}

}  // extern "C"
