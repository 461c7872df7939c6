// infur_regions.cpp -- Regions, the third decode stage (include/infur_hip.h): the connected components of the class plane
// Segments writes, as a u32 label plane, a per-region table and a count, so that a headless host captions objects and not
// classes.  Kernels: regions.hip.  Everything is enqueued on the context's stream.  Like infur_segments.cpp the frame path
// here always enqueues eagerly, and every buffer of this file is private scratch no captured graph can point into: growing it
// leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include <cstring>
#include <new>

#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"

using namespace infur;

namespace {

static_assert(kRegWords == INFUR_REGION_WORDS, "regions.hip and the header disagree about the row");

// st_reg_io: [count][table, at most one row per pixel][label plane][class plane][confidence plane], on 256-byte boundaries
struct RegStage {
    size_t rows, table, labels, klass, conf, bytes;
    RegStage(size_t npix, uint32_t table_rows) {
        rows = table_rows < npix ? table_rows : npix;
        table = 256;
        labels = table + align_up(rows * INFUR_REGION_WORDS * 8, 256);
        klass = labels + align_up(npix * 4, 256);
        conf = klass + align_up(npix, 256);
        bytes = conf + align_up(npix, 256);
    }
};

// count and the written rows of the table to the host: the count decides how many rows there are to copy
int32_t reg_read_back(infur_ctx* c, const uint8_t* base, const RegStage& st, size_t npix, uint32_t* labels, uint64_t* table, uint32_t* n_regions) {
    uint32_t n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
    if (labels) HIPCHK(c, hipMemcpyAsync(labels, base + st.labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t rows = n < st.rows ? n : st.rows;
    if (table && rows) HIPCHK(c, hipMemcpy(table, base + st.table, rows * INFUR_REGION_WORDS * 8, hipMemcpyDeviceToHost));
    if (n_regions) *n_regions = n;
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_regions_dev(infur_ctx* c, const void* d_klass, const void* d_conf, uint32_t h, uint32_t w, uint32_t connectivity,
                          uint32_t min_pixels, uint32_t flags, void* d_labels, void* d_table, uint32_t table_rows, void* d_n) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        RETIF(plane_check(c, h, w, "a label plane"));
        const size_t hw = (size_t)h * w;
        if (!d_labels && !d_table && !d_n) return INFUR_E_INVALID_ARG;
        if (hw == 0) {  // empty image: no region, nothing else to write
            if (d_n) HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
            return INFUR_OK;
        }
        if (!d_klass) return INFUR_E_INVALID_ARG;
        RETIF(ensure_private(c, c->st_reg, regions_scratch_bytes(hw)));
        ProfScope ps(c, "regions", "regions", 0, (double)hw * (1 + (d_conf ? 1 : 0) + (d_labels ? 4 : 0)));
        HIPCHK(c, launch_regions((const uint8_t*)d_klass, (const uint8_t*)d_conf, h, w, connectivity == INFUR_CONNECT_8, min_pixels,
                                 (flags & INFUR_REGIONS_SKIP_BACKGROUND) != 0, c->st_reg.p, (unsigned*)d_labels, (unsigned long long*)d_table,
                                 table_rows, (unsigned*)d_n, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_regions(infur_ctx* c, const uint8_t* klass, const uint8_t* conf, uint32_t h, uint32_t w, uint32_t connectivity,
                      uint32_t min_pixels, uint32_t flags, uint32_t* labels, uint64_t* table, uint32_t table_rows, uint32_t* n_regions) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        RETIF(plane_check(c, h, w, "a label plane"));
        const size_t hw = (size_t)h * w;
        if (!labels && !table && !n_regions) return INFUR_E_INVALID_ARG;
        if (hw == 0) {
            if (n_regions) *n_regions = 0;
            return INFUR_OK;
        }
        if (!klass) return INFUR_E_INVALID_ARG;
        const RegStage st(hw, table ? table_rows : 0);
        RETIF(ensure_private(c, c->st_reg_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_reg_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.klass, klass, hw, hipMemcpyHostToDevice, c->stream));
        if (conf) HIPCHK(c, hipMemcpyAsync(base + st.conf, conf, hw, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_regions_dev(c, base + st.klass, conf ? base + st.conf : nullptr, h, w, connectivity, min_pixels, flags,
                                labels ? base + st.labels : nullptr, (table && st.rows) ? base + st.table : nullptr, (uint32_t)st.rows, base));
        return reg_read_back(c, base, st, hw, labels, table, n_regions);
    });
}

int32_t infur_frame_regions_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                                uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap,
                                void* d_labels, size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow,
                                uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const size_t npix = scale_npix(w, h, factor);
        void* kl = d_klass;
        void* cf = d_conf;
        if (c->loaded && npix) {
            if (!d_labels && !d_table && !d_n) return INFUR_E_INVALID_ARG;
            if (d_labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
            // the planes the caller does not want are decoded into scratch: the class plane always, the confidences for a table
            if (!kl || (!cf && d_table)) {
                RETIF(ensure_private(c, c->st_reg_planes, 2 * align_up(npix, 256)));
                if (!kl) kl = c->st_reg_planes.p;
                if (!cf && d_table) cf = (uint8_t*)c->st_reg_planes.p + align_up(npix, 256);
            }
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_segments_dev(c, d_bgr, w, h, factor, mode, decode, kl, cf, (d_klass || d_conf) ? plane_cap : npix, nullptr, 0, nullptr,
                                       0, d_scaled, ow, oh));
        return infur_regions_dev(c, kl, cf, *oh, *ow, connectivity, min_pixels, flags, d_labels, d_table, table_rows, d_n);
    });
}

int32_t infur_frame_regions(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                            uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap,
                            uint32_t* labels, size_t labels_cap, uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled,
                            uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        RegStage st(0, 0);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
                st = RegStage(npix, table ? table_rows : 0);
                RETIF(ensure_private(c, c->st_reg_io, st.bytes));
                base = (uint8_t*)c->st_reg_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, base + st.klass,
                                               (conf || table) ? base + st.conf : nullptr, npix, labels ? base + st.labels : nullptr, npix * 4,
                                               (table && st.rows) ? base + st.table : nullptr, (uint32_t)st.rows,
                                               (labels || table || n_regions) ? base : nullptr, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, npix, hipMemcpyDeviceToHost, c->stream));
                return reg_read_back(c, base, st, npix, labels, table, n_regions);
            });
    });
}

}  // extern "C"
