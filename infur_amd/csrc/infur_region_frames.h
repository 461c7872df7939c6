// infur_region_frames.h -- the host side the frame calls behind Regions share (Regions, Tracks, Anchors, Sieve, Shapes, Split,
// Skeleton, Centrelines, Expand, Appearance; internal, beside infur_egress.h): the capacity checks with their messages, the caller's arrays
// for Regions' and Anchors' products with the device arguments made of them and their read-back, and the planes a _dev form
// borrows when the caller does not want what the stage behind reads.  The offsets are region_layout.h's.  Every frame path here
// enqueues eagerly on the context's stream, and every buffer is private scratch no captured graph of the library can point into.
#pragma once
#include "infur_egress.h"
#include "region_layout.h"

namespace infur {

static_assert(kRegionRowBytes == INFUR_REGION_WORDS * 8 && kAnchorRowBytes == INFUR_ANCHOR_WORDS * 4, "region_layout.h and the public header disagree");

// ---- capacity checks, in the words the stages have always used ----
// The rule of `guard`: a host-pointer form checks Regions' own planes with or without a model (its staging comes before the device
// call that finds there is none) and passes c->loaded for the planes of the stages behind; a _dev form checks everything inside
// its `if (c->loaded && npix)` and passes true.
// `what`: "label", "distance", "grown", "source", "segment", "kind"
inline int32_t cap_check(infur_ctx* c, const char* what, bool guard, const void* p, size_t cap, size_t need) {
    if (guard && p && cap < need) return fail(c, INFUR_E_CAPACITY, "the %s plane needs %zu bytes, buffer has %zu", what, need, cap);
    return INFUR_OK;
}
// the byte planes that share plane_cap: class, confidence and, behind Sieve, the cleaned plane
inline int32_t byte_planes_check(infur_ctx* c, bool wanted, size_t plane_cap, size_t npix) {
    if (wanted && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
    return INFUR_OK;
}

// ---- the host-pointer form: the caller's arrays for Regions' products, and Anchors' where the call has them ----
struct RegHostOut {
    uint8_t *klass, *conf;
    size_t plane_cap;
    uint32_t* labels;
    size_t labels_cap;
    uint64_t* table;
    uint32_t table_rows;
    uint32_t* n_regions;
    uint32_t* dist2 = nullptr;
    size_t dist2_cap = 0;
    uint32_t* anchors = nullptr;
    uint32_t staged_rows() const { return table ? table_rows : 0; }   // the rows RegLayout is built for
    uint32_t anchor_rows() const { return anchors ? table_rows : 0; }  // every one of them is written
    bool regions() const { return labels || table || n_regions; }
};
// their capacities; `extra`: another byte plane that shares plane_cap
inline int32_t reg_caps_check(infur_ctx* c, const RegHostOut& o, size_t npix, bool extra = false) {
    RETIF(byte_planes_check(c, o.klass || o.conf || extra, o.plane_cap, npix));
    RETIF(cap_check(c, "label", true, o.labels, o.labels_cap, npix * 4));
    return cap_check(c, "distance", c->loaded, o.dist2, o.dist2_cap, npix * 4);
}
// their staging as the _dev sibling takes it: null where nobody wants a product
struct RegDevArgs {
    void *klass, *conf;
    size_t plane_cap;
    void* labels;
    size_t labels_cap;
    void* table;
    uint32_t table_rows;
    void* n;
    void* dist2;
    size_t dist2_cap;
    void* anchors;
};
//   behind     a stage behind Regions has work to do: it reads the label plane
//   all_rows   table_rows reaches the device call as given, not clamped to the pixels: a per-region output of the stage behind
//              (Anchors' rows, Shapes' values) has that many rows, and all are written
inline RegDevArgs reg_dev_args(const RegHostOut& o, uint8_t* base, const RegLayout& r, size_t npix, bool behind, bool all_rows = false) {
    return {base + r.klass,
            (o.conf || o.table) ? base + r.conf : nullptr,
            npix,
            (o.labels || behind) ? base + r.labels : nullptr,
            npix * 4,
            (o.table && r.rows) ? base + r.table : nullptr,
            all_rows ? o.table_rows : (uint32_t)r.rows,
            o.regions() ? base + r.n : nullptr,
            nullptr,
            npix * 4,
            nullptr};
}
// ... with Anchors behind Regions: `behind` now says that a stage behind Anchors reads the label plane and dist2
inline RegDevArgs reg_dev_args(const RegHostOut& o, uint8_t* base, const RegAnchLayout& r, size_t npix, bool behind) {
    const bool arows = o.anchor_rows() != 0;
    RegDevArgs a = reg_dev_args(o, base, (const RegLayout&)r, npix, o.dist2 || arows || behind, arows);
    a.dist2 = (o.dist2 || behind) ? base + r.dist2 : nullptr;
    a.anchors = arows ? base + r.anchors : nullptr;
    return a;
}
// The planes, then -- where anything of Regions' is wanted -- the count, which decides how many rows of the table there are to copy.
inline int32_t reg_read_back(infur_ctx* c, const uint8_t* base, const RegLayout& r, size_t npix, const RegHostOut& o) {
    if (o.klass) HIPCHK(c, hipMemcpyAsync(o.klass, base + r.klass, npix, hipMemcpyDeviceToHost, c->stream));
    if (o.conf) HIPCHK(c, hipMemcpyAsync(o.conf, base + r.conf, npix, hipMemcpyDeviceToHost, c->stream));
    if (!o.regions()) return INFUR_OK;
    uint32_t n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, base + r.n, 4, hipMemcpyDeviceToHost, c->stream));
    if (o.labels) HIPCHK(c, hipMemcpyAsync(o.labels, base + r.labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t rows = copy_rows(n, r.rows);
    if (o.table && rows) HIPCHK(c, hipMemcpy(o.table, base + r.table, rows * kRegionRowBytes, hipMemcpyDeviceToHost));
    if (o.n_regions) *o.n_regions = n;
    return INFUR_OK;
}
inline int32_t reg_read_back(infur_ctx* c, const uint8_t* base, const RegAnchLayout& r, size_t npix, const RegHostOut& o) {
    if (o.dist2) HIPCHK(c, hipMemcpyAsync(o.dist2, base + r.dist2, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (o.anchor_rows())
        HIPCHK(c, hipMemcpyAsync(o.anchors, base + r.anchors, (size_t)o.anchor_rows() * kAnchorRowBytes, hipMemcpyDeviceToHost, c->stream));
    return reg_read_back(c, base, (const RegLayout&)r, npix, o);
}

// ---- the _dev forms ----
// The planes the stage behind reads, when the caller does not want them: the label plane, and with `dist2` [labels][dist2], in
// the private scratch `b`.  Sets whichever pointer is null, and its capacity.
inline int32_t borrow_planes(infur_ctx* c, Buf& b, size_t npix, void** labels, size_t* labels_cap, void** dist2 = nullptr, size_t* dist2_cap = nullptr) {
    if (*labels && (!dist2 || *dist2)) return INFUR_OK;
    const size_t one = align_up(npix * 4, kSlotAlign);
    RETIF(ensure_private(c, b, dist2 ? 2 * one : npix * 4));
    if (!*labels) *labels = b.p, *labels_cap = npix * 4;
    if (dist2 && !*dist2) *dist2 = (uint8_t*)b.p + one, *dist2_cap = npix * 4;
    return INFUR_OK;
}

}  // namespace infur
