// infur_matte.cpp -- Matte and Composite (include/infur_hip.h): the soft, edge-aware alpha of the pixels a byte or u32 plane selects
// through a table of bytes, and the frame laid over a colour or a picture with it, or cut out.  Kernels: matte.hip.  Everything is
// enqueued on the context's stream; the frame calls sit on the shared front half (frame_host, infur_rt.h) and on
// infur_frame_segments_dev, whose checks and errors they inherit; the argument checks are infur_egress.h's, and so is the rule that
// its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kMatteCountWords == INFUR_MATTE_COUNT_WORDS && kMatteInvert == INFUR_MATTE_INVERT && kMatteConf == INFUR_MATTE_CONF &&
                  kMatteNothing == INFUR_MATTE_NOTHING && kMatteMaxRadius == INFUR_MATTE_MAX_RADIUS && kMatteMaxSide == INFUR_MATTE_MAX_SIDE &&
                  kCompositeColour == INFUR_COMPOSITE_COLOUR && kCompositeImage == INFUR_COMPOSITE_IMAGE && kCompositeCutout == INFUR_COMPOSITE_CUTOUT,
              "matte.hip and the header disagree");

// the checks that need neither a pointer nor the sides: element size, flag bits, radius, sigma
int32_t matte_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t radius, uint32_t sigma) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_MATTE_INVERT | INFUR_MATTE_CONF, "matte", 0));
    if (radius < 1 || radius > INFUR_MATTE_MAX_RADIUS) return fail(c, INFUR_E_INVALID_ARG, "radius %u: 1 to %d pixels", radius, INFUR_MATTE_MAX_RADIUS);
    if (sigma < 1 || sigma > 255) return fail(c, INFUR_E_INVALID_ARG, "sigma %u: 1 to 255", sigma);
    return INFUR_OK;
}
int32_t matte_select(infur_ctx* c, const void* select, uint32_t select_rows) {
    if (select_rows && !select) return fail(c, INFUR_E_INVALID_ARG, "%u selection rows and no select pointer", select_rows);
    return INFUR_OK;
}
int32_t matte_pointers(infur_ctx* c, const void* frame, const void* plane, const void* conf, uint32_t flags, const void* alpha, const void* counts,
                       uint32_t h, uint32_t w) {
    if (!alpha && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: alpha or counts");
    if (!plane) return no_plane(c, h, w);
    if (!frame) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u frame and no frame pointer", w, h);
    if ((flags & INFUR_MATTE_CONF) && !conf) return fail(c, INFUR_E_INVALID_ARG, "INFUR_MATTE_CONF and no conf pointer");
    return INFUR_OK;
}
int32_t composite_mode_check(infur_ctx* c, uint32_t mode) {
    if (mode > INFUR_COMPOSITE_CUTOUT) return fail(c, INFUR_E_INVALID_ARG, "unknown composite mode %u", mode);
    return INFUR_OK;
}
size_t composed_bytes(uint32_t mode, size_t npix) { return npix * (mode == INFUR_COMPOSITE_CUTOUT ? 4 : 3); }
int32_t composite_pointers(infur_ctx* c, const void* frame, const void* alpha, uint32_t mode, const void* back, const void* out, uint32_t h,
                           uint32_t w) {
    if (!frame) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u frame and no frame pointer", w, h);
    if (!alpha) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u frame and no alpha pointer", w, h);
    if (!out) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: out");
    if (mode == INFUR_COMPOSITE_IMAGE && !back) return fail(c, INFUR_E_INVALID_ARG, "INFUR_COMPOSITE_IMAGE and no back pointer");
    const size_t npix = (size_t)h * w, fbytes = npix * 3, obytes = composed_bytes(mode, npix);
    const uintptr_t f = (uintptr_t)frame, o = (uintptr_t)out;
    if ((mode == INFUR_COMPOSITE_CUTOUT || o != f) && o < f + fbytes && f < o + obytes)
        return fail(c, INFUR_E_INVALID_ARG, "out overlaps the frame: the frame itself (in place, not a cut-out) or apart from it");
    return INFUR_OK;
}

// st_matte_io of infur_matte: [counts][select][plane][conf][frame][alpha]; of infur_composite: frame, alpha, back and out in the
// same way; on 256-byte boundaries
struct Lay {
    size_t bytes = 256;  // (the counts)
    size_t add(size_t n) {
        const size_t at = bytes;
        bytes += align_up(n, 256);
        return at;
    }
};

// st_matte_plane of infur_frame_matte_dev: the planes the caller does not want: [class][confidence][alpha]
struct FramePlanes {
    size_t klass, conf, alpha, bytes;
    explicit FramePlanes(size_t npix) {
        klass = 0;
        conf = align_up(npix, 256);
        alpha = 2 * conf;
        bytes = 3 * conf;
    }
};

}  // namespace

extern "C" {

int32_t infur_matte_dev(infur_ctx* c, const void* d_frame, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, const void* d_select,
                        uint32_t select_rows, uint32_t flags, const void* d_conf, uint32_t radius, uint32_t sigma, void* d_alpha, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(matte_check(c, elem_bytes, flags, radius, sigma));
        RETIF(side_check(c, h, w, false, kMatteMaxSide));
        RETIF(matte_select(c, d_select, select_rows));
        RETIF(matte_pointers(c, d_frame, d_plane, d_conf, flags, d_alpha, d_counts, h, w));
        RETIF(ensure_private(c, c->st_matte, matte_scratch_bytes()));
        const size_t hw = (size_t)h * w;
        ProfScope ps(c, "matte", "matte", 0, (double)hw * (elem_bytes + 3.0 + ((flags & INFUR_MATTE_CONF) ? 1.0 : 0.0) + (d_alpha ? 1.0 : 0.0)));
        HIPCHK(c, launch_matte((const uint8_t*)d_frame, d_plane, (int)elem_bytes, h, w, (const uint8_t*)d_select, select_rows,
                               (flags & INFUR_MATTE_INVERT) != 0, (flags & INFUR_MATTE_CONF) ? (const uint8_t*)d_conf : nullptr, radius, sigma,
                               c->st_matte.p, (uint8_t*)d_alpha, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_matte(infur_ctx* c, const uint8_t* frame, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, const uint8_t* select,
                    uint32_t select_rows, uint32_t flags, const uint8_t* conf, uint32_t radius, uint32_t sigma, uint8_t* alpha, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(matte_check(c, elem_bytes, flags, radius, sigma));
        RETIF(side_check(c, h, w, false, kMatteMaxSide));
        RETIF(matte_select(c, select, select_rows));
        RETIF(matte_pointers(c, frame, plane, conf, flags, alpha, counts, h, w));
        const size_t hw = (size_t)h * w;
        const bool with_conf = (flags & INFUR_MATTE_CONF) != 0;
        Lay st;
        const size_t o_select = st.add(select_rows), o_plane = st.add(hw * elem_bytes), o_conf = st.add(with_conf ? hw : 0), o_frame = st.add(hw * 3),
                     o_alpha = st.add(hw);
        RETIF(ensure_private(c, c->st_matte_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_matte_io.p;
        if (select_rows) HIPCHK(c, hipMemcpyAsync(base + o_select, select, select_rows, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + o_plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        if (with_conf) HIPCHK(c, hipMemcpyAsync(base + o_conf, conf, hw, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + o_frame, frame, hw * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_matte_dev(c, base + o_frame, base + o_plane, elem_bytes, h, w, select_rows ? base + o_select : nullptr, select_rows, flags,
                              with_conf ? base + o_conf : nullptr, radius, sigma, alpha ? base + o_alpha : nullptr, counts ? base : nullptr));
        if (alpha) HIPCHK(c, hipMemcpyAsync(alpha, base + o_alpha, hw, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_MATTE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_composite_dev(infur_ctx* c, const void* d_frame, const void* d_alpha, uint32_t h, uint32_t w, uint32_t mode, const void* d_back,
                            uint32_t colour, void* d_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(composite_mode_check(c, mode));
        RETIF(side_check(c, h, w, false, kMatteMaxSide));
        RETIF(composite_pointers(c, d_frame, d_alpha, mode, d_back, d_out, h, w));
        const size_t hw = (size_t)h * w;
        ProfScope ps(c, "composite", "composite", 0, (double)hw * (4.0 + (mode == INFUR_COMPOSITE_IMAGE ? 3.0 : 0.0)) + (double)composed_bytes(mode, hw));
        HIPCHK(c, launch_composite((const uint8_t*)d_frame, (const uint8_t*)d_alpha, h, w, mode, (const uint8_t*)d_back, colour, (uint8_t*)d_out, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_composite(infur_ctx* c, const uint8_t* frame, const uint8_t* alpha, uint32_t h, uint32_t w, uint32_t mode, const uint8_t* back,
                        uint32_t colour, uint8_t* out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(composite_mode_check(c, mode));
        RETIF(side_check(c, h, w, false, kMatteMaxSide));
        RETIF(composite_pointers(c, frame, alpha, mode, back, out, h, w));
        const size_t hw = (size_t)h * w, obytes = composed_bytes(mode, hw);
        const bool image = mode == INFUR_COMPOSITE_IMAGE;
        Lay st;
        const size_t o_frame = st.add(hw * 3), o_alpha = st.add(hw), o_back = st.add(image ? hw * 3 : 0), o_out = st.add(obytes);
        RETIF(ensure_private(c, c->st_matte_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_matte_io.p;
        HIPCHK(c, hipMemcpyAsync(base + o_frame, frame, hw * 3, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + o_alpha, alpha, hw, hipMemcpyHostToDevice, c->stream));
        if (image) HIPCHK(c, hipMemcpyAsync(base + o_back, back, hw * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_composite_dev(c, base + o_frame, base + o_alpha, h, w, mode, image ? base + o_back : nullptr, colour, base + o_out));
        HIPCHK(c, hipMemcpyAsync(out, base + o_out, obytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_matte_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode, uint32_t decode,
                              const void* d_select, uint32_t select_rows, uint32_t flags, uint32_t radius, uint32_t sigma, uint32_t mode,
                              const void* d_back, uint32_t colour, void* d_alpha, void* d_composed, size_t composed_cap, void* d_klass, void* d_conf,
                              size_t plane_cap, void* d_counts, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(matte_check(c, 1, flags, radius, sigma));
        RETIF(composite_mode_check(c, mode));
        RETIF(matte_select(c, d_select, select_rows));
        if (d_composed && mode == INFUR_COMPOSITE_IMAGE && !d_back) return fail(c, INFUR_E_INVALID_ARG, "INFUR_COMPOSITE_IMAGE and no back pointer");
        uint32_t sw = 0, sh = 0;
        const size_t npix = scale_npix(w, h, factor);
        const bool with_conf = (flags & INFUR_MATTE_CONF) != 0, matting = d_alpha || d_composed || d_counts;
        void *kl = d_klass, *cf = d_conf, *al = d_alpha;
        if (c->loaded && npix && infur_scale_out_dims(w, h, factor, &sw, &sh) == INFUR_OK) {
            RETIF(side_check(c, sh, sw, false, kMatteMaxSide));
            if (!matting && !d_klass && !d_conf) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: alpha, composed, klass, conf or counts");
            if (d_composed && composed_cap < composed_bytes(mode, npix))
                return fail(c, INFUR_E_CAPACITY, "the composed frame needs %zu bytes, buffer has %zu", composed_bytes(mode, npix), composed_cap);
            if (d_alpha && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
            const FramePlanes at(npix);  // the planes Matte and Composite read and the caller does not want
            if (!kl || (with_conf && !cf) || (d_composed && !al)) {
                RETIF(ensure_private(c, c->st_matte_plane, at.bytes));
                uint8_t* base = (uint8_t*)c->st_matte_plane.p;
                if (!kl) kl = base + at.klass;
                if (with_conf && !cf) cf = base + at.conf;
                if (d_composed && !al) al = base + at.alpha;
            }
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_segments_dev(c, d_bgr, w, h, factor, scale_mode, decode, kl, cf, (d_klass || d_conf) ? plane_cap : npix, nullptr, 0, nullptr, 0,
                                       d_scaled, ow, oh));
        if (!matting) return INFUR_OK;
        const void* frame = d_scaled ? d_scaled : (factor != 1.0f ? c->st_scaled.p : d_bgr);  // where scale_forward left the scaled frame
        RETIF(infur_matte_dev(c, frame, kl, 1, *oh, *ow, d_select, select_rows, flags, cf, radius, sigma, al, d_counts));
        if (!d_composed) return INFUR_OK;
        return infur_composite_dev(c, frame, al, *oh, *ow, mode, d_back, colour, d_composed);
    });
}

int32_t infur_frame_matte(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode, uint32_t decode,
                          const uint8_t* select, uint32_t select_rows, uint32_t flags, uint32_t radius, uint32_t sigma, uint32_t mode,
                          const uint8_t* back, uint32_t colour, uint8_t* alpha, uint8_t* composed, size_t composed_cap, uint8_t* klass, uint8_t* conf,
                          size_t plane_cap, uint32_t* counts, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(matte_check(c, 1, flags, radius, sigma));
        RETIF(composite_mode_check(c, mode));
        RETIF(matte_select(c, select, select_rows));
        const bool image = composed && mode == INFUR_COMPOSITE_IMAGE;
        if (image && !back) return fail(c, INFUR_E_INVALID_ARG, "INFUR_COMPOSITE_IMAGE and no back pointer");
        size_t o_select = 0, o_klass = 0, o_conf = 0, o_alpha = 0, o_back = 0, o_composed = 0;
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf || alpha) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (c->loaded && composed && composed_cap < composed_bytes(mode, npix))
                    return fail(c, INFUR_E_CAPACITY, "the composed frame needs %zu bytes, buffer has %zu", composed_bytes(mode, npix), composed_cap);
                if (c->loaded && npix && !alpha && !composed && !counts && !klass && !conf)
                    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: alpha, composed, klass, conf or counts");
                Lay st;
                o_select = st.add(select_rows), o_klass = st.add(npix), o_conf = st.add(npix), o_alpha = st.add(npix);
                o_back = st.add(image ? npix * 3 : 0), o_composed = st.add(composed ? composed_bytes(mode, npix) : 0);
                RETIF(ensure_private(c, c->st_matte_io, st.bytes));
                base = (uint8_t*)c->st_matte_io.p;
                if (select_rows) HIPCHK(c, hipMemcpyAsync(base + o_select, select, select_rows, hipMemcpyHostToDevice, c->stream));
                if (image && npix) HIPCHK(c, hipMemcpyAsync(base + o_back, back, npix * 3, hipMemcpyHostToDevice, c->stream));
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_matte_dev(c, d_bgr, w, h, factor, scale_mode, decode, select_rows ? base + o_select : nullptr, select_rows, flags, radius,
                                             sigma, mode, image ? base + o_back : nullptr, colour, (alpha || composed) ? base + o_alpha : nullptr,
                                             composed ? base + o_composed : nullptr, composed_bytes(mode, npix), base + o_klass,
                                             (conf || (flags & INFUR_MATTE_CONF)) ? base + o_conf : nullptr, npix, counts ? base : nullptr, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (alpha) HIPCHK(c, hipMemcpyAsync(alpha, base + o_alpha, npix, hipMemcpyDeviceToHost, c->stream));
                if (composed) HIPCHK(c, hipMemcpyAsync(composed, base + o_composed, composed_bytes(mode, npix), hipMemcpyDeviceToHost, c->stream));
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + o_klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + o_conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_MATTE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                return INFUR_OK;
            });
    });
}

}  // extern "C"
