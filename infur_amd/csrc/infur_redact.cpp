// infur_redact.cpp -- Redact, the stage that writes the frame (include/infur_hip.h): the pixels a byte or u32 plane selects through a
// table of bytes are filled, pixelated or blurred in a packed BGR frame, out of place or in place, with eight counts.  Kernels:
// redact.hip.  Everything is enqueued on the context's stream; the frame calls sit on the shared front half (frame_host, infur_rt.h)
// and on infur_frame_segments_dev, whose checks and errors they inherit; the argument checks are infur_egress.h's, and so is the rule
// that its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached --
// alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kRedactCountWords == INFUR_REDACT_COUNT_WORDS && kRedactFill == INFUR_REDACT_FILL && kRedactPixelate == INFUR_REDACT_PIXELATE &&
                  kRedactBlur == INFUR_REDACT_BLUR && kRedactNothing == INFUR_REDACT_NOTHING && kRedactMaxSide == INFUR_REDACT_MAX_SIDE &&
                  kRedactMaxPixels == INFUR_REDACT_MAX_PIXELS,
              "redact.hip and the header disagree");

// the checks that need neither a pointer nor the sides: element size, flag bits, mode, then size and passes in the modes that use them
int32_t redact_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t mode, uint32_t size, uint32_t passes) {
    RETIF(elem_check(c, elem_bytes, flags, INFUR_REDACT_INVERT, "redact", 0));
    if (mode > INFUR_REDACT_BLUR) return fail(c, INFUR_E_INVALID_ARG, "unknown redact mode %u", mode);
    if (mode == INFUR_REDACT_PIXELATE && (size < 2 || size > 256)) return fail(c, INFUR_E_INVALID_ARG, "size %u: a cell of 2 to 256 pixels", size);
    if (mode == INFUR_REDACT_BLUR && (size < 1 || size > 255)) return fail(c, INFUR_E_INVALID_ARG, "size %u: a radius of 1 to 255 pixels", size);
    if (mode == INFUR_REDACT_BLUR && (passes < 1 || passes > 3)) return fail(c, INFUR_E_INVALID_ARG, "passes %u: 1 to 3", passes);
    return INFUR_OK;
}
// the sides, and the pixels of the averaging modes: every running sum of the table fits a u32
int32_t redact_sides(infur_ctx* c, uint32_t mode, uint32_t h, uint32_t w) {
    RETIF(side_check(c, h, w, false, kRedactMaxSide));
    if (mode != INFUR_REDACT_FILL && (size_t)h * w > kRedactMaxPixels)
        return fail(c, INFUR_E_INVALID_ARG, "%ux%u: pixelate and blur take at most 2^24 pixels", w, h);
    return INFUR_OK;
}
int32_t redact_select(infur_ctx* c, const void* select, uint32_t select_rows) {
    if (select_rows && !select) return fail(c, INFUR_E_INVALID_ARG, "%u selection rows and no select pointer", select_rows);
    return INFUR_OK;
}
int32_t redact_pointers(infur_ctx* c, const void* frame, const void* plane, const void* out, const void* counts, uint32_t h, uint32_t w) {
    if (!out && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: out or counts");
    if (!plane) return no_plane(c, h, w);
    if (!frame) return fail(c, INFUR_E_INVALID_ARG, "a %ux%u frame and no frame pointer", w, h);
    const size_t bytes = (size_t)h * w * 3;
    const uintptr_t f = (uintptr_t)frame, o = (uintptr_t)out;
    if (out && o != f && o < f + bytes && f < o + bytes) return fail(c, INFUR_E_INVALID_ARG, "out overlaps the frame: the frame itself (in place) or apart from it");
    return INFUR_OK;
}

// st_redact_io of infur_redact: [counts][select][plane][frame][out], on 256-byte boundaries; out is the frame for a call in place
struct RedStage {
    size_t select, plane, frame, out, bytes;
    RedStage(size_t select_rows, size_t plane_bytes, size_t frame_bytes, bool apart) {
        select = 256;
        plane = select + align_up(select_rows, 256);
        frame = plane + align_up(plane_bytes, 256);
        out = apart ? frame + align_up(frame_bytes, 256) : frame;
        bytes = out + align_up(frame_bytes, 256);
    }
};

// st_redact_io of infur_frame_redact: [counts][select][class plane][confidence plane][redacted], on 256-byte boundaries
struct RedFrameStage {
    size_t select, klass, conf, redacted, bytes;
    RedFrameStage(size_t select_rows, size_t npix) {
        select = 256;
        klass = select + align_up(select_rows, 256);
        conf = klass + align_up(npix, 256);
        redacted = conf + align_up(npix, 256);
        bytes = redacted + align_up(npix * 3, 256);
    }
};

int32_t redacted_cap_check(infur_ctx* c, const void* redacted, size_t cap, size_t npix) {
    if (c->loaded && redacted && cap < npix * 3) return fail(c, INFUR_E_CAPACITY, "the redacted frame needs %zu bytes, buffer has %zu", npix * 3, cap);
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_redact_dev(infur_ctx* c, const void* d_frame, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, const void* d_select,
                         uint32_t select_rows, uint32_t flags, uint32_t mode, uint32_t size, uint32_t passes, uint32_t colour, void* d_out,
                         void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(redact_check(c, elem_bytes, flags, mode, size, passes));
        RETIF(redact_sides(c, mode, h, w));
        RETIF(redact_select(c, d_select, select_rows));
        RETIF(redact_pointers(c, d_frame, d_plane, d_out, d_counts, h, w));
        const size_t hw = (size_t)h * w;
        const bool table = d_out && mode != INFUR_REDACT_FILL;
        RETIF(ensure_private(c, c->st_redact, redact_scratch_bytes(hw, table ? mode : kRedactFill)));
        const unsigned n = mode == INFUR_REDACT_BLUR ? passes : 1u;
        ProfScope ps(c, "redact", "redact", 0, (double)hw * (elem_bytes + (d_out ? 6.0 : 0.0) + (table ? n * (3.0 + 16.0 * 6) : 0.0)));
        HIPCHK(c, launch_redact((const uint8_t*)d_frame, d_plane, (int)elem_bytes, h, w, (const uint8_t*)d_select, select_rows,
                                (flags & INFUR_REDACT_INVERT) != 0, mode, size, passes, colour, c->st_redact.p, (uint8_t*)d_out, (unsigned*)d_counts,
                                c->stream));
        return INFUR_OK;
    });
}

int32_t infur_redact(infur_ctx* c, const uint8_t* frame, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, const uint8_t* select,
                     uint32_t select_rows, uint32_t flags, uint32_t mode, uint32_t size, uint32_t passes, uint32_t colour, uint8_t* out,
                     uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(redact_check(c, elem_bytes, flags, mode, size, passes));
        RETIF(redact_sides(c, mode, h, w));
        RETIF(redact_select(c, select, select_rows));
        RETIF(redact_pointers(c, frame, plane, out, counts, h, w));
        const size_t hw = (size_t)h * w;
        const RedStage st(select_rows, hw * elem_bytes, hw * 3, out && out != frame);
        RETIF(ensure_private(c, c->st_redact_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_redact_io.p;
        if (select_rows) HIPCHK(c, hipMemcpyAsync(base + st.select, select, select_rows, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + st.frame, frame, hw * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_redact_dev(c, base + st.frame, base + st.plane, elem_bytes, h, w, select_rows ? base + st.select : nullptr, select_rows, flags, mode,
                               size, passes, colour, out ? base + st.out : nullptr, counts ? base : nullptr));
        if (out) HIPCHK(c, hipMemcpyAsync(out, base + st.out, hw * 3, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_REDACT_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_redact_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode, uint32_t decode,
                               const void* d_select, uint32_t select_rows, uint32_t flags, uint32_t mode, uint32_t size, uint32_t passes,
                               uint32_t colour, void* d_redacted, size_t redacted_cap, void* d_klass, void* d_conf, size_t plane_cap, void* d_counts,
                               void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(redact_check(c, 1, flags, mode, size, passes));
        RETIF(redact_select(c, d_select, select_rows));
        uint32_t sw = 0, sh = 0;
        const size_t npix = scale_npix(w, h, factor);
        void* kl = d_klass;
        if (c->loaded && npix && infur_scale_out_dims(w, h, factor, &sw, &sh) == INFUR_OK) {
            RETIF(redact_sides(c, mode, sh, sw));
            if (!d_redacted && !d_counts && !d_klass && !d_conf) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: redacted, klass, conf or counts");
            RETIF(redacted_cap_check(c, d_redacted, redacted_cap, npix));
            if (!kl) {  // the class plane Redact reads
                RETIF(ensure_private(c, c->st_redact_plane, npix));
                kl = c->st_redact_plane.p;
            }
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_segments_dev(c, d_bgr, w, h, factor, scale_mode, decode, kl, d_conf, (d_klass || d_conf) ? plane_cap : npix, nullptr, 0, nullptr, 0,
                                       d_scaled, ow, oh));
        if (!d_redacted && !d_counts) return INFUR_OK;
        const void* frame = d_scaled ? d_scaled : (factor != 1.0f ? c->st_scaled.p : d_bgr);  // where scale_forward left the scaled frame
        return infur_redact_dev(c, frame, kl, 1, *oh, *ow, d_select, select_rows, flags, mode, size, passes, colour, d_redacted, d_counts);
    });
}

int32_t infur_frame_redact(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode, uint32_t decode,
                           const uint8_t* select, uint32_t select_rows, uint32_t flags, uint32_t mode, uint32_t size, uint32_t passes, uint32_t colour,
                           uint8_t* redacted, size_t redacted_cap, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* counts, uint8_t* scaled,
                           uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(redact_check(c, 1, flags, mode, size, passes));
        RETIF(redact_select(c, select, select_rows));
        RedFrameStage st(0, 0);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                RETIF(redacted_cap_check(c, redacted, redacted_cap, npix));
                if (c->loaded && npix && !redacted && !counts && !klass && !conf)
                    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: redacted, klass, conf or counts");
                st =RedFrameStage(select_rows, npix);
                RETIF(ensure_private(c, c->st_redact_io, st.bytes));
                base = (uint8_t*)c->st_redact_io.p;
                if (select_rows) HIPCHK(c, hipMemcpyAsync(base + st.select, select, select_rows, hipMemcpyHostToDevice, c->stream));
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_redact_dev(c, d_bgr, w, h, factor, scale_mode, decode, select_rows ? base + st.select : nullptr, select_rows, flags, mode,
                                              size, passes, colour, redacted ? base + st.redacted : nullptr, npix * 3, base + st.klass,
                                              conf ? base + st.conf : nullptr, npix, counts ? base : nullptr, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (redacted) HIPCHK(c, hipMemcpyAsync(redacted, base + st.redacted, npix * 3, hipMemcpyDeviceToHost, c->stream));
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_REDACT_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                return INFUR_OK;
            });
    });
}

}  // extern "C"
