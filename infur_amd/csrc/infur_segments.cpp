// infur_segments.cpp -- the Segments decode: ColorCode's sibling for a headless host (include/infur_hip.h).  Where ColorCode turns
// the K class values of a pixel into one shaded RGBA colour (decode_predict.rs:53-79), this writes the segmentation result
// itself: the argmax class plane, a confidence plane (raw, or the softmax probability the reference's README.md:76 asks for),
// a per-class statistics table (what README.md:77's "class label captions" need) and, optionally, the RGBA overlay shaded by
// that confidence.  Kernels: prepost.hip.  Everything is enqueued on the context's stream; the frame path here always enqueues
// eagerly and never touches the graphs infur_frame_advance_dev has cached.
#include <cstring>
#include <new>

#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"

using namespace infur;

namespace {

// st_seg: [statistics table k x 8 u64][class plane][confidence plane], the planes on 16-byte boundaries
struct SegStage {
    size_t klass, conf, bytes;
    SegStage(uint32_t k, size_t npix) {
        klass = (size_t)k * INFUR_STAT_WORDS * 8;
        conf = klass + align_up(npix, 16);
        bytes = conf + align_up(npix, 16);
    }
};

int32_t seg_check(infur_ctx* c, uint32_t decode, uint32_t k) {
    if (decode > INFUR_DECODE_SOFTMAX) return fail(c, INFUR_E_INVALID_ARG, "unknown decode mode %u", decode);
    if (k > (uint32_t)kSegMaxClasses) return fail(c, INFUR_E_INVALID_ARG, "%u classes: the class byte holds at most %d", k, kSegMaxClasses);
    return INFUR_OK;
}

// zero the shards the kernel is about to accumulate into / fold them into the caller's table
int32_t seg_stats_begin(infur_ctx* c, int k) {
    HIPCHK(c, hipMemsetAsync(c->d_seg_shards, 0, (size_t)kSegShards * k * INFUR_STAT_WORDS * 8, c->stream));
    return INFUR_OK;
}

// the fused frame path with the Segments decode: Scale -> forward -> up-sample + argmax [+ softmax] + planes / statistics
int32_t frame_segments_body(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                            void* d_klass, void* d_conf, void* d_stats, void* d_rgba, void* d_scaled, uint32_t ow, uint32_t oh) {
    RoctxRange rr("infur frame segments");
    RETIF(scale_forward(c, d_bgr, w, h, factor, mode, d_scaled, ow, oh));
    const Tensor& t = c->out_low;  // only out[0] is decoded, app.rs:116
    SegOut o;
    o.klass = (uint8_t*)d_klass;
    o.conf = (uint8_t*)d_conf;
    o.rgba = (uint32_t*)d_rgba;
    o.shards = d_stats ? c->d_seg_shards : nullptr;
    const double out_bytes = (double)ow * oh * ((d_klass ? 1 : 0) + (d_conf ? 1 : 0) + (d_rgba ? 4 : 0));
    ProfScope ps(c, "out.resize+segments", "upsample_argmax_segments", 0, (double)t.bytes() + out_bytes);
    if (d_stats) RETIF(seg_stats_begin(c, t.c));
    HIPCHK(c, launch_upsample_argmax_segments((const float*)t.p, t.h, t.w, t.c, (int)decode, c->d_color_lut, o, (int)oh, (int)ow, c->stream,
                                              head_quant(c, 0)));
    if (d_stats) HIPCHK(c, launch_segments_stats_finalize(c->d_seg_shards, t.c, (unsigned long long*)d_stats, c->stream));
    return INFUR_OK;
}

const char* const kVocNames[21] = {"__background__", "aeroplane", "bicycle", "bird",  "boat",        "bottle", "bus",
                                   "car",            "cat",       "chair",   "cow",   "diningtable", "dog",    "horse",
                                   "motorbike",      "person",    "pottedplant", "sheep", "sofa",    "train",  "tvmonitor"};

}  // namespace

extern "C" {

uint32_t infur_features(void) { return INFUR_FEATURE_SEGMENTS | INFUR_FEATURE_REGIONS | INFUR_FEATURE_TRACKS | INFUR_FEATURE_RUNS | INFUR_FEATURE_OUTLINES |
           INFUR_FEATURE_SIMPLIFY | INFUR_FEATURE_COVERAGE | INFUR_FEATURE_TRACK_MEMORY | INFUR_FEATURE_ANCHORS | INFUR_FEATURE_COMPARE | INFUR_FEATURE_SIEVE | INFUR_FEATURE_SHAPES |
           INFUR_FEATURE_RASTER;
}

const char* infur_voc_class_name(uint32_t k) { return k < 21 ? kVocNames[k] : nullptr; }

int32_t infur_segments_dev(infur_ctx* c, const void* d_khw, uint32_t k, uint32_t h, uint32_t w, uint32_t decode, void* d_klass,
                           void* d_conf, void* d_stats, void* d_rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(seg_check(c, decode, k));
        if ((size_t)h * w == 0) return INFUR_OK;  // empty image: nothing to write, as infur_colorcode
        if ((!d_klass && !d_conf && !d_stats && !d_rgba) || (k > 0 && !d_khw)) return INFUR_E_INVALID_ARG;
        SegOut o;
        o.klass = (uint8_t*)d_klass;
        o.conf = (uint8_t*)d_conf;
        o.rgba = (uint32_t*)d_rgba;
        o.shards = (d_stats && k > 0) ? c->d_seg_shards : nullptr;  // k == 0: there is no table to write
        ProfScope ps(c, "segments", "segments_planar", 0, (double)h * w * (4.0 * k + (d_klass ? 1 : 0) + (d_conf ? 1 : 0) + (d_rgba ? 4 : 0)));
        if (o.shards) RETIF(seg_stats_begin(c, (int)k));
        HIPCHK(c, launch_segments_planar((const float*)d_khw, (int)k, (int)h, (int)w, (int)decode, c->d_color_lut, o, c->stream));
        if (o.shards) HIPCHK(c, launch_segments_stats_finalize(c->d_seg_shards, (int)k, (unsigned long long*)d_stats, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_segments(infur_ctx* c, const float* khw, uint32_t k, uint32_t h, uint32_t w, uint32_t decode, uint8_t* klass,
                       uint8_t* conf, uint64_t* stats, uint8_t* rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(seg_check(c, decode, k));
        const size_t hw = (size_t)h * w;
        if (hw == 0) return INFUR_OK;
        if ((!klass && !conf && !stats && !rgba) || (k > 0 && !khw)) return INFUR_E_INVALID_ARG;
        const SegStage st(k, hw);
        RETIF(ensure(c, c->st_f32a, hw * (k ? k : 1) * 4));
        if (rgba) RETIF(ensure(c, c->st_rgba, hw * 4));
        RETIF(ensure_private(c, c->st_seg, st.bytes));
        uint8_t* base = (uint8_t*)c->st_seg.p;
        if (k) HIPCHK(c, hipMemcpyAsync(c->st_f32a.p, khw, hw * k * 4, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_segments_dev(c, c->st_f32a.p, k, h, w, decode, klass ? base + st.klass : nullptr, conf ? base + st.conf : nullptr,
                                 stats ? base : nullptr, rgba ? c->st_rgba.p : nullptr));
        if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, hw, hipMemcpyDeviceToHost, c->stream));
        if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, hw, hipMemcpyDeviceToHost, c->stream));
        if (stats && k) HIPCHK(c, hipMemcpyAsync(stats, base, st.klass, hipMemcpyDeviceToHost, c->stream));
        if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->st_rgba.p, hw * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_segments_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                                 void* d_klass, void* d_conf, size_t plane_cap, void* d_stats, uint32_t stats_classes, void* d_rgba,
                                 size_t rgba_cap, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(seg_check(c, decode, 0));
        size_t npix;
        RETIF(frame_check(c, d_bgr, w, h, factor, mode, d_scaled, ow, oh, &npix));
        if (!d_klass && !d_conf && !d_stats && !d_rgba) return INFUR_E_INVALID_ARG;
        RETIF(seg_check(c, decode, (uint32_t)c->num_classes));
        if ((d_klass || d_conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
        if (d_rgba && rgba_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "mask needs %zu bytes, buffer has %zu", npix * 4, rgba_cap);
        if (d_stats && stats_classes < (uint32_t)c->num_classes)
            return fail(c, INFUR_E_CAPACITY, "the statistics table needs %d classes, buffer has %u", c->num_classes, stats_classes);
        return frame_segments_body(c, d_bgr, w, h, factor, mode, decode, d_klass, d_conf, d_stats, d_rgba, d_scaled, *ow, *oh);
    });
}

int32_t infur_frame_segments(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                             uint8_t* klass, uint8_t* conf, size_t plane_cap, uint64_t* stats, uint32_t stats_classes, uint8_t* rgba,
                             size_t rgba_cap, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(seg_check(c, decode, 0));
        SegStage st(0, 0);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (rgba && rgba_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "mask needs %zu bytes, buffer has %zu", npix * 4, rgba_cap);
                st = SegStage(staged_classes(stats, stats_classes), npix);
                if (rgba) RETIF(ensure(c, c->st_rgba, npix ? npix * 4 : 1));
                RETIF(ensure_private(c, c->st_seg, st.bytes ? st.bytes : 1));
                base = (uint8_t*)c->st_seg.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_segments_dev(c, d_bgr, w, h, factor, mode, decode, klass ? base + st.klass : nullptr, conf ? base + st.conf : nullptr,
                                                npix, stats ? base : nullptr, stats_classes, rgba ? c->st_rgba.p : nullptr, npix * 4, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (stats) HIPCHK(c, hipMemcpyAsync(stats, base, (size_t)c->num_classes * INFUR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
                if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->st_rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
                return INFUR_OK;
            });
    });
}

}  // extern "C"
