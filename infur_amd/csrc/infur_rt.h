// infur_rt.h -- internal interface between the host runtime's translation units (round 5: infur_capi.cpp was 2,900 lines):
//   infur_capi.cpp          context, arena, the float model (load, conv dispatch, forward), the C entry points of the stages
//   infur_quant_model.cpp   quantised models (INFURQ01): load + forward
//   infur_tuner.cpp         tile-configuration tuner (pick_cfg, tune_key, min_launch_ms) and its database (infur_tune_import / _export)
//   infur_stream.cpp        streaming ring, frame batch, pinned host buffers
//   infur_multi.cpp         groups of contexts, RCCL
//   infur_segments.cpp      the Segments decode (class / confidence planes, statistics): C entry points
//   infur_regions.cpp       Regions (connected components of the class plane, per-region table): C entry points
//   infur_tracks.cpp        Tracks (region identities from frame to frame): the tracker object and its C entry points
//   infur_runs.cpp          Runs (a class, label or track plane as run-length records): C entry points
//   infur_outlines.cpp      Outlines (region boundaries of a class, label or track plane as polygon loops): C entry points
//   infur_simplify.cpp      Simplify (Douglas-Peucker on Outlines' loops) and the polygon frame calls: C entry points
//   infur_coverage.cpp      Coverage (Outlines' loops simplified arc by arc, shared borders once) and its frame calls: C entry points
//   infur_anchors.cpp       Anchors (distance transform of a class, label or track plane, one interior point per value): C entry points
//   infur_compare.cpp       Compare (confusion matrix and best partner per value between two planes): C entry points
//   infur_shapes.cpp        Shapes (area, moments, convex hull and minimum rectangle per outline loop, sums per value): C entry points
//   infur_raster.cpp        Raster (polygon loops or run-length records filled back into a plane, with the pixels no loop or several claim): C entry points
//   infur_sieve.cpp         Adjacency (which values of a plane touch, along how many edges) and Sieve (speckle regions merged into their neighbours): C entry points
// (infur_egress.h, beside this header: what the last four share -- the argument checks with their messages, the read-back of a
//  polygon stage, the host-pointer frame wrapper and the front halves of the _dev frame calls)
// (egress_layout.h, HIP-free and included here: align_up, which moved there, the polygon stages' staging layout PolyStage, what
//  Outlines leaves behind it PolyScratch, edge_capacity, kMaxSide, the statistics-class clamp and the row rules of the copies)
// (conv_forms.h, the table of conv modes, configurations and forms, comes with kernels.h)
// (wave_scan.h, the device code regions.hip, tracks.hip and runs.hip share, also holds kScanBlock, which sizes their block sums)
// Everything here lives in namespace infur and is NOT part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "egress_layout.h"
#include "infur_ctx.h"
#include "kernels.h"

namespace infur {

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return ::infur::fail((c), INFUR_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                 __FILE__, __LINE__);                                           \
    } while (0)

#define RETIF(expr)                 \
    do {                            \
        int32_t rc__ = (expr);      \
        if (rc__ != INFUR_OK) return rc__; \
    } while (0)

// The exception boundary of the C ABI: every entry point that can reach an allocation (a std::string, a std::vector, `new`) runs
// its body through this, so that nothing unwinds into a C, Python or Rust caller.  Makes the context's device current first.
template <class F>
int32_t abi_call(infur_ctx* c, F&& body) {
    try {
        enter(c);
        return body();
    } catch (const std::bad_alloc&) {
        return fail(c, INFUR_E_CAPACITY, "out of host memory");
    } catch (const std::exception& e) {
        return fail(c, INFUR_E_INVALID_ARG, "internal error: %s", e.what());
    }
}

// ---- arena ----
int32_t ensure(infur_ctx* c, Buf& b, size_t bytes);
int32_t ensure_private(infur_ctx* c, Buf& b, size_t bytes);
int32_t pool_acquire(infur_ctx* c, size_t bytes, int* slot);
void pool_release(infur_ctx* c, Tensor& t);
void pool_release_all(infur_ctx* c);
void pool_free(infur_ctx* c);
void pool_trim(infur_ctx* c);
int32_t talloc(infur_ctx* c, int h, int w, int ch, int es, Tensor* t);
constexpr uint32_t kPoolTrimAfter = 4;

// ---- arithmetic mode of a context ----
inline bool ctx_f16(const infur_ctx* c) { return c->opt.compute_dtype == INFUR_DTYPE_F16; }
// GEMM arithmetic of launch_conv_igemm (ConvMode, conv_forms.h): a context's compute_dtype, except that INFUR_DTYPE_F32_SPLIT_FP8 is
// the split mode everywhere but inside the GEMM -- conv_mode() = kModeSplitFp8 selects its MFMA sequence, its weight rows and its own
// tuning entries -- and that a quantised model runs kModeI8 whatever the context's dtype
static_assert(kModeF32 == INFUR_DTYPE_F32 && kModeF16 == INFUR_DTYPE_F16 && kModeSplit == INFUR_DTYPE_F32_SPLIT &&
              kModeSplitFp8 == INFUR_DTYPE_F32_SPLIT_FP8 && kModeHL == INFUR_DTYPE_F16_HL, "ConvMode is the INFUR_DTYPE_* numbering");
inline bool ctx_fp8x(const infur_ctx* c) { return c->opt.compute_dtype == INFUR_DTYPE_F32_SPLIT_FP8; }
inline ConvMode ctx_mode(const infur_ctx* c) { return ctx_fp8x(c) ? kModeSplit : (ConvMode)c->opt.compute_dtype; }
inline ConvMode conv_mode(const infur_ctx* c) { return ctx_fp8x(c) ? kModeSplitFp8 : ctx_mode(c); }
// INFUR_DTYPE_F16_HL (= kModeHL): three-byte tensors (f16 hi + e5m2 lo planes), conv_hl.hip
inline bool ctx_hl(const infur_ctx* c) { return c->opt.compute_dtype == INFUR_DTYPE_F16_HL; }
inline int act_es(const infur_ctx* c) { return ctx_f16(c) ? 2 : (ctx_hl(c) ? 3 : 4); }
inline const float* stem_lut(const infur_ctx* c) { return c->input_u8 ? c->d_u8_lut : c->d_pre_lut; }
inline int conv_out(int n, int k, int s, int p, int d) { return (n + 2 * p - d * (k - 1) - 1) / s + 1; }

// ---- roctx ranges + per-kernel HIP events (infur_capi.cpp) ----
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
const Roctx* roctx();
struct RoctxRange {
    const Roctx* rx;
    explicit RoctxRange(const char* name) : rx(roctx()) {
        if (rx) rx->push(name);
    }
    ~RoctxRange() {
        if (rx) rx->pop();
    }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};
struct ProfScope {
    infur_ctx* c;
    bool on;
    const Roctx* rx;
    ProfRec r;
    ProfScope(infur_ctx* c_, const std::string& name, const char* kernel, double flops, double bytes, double algo_flops = -1.0);
    ~ProfScope();
};
void prof_reset(infur_ctx* c);

// ---- lookup tables (host side, exact reference operation order) ----
void build_pre_lut(float* lut);
void build_color_lut(uint32_t* lut);

// ---- the model ----
std::vector<ConvLayer> build_graph(int depth, int ncls, bool aux);
void model_free(infur_ctx* c);
UpQuant head_quant(const infur_ctx* c, int k);
// FCN-ResNet forward from a packed BGR frame on the device; leaves the output-stride-8 logits in c->out_low / c->aux_low
int32_t forward(infur_ctx* c, const uint8_t* d_bgr, int w, int h);
int32_t stem16_image(infur_ctx* c, const float* wt, float w_scale, int split, const void** img);
// measured tile configuration of the conv kernel for one problem shape (infur_tuner.cpp)
int32_t pick_cfg(infur_ctx* c, const ConvArgs& a, ConvMode mode, int out_f32, int* cfg);
// pick_cfg, then the launch inside its profile record (`layer`, the configuration's name)
int32_t run_tuned(infur_ctx* c, const std::string& layer, const ConvArgs& a, ConvMode mode, int out_f32, double flops, double bytes,
                  double algo_flops = -1.0);
// The 13 integers a decision is filed under in the tuning database.  [10]: what enters beside the input -- 0 nothing, 1 a residual,
// 2 a second source -- or kTunePairFlag: not a conv but the decision "conv3 -> next conv1 pair as one launch" (run_b2b; value 1 = fuse)
constexpr int kTunePairFlag = 3;
using TuneKey = std::array<int, 13>;
inline TuneKey tune_key(const ConvArgs& a, ConvMode mode, int out_f32) {
    return {a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.stride, a.dil, a.batch, a.res ? 1 : (a.in2 ? 2 : 0), mode, out_f32};
}
struct EventPair {  // two timing events, released on every return path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() {
        hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
// *ms = the minimum of n single-launch event timings of launch() on the context's stream, the first `discard` of them left out
template <class Launch>
int32_t min_launch_ms(infur_ctx* c, EventPair& ev, int discard, int n, float* ms, Launch&& launch) {
    *ms = 1e30f;
    for (int r = 0; r < n; r++) {
        HIPCHK(c, hipEventRecord(ev.e0, c->stream));
        HIPCHK(c, launch());
        HIPCHK(c, hipEventRecord(ev.e1, c->stream));
        HIPCHK(c, hipEventSynchronize(ev.e1));
        float t = 0;
        HIPCHK(c, hipEventElapsedTime(&t, ev.e0, ev.e1));
        if (r >= discard && t < *ms) *ms = t;
    }
    return INFUR_OK;
}
// ---- the front half of every fused frame call (infur_capi.cpp) ----
// infur_scale_validate + infur_scale_out_dims, with their messages: -> the scaled dimensions
int32_t scale_dims(infur_ctx* c, uint32_t w, uint32_t h, float factor, uint32_t* ow, uint32_t* oh);
// The same, silently, for the _dev frame calls of the stages behind Segments, which size their scratch before the call that
// reports the error: -> the scaled frame's pixels (*oh, optional: its rows); 0 when the factor or the dimensions are refused
inline size_t scale_npix(uint32_t w, uint32_t h, float factor, uint32_t* oh = nullptr) {
    uint32_t a = 0, b = 0;
    if (infur_scale_validate(factor) != INFUR_OK || infur_scale_out_dims(w, h, factor, &a, &b) != INFUR_OK) return 0;
    if (oh) *oh = b;
    return (size_t)a * b;
}
// What the _dev frame calls check before their own outputs: the scale mode, scale_dims, the frame, an empty frame -> E_SHAPE,
// and the no-model rule (the Scale stage still runs, then E_MODEL_NOT_LOADED).  -> *ow x *oh = *npix pixels
int32_t frame_check(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_scaled, uint32_t* ow,
                    uint32_t* oh, size_t* npix);
// Scale (into d_scaled or st_scaled, when there is anything to scale or the caller wants the frame) -> forward(), leaving the
// scale's profile records in front of the model's.  The caller holds the frame's RoctxRange, so that it spans the decode too.
int32_t scale_forward(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_scaled, uint32_t ow,
                      uint32_t oh);

// The host-pointer form of a fused frame call around its _dev sibling: dimensions, staging of the frame and the scaled frame,
// H2D, the device call, scaled frame back (also when no model is loaded), the outputs back on OK, synchronise.
//   stage(npix)        the call's own capacity checks and output staging
//   dev(d_bgr, d_sc)   the _dev sibling on the staged frame; d_sc is null when no scaled frame is needed
//   read_back(npix)    enqueues the copies of the call's outputs to the host
template <class Stage, class Dev, class ReadBack>
int32_t frame_host(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint8_t* scaled, uint32_t* ow, uint32_t* oh,
                   Stage&& stage, Dev&& dev, ReadBack&& read_back) {
    RETIF(scale_dims(c, w, h, factor, ow, oh));
    if (!bgr) return INFUR_E_INVALID_ARG;
    const size_t in_bytes = (size_t)w * h * 3, npix = (size_t)*ow * *oh, sbytes = npix * 3;
    RETIF(stage(npix));
    RETIF(ensure(c, c->st_in, in_bytes ? in_bytes : 1));
    RETIF(ensure(c, c->st_scaled, sbytes ? sbytes : 1));
    HIPCHK(c, hipMemcpyAsync(c->st_in.p, bgr, in_bytes, hipMemcpyHostToDevice, c->stream));
    const int32_t rc = dev(c->st_in.p, (scaled || factor != 1.0f) ? c->st_scaled.p : nullptr);
    if (rc != INFUR_OK && rc != INFUR_E_MODEL_NOT_LOADED) return rc;
    if (scaled) HIPCHK(c, hipMemcpyAsync(scaled, c->st_scaled.p, sbytes, hipMemcpyDeviceToHost, c->stream));
    if (rc == INFUR_OK) RETIF(read_back(npix));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return rc;
}

// ---- argument checks several stages share ----
// a plane of 32-bit pixel indices; noun: what indexes it ("a run", "a label plane")
inline int32_t plane_check(infur_ctx* c, uint32_t h, uint32_t w, const char* noun) {
    if ((size_t)h * w >= 0xFFFFFFFFull) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: %s indexes at most 2^32 - 2 pixels", w, h, noun);
    return INFUR_OK;
}
// Regions' connectivity and flags (infur_regions.cpp, and the fused calls of infur_tracks.cpp)
inline int32_t reg_check(infur_ctx* c, uint32_t connectivity, uint32_t flags) {
    if (connectivity != INFUR_CONNECT_4 && connectivity != INFUR_CONNECT_8)
        return fail(c, INFUR_E_INVALID_ARG, "connectivity %u: 4 or 8", connectivity);
    if (flags & ~(uint32_t)INFUR_REGIONS_SKIP_BACKGROUND) return fail(c, INFUR_E_INVALID_ARG, "unknown regions flags 0x%x", flags);
    return INFUR_OK;
}

// quantised models (infur_quant_model.cpp)
int32_t model_load_q_dev(infur_ctx* c, const void* d_blob, size_t len);
int32_t forward_q(infur_ctx* c, const uint8_t* d_bgr, int w, int h);

}  // namespace infur
