// infur_capi.cpp -- host runtime behind the C ABI in include/infur_hip.h.
//
// One infur_ctx = one GPU, one HIP stream, a pooled activation arena, the resident weights
// of one FCN-ResNet and the small lookup tables of the pre/post stages.  Everything is
// enqueued on the context's stream; the host-pointer entry points copy in, run, copy out
// and synchronise.  There is deliberately no CPU fallback anywhere in this file.
//
// Reference behaviour mirrored here (path:line in ahirner/infur):
//   Scale       infur/src/processing.rs:142-282
//   Model       infur/src/predict_onnx.rs:97-142, 283-345
//   ColorCode   infur/src/decode_predict.rs:9-79
//   stage order infur/src/app.rs:107-153
#include "../../include/infur_hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <array>
#include <atomic>
#include <climits>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "blob_dir.h"
#include "hl_format.h"
#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"
#include "onnx_reader.h"

using namespace infur;

namespace infur {

int32_t fail(infur_ctx* c, int32_t code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

int32_t ensure(infur_ctx* c, Buf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return INFUR_OK;
    c->mem_gen++;
    return ensure_private(c, b, bytes);
}

// Staging only the host-pointer calls of Segments and Regions use: no captured graph can hold a pointer into it (the graphs of
// infur_frame_advance_dev hold the caller's pointers, the arena and st_scaled), so growing it leaves mem_gen -- and with it
// the cached graphs -- alone.  (hipFree synchronises: nothing in flight can still touch the old buffer.)
int32_t ensure_private(infur_ctx* c, Buf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return INFUR_OK;
    if (b.p) HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return INFUR_OK;
}

// ---- activation pool: stream-ordered reuse on the single context stream ----
int32_t pool_acquire(infur_ctx* c, size_t bytes, int* slot) {
    int best = -1;
    for (size_t i = 0; i < c->pool.size(); i++) {
        Buf& b = c->pool[i];
        if (!b.used && b.bytes >= bytes && (best < 0 || b.bytes < c->pool[best].bytes)) best = (int)i;
    }
    if (best < 0) {
        Buf b;
        c->mem_gen++;
        HIPCHK(c, hipMalloc(&b.p, bytes));
        b.bytes = bytes;
        c->pool.push_back(b);
        best = (int)c->pool.size() - 1;
    }
    c->pool[best].used = true;
    c->pool[best].last_use = c->frame_no;
    *slot = best;
    return INFUR_OK;
}

void pool_release(infur_ctx* c, Tensor& t) {
    if (c->opt.keep_activations) return;
    if (t.slot >= 0) c->pool[t.slot].used = false;
    t.slot = -1;
}

void pool_release_all(infur_ctx* c) {
    for (auto& b : c->pool) b.used = false;
    c->kept.clear();
    c->out_low = Tensor();
    c->aux_low = Tensor();
}

void pool_free(infur_ctx* c) {
    c->mem_gen++;
    for (auto& b : c->pool)
        if (b.p) (void)hipFree(b.p);
    c->pool.clear();
}

// A long-lived context that has seen several frame sizes (the GUI's scale slider) would otherwise keep the
// largest arena forever: once kPoolTrimAfter consecutive frames had the same size, buffers no frame of that
// run has used are returned to the device.  hipFree synchronises, so nothing in flight can still touch them.
void pool_trim(infur_ctx* c) {
    size_t kept = 0;
    for (auto& b : c->pool) {
        if (!b.used && b.p && b.last_use + kPoolTrimAfter <= c->frame_no) {
            c->mem_gen++;
            (void)hipFree(b.p);
            b.p = nullptr;
            b.bytes = 0;
        }
        if (b.p) c->pool[kept++] = b;
    }
    c->pool.resize(kept);
}

int32_t talloc(infur_ctx* c, int h, int w, int ch, int es, Tensor* t) {
    t->h = h;
    t->w = w;
    t->c = ch;
    t->es = es;
    int slot;
    RETIF(pool_acquire(c, t->bytes(), &slot));
    t->slot = slot;
    t->p = c->pool[slot].p;
    t->lo = es == 3 ? (uint8_t*)t->p + hl_lo_offset(t->elems()) : nullptr;
    return INFUR_OK;
}

// ---- roctx ranges ----
// The reference wraps its stages in `tracing` spans / events (infur/src/main.rs:18-24, RUST_LOG); here INFUR_ROCTX=1 makes every
// stage and layer launch a named roctx range ("<layer> [<kernel>]", inside "infur frame"), so that
// `rocprofv3 --marker-trace --kernel-trace` shows which layer a kernel belongs to.  The library is taken by dlopen at the first
// use (no link-time dependency; without it, or without the variable, a range costs one predictable branch).  Ranges are host
// side: they bracket the ENQUEUE of a launch, so look at them with graph replay off (the default).
const Roctx* roctx() {
    static Roctx r;
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [] {
        const char* e = getenv("INFUR_ROCTX");
        if (!e || !*e || *e == '0') return;
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            r.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            r.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (r.push && r.pop) {
                ok = true;
                return;
            }
        }
        fprintf(stderr, "infur: INFUR_ROCTX is set but no roctx library could be loaded\n");
    });
    return ok ? &r : nullptr;
}
// ---- profiling ----
ProfScope::ProfScope(infur_ctx* c_, const std::string& name, const char* kernel, double flops, double bytes, double algo_flops)
    : c(c_), on(c_->opt.profile != 0), rx(roctx()) {
    if (rx) rx->push((name + " [" + kernel + "]").c_str());
    if (!on) return;
    r.name = name;
    r.kernel = kernel;
    r.flops = flops;
    r.bytes = bytes;
    r.algo_flops = algo_flops < 0.0 ? flops : algo_flops;
    for (hipEvent_t* e : {&r.e0, &r.e1}) {
        if (!c->ev_free.empty()) {
            *e = c->ev_free.back();
            c->ev_free.pop_back();
        } else {
            (void)hipEventCreate(e);
        }
    }
    (void)hipEventRecord(r.e0, c->stream);
}
ProfScope::~ProfScope() {
    if (on) {
        (void)hipEventRecord(r.e1, c->stream);
        c->prof.push_back(r);
    }
    if (rx) rx->pop();
}

void prof_reset(infur_ctx* c) {
    for (auto& r : c->prof) {
        c->ev_free.push_back(r.e0);
        c->ev_free.push_back(r.e1);
    }
    c->prof.clear();
}

// ---- lookup tables (host side, exact reference operation order) ----
// predict_onnx.rs:128 `f32::from(v) * 1f32 / 255f32`, :131-136 `(x - mean) * (1/std)`;
// ColorNorm::new_torchvision_rgb :175-180.  volatile keeps every rounding step.
// the table the stem kernels index with a pixel's bytes: the Float pre-proc, or the identity for Uint8-input models

void build_pre_lut(float* lut) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int ch = 0; ch < 3; ch++) {
        volatile float std1 = 1.0f / stdv[ch];
        for (int v = 0; v < 256; v++) {
            volatile float x = ((float)v * 1.0f) / 255.0f;
            volatile float d = x - mean[ch];
            lut[ch * 256 + v] = d * std1;
        }
    }
}

// COLORS_PALETTE, decode_predict.rs:9-30
const uint8_t kPalette[20][3] = {
    {75, 180, 60},   {75, 25, 230},   {25, 225, 255},  {200, 130, 0},   {48, 130, 245},
    {240, 240, 70},  {230, 50, 240},  {60, 245, 210},  {180, 30, 145},  {190, 190, 250},
    {128, 128, 0},   {255, 190, 230}, {40, 110, 170},  {200, 250, 255}, {0, 0, 128},
    {195, 255, 170}, {0, 128, 128},   {180, 215, 255}, {128, 0, 0},     {128, 128, 128},
};

// epaint 0.19 Color32::from_rgba_unmultiplied (called at decode_predict.rs:35): gamma-aware
// premultiply.  The device kernels only index the resulting table.
float lin_from_gamma_u8(uint8_t s) {
    if (s <= 10) return (float)s / 3294.6f;
    return powf(((float)s + 14.025f) / 269.025f, 2.4f);
}
uint8_t round_u8(float r) {
    float f = floorf(r + 0.5f);
    if (!(f == f) || f <= 0.0f) return 0;
    if (f >= 255.0f) return 255;
    return (uint8_t)f;
}
uint8_t gamma_u8_from_lin(float l) {
    if (l <= 0.0f) return 0;
    if (l <= 0.0031308f) return round_u8(3294.6f * l);
    if (l <= 1.0f) return round_u8(269.025f * powf(l, 1.0f / 2.4f) - 14.025f);
    return 255;
}
void build_color_lut(uint32_t* lut) {
    for (int k = 0; k < 20; k++)
        for (int a = 0; a < 256; a++) {
            uint8_t r = kPalette[k][0], g = kPalette[k][1], b = kPalette[k][2], o[4];
            if (a == 255) {
                o[0] = r; o[1] = g; o[2] = b; o[3] = 255;
            } else if (a == 0) {
                o[0] = o[1] = o[2] = o[3] = 0;
            } else {
                const float al = (float)a / 255.0f;
                o[0] = gamma_u8_from_lin(lin_from_gamma_u8(r) * al);
                o[1] = gamma_u8_from_lin(lin_from_gamma_u8(g) * al);
                o[2] = gamma_u8_from_lin(lin_from_gamma_u8(b) * al);
                o[3] = (uint8_t)a;
            }
            lut[k * 256 + a] = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
        }
}

// ---- Scale host logic (processing.rs:158-168, 238-256) ----
uint32_t f32_as_u32(float v) {  // Rust `as u32`: saturating, NaN -> 0
    if (!(v == v) || v <= 0.0f) return 0;
    if (v >= 4294967296.0f) return 4294967295u;
    return (uint32_t)v;
}


// output tile of the Winograd convs: the caller's choice, else F(6x6): 5.06x fewer MFMA FLOPs than the direct 3x3 (F(4x4):
// 4x) and 1.9x instead of 2.27x the tensor in transform traffic.  Measured against the f32 CPU oracle (scripts/
// f6_split_check.py): per-layer worst 1.07e-5 (F(4x4): 1.12e-5), whole-network logits 6-7e-6 in the exact-f32 mode
// (F(4x4): 4-5e-6) and 4-6e-6 in the split mode (3e-6) -- north_star's budget is 1e-3.
// (INFUR_DTYPE_F32_SPLIT_FP8, bf8 cross terms: F(4x4) was tried as that mode's default because the F(6x6) output transform
// amplifies the product error a little -- hostile parameters, 1080p: 1.4e-4 max-abs / 1.03e-2 worst per-element with F(6x6),
// 1.1e-4 / 6.95e-3 with F(4x4), 1.0e-4 / 8.2e-3 with direct convolutions (profiles/r04_hostile_probe.log): all at the 1e-2 line
// within the noise of a maximum over 680,000 elements -- but it costs 7.5 % of the frame (5.00 -> 5.38 ms) and puts the mode BELOW
// the three-MFMA split mode it exists to beat (205 against 209 frames/s, bench.py on one box).  F(6x6) stays; options.winograd_tile
// = 4 is the knob for a host that wants the margin.)
inline int wino_mt(const infur_ctx* c) {
    const uint32_t t = c->opt.winograd_tile;
    if (t == 2 || t == 4 || t == 6) return (int)t;
    return 6;
}
inline int wino_planes(const infur_ctx* c) { return (wino_mt(c) + 2) * (wino_mt(c) + 2); }

// stride-1 3x3 convs whose direct form is MFMA-bound run in the Winograd domain (f32 mode only:
// the transforms amplify f16 rounding)
bool wino_eligible(const infur_ctx* c, const ConvLayer& L) {
    if (ctx_f16(c) || L.k != 3 || L.stride != 1 || L.pad != L.dil) return false;
    const uint32_t thr = c->opt.winograd_min_cin ? c->opt.winograd_min_cin : 128u;  // measured: 128 beats 256 (+1.4 %) and 64
    if (ctx_hl(c) && ((L.cin % 128) != 0 || (L.cout % 128) != 0)) return false;  // (the three-byte transforms work on 128-channel groups)
    return thr != 0xFFFFFFFFu && (uint32_t)L.cin >= thr && (L.cin % 32) == 0 && (L.cout % 4) == 0;
}

// ---- graph description: torchvision fcn_resnet{50,101}, output stride 8 (blob_dir.h: shared with the format harness) ----
std::vector<ConvLayer> build_graph(int depth, int ncls, bool aux) {
    std::vector<ConvLayer> g;
    for (const ConvSpec& sp : graph_spec(depth, ncls, aux)) {
        ConvLayer c;
        c.name = sp.name; c.cout = sp.cout; c.cin = sp.cin; c.k = sp.k; c.stride = sp.stride; c.pad = sp.pad; c.dil = sp.dil;
        c.relu = sp.relu; c.role = sp.role;
        g.push_back(c);
    }
    return g;
}

bool b2b_candidate(const infur_ctx* c, const ConvLayer& c3, const ConvLayer& n1);

void model_free(infur_ctx* c) {
    c->mem_gen++;
    if (c->d_weights) (void)hipFree(c->d_weights);
    c->d_weights = nullptr;
    c->convs.clear();
    c->qadds.clear();
    c->quant = false;
    c->stem16_wt = nullptr;  // (the image is rebuilt for the next model even if its weights land at the same address)
    c->stem16_split = -1;
    c->d_qlut = nullptr;
    c->d_qstem_w = nullptr;
    c->d_qstem_lut = nullptr;
    c->d_qstem_bias = nullptr;
    c->q_resize_u8 = false;
    c->loaded = false;
    c->weight_bytes = 0;
    pool_release_all(c);
}


// the post stage's view of head k (0 = out, 1 = aux): plain logits, or u8 codes to be dequantised after the interpolation
UpQuant head_quant(const infur_ctx* c, int k) {
    UpQuant q;
    if (c->quant && c->q_resize_u8) {
        q.on = 1;
        q.zp = c->q_head_zp[k];
        q.scale = c->q_head_scale[k];
    }
    return q;
}


// INFUR_DTYPE_F32_SPLIT: scale every conv's GEMM weights (and Winograd-domain weights) by the power of
// two that puts max |w| in [2^13, 2^14) -- lo = w - hi then stays a normal f16 for all weights within
// 2^-16 of the largest -- and replace them in place by (hi, lo) f16 pairs.  The stem is not a GEMM.
// INFUR_DTYPE_F16_HL takes the same route with a different last step: the scaled tensor becomes an f16 hi plane (in place of the
// f32 tensor) and an e5m2 lo plane behind it (launch_hl_pack_weights through a scratch buffer: the planes overlap their source).
int32_t split_weights(infur_ctx* c, std::vector<ConvLayer>& g) {
    const size_t n = g.size();
    const bool hl = ctx_hl(c);
    struct Scratch {
        void* p = nullptr;
        ~Scratch() { if (p) (void)hipFree(p); }
    } scratch;
    if (hl) {
        size_t most = 0;
        for (const ConvLayer& L : g) {
            most = std::max(most, (size_t)L.cout * L.cin * L.k * L.k);
            if (L.d_u) most = std::max(most, (size_t)wino_planes(c) * L.cout * L.cin);
        }
        for (size_t i = 0; i + 1 < n; i++)
            if (g[i].d_wcat) most = std::max(most, (size_t)g[i].cout * (g[i].cin + g[i + 1].cin));
        HIPCHK(c, hipMalloc(&scratch.p, hl_tensor_bytes(most)));
    }
    // f32 [planes][rows][per / rows] at `w`, plane p scaled by sc[p] -> hi planes at w, lo planes at w + hl_lo_offset(planes * per), each plane
    // K-block-major (conv_hl.hip: hl_pack_weights_kernel); *lo_out = the lo base
    auto hl_pack = [&](float* w, size_t planes, size_t rows, size_t per, const float* sc, void** lo_out) -> int32_t {
        const size_t tot = planes * per;
        uint8_t* t_hi = (uint8_t*)scratch.p;
        uint8_t* t_lo = t_hi + hl_lo_offset(tot);
        // (all planes of the tensor in one launch: hi planes back to back at t_hi, lo planes back to back at t_lo)
        HIPCHK(c, launch_hl_pack_weights_planes(w, rows, per / rows, (int)planes, sc, t_hi, t_lo, c->stream));
        HIPCHK(c, hipMemcpyAsync(w, t_hi, hl_tensor_bytes(tot), hipMemcpyDeviceToDevice, c->stream));
        *lo_out = (uint8_t*)w + hl_lo_offset(tot);
        return INFUR_OK;
    };
    const size_t P = (size_t)wino_planes(c);
    // per conv: [0] max |w|, [1] max |conv3 ++ downsample matrix|, [2 .. 2 + P) max |U| of every Winograd plane
    const size_t per = 2 + P;
    float* d_max = nullptr;
    HIPCHK(c, hipMalloc(&d_max, per * n * sizeof(float)));
    hipError_t e = hipMemsetAsync(d_max, 0, per * n * sizeof(float), c->stream);
    for (size_t i = 0; i < n && e == hipSuccess; i++) {
        const ConvLayer& L = g[i];
        e = launch_absmax((const float*)L.d_w, (size_t)L.cout * L.cin * L.k * L.k, d_max + per * i, c->stream);
        if (L.role == 's') continue;  // the stem keeps f32 weights (its kernel splits them while it stages them): scale only
        if (e == hipSuccess && L.d_u)  // every Winograd plane's maximum in one launch
            e = launch_absmax_planes(L.d_u, (size_t)L.cout * L.cin, (int)P, d_max + per * i + 2, c->stream);
        if (e == hipSuccess && L.d_wcat)
            e = launch_absmax((const float*)L.d_wcat, (size_t)L.cout * (L.cin + g[i + 1].cin), d_max + per * i + 1, c->stream);
    }
    std::vector<float> mx(per * n, 0.0f);
    if (e == hipSuccess) e = hipMemcpyAsync(mx.data(), d_max, per * n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_max);
    HIPCHK(c, e);
    auto pow2_for = [](float amax) {
        if (!(amax > 0.0f) || !std::isfinite(amax)) return 1.0f;
        return std::ldexp(1.0f, 13 - std::ilogb(amax));
    };
    for (size_t i = 0; i < n; i++) {
        ConvLayer& L = g[i];
        L.w_scale = pow2_for(mx[per * i]);
        if (L.role == 's') continue;
        if (hl)
            RETIF(hl_pack((float*)L.d_w, 1, L.cout, (size_t)L.cout * L.cin * L.k * L.k, &L.w_scale, &L.d_wl));
        else
            HIPCHK(c, launch_split_weights((float*)L.d_w, (size_t)L.cout * L.cin * L.k * L.k, L.w_scale, ctx_fp8x(c) ? 1 : 0, c->stream));
        if (L.d_u) {
            // Every Winograd plane gets its OWN power-of-two scale: U = G g G^T mixes G's entries (1 ... 1/180 for F(6x6)), so the
            // planes' magnitudes span four decades before the weights' own spread; under one scale per layer the small planes
            // lost their lo halves to f16 underflow -- invisible on uniform synthetic weights (4-6e-6), 9e-3 .. 1.6e-2 on
            // heavy-tailed ones with per-channel scales over three decades (tests/test_gpu_hostile.py).  The GEMM of plane p
            // multiplies its accumulators by d_uacc[p] = 1 / (activation scale * scale of plane p).
            const int mt = wino_mt(c);
            const float a_scale = mt == 6 ? 0.0625f : (mt == 4 ? 0.125f : 1.0f);  // = split_wino_scale(mt)
            std::vector<float> acc(P), scs(P);
            float smin = 0.f;
            for (size_t pl = 0; pl < P; pl++) {
                const float sc = pow2_for(mx[per * i + 2 + pl]);
                scs[pl] = sc;
                acc[pl] = 1.0f / (a_scale * sc);
                if (pl == 0 || sc < smin) smin = sc;
                if (!hl) HIPCHK(c, launch_split_weights(L.d_u + pl * (size_t)L.cout * L.cin, (size_t)L.cout * L.cin, sc, ctx_fp8x(c) ? 1 : 0, c->stream));
            }
            if (hl) RETIF(hl_pack(L.d_u, P, L.cout, (size_t)L.cout * L.cin, scs.data(), &L.d_ul));
            L.u_scale = smin;
            HIPCHK(c, hipMemcpyAsync(L.d_uacc, acc.data(), P * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // (acc goes out of scope)
        }
        if (L.d_wcat) {
            L.wcat_scale = pow2_for(mx[per * i + 1]);
            if (hl)
                RETIF(hl_pack((float*)L.d_wcat, 1, L.cout, (size_t)L.cout * (L.cin + g[i + 1].cin), &L.wcat_scale, &L.d_wcatl));
            else
                HIPCHK(c, launch_split_weights((float*)L.d_wcat, (size_t)L.cout * (L.cin + g[i + 1].cin), L.wcat_scale, ctx_fp8x(c) ? 1 : 0, c->stream));
        }
    }
    return INFUR_OK;
}

// d_blob: INFURW01 blob resident on the device.  Parses the directory (copied to the host),
// checks it against the expected graph and repacks every tensor into kernel layout.
int32_t model_load_dev(infur_ctx* c, const void* d_blob, size_t len) {
    if (len < kBlobHdr) return fail(c, INFUR_E_MODEL_FORMAT, "weight blob too short (%zu bytes)", len);
    uint8_t hdr[kBlobHdr];
    HIPCHK(c, hipMemcpyAsync(hdr, d_blob, kBlobHdr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // header and directory are checked by blob_dir.h (host-only: the code `make asan` mutates files against)
    BlobHeader bh;
    std::vector<ConvSpec> spec;
    std::string perr;
    if (!blob_parse_header(hdr, len, &bh, &spec, &perr)) return fail(c, INFUR_E_MODEL_FORMAT, "%s", perr.c_str());
    const int depth = bh.depth, ncls = bh.num_classes;
    const bool aux = bh.aux, input_u8 = bh.input_u8;
    const uint32_t n = bh.n_convs;
    std::vector<ConvLayer> g = build_graph(depth, ncls, aux);
    std::vector<uint8_t> table((size_t)n * kBlobEntry);
    HIPCHK(c, hipMemcpyAsync(table.data(), (const uint8_t*)d_blob + kBlobHdr, table.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<BlobEntry> ents;
    if (!blob_parse_directory(table.data(), len, spec, &ents, &perr)) return fail(c, INFUR_E_MODEL_FORMAT, "%s", perr.c_str());
    size_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        const ConvLayer& L = g[i];
        const size_t wn = (size_t)L.cout * L.cin * L.k * L.k * 4, bn = (size_t)L.cout * 4;
        total += align_up(wn, 256) + align_up(bn, 256);  // upper bound (f16 weights take half)
        if (wino_eligible(c, L)) total += align_up((size_t)wino_planes(c) * L.cout * L.cin * 4, 256) + align_up((size_t)wino_planes(c) * 4, 256);
        if (L.role == '3' && i + 1 < n && g[i + 1].role == 'd')
            total += align_up((size_t)L.cout * (L.cin + g[i + 1].cin) * 4, 256) + align_up(bn, 256);
        if (i + 1 < n && b2b_candidate(c, L, g[i + 1])) total += align_up((size_t)L.cout * L.cin * 2, 256);
    }

    // The new weight set is built beside the loaded one and swapped in only when everything succeeded: a failed
    // (re)load leaves the previous model in place, as Model::control does on any load error (predict_onnx.rs:288-309).
    struct DevMem {
        void* p = nullptr;
        ~DevMem() { if (p) (void)hipFree(p); }
    } arena;
    HIPCHK(c, hipMalloc(&arena.p, total));
    void* const d_weights = arena.p;
    size_t off = 0;
    for (uint32_t i = 0; i < n; i++) {
        ConvLayer& L = g[i];
        const size_t wn = (size_t)L.cout * L.cin * L.k * L.k * 4, bn = (size_t)L.cout * 4;
        L.d_w = (float*)((uint8_t*)d_weights + off);
        off += align_up(wn, 256);
        L.d_b = (float*)((uint8_t*)d_weights + off);
        off += align_up(bn, 256);
        const float* src_w = (const float*)((const uint8_t*)d_blob + ents[i].w_off);
        if (L.role == 's')
            HIPCHK(c, launch_repack_stem(src_w, (float*)L.d_w, input_u8 ? 1 : 0, c->stream));
        else if (L.k == 1 && !ctx_f16(c))
            HIPCHK(c, hipMemcpyAsync(L.d_w, src_w, wn, hipMemcpyDeviceToDevice, c->stream));  // OI11 == O11I
        else
            HIPCHK(c, launch_repack_oihw_to_ohwi(src_w, L.d_w, ctx_f16(c) ? 1 : 0, L.cout, L.cin, L.k, L.k, c->stream));
        HIPCHK(c, hipMemcpyAsync(L.d_b, (const uint8_t*)d_blob + ents[i].b_off, bn, hipMemcpyDeviceToDevice, c->stream));
        if (wino_eligible(c, L)) {
            L.d_u = (float*)((uint8_t*)d_weights + off);
            off += align_up((size_t)wino_planes(c) * L.cout * L.cin * 4, 256);
            L.d_uacc = (float*)((uint8_t*)d_weights + off);  // per-plane accumulator scales (split modes; split_weights fills them)
            off += align_up((size_t)wino_planes(c) * 4, 256);
            HIPCHK(c, launch_wino_weights(src_w, L.cout, L.cin, wino_mt(c), L.d_u, c->stream));
        }
    }
    // conv3 ++ downsample weight matrices for the two-source GEMM
    for (uint32_t i = 0; i + 1 < n; i++) {
        ConvLayer& L = g[i];
        const ConvLayer& D = g[i + 1];
        if (L.role != '3' || D.role != 'd') continue;
        const size_t es = ctx_f16(c) ? 2 : 4;
        L.d_wcat = (uint8_t*)d_weights + off;
        off += align_up((size_t)L.cout * (L.cin + D.cin) * 4, 256);
        L.d_bcat = (float*)((uint8_t*)d_weights + off);
        off += align_up((size_t)L.cout * 4, 256);
        HIPCHK(c, launch_concat_rows(L.d_w, (size_t)L.cin * es, D.d_w, (size_t)D.cin * es, L.d_wcat, L.cout, c->stream));
        HIPCHK(c, launch_add_f32(L.d_b, D.d_b, L.d_bcat, L.cout, c->stream));
    }
    // conv3 weights in the row order of the fused conv3 -> next conv1 launch (f16 mode, inside a stage)
    for (uint32_t i = 0; i + 1 < n; i++) {
        ConvLayer& L = g[i];
        if (!b2b_candidate(c, L, g[i + 1])) continue;
        L.d_w3i = (uint8_t*)d_weights + off;
        off += align_up((size_t)L.cout * L.cin * 2, 256);
        HIPCHK(c, launch_b2b_pack_w3(L.d_w, L.d_w3i, L.cin, c->stream));
    }
    if (ctx_mode(c) == kModeSplit || ctx_hl(c)) RETIF(split_weights(c, g));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    model_free(c);  // the old model goes only now
    c->d_weights = d_weights;
    arena.p = nullptr;
    c->convs.swap(g);
    c->depth = depth;
    c->num_classes = ncls;
    c->has_aux = aux;
    c->input_u8 = input_u8;
    c->weight_bytes = total;
    c->loaded = true;
    infur_model_info& mi = c->info;
    memset(&mi, 0, sizeof mi);
    // names as the reference prints them: "input -> out,aux" (predict_onnx.rs:378-380)
    snprintf(mi.input_name, sizeof mi.input_name, "input");
    snprintf(mi.input0_dtype, sizeof mi.input0_dtype, input_u8 ? "Uint8" : "Float");  // the model's declared input type (predict_onnx.rs:90)
    snprintf(mi.output_names[0], 32, "out");
    // the aux output exists when the file has the head AND this context evaluates it (options.compute_aux)
    mi.n_outputs = 1 + ((aux && c->opt.compute_aux) ? 1 : 0);
    if (mi.n_outputs == 2) snprintf(mi.output_names[1], 32, "aux");
    mi.num_classes = (uint32_t)ncls;
    mi.depth = (uint32_t)depth;
    mi.n_convs = n;
    mi.weight_bytes = total;
    mi.quantised = 0;
    mi.resize_u8_heads = 0;
    return INFUR_OK;
}

// ---- tile configuration of the conv kernel for one problem shape: infur_tuner.cpp (pick_cfg) ----

// INFUR_DTYPE_F32_SPLIT: activations are multiplied by 2^2 while they are staged: |x| >= 2^-5 keeps a normal
// f16 lo part (all 22 bits), smaller values an absolute error <= 2^-27 (f16 subnormals), and the f16 pair
// saturates only beyond |x| ~ 32000.  The Winograd input transform amplifies (F(4x4): up to 100x, ~40x
// typically; F(2x2): up to 4x), so V is scaled down instead: 2^-3 keeps |activation| up to ~5000 in range in
// the worst case.  FCN-ResNet activations are O(1..100); the precision floor of small values is absolute
// (1e-8 of unit scale) and does not show in the logits (tests/test_gpu_split.py).
constexpr float kSplitActScale = 4.0f;
constexpr float kSplitWinoScaleF4 = 0.125f, kSplitWinoScaleF2 = 1.0f, kSplitWinoScaleF6 = 0.0625f;  // F6 amplifies up to 225x
inline float split_wino_scale(int mt) { return mt == 6 ? kSplitWinoScaleF6 : (mt == 4 ? kSplitWinoScaleF4 : kSplitWinoScaleF2); }

// the plain (non-Winograd) launch description of layer L on `in` (+ optional residual) -> `out`
ConvArgs conv_args(const ConvLayer& L, const Tensor& in, const Tensor* res, const Tensor& out) {
    ConvArgs a;
    a.in = in.p; a.wt = L.d_w; a.bias = L.d_b; a.res = res ? res->p : nullptr; a.out = out.p;
    a.H = in.h; a.W = in.w; a.Cin = in.c; a.OH = out.h; a.OW = out.w; a.Cout = L.cout;
    a.KH = L.k; a.KW = L.k; a.stride = L.stride; a.pad = L.pad; a.dil = L.dil; a.relu = L.relu ? 1 : 0;
    a.in_lo = in.lo; a.wt_lo = L.d_wl; a.res_lo = res ? res->lo : nullptr; a.out_lo = out.lo;  // (three-byte mode; null otherwise)
    return a;
}

// ---- one convolution on the implicit-GEMM kernel ----
int32_t run_conv(infur_ctx* c, const ConvLayer& L, const Tensor& in, const Tensor* res, Tensor* out) {
    const int oh = conv_out(in.h, L.k, L.stride, L.pad, L.dil), ow = conv_out(in.w, L.k, L.stride, L.pad, L.dil);
    const ConvMode mode = ctx_mode(c);
    const bool hl = ctx_hl(c);
    const int out_f32 = ((mode != kModeF16 && !hl) || L.role == 'c') ? 1 : 0;  // the logits leave the conv stack in f32
    RETIF(talloc(c, oh, ow, L.cout, out_f32 ? 4 : (hl ? 3 : 2), out));
    if (L.d_u && !res) {
        // Winograd F(mt x mt, 3x3): input transform -> (mt+2)^2 batched GEMMs -> output transform (+bias, ReLU).  Three-byte mode: V
        // and the conv output are hi / lo planes (es 3; the operand strides count the hi plane), the Winograd-domain product M stays f32
        const int mt = wino_mt(c), P = wino_planes(c);
        const int T = wino_num_tiles(in.h, in.w, L.dil, mt);
        const int es = hl ? 3 : 4, op_es = hl ? 2 : 4;
        Tensor V, M;
        RETIF(talloc(c, P, T, in.c, es, &V));
        RETIF(talloc(c, P, T, L.cout, 4, &M));
        const double direct = 2.0 * oh * ow * (double)L.cout * L.cin * 9.0;
        {
            ProfScope ps(c, L.name + "/in", hl ? "wino_input_hl" : "wino_input", 0, (double)in.elems() * es + (double)V.elems() * es, 0.0);
            if (!hl) ps.r.variant = wino_variant(in.c, mt);
            if (hl) HIPCHK(c, launch_wino_input_hl(in.p, in.lo, in.h, in.w, in.c, L.dil, mt, split_wino_scale(mt), V.p, V.lo, c->d_hlmon, c->stream));
            else HIPCHK(c, launch_wino_input((const float*)in.p, in.h, in.w, in.c, L.dil, mt, (float*)V.p, c->d_range ? c->d_range + 1 : nullptr, c->stream));
        }
        ConvArgs g;
        g.in = V.p; g.in_lo = V.lo; g.wt = L.d_u; g.wt_lo = L.d_ul; g.bias = nullptr; g.res = nullptr; g.out = M.p;
        g.H = 1; g.W = T; g.Cin = in.c; g.OH = 1; g.OW = T; g.Cout = L.cout;
        g.KH = 1; g.KW = 1; g.stride = 1; g.pad = 0; g.dil = 1; g.relu = 0;
        g.batch = P;
        g.in_bs = (size_t)T * in.c * op_es; g.wt_bs = (size_t)L.cout * L.cin * op_es; g.out_bs = (size_t)T * L.cout * 4;
        if (mode == kModeSplit) {
            g.a_scale = split_wino_scale(mt);
            g.acc_scale = 1.0f / (g.a_scale * L.u_scale);
        }
        if (mode == kModeSplit || hl) g.acc_scale_b = L.d_uacc;  // one scale per Winograd plane
        RETIF(run_tuned(c, L.name, g, conv_mode(c), 1, 2.0 * P * T * (double)L.cout * L.cin,
                        (double)V.elems() * es + (double)M.bytes() + (double)P * L.cout * L.cin * es, direct));
        pool_release(c, V);
        {
            ProfScope ps(c, L.name + "/out", hl ? "wino_output_hl" : "wino_output", 0, (double)M.bytes() + (double)out->elems() * es, 0.0);
            if (!hl) ps.r.variant = wino_variant(L.cout, mt);
            if (hl) HIPCHK(c, launch_wino_output_hl((const float*)M.p, oh, ow, L.cout, L.dil, mt, L.d_b, L.relu ? 1 : 0, out->p, out->lo, c->d_hlmon, c->stream));
            else HIPCHK(c, launch_wino_output((const float*)M.p, oh, ow, L.cout, L.dil, mt, L.d_b, L.relu ? 1 : 0, (float*)out->p,
                                              L.role == 'c' ? nullptr : c->d_range, c->stream));
        }
        pool_release(c, M);
        if (c->opt.keep_activations) c->kept.push_back(*out);
        return INFUR_OK;
    }
    ConvArgs a = conv_args(L, in, res, *out);
    const double flops = 2.0 * oh * ow * (double)L.cout * L.cin * L.k * L.k;
    const double bytes = (double)in.bytes() + (double)out->bytes() + (res ? (double)res->bytes() : 0.0) +
                         (double)L.cout * L.cin * L.k * L.k * in.es;
    if (mode == kModeSplit) {
        a.a_scale = kSplitActScale;
        a.acc_scale = 1.0f / (a.a_scale * L.w_scale);
        a.amax = L.role == 'c' ? nullptr : c->d_range;  // the logits feed no GEMM
    }
    if (hl) a.acc_scale = 1.0f / L.w_scale;  // (activations are stored unscaled: e5m2 lo planes share f16's exponent range)
    if (hl && !out_f32) a.hl_mon = c->d_hlmon;
    RETIF(run_tuned(c, L.name, a, conv_mode(c), out_f32, flops, bytes));
    if (c->opt.keep_activations) c->kept.push_back(*out);
    return INFUR_OK;
}

// ---- a stage's first block: conv3(t2) + downsample(x) + biases, ReLU, as one two-source GEMM ----
// (instead of downsample -> tensor -> conv3 with that tensor as the residual: the branch output is never
// written or re-read, and one kernel's prologue/epilogue disappears)
int32_t run_conv_dual(infur_ctx* c, const ConvLayer& L3, const ConvLayer& D, const Tensor& t2, const Tensor& x, Tensor* out) {
    const int oh = t2.h, ow = t2.w;
    if (conv_out(x.h, 1, D.stride, 0, 1) != oh || conv_out(x.w, 1, D.stride, 0, 1) != ow)
        return fail(c, INFUR_E_SHAPE, "downsample branch %dx%d/%d does not land on %dx%d", x.w, x.h, D.stride, ow, oh);
    const ConvMode mode = ctx_mode(c);
    RETIF(talloc(c, oh, ow, L3.cout, act_es(c), out));
    ConvArgs a;
    a.in = t2.p; a.wt = L3.d_wcat; a.bias = L3.d_bcat; a.res = nullptr; a.out = out->p;
    a.H = t2.h; a.W = t2.w; a.Cin = t2.c; a.OH = oh; a.OW = ow; a.Cout = L3.cout;
    a.KH = 1; a.KW = 1; a.stride = 1; a.pad = 0; a.dil = 1; a.relu = L3.relu ? 1 : 0;
    a.in2 = x.p; a.H2 = x.h; a.W2 = x.w; a.Cin2 = x.c; a.stride2 = D.stride;
    if (mode == kModeSplit) {
        a.a_scale = kSplitActScale;
        a.acc_scale = 1.0f / (a.a_scale * L3.wcat_scale);
        a.amax = c->d_range;
    }
    const bool hl = ctx_hl(c);
    if (hl) {
        a.in_lo = t2.lo; a.in2_lo = x.lo; a.wt_lo = L3.d_wcatl; a.out_lo = out->lo;
        a.acc_scale = 1.0f / L3.wcat_scale;
        a.hl_mon = c->d_hlmon;
    }
    const double flops = 2.0 * oh * ow * (double)L3.cout * (L3.cin + D.cin);
    const double bytes = (double)t2.bytes() + (double)oh * ow * x.c * x.es + (double)out->bytes() + (double)L3.cout * (L3.cin + D.cin) * t2.es;
    return run_tuned(c, L3.name + "+downsample", a, conv_mode(c), (mode != kModeF16 && !hl) ? 1 : 0, flops, bytes);
}

// ---- conv3 + residual + ReLU of one bottleneck and conv1 + ReLU of the NEXT one as ONE launch (conv1x1_b2b.hip) ----
// f16 mode, inside a stage (the next conv1 reads exactly what this conv3 writes), C2 = 128 / 256 (layer2 / layer3).  y is
// still written once -- it is the next block's residual -- but never read back by conv1.  Bit-identical to the two
// launches, so whether to fuse is measured like a tile configuration: the first time a shape is seen both forms run on
// the real operands and the faster one is remembered (at 1080p a 256-pixel workgroup tile fills only half the CUs; at 4K
// the fused form wins).  *done == false: nothing was produced, the caller runs the two convolutions.
bool b2b_candidate(const infur_ctx* c, const ConvLayer& c3, const ConvLayer& n1) {
    return ctx_f16(c) && !c->opt.no_fuse_b2b && c3.role == '3' && n1.role == '1' && c3.k == 1 && n1.k == 1 && n1.stride == 1 &&
           n1.cin == c3.cout && n1.cout == c3.cin && c3.cout == 4 * c3.cin && (c3.cin == 128 || c3.cin == 256) && c3.relu &&
           n1.relu;
}

int32_t run_b2b(infur_ctx* c, const ConvLayer& c3, const ConvLayer& n1, const Tensor& t2, const Tensor& x, Tensor* y, Tensor* t1n, bool* done) {
    *done = false;
    if (!b2b_candidate(c, c3, n1) || !c3.d_w3i || x.h != t2.h || x.w != t2.w || x.c != c3.cout || t2.c != c3.cin || t2.es != 2 || x.es != 2) return INFUR_OK;
    RETIF(talloc(c, t2.h, t2.w, c3.cout, 2, y));
    RETIF(talloc(c, t2.h, t2.w, n1.cout, 2, t1n));
    auto give_back = [&]() {  // (pool_release keeps buffers under keep_activations: these two were never results)
        for (Tensor* t : {y, t1n}) {
            if (t->slot >= 0) c->pool[t->slot].used = false;
            *t = Tensor();
        }
    };
    B2bArgs b;
    b.in = t2.p; b.w3 = c3.d_w3i; b.b3 = c3.d_b; b.res = x.p; b.y = y->p; b.w1 = n1.d_w; b.b1 = n1.d_b; b.out2 = t1n->p;
    b.M = t2.h * t2.w; b.C2 = c3.cin; b.relu1 = 1; b.relu2 = 1;
    if (!conv1x1_b2b_valid(b)) {
        give_back();
        return INFUR_OK;
    }
    // the decision lives in the tuning database next to the tile configurations, under the conv3's shape with kTunePairFlag
    ConvArgs gemm = conv_args(c3, t2, nullptr, *y);  // (c3.k == 1: b2b_candidate)
    gemm.stride = gemm.dil = 1;
    TuneKey key = tune_key(gemm, kModeF16, 0);
    key[10] = kTunePairFlag;
    static const int forced = getenv("INFUR_B2B") ? atoi(getenv("INFUR_B2B")) : -1;  // test hook: 1 always, 0 never
    bool use;
    auto it = c->tuned.find(key);
    if (forced >= 0) {
        use = forced != 0;
    } else if (it != c->tuned.end()) {
        use = it->second != 0;
    } else if (c->opt.no_autotune) {
        use = (b.M + 255) / 256 >= 384;  // one and a half waves of workgroups on 256 CUs
    } else {
        const ConvArgs a3 = conv_args(c3, t2, &x, *y), a1 = conv_args(n1, *y, nullptr, *t1n);
        int cfg3 = -1, cfg1 = -1;
        RETIF(pick_cfg(c, a3, kModeF16, 0, &cfg3));
        RETIF(pick_cfg(c, a1, kModeF16, 0, &cfg1));
        EventPair ev;
        HIPCHK(c, ev.create());
        float t_pair, t_fused;  // 5 timings each, the first a warm-up
        RETIF(min_launch_ms(c, ev, 1, 5, &t_pair, [&] {
            const hipError_t e = launch_conv_igemm(a3, kModeF16, 0, cfg3, c->stream);
            return e != hipSuccess ? e : launch_conv_igemm(a1, kModeF16, 0, cfg1, c->stream);
        }));
        RETIF(min_launch_ms(c, ev, 1, 5, &t_fused, [&] { return launch_conv1x1_b2b(b, c->stream); }));
        use = t_fused < t_pair;
        c->tuned[key] = use ? 1 : 0;
        c->mem_gen++;
    }
    if (!use) {
        give_back();
        return INFUR_OK;
    }
    const double M = (double)b.M;
    {
        ProfScope ps(c, c3.name + "+next.conv1", "conv1x1_b2b_f16", 2.0 * M * c3.cout * c3.cin * 2.0,
                     (double)t2.bytes() + (double)x.bytes() + (double)y->bytes() + (double)t1n->bytes() + 2.0 * c3.cout * c3.cin * 2.0);
        ps.r.variant = conv1x1_b2b_variant(b);
        HIPCHK(c, launch_conv1x1_b2b(b, c->stream));
    }
    if (c->opt.keep_activations) {
        c->kept.push_back(*y);
        c->kept.push_back(*t1n);
    }
    *done = true;
    return INFUR_OK;
}


// the weight image of the f16-MFMA stems (stem_pool.hip), built on the context's stream the first time a model's stem runs in this
// form and whenever the weights, their scale or the arithmetic change (model_free forgets it)
int32_t stem16_image(infur_ctx* c, const float* wt, float w_scale, int split, const void** img) {
    if (!c->d_stem16) HIPCHK(c, hipMalloc(&c->d_stem16, stem16_image_bytes()));
    if (c->stem16_wt != wt || c->stem16_scale != w_scale || c->stem16_split != split) {
        HIPCHK(c, launch_stem16_pack(wt, w_scale, split, c->d_stem16, c->stream));
        c->stem16_wt = wt;
        c->stem16_scale = w_scale;
        c->stem16_split = split;
        c->mem_gen++;  // (a frame captured as a graph before this must not be replayed without the pack launch)
    }
    *img = c->d_stem16;
    return INFUR_OK;
}

// ---- quantised models (INFURQ01): infur_quant_model.cpp (model_load_q_dev, forward_q) ----

// FCN-ResNet forward from a packed BGR frame resident on the device.
// Leaves the output-stride-8 logits in c->out_low / c->aux_low (NHWC).
int32_t forward(infur_ctx* c, const uint8_t* d_bgr, int w, int h) {
    if (w <= 0 || h <= 0) return fail(c, INFUR_E_SHAPE, "couldn't transform image: %dx%d", w, h);
    RoctxRange rr("infur forward");
    pool_release_all(c);
    prof_reset(c);
    c->frame_no++;
    c->same_size = (h == c->last_h && w == c->last_w) ? c->same_size + 1 : 0;
    if (c->same_size == kPoolTrimAfter) pool_trim(c);  // no tensor is live here: slots may be renumbered
    if (c->quant) return forward_q(c, d_bgr, w, h);  // a quantised model defines its own arithmetic
    if (c->d_range) HIPCHK(c, hipMemsetAsync(c->d_range, 0, 2 * sizeof(unsigned), c->stream));
    size_t ci = 0;
    const ConvLayer& stem = c->convs[ci++];
    Tensor s, x;
    const int sh = conv_out(h, 7, 2, 3, 1), sw = conv_out(w, 7, 2, 3, 1);
    const int ph = conv_out(sh, 3, 2, 1, 1), pw = conv_out(sw, 3, 2, 1, 1);
    // stem and max-pool as one kernel unless the per-layer read-back wants the stem tensor (keep_activations) or
    // the caller asked for the two-kernel form (options.no_fuse_stem_pool: a test / measurement knob)
    if (!c->opt.keep_activations && !c->opt.no_fuse_stem_pool) {
        RETIF(talloc(c, ph, pw, 64, act_es(c), &x));
        const void* wimg = nullptr;
        if (ctx_mode(c) == kModeF16) RETIF(stem16_image(c, (const float*)stem.d_w, 1.0f, 0, &wimg));
        if (ctx_mode(c) == kModeSplit || ctx_hl(c)) RETIF(stem16_image(c, (const float*)stem.d_w, stem.w_scale, 1, &wimg));
        ProfScope ps(c, "backbone.conv1+maxpool", "stem_pool", 2.0 * sh * sw * 64 * 147, (double)h * w * 3 + (double)x.bytes(),
                     2.0 * sh * sw * 64 * 147);
        ps.r.variant = stem_pool_variant(ctx_mode(c));
        // exact f32 MFMA in the f32 mode; in the f16-rate modes the stem runs on the f16 matrix cores as the conv stack does
        HIPCHK(c, launch_stem_pool(d_bgr, h, w, (const float*)stem.d_w, wimg, stem.d_b, stem_lut(c), x.p, ctx_mode(c), sh, sw, ph, pw,
                                   kSplitActScale, stem.w_scale, ctx_hl(c) ? c->d_hlmon : c->d_range, c->stream));  // (mode 5: hi / lo planes, x.lo = x.p + hl_lo_offset)
    } else {
        const int es01 = ctx_hl(c) ? 4 : act_es(c);  // three-byte mode: stem and pool in f32 (the exact f32 stem), converted below
        {
            RETIF(talloc(c, sh, sw, 64, es01, &s));
            ProfScope ps(c, stem.name, "stem_conv7x7", 2.0 * sh * sw * 64 * 147, (double)h * w * 3 + (double)s.bytes());
            HIPCHK(c, launch_stem_conv7x7(d_bgr, h, w, (const float*)stem.d_w, stem.d_b, stem_lut(c), s.p, ctx_f16(c) ? 1 : 0, sh, sw, c->stream));
        }
        if (c->opt.keep_activations) c->kept.push_back(s);
        Tensor xp;
        {
            RETIF(talloc(c, ph, pw, 64, es01, &xp));
            ProfScope ps(c, "backbone.maxpool", "maxpool3x3s2", 0, (double)s.bytes() + (double)xp.bytes());
            HIPCHK(c, launch_maxpool3x3s2(s.p, s.h, s.w, 64, xp.p, ctx_f16(c) ? 1 : 0, ph, pw, c->d_range, c->stream));
        }
        if (ctx_hl(c)) {
            RETIF(talloc(c, ph, pw, 64, 3, &x));
            HIPCHK(c, launch_hl_from_f32((const float*)xp.p, xp.elems(), x.p, x.lo, c->d_hlmon, c->stream));
            pool_release(c, xp);
        } else {
            x = xp;
        }
        pool_release(c, s);
    }

    Tensor l3;
    Tensor t1_pre;  // this block's conv1 output when the previous block's conv3 launch already produced it (run_b2b)
    while (c->convs[ci].role == '1') {
        const ConvLayer& c1 = c->convs[ci];
        const ConvLayer& c2 = c->convs[ci + 1];
        const ConvLayer& c3 = c->convs[ci + 2];
        const bool has_ds = c->convs[ci + 3].role == 'd';
        Tensor t1, t2, idt, y;
        if (t1_pre.p) {
            t1 = t1_pre;
            t1_pre = Tensor();
        } else {
            RETIF(run_conv(c, c1, x, nullptr, &t1));
        }
        RETIF(run_conv(c, c2, t1, nullptr, &t2));
        pool_release(c, t1);
        // the per-layer read-back (keep_activations) wants the branch tensor, so it runs the unfused form
        const bool fused = has_ds && c3.d_wcat && !c->opt.keep_activations && !c->opt.no_fuse_downsample;
        if (fused) {
            RETIF(run_conv_dual(c, c3, c->convs[ci + 3], t2, x, &y));
        } else {
            if (has_ds) {
                // keep_activations order follows the blob (conv3 before downsample): fix up below
                RETIF(run_conv(c, c->convs[ci + 3], x, nullptr, &idt));
            }
            bool b2b = false;
            if (!has_ds) RETIF(run_b2b(c, c3, c->convs[ci + 3], t2, x, &y, &t1_pre, &b2b));
            if (!b2b) RETIF(run_conv(c, c3, t2, has_ds ? &idt : &x, &y));
            if (has_ds && c->opt.keep_activations) std::swap(c->kept[c->kept.size() - 1], c->kept[c->kept.size() - 2]);
        }
        pool_release(c, t2);
        if (has_ds && !fused) pool_release(c, idt);
        ci += has_ds ? 4 : 3;
        const bool end_l3 = c1.name.compare(0, 16, "backbone.layer3.") == 0 &&
                            c->convs[ci].name.compare(0, 16, "backbone.layer4.") == 0;
        // the layer3 output feeds the aux head: it stays acquired until that head has run
        if (!(l3.p && x.p == l3.p)) pool_release(c, x);
        x = y;
        if (end_l3 && c->has_aux && c->opt.compute_aux) l3 = y;
    }
    {
        Tensor h1;
        RETIF(run_conv(c, c->convs[ci], x, nullptr, &h1));
        // x (layer4 output) may alias l3 only when there is no layer4 -- never for 50/101
        pool_release(c, x);
        RETIF(run_conv(c, c->convs[ci + 1], h1, nullptr, &c->out_low));
        pool_release(c, h1);
        ci += 2;
    }
    if (c->has_aux && c->opt.compute_aux) {
        Tensor a1;
        RETIF(run_conv(c, c->convs[ci], l3, nullptr, &a1));
        pool_release(c, l3);
        RETIF(run_conv(c, c->convs[ci + 1], a1, nullptr, &c->aux_low));
        pool_release(c, a1);
    }
    c->last_h = h;
    c->last_w = w;
    return INFUR_OK;
}

}  // namespace

// ---- the front half of the fused frame calls (infur_rt.h) ----
namespace infur {

int32_t scale_dims(infur_ctx* c, uint32_t w, uint32_t h, float factor, uint32_t* ow, uint32_t* oh) {
    int32_t rc = infur_scale_validate(factor);
    if (rc) return fail(c, rc, "%s", infur_status_string(rc));
    rc = infur_scale_out_dims(w, h, factor, ow, oh);
    if (rc) return fail(c, rc, "%s", infur_status_string(rc));
    return INFUR_OK;
}

// the Scale stage of a frame: into the caller's d_scaled, or into st_scaled when only the model needs the scaled frame
static int32_t frame_scale(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_scaled, size_t sbytes,
                           const void** frame) {
    void* dst = d_scaled;
    if (!dst) {
        RETIF(ensure(c, c->st_scaled, sbytes));
        dst = c->st_scaled.p;
    }
    uint32_t a, b;
    RETIF(infur_scale_dev(c, d_bgr, w, h, factor, mode, dst, sbytes, &a, &b));
    *frame = dst;
    return INFUR_OK;
}

int32_t frame_check(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_scaled, uint32_t* ow,
                    uint32_t* oh, size_t* npix) {
    if (mode > INFUR_SCALE_BILINEAR) return fail(c, INFUR_E_INVALID_ARG, "unknown scale mode %u", mode);
    RETIF(scale_dims(c, w, h, factor, ow, oh));
    if (!d_bgr) return INFUR_E_INVALID_ARG;
    *npix = (size_t)*ow * *oh;
    if (*npix == 0) return fail(c, INFUR_E_SHAPE, "couldn't transform image: %ux%u", *ow, *oh);
    if (!c->loaded) {
        // app.rs:127-129: no model -> the mask is cleared by the caller; the Scale stage still runs
        if (factor != 1.0f || d_scaled) {
            const void* frame;
            prof_reset(c);
            RETIF(frame_scale(c, d_bgr, w, h, factor, mode, d_scaled, *npix * 3, &frame));
        }
        return fail(c, INFUR_E_MODEL_NOT_LOADED, "no model loaded");
    }
    return INFUR_OK;
}

int32_t scale_forward(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_scaled, uint32_t ow,
                      uint32_t oh) {
    const void* frame = d_bgr;
    prof_reset(c);
    std::vector<ProfRec> pre;
    if (factor != 1.0f || d_scaled) {
        RETIF(frame_scale(c, d_bgr, w, h, factor, mode, d_scaled, (size_t)ow * oh * 3, &frame));
        pre.swap(c->prof);  // forward() resets the records; keep the scale's
    }
    RETIF(forward(c, (const uint8_t*)frame, (int)ow, (int)oh));
    c->prof.insert(c->prof.begin(), pre.begin(), pre.end());
    return INFUR_OK;
}

}  // namespace infur

// =====================================================================================
// C ABI
// =====================================================================================
// Every entry point runs on its context's device (enter, infur_ctx.h) and lets no exception out (abi_call, infur_rt.h).
// (infur::stream_orphan -- infur_stream.cpp -- releases a stream's resources and detaches it from its context)

extern "C" {

uint32_t infur_abi_version(void) { return INFUR_ABI_VERSION; }

const char* infur_status_string(int32_t s) {
    switch (s) {
        case INFUR_OK: return "ok";
        case INFUR_E_INVALID_SCALE: return "Cannot scale by negative number";  // processing.rs:163
        case INFUR_E_ZERO_SIZE_IN: return "scaling from 0-sized input";        // processing.rs:203
        case INFUR_E_ZERO_SIZE_OUT: return "scaling to 0-sized output";        // processing.rs:205
        case INFUR_E_SHAPE: return "couldn't transform image";                 // predict_onnx.rs:35
        case INFUR_E_MODEL_NOT_LOADED: return "no model loaded";
        case INFUR_E_MODEL_FORMAT: return "couldn't load model";
        case INFUR_E_HIP: return "HIP runtime error";
        case INFUR_E_RCCL: return "RCCL error";
        case INFUR_E_INVALID_ARG: return "invalid argument";
        case INFUR_E_IO: return "couldn't read model file";
        case INFUR_E_CAPACITY: return "output buffer too small";
        default: return "unknown status";
    }
}

int32_t infur_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void infur_options_default(infur_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->compute_dtype = INFUR_DTYPE_F32;
    o->compute_aux = 1;
}

// the stream pool of infur_ctx_create (see there).  Every pool stream knows how many live contexts hold it: a context that
// wants to CAPTURE its stream (infur_ctx_set_graph_replay) must not share it -- another context's thread enqueueing to a
// capturing stream would have its kernels recorded into this context's graph instead of executed.
namespace {
constexpr int kPool = 8, kMaxDev = 64;
std::mutex g_pool_mu;
hipStream_t g_pool[kMaxDev][kPool];
bool g_pool_made[kMaxDev];
unsigned g_pool_next[kMaxDev];
int g_pool_users[kMaxDev][kPool];
// a slot whose single user has graph replay enabled: it stays that context's alone (pool_stream skips it), so the decision "this
// stream may capture" cannot be invalidated by a context created on another thread during the capture window
bool g_pool_excl[kMaxDev][kPool];
}  // namespace

static hipStream_t pool_stream(int device, int* slot) {
    *slot = -1;
    if (device < 0 || device >= kMaxDev) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pool_made[device]) {
        for (int i = 0; i < kPool; i++)
            if (hipStreamCreateWithFlags(&g_pool[device][i], hipStreamNonBlocking) != hipSuccess) {
                for (int j = 0; j < i; j++) (void)hipStreamDestroy(g_pool[device][j]);
                return nullptr;
            }
        g_pool_made[device] = true;
    }
    // the next FREE entry in round-robin order (contexts created one after the other get consecutive entries, and a context never
    // shares a stream while an unused one exists -- sharing also costs the sharer its graph replay); when all eight are held, the
    // least-used one that no capturing context has reserved
    int pick = -1;
    for (int tries = 0; tries < kPool && pick < 0; tries++) {
        const int k = (int)((g_pool_next[device] + (unsigned)tries) % kPool);
        if (!g_pool_excl[device][k] && g_pool_users[device][k] == 0) pick = k;
    }
    for (int tries = 0; tries < kPool && pick < 0; tries++) {
        const int k = (int)((g_pool_next[device] + (unsigned)tries) % kPool);
        if (g_pool_excl[device][k]) continue;  // reserved by a capturing context
        bool least = true;
        for (int j = 0; j < kPool; j++)
            if (!g_pool_excl[device][j] && g_pool_users[device][j] < g_pool_users[device][k]) least = false;
        if (least) pick = k;
    }
    if (pick >= 0) {
        g_pool_next[device] = (unsigned)pick + 1;
        *slot = pick;
        g_pool_users[device][pick]++;
        return g_pool[device][pick];
    }
    // every pool stream is reserved: a private stream (slot stays -1, the caller owns and destroys it)
    hipStream_t own = nullptr;
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return own;
}

static void pool_stream_release(int device, int slot) {
    if (device < 0 || device >= kMaxDev || slot < 0 || slot >= kPool) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool_users[device][slot] > 0) g_pool_users[device][slot]--;
    if (g_pool_users[device][slot] == 0) g_pool_excl[device][slot] = false;
}

// reserve (or give back) the context's pool stream for capture: succeeds only while the context is the slot's single user
static bool pool_stream_reserve(const infur_ctx* c, bool on) {
    if (c->pool_slot < 0) return true;  // the caller's stream or a private one: nothing to reserve
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!on) {
        g_pool_excl[c->device][c->pool_slot] = false;
        return true;
    }
    if (g_pool_users[c->device][c->pool_slot] != 1) return false;
    g_pool_excl[c->device][c->pool_slot] = true;
    return true;
}

int32_t infur_ctx_create(const infur_options* opts, infur_ctx** out) {
    return abi_call(nullptr, [&]() -> int32_t {
        if (!out) return INFUR_E_INVALID_ARG;
        *out = nullptr;
        infur_options o;
        infur_options_default(&o);
        if (opts) {
            if (opts->struct_size != sizeof(infur_options)) return INFUR_E_INVALID_ARG;
            o = *opts;
        }
        if (o.compute_dtype > INFUR_DTYPE_F32_SPLIT_FP8 && o.compute_dtype != INFUR_DTYPE_F16_HL) return INFUR_E_INVALID_ARG;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || o.device < 0 || o.device >= n) return INFUR_E_HIP;
        if (hipSetDevice(o.device) != hipSuccess) return INFUR_E_HIP;
        infur_ctx* c = new infur_ctx();
        struct Guard {  // an exception below (the look-up tables are std::vectors) must give the stream-pool slot and the context back
            infur_ctx* c;
            ~Guard() { if (c) infur_ctx_destroy(c); }
        } guard{c};
        c->opt = o;
        c->device = o.device;
        if (o.stream) {
            c->stream = (hipStream_t)o.stream;
        } else {
            // The streams the library hands out come from a per-device POOL of eight, created back to back the first time a context
            // of the device asks, handed out round-robin and never destroyed.  Why: two contexts that work on different frames at the
            // same time (bench.py, infur_stream_add_lane, infur_group_* on one device) only overlap if their streams sit on different
            // hardware queues, and the runtime gives a NEW stream the least-used of its four queues -- in a process that has created and
            // destroyed streams unevenly, two streams created back to back can land on the same queue and the two frames in flight
            // behave like one (scripts/ctx_streams.py: the quantised model 580 instead of 640 frames/s, f32x 213 instead of 229,
            // depending on nothing but the process's history).  Pool streams are created in one go (they spread over the queues) and
            // contexts created one after the other get consecutive entries.  (Alternating the PRIORITY class also separates the queues,
            // but the ring's copies, which run at normal priority, then starve behind the high-priority lane: configs[2]'s stream path
            // fell from 341 to 286 frames/s.)  More than eight live contexts of a device share streams pairwise -- as they would share a
            // hardware queue anyway; a host with its own stream policy passes its stream in the options.
            c->stream = pool_stream(o.device, &c->pool_slot);
            if (!c->stream) {
                return INFUR_E_HIP;
            }
            c->own_stream = c->pool_slot < 0;  // (every pool stream reserved by a capturing context: a private stream)
        }
        std::vector<float> pre(768);
        std::vector<uint32_t> col(20 * 256);
        build_pre_lut(pre.data());
        build_color_lut(col.data());
        std::vector<float> ident(768);
        for (int i = 0; i < 768; i++) ident[i] = (float)(i & 255);
        bool ok = hipMalloc((void**)&c->d_pre_lut, pre.size() * 4) == hipSuccess &&
                  hipMalloc((void**)&c->d_u8_lut, ident.size() * 4) == hipSuccess &&
                  hipMemcpy(c->d_u8_lut, ident.data(), ident.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc((void**)&c->d_color_lut, col.size() * 4) == hipSuccess &&
                  hipMemcpy(c->d_pre_lut, pre.data(), pre.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(c->d_color_lut, col.data(), col.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc((void**)&c->d_seg_shards, kSegShardBytes) == hipSuccess &&
                  ((o.compute_dtype != INFUR_DTYPE_F32_SPLIT && o.compute_dtype != INFUR_DTYPE_F32_SPLIT_FP8) ||
                   (hipMalloc((void**)&c->d_range, 2 * sizeof(unsigned)) == hipSuccess && hipMemset(c->d_range, 0, 2 * sizeof(unsigned)) == hipSuccess));
        if (!ok) return INFUR_E_HIP;  // (guard destroys the context)
        guard.c = nullptr;
        *out = c;
        return INFUR_OK;
    });
}

static void graphs_drop(infur_ctx* c);

void infur_ctx_destroy(infur_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // streams that outlive their context become empty shells: infur_stream_destroy on them only frees the handle
    while (!c->streams.empty()) stream_orphan(c->streams.back());
    while (!c->trackers.empty()) tracker_orphan(c->trackers.back());
    if (c->batch_ring) {  // the context's own ring (infur_batch_advance): orphaned above, the handle goes here
        infur_stream_destroy(c->batch_ring);
        c->batch_ring = nullptr;
    }
    graphs_drop(c);
    model_free(c);
    pool_free(c);
    for (Buf* b : {&c->st_in, &c->st_scaled, &c->st_rgba, &c->st_f32a, &c->st_f32b, &c->st_seg, &c->st_reg, &c->st_reg_planes,
                   &c->st_reg_io, &c->st_runs, &c->st_runs_plane, &c->st_runs_io, &c->st_outl, &c->st_outl_plane, &c->st_outl_io,
                   &c->st_simp, &c->st_simp_io, &c->st_poly, &c->st_cov, &c->st_cov_io, &c->st_anch, &c->st_anch_plane, &c->st_anch_io,
                   &c->st_cmp, &c->st_cmp_plane, &c->st_cmp_io, &c->st_sieve, &c->st_sieve_frame, &c->st_sieve_io, &c->st_shapes,
                   &c->st_shapes_plane, &c->st_shapes_poly, &c->st_shapes_io, &c->st_raster, &c->st_raster_io})
        if (b->p) (void)hipFree(b->p);
    prof_reset(c);
    for (auto e : c->ev_free) (void)hipEventDestroy(e);
    if (c->d_pre_lut) (void)hipFree(c->d_pre_lut);
    if (c->d_u8_lut) (void)hipFree(c->d_u8_lut);
    if (c->d_color_lut) (void)hipFree(c->d_color_lut);
    if (c->d_seg_shards) (void)hipFree(c->d_seg_shards);
    if (c->d_range) (void)hipFree(c->d_range);
    if (c->d_hlmon) (void)hipFree(c->d_hlmon);
    if (c->d_stem16) (void)hipFree(c->d_stem16);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    pool_stream_release(c->device, c->pool_slot);
    delete c;
}

const char* infur_last_error(const infur_ctx* c) { return c ? c->err.c_str() : "null context"; }

int32_t infur_ctx_synchronize(infur_ctx* c) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

void* infur_ctx_stream(infur_ctx* c) { return c ? (void*)c->stream : nullptr; }

// ---- Scale ----
int32_t infur_scale_validate(float factor) {
    // ValidScale::try_from (processing.rs:161-163): only `<= 0` is rejected; NaN passes
    return factor <= 0.0f ? INFUR_E_INVALID_SCALE : INFUR_OK;
}

int32_t infur_scale_out_dims(uint32_t w, uint32_t h, float factor, uint32_t* ow, uint32_t* oh) {
    if (!ow || !oh) return INFUR_E_INVALID_ARG;
    if (factor == 1.0f) {  // unit scale clones before any size check (processing.rs:238-242)
        *ow = w;
        *oh = h;
        return INFUR_OK;
    }
    if (w == 0 || h == 0) return INFUR_E_ZERO_SIZE_IN;  // processing.rs:247-248
    const uint32_t nw = f32_as_u32((float)w * factor), nh = f32_as_u32((float)h * factor);  // :253-254
    if (nw == 0 || nh == 0) return INFUR_E_ZERO_SIZE_OUT;  // :255-256
    *ow = nw;
    *oh = nh;
    return INFUR_OK;
}

int32_t infur_scale_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode,
                        void* d_out, size_t cap, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        if (mode > INFUR_SCALE_BILINEAR) return fail(c, INFUR_E_INVALID_ARG, "unknown scale mode %u", mode);
        RETIF(scale_dims(c, w, h, factor, ow, oh));
        const size_t need = (size_t)*ow * *oh * 3;
        if (need == 0) return INFUR_OK;
        if (!d_bgr || !d_out) return INFUR_E_INVALID_ARG;
        if (cap < need) return fail(c, INFUR_E_CAPACITY, "scaled frame needs %zu bytes, buffer has %zu", need, cap);
        if (factor == 1.0f) {
            HIPCHK(c, hipMemcpyAsync(d_out, d_bgr, need, hipMemcpyDeviceToDevice, c->stream));
        } else {
            ProfScope ps(c, "scale", mode ? "scale_bilinear" : "scale_nearest", 0, (double)w * h * 3 + (double)need);
            HIPCHK(c, launch_scale_bgr((const uint8_t*)d_bgr, (int)w, (int)h, (uint8_t*)d_out, (int)*ow, (int)*oh, (int)mode, c->stream));
        }
        return INFUR_OK;
    });
}

int32_t infur_scale(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode,
                    uint8_t* out, size_t cap, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(scale_dims(c, w, h, factor, ow, oh));
        const size_t in_bytes = (size_t)w * h * 3, need = (size_t)*ow * *oh * 3;
        if (need == 0) return INFUR_OK;
        if (!bgr || !out) return INFUR_E_INVALID_ARG;
        if (cap < need) return fail(c, INFUR_E_CAPACITY, "scaled frame needs %zu bytes, buffer has %zu", need, cap);
        RETIF(ensure(c, c->st_in, in_bytes));
        RETIF(ensure(c, c->st_scaled, need));
        HIPCHK(c, hipMemcpyAsync(c->st_in.p, bgr, in_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_scale_dev(c, c->st_in.p, w, h, factor, mode, c->st_scaled.p, c->st_scaled.bytes, ow, oh));
        HIPCHK(c, hipMemcpyAsync(out, c->st_scaled.p, need, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

// ---- Model ----
int32_t infur_model_unload(infur_ctx* c) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        model_free(c);
        return INFUR_OK;
    });
}

int32_t infur_model_load_blob_dev(infur_ctx* c, const void* d_blob, size_t len) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !d_blob) return INFUR_E_INVALID_ARG;
        char magic[8] = {0};
        if (len >= 8) {
            HIPCHK(c, hipMemcpyAsync(magic, d_blob, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (memcmp(magic, "INFURQ01", 8) == 0) return model_load_q_dev(c, d_blob, len);
        return model_load_dev(c, d_blob, len);
    });
}

int32_t infur_model_load_blob(infur_ctx* c, const void* blob, size_t len) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !blob) return INFUR_E_INVALID_ARG;
        const bool quant = len >= kBlobHdr && memcmp(blob, "INFURQ01", 8) == 0;
        if (len < kBlobHdr || (!quant && memcmp(blob, "INFURW01", 8) != 0))
            return fail(c, INFUR_E_MODEL_FORMAT, "bad magic: not an INFURW01 / INFURQ01 weight blob");
        void* d = nullptr;
        HIPCHK(c, hipMalloc(&d, len));
        hipError_t e = hipMemcpyAsync(d, blob, len, hipMemcpyHostToDevice, c->stream);
        int32_t rc = e != hipSuccess ? fail(c, INFUR_E_HIP, "weight upload failed: %s", hipGetErrorString(e))
                                     : (quant ? model_load_q_dev(c, d, len) : model_load_dev(c, d, len));
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        return rc;
    });
}

int32_t infur_model_load(infur_ctx* c, const char* path) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !path) return INFUR_E_INVALID_ARG;
        if (path[0] == 0) return infur_model_unload(c);  // ModelCmd::Load("") unloads, predict_onnx.rs:310-312
        FILE* f = fopen(path, "rb");
        if (!f) return fail(c, INFUR_E_IO, "couldn't open model file '%s'", path);
        fseek(f, 0, SEEK_END);
        long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> buf(n > 0 ? (size_t)n : 0);
        const size_t got = buf.empty() ? 0 : fread(buf.data(), 1, buf.size(), f);
        fclose(f);
        if (got != buf.size()) return fail(c, INFUR_E_IO, "short read on '%s'", path);
        if (buf.empty()) return fail(c, INFUR_E_MODEL_FORMAT, "model file '%s' is empty", path);
        if (buf.size() >= 8 && (memcmp(buf.data(), "INFURW01", 8) == 0 || memcmp(buf.data(), "INFURQ01", 8) == 0))
            return infur_model_load_blob(c, buf.data(), buf.size());
        if (looks_like_onnx(buf.data(), buf.size())) {
            std::vector<uint8_t> blob;
            OnnxInfo oi;
            std::string err;
            if (onnx_to_blob(buf.data(), buf.size(), blob, oi, err) != 0)
                return fail(c, INFUR_E_MODEL_FORMAT, "couldn't infer image input / load '%s': %s", path, err.c_str());
            int32_t rc = infur_model_load_blob(c, blob.data(), blob.size());
            if (rc == INFUR_OK) {  // report the file's own tensor names (predict_onnx.rs:89-92)
                snprintf(c->info.input_name, sizeof c->info.input_name, "%s", oi.input_name.c_str());
                for (size_t i = 0; i < oi.output_names.size() && i < c->info.n_outputs; i++)
                    snprintf(c->info.output_names[i], 32, "%s", oi.output_names[i].c_str());
            }
            return rc;
        }
        return fail(c, INFUR_E_MODEL_FORMAT, "'%s' is neither an INFURW01 blob nor an ONNX model", path);
    });
}

int32_t infur_onnx_to_blob(const void* onnx, size_t len, void** blob, size_t* blob_len, char* err, size_t errcap) {
    return abi_call(nullptr, [&]() -> int32_t {
        if (!onnx || !blob || !blob_len) return INFUR_E_INVALID_ARG;
        *blob = nullptr;
        *blob_len = 0;
        std::vector<uint8_t> out;
        OnnxInfo oi;
        std::string e;
        if (onnx_to_blob((const uint8_t*)onnx, len, out, oi, e) != 0) {
            if (err && errcap) snprintf(err, errcap, "%s", e.c_str());
            return INFUR_E_MODEL_FORMAT;
        }
        void* p = malloc(out.size());
        if (!p) return INFUR_E_INVALID_ARG;
        memcpy(p, out.data(), out.size());
        *blob = p;
        *blob_len = out.size();
        return INFUR_OK;
    });
}

void infur_buffer_free(void* p) { free(p); }

int32_t infur_model_info_get(const infur_ctx* c, infur_model_info* info) { return infur_model_info_get_sized(c, info, sizeof *info); }

int32_t infur_model_info_get_sized(const infur_ctx* c, void* info, size_t info_size) {
    enter(c);
    if (!c || !info || info_size == 0) return INFUR_E_INVALID_ARG;
    if (!c->loaded) return INFUR_E_MODEL_NOT_LOADED;
    memcpy(info, &c->info, info_size < sizeof c->info ? info_size : sizeof c->info);  // (an older, shorter struct gets its prefix)
    return INFUR_OK;
}

int32_t infur_model_lowres_dims(uint32_t h, uint32_t w, uint32_t* lh, uint32_t* lw) {
    if (!lh || !lw || h == 0 || w == 0) return INFUR_E_INVALID_ARG;
    int a = (int)h, b = (int)w;
    a = conv_out(a, 7, 2, 3, 1); b = conv_out(b, 7, 2, 3, 1);
    a = conv_out(a, 3, 2, 1, 1); b = conv_out(b, 3, 2, 1, 1);
    a = conv_out(a, 3, 2, 1, 1); b = conv_out(b, 3, 2, 1, 1);
    *lh = (uint32_t)a;
    *lw = (uint32_t)b;
    return INFUR_OK;
}

int32_t infur_model_advance_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, void* d_out, void* d_aux,
                                uint32_t* n_outputs) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (n_outputs) *n_outputs = 0;
        if (!c->loaded) return INFUR_OK;  // no session: out untouched, Ok(()) (predict_onnx.rs:318,333)
        if (!d_bgr) return INFUR_E_INVALID_ARG;
        if (w == 0 || h == 0) return fail(c, INFUR_E_SHAPE, "couldn't transform image: %ux%u", w, h);
        // checked BEFORE the forward pass: a model without the aux head (or a context with compute_aux = 0) has ONE output
        if (d_aux && c->info.n_outputs < 2)
            return fail(c, INFUR_E_INVALID_ARG, "aux output requested but this model/context has one output (infur_model_info.n_outputs)");
        RETIF(forward(c, (const uint8_t*)d_bgr, (int)w, (int)h));
        const int K = c->num_classes;
        const double up_bytes = (double)c->out_low.bytes() + 4.0 * (double)K * h * w;
        if (d_out) {
            ProfScope ps(c, "out.resize", "upsample_planar", 0, up_bytes);
            HIPCHK(c, launch_upsample_planar((const float*)c->out_low.p, c->out_low.h, c->out_low.w, K, (float*)d_out, (int)h, (int)w, c->stream, head_quant(c, 0)));
        }
        if (d_aux) {
            ProfScope ps(c, "aux.resize", "upsample_planar", 0, up_bytes);
            HIPCHK(c, launch_upsample_planar((const float*)c->aux_low.p, c->aux_low.h, c->aux_low.w, K, (float*)d_aux, (int)h, (int)w, c->stream, head_quant(c, 1)));
        }
        if (n_outputs) *n_outputs = c->info.n_outputs;
        return INFUR_OK;
    });
}

int32_t infur_model_advance(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float* out, float* aux,
                            uint32_t* n_outputs) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (n_outputs) *n_outputs = 0;
        if (!c->loaded) return INFUR_OK;
        if (!bgr) return INFUR_E_INVALID_ARG;
        if (w == 0 || h == 0) return fail(c, INFUR_E_SHAPE, "couldn't transform image: %ux%u", w, h);
        if (aux && c->info.n_outputs < 2)
            return fail(c, INFUR_E_INVALID_ARG, "aux output requested but this model/context has one output (infur_model_info.n_outputs)");
        const size_t in_bytes = (size_t)w * h * 3, lg = (size_t)c->num_classes * w * h * 4;
        RETIF(ensure(c, c->st_in, in_bytes));
        if (out) RETIF(ensure(c, c->st_f32a, lg));
        if (aux) RETIF(ensure(c, c->st_f32b, lg));
        HIPCHK(c, hipMemcpyAsync(c->st_in.p, bgr, in_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_model_advance_dev(c, c->st_in.p, w, h, out ? c->st_f32a.p : nullptr, aux ? c->st_f32b.p : nullptr, n_outputs));
        if (out) HIPCHK(c, hipMemcpyAsync(out, c->st_f32a.p, lg, hipMemcpyDeviceToHost, c->stream));
        if (aux) HIPCHK(c, hipMemcpyAsync(aux, c->st_f32b.p, lg, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_model_warmup(infur_ctx* c, uint32_t w, uint32_t h) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (!c->loaded) return fail(c, INFUR_E_MODEL_NOT_LOADED, "no model loaded");
        if (w == 0 || h == 0) return fail(c, INFUR_E_SHAPE, "couldn't transform image: %ux%u", w, h);
        const size_t in_bytes = (size_t)w * h * 3;
        RETIF(ensure(c, c->st_in, in_bytes));
        HIPCHK(c, hipMemsetAsync(c->st_in.p, 0x55, in_bytes, c->stream));  // any frame will do: timings do not depend on values
        const uint32_t prof = c->opt.profile;
        c->opt.profile = 0;
        const int32_t rc = forward(c, (const uint8_t*)c->st_in.p, (int)w, (int)h);
        c->opt.profile = prof;
        RETIF(rc);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_model_read_lowres(infur_ctx* c, float* out_low, float* aux_low, uint32_t* lh, uint32_t* lw) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (!c->loaded || !c->out_low.p) return fail(c, INFUR_E_MODEL_NOT_LOADED, "no forward pass has run");
        if (aux_low && !c->aux_low.p) return fail(c, INFUR_E_INVALID_ARG, "aux output requested but the aux head is disabled");
        const Tensor& t = c->out_low;
        if (lh) *lh = (uint32_t)t.h;
        if (lw) *lw = (uint32_t)t.w;
        const size_t bytes = t.elems() * 4;
        RETIF(ensure(c, c->st_f32a, bytes));
        for (int i = 0; i < 2; i++) {
            float* dst = i == 0 ? out_low : aux_low;
            const Tensor& src = i == 0 ? c->out_low : c->aux_low;
            if (!dst) continue;
            HIPCHK(c, launch_nhwc_to_planar(src.p, src.es == 2, src.h, src.w, src.c, (float*)c->st_f32a.p, c->stream));
            HIPCHK(c, hipMemcpyAsync(dst, c->st_f32a.p, bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->quant && c->q_resize_u8) {  // the device tensor holds the codes: DequantizeLinear here, (q - zp) * scale
                const volatile float zp = c->q_head_zp[i], sc = c->q_head_scale[i];
                for (size_t k = 0; k < t.elems(); k++) {
                    volatile float d = dst[k] - zp;
                    dst[k] = d * sc;
                }
            }
        }
        return INFUR_OK;
    });
}

int32_t infur_debug_read_activation(infur_ctx* c, uint32_t index, float* host, size_t cap, uint32_t* ch, uint32_t* h,
                                    uint32_t* w) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !host) return INFUR_E_INVALID_ARG;
        if (!c->opt.keep_activations) return fail(c, INFUR_E_INVALID_ARG, "context was created without keep_activations");
        if (index >= c->kept.size()) return fail(c, INFUR_E_INVALID_ARG, "activation %u of %zu", index, c->kept.size());
        const Tensor& t = c->kept[index];
        if (ch) *ch = (uint32_t)t.c;
        if (h) *h = (uint32_t)t.h;
        if (w) *w = (uint32_t)t.w;
        if (cap < t.elems()) return fail(c, INFUR_E_CAPACITY, "activation needs %zu floats", t.elems());
        RETIF(ensure(c, c->st_f32a, t.elems() * 4));
        if (t.es == 1)  // a quantised activation: the byte values
            HIPCHK(c, launch_u8_nhwc_to_planar((const uint8_t*)t.p, t.h, t.w, t.c, (float*)c->st_f32a.p, c->stream));
        else if (t.es == 3)  // three-byte format: hi + lo / kHlLoScale
            HIPCHK(c, launch_hl_nhwc_to_planar(t.p, t.lo, t.h, t.w, t.c, (float*)c->st_f32a.p, c->stream));
        else
            HIPCHK(c, launch_nhwc_to_planar(t.p, t.es == 2, t.h, t.w, t.c, (float*)c->st_f32a.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(host, c->st_f32a.p, t.elems() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

// ---- pre-proc alone ----
int32_t infur_pack_normalize_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, void* d_chw) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if ((size_t)w * h == 0) return INFUR_OK;
        if (!d_bgr || !d_chw) return INFUR_E_INVALID_ARG;
        ProfScope ps(c, "pre-proc", "pack_normalize", 0, (double)w * h * 15.0);
        HIPCHK(c, launch_pack_normalize((const uint8_t*)d_bgr, (int)w, (int)h, c->d_pre_lut, (float*)d_chw, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_pack_normalize(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float* chw) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        const size_t npix = (size_t)w * h;
        if (npix == 0) return INFUR_OK;
        if (!bgr || !chw) return INFUR_E_INVALID_ARG;
        RETIF(ensure(c, c->st_in, npix * 3));
        RETIF(ensure(c, c->st_f32a, npix * 12));
        HIPCHK(c, hipMemcpyAsync(c->st_in.p, bgr, npix * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_pack_normalize_dev(c, c->st_in.p, w, h, c->st_f32a.p));
        HIPCHK(c, hipMemcpyAsync(chw, c->st_f32a.p, npix * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

// ---- ColorCode ----
int32_t infur_colorcode_dev(infur_ctx* c, const void* d_khw, uint32_t k, uint32_t h, uint32_t w, void* d_rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if ((size_t)h * w == 0) return INFUR_OK;  // empty image: nothing to write (decode_predict.rs:68 zips 0 pixels)
        if (!d_rgba || (k > 0 && !d_khw)) return INFUR_E_INVALID_ARG;
        ProfScope ps(c, "colorcode", "colorcode_planar", 0, (double)h * w * (4.0 * k + 4.0));
        HIPCHK(c, launch_colorcode_planar((const float*)d_khw, (int)k, (int)h, (int)w, c->d_color_lut, (uint32_t*)d_rgba, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_colorcode(infur_ctx* c, const float* khw, uint32_t k, uint32_t h, uint32_t w, uint8_t* rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        const size_t hw = (size_t)h * w;
        if (hw == 0) return INFUR_OK;
        if (!rgba || (k > 0 && !khw)) return INFUR_E_INVALID_ARG;
        RETIF(ensure(c, c->st_f32a, hw * (k ? k : 1) * 4));
        RETIF(ensure(c, c->st_rgba, hw * 4));
        if (k) HIPCHK(c, hipMemcpyAsync(c->st_f32a.p, khw, hw * k * 4, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_colorcode_dev(c, c->st_f32a.p, k, h, w, c->st_rgba.p));
        HIPCHK(c, hipMemcpyAsync(rgba, c->st_rgba.p, hw * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

// ---- display conversion ----
int32_t infur_bgr_to_rgba_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, void* d_rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if ((size_t)w * h == 0) return INFUR_OK;
        if (!d_bgr || !d_rgba) return INFUR_E_INVALID_ARG;
        ProfScope ps(c, "display", "bgr_to_rgba", 0, (double)w * h * 7.0);
        HIPCHK(c, launch_bgr_to_rgba((const uint8_t*)d_bgr, (int)w, (int)h, (uint32_t*)d_rgba, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_bgr_to_rgba(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, uint8_t* rgba) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        const size_t npix = (size_t)w * h;
        if (npix == 0) return INFUR_OK;
        if (!bgr || !rgba) return INFUR_E_INVALID_ARG;
        RETIF(ensure(c, c->st_in, npix * 3));
        RETIF(ensure(c, c->st_rgba, npix * 4));
        HIPCHK(c, hipMemcpyAsync(c->st_in.p, bgr, npix * 3, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_bgr_to_rgba_dev(c, c->st_in.p, w, h, c->st_rgba.p));
        HIPCHK(c, hipMemcpyAsync(rgba, c->st_rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

// ---- fused frame path ----
// the fused frame path: Scale -> forward -> up-sample + argmax + shade, everything enqueued on c->stream (arguments validated by
// the caller; ow x oh are the scaled dimensions)
static int32_t frame_body(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, void* d_rgba, void* d_scaled,
                          uint32_t ow, uint32_t oh) {
    RoctxRange rr("infur frame");
    RETIF(scale_forward(c, d_bgr, w, h, factor, mode, d_scaled, ow, oh));
    const Tensor& t = c->out_low;  // only out[0] is decoded, app.rs:116
    ProfScope ps(c, "out.resize+colorcode", "upsample_argmax_shade", 0, (double)t.bytes() + (double)ow * oh * 4);
    HIPCHK(c, launch_upsample_argmax_shade((const float*)t.p, t.h, t.w, t.c, c->d_color_lut, (uint32_t*)d_rgba, (int)oh, (int)ow, c->stream, head_quant(c, 0)));
    return INFUR_OK;
}

// ---- hipGraph replay (infur_ctx_set_graph_replay) ----
// A frame is 55-110 kernel launches; for small frames in the fast modes (a 640x480 frame through the quantised model: 0.74 ms)
// the host's enqueue time is what bounds the rate.  Once a frame shape has run eagerly often enough for the arena to have settled
// (no allocation, release or tuning decision during the last kGraphSettle frames -- the pool trims itself after 4 frames of one
// size), the next frame with a given (input, output, shape) is CAPTURED from the very same enqueue code and replayed from then on.
// The graph holds raw pointers into the arena: every device allocation / release, model change or tuning change bumps
// ctx->mem_gen and drops all cached graphs.
constexpr uint32_t kGraphSettle = 6;
constexpr size_t kGraphCache = 12;

static void graphs_drop(infur_ctx* c) {
    if (!c->graphs.empty() && c->stream) (void)hipStreamSynchronize(c->stream);  // (a replay may still be in flight)
    for (auto& g : c->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
    c->graphs_gen = c->mem_gen;
}

int32_t infur_frame_advance_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode,
                                void* d_rgba, size_t cap, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        size_t npix;
        RETIF(frame_check(c, d_bgr, w, h, factor, mode, d_scaled, ow, oh, &npix));
        if (!d_rgba) return INFUR_E_INVALID_ARG;
        if (cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "mask needs %zu bytes, buffer has %zu", npix * 4, cap);

        const bool graphs_on = c->graph_replay && !c->opt.profile && !c->opt.keep_activations;
        if (!graphs_on) return frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
        if (c->graphs_gen != c->mem_gen) graphs_drop(c);
        uint32_t fbits;
        memcpy(&fbits, &factor, 4);
        for (auto& g : c->graphs)
            if (g.d_bgr == d_bgr && g.d_rgba == d_rgba && g.d_scaled == d_scaled && g.w == w && g.h == h && g.mode == mode && g.factor_bits == fbits) {
                HIPCHK(c, hipGraphLaunch(g.exec, c->stream));
                c->out_low = g.out_low;
                c->aux_low = g.aux_low;
                g.stamp = ++c->graph_clock;
                c->graph_replays++;
                return INFUR_OK;
            }
        // how long has this shape been running without the arena moving?
        if (c->streak_w == w && c->streak_h == h && c->streak_mode == mode && c->streak_factor == fbits && c->streak_gen == c->mem_gen)
            c->graph_streak++;
        else
            c->graph_streak = 0;
        c->streak_w = w; c->streak_h = h; c->streak_mode = mode; c->streak_factor = fbits;
        if (c->graph_streak < kGraphSettle) {
            const int32_t rc = frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
            c->streak_gen = c->mem_gen;  // (a frame that allocated, trimmed or tuned restarts the count)
            return rc;
        }
        // capture: the same enqueue code, recorded instead of executed -- never on a stream another context enqueues to
        // (RESERVE the pool slot here, at capture time, not only in infur_ctx_set_graph_replay: a slot that was shared back then and has
        //  since become this context's alone would otherwise be captured unreserved, and pool_stream() on another thread could hand
        //  it to a new context in the middle of the capture -- ADVICE r5.  A slot that is shared NOW stays eager.)
        if (!pool_stream_reserve(c, true)) return frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
        const uint64_t gen0 = c->mem_gen;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            c->graph_replay = false;  // (a stream that cannot capture: stay eager)
            return frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
        }
        const int32_t rc = frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
        hipGraph_t graph = nullptr;
        const hipError_t ee = hipStreamEndCapture(c->stream, &graph);
        hipGraphExec_t exec = nullptr;
        if (rc == INFUR_OK && ee == hipSuccess && graph && c->mem_gen == gen0 && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            (void)hipGraphDestroy(graph);
            if (c->graphs.size() >= kGraphCache) {  // evict the least recently used
                size_t lru = 0;
                for (size_t i = 1; i < c->graphs.size(); i++)
                    if (c->graphs[i].stamp < c->graphs[lru].stamp) lru = i;
                (void)hipGraphExecDestroy(c->graphs[lru].exec);
                c->graphs.erase(c->graphs.begin() + (long)lru);
            }
            infur_ctx::FrameGraph g;
            g.d_bgr = d_bgr; g.d_rgba = d_rgba; g.d_scaled = d_scaled; g.w = w; g.h = h; g.mode = mode; g.factor_bits = fbits;
            g.exec = exec; g.ow = *ow; g.oh = *oh; g.out_low = c->out_low; g.aux_low = c->aux_low; g.stamp = ++c->graph_clock;
            c->graphs.push_back(g);
            c->graph_captures++;
            HIPCHK(c, hipGraphLaunch(exec, c->stream));
            return INFUR_OK;
        }
        // the capture did not yield a graph (something in the frame is not capturable, or it allocated after all): nothing
        // has executed -- run this frame eagerly and stay eager
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        c->graph_replay = false;
        return frame_body(c, d_bgr, w, h, factor, mode, d_rgba, d_scaled, *ow, *oh);
    });
}

int32_t infur_ctx_set_graph_replay(infur_ctx* c, uint32_t enable) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        c->graph_replay = enable != 0;
        if (!enable) {
            (void)hipSetDevice(c->device);
            if (c->stream) (void)hipStreamSynchronize(c->stream);
            graphs_drop(c);
            (void)pool_stream_reserve(c, false);
        } else {
            // The context's stream NEVER changes behind infur_ctx_stream() (a host that had read the handle kept enqueueing
            // producers of d_bgr on the old stream).  Pool streams are shared from the ninth context of a device on, and a kernel another
            // context's thread enqueues between BeginCapture and EndCapture would be recorded into this context's graph, not executed
            // (ThreadLocal capture mode only restricts the capturing thread) -- so the slot is RESERVED instead: while this context is
            // its only user, pool_stream hands it to nobody else.  A slot that is already shared stays shared and simply never captures
            // (frame_advance_dev runs eagerly: the reservation at capture time fails).
            (void)pool_stream_reserve(c, true);
        }
        c->graph_streak = 0;
        return INFUR_OK;
    });
}

int32_t infur_ctx_graph_stats(const infur_ctx* c, uint64_t* captures, uint64_t* replays, uint32_t* cached) {
    enter(c);
    if (!c) return INFUR_E_INVALID_ARG;
    if (captures) *captures = c->graph_captures;
    if (replays) *replays = c->graph_replays;
    if (cached) *cached = (uint32_t)c->graphs.size();
    return INFUR_OK;
}

int32_t infur_frame_advance(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode,
                            uint8_t* rgba, size_t cap, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if (rgba && cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "mask needs %zu bytes, buffer has %zu", npix * 4, cap);
                return ensure(c, c->st_rgba, npix ? npix * 4 : 1);
            },
            [&](void* d_bgr, void* d_scaled) {
                return infur_frame_advance_dev(c, d_bgr, w, h, factor, mode, c->st_rgba.p, c->st_rgba.bytes, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->st_rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
                return INFUR_OK;
            });
    });
}

// ---- streaming ring, frame batch, pinned host buffers: infur_stream.cpp ----

// ---- range monitor of the split mode ----
int32_t infur_split_range(infur_ctx* c, float* act_amax, float* wino_amax, uint32_t* saturated) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (!c->d_range) return fail(c, INFUR_E_INVALID_ARG, "context is not in INFUR_DTYPE_F32_SPLIT mode");
        float v[2] = {0.f, 0.f};
        HIPCHK(c, hipMemcpyAsync(v, c->d_range, sizeof v, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (act_amax) *act_amax = v[0];
        if (wino_amax) *wino_amax = v[1];
        // beyond 65504 the hi half clamps (MODE.FP16_OVFL) and the pair stops being exact
        const float ws = split_wino_scale(wino_mt(c));
        if (saturated) *saturated = (v[0] * kSplitActScale > 65504.0f || v[1] * ws > 65504.0f) ? 1u : 0u;
        return INFUR_OK;
    });
}

// ---- range monitor of the three-byte mode (opt-in: hl_format.h, kHlMon*) ----
int32_t infur_hl_monitor_enable(infur_ctx* c, uint32_t on) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (c->opt.compute_dtype != INFUR_DTYPE_F16_HL) return fail(c, INFUR_E_INVALID_ARG, "the range monitor is a mode of INFUR_DTYPE_F16_HL contexts");
        if (on && !c->d_hlmon) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            unsigned* p = nullptr;
            HIPCHK(c, hipMalloc((void**)&p, kHlMonWords * sizeof(unsigned)));
            if (hipMemset(p, 0, kHlMonWords * sizeof(unsigned)) != hipSuccess) {
                (void)hipFree(p);
                return fail(c, INFUR_E_HIP, "hipMemset of the range monitor failed");
            }
            c->d_hlmon = p;
        } else if (!on && c->d_hlmon) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_hlmon);
            c->d_hlmon = nullptr;
        } else {
            return INFUR_OK;
        }
        // the kernel arguments of a captured frame name the words (or their absence): like any allocation or release
        c->mem_gen++;
        graphs_drop(c);
        return INFUR_OK;
    });
}

int32_t infur_hl_range(infur_ctx* c, float* act_amax, float* wino_amax, uint32_t* saturated, uint32_t* nan_seen) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        if (!c->d_hlmon) return fail(c, INFUR_E_INVALID_ARG, "the range monitor is not enabled (infur_hl_monitor_enable)");
        unsigned v[kHlMonWords];
        HIPCHK(c, hipMemcpyAsync(v, c->d_hlmon, sizeof v, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_hlmon, 0, sizeof v, c->stream));  // (ordered before the next forward on this stream)
        float act, wino;
        memcpy(&act, &v[kHlMonAct], 4);
        memcpy(&wino, &v[kHlMonWino], 4);
        // values up to kHlHiMax are stored exactly as hi + lo; beyond it the split's upper clamp changed them (+inf included)
        if (act_amax) *act_amax = act;
        if (wino_amax) *wino_amax = wino / split_wino_scale(wino_mt(c));  // (the transform stores V * split_wino_scale: a power of two)
        if (saturated) *saturated = (act > kHlHiMax || wino > kHlHiMax) ? 1u : 0u;
        if (nan_seen) *nan_seen = v[kHlMonNan] ? 1u : 0u;
        return INFUR_OK;
    });
}

// ---- tuning database: infur_tuner.cpp ----

// ---- profiling ----
int32_t infur_profile_enable(infur_ctx* c, uint32_t on) {
    enter(c);
    if (!c) return INFUR_E_INVALID_ARG;
    c->opt.profile = on ? 1 : 0;
    return INFUR_OK;
}

int32_t infur_profile_count(infur_ctx* c, uint32_t* n) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !n) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *n = (uint32_t)c->prof.size();
        return INFUR_OK;
    });
}

int32_t infur_profile_get(infur_ctx* c, uint32_t i, infur_kernel_record* rec) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !rec || i >= c->prof.size()) return INFUR_E_INVALID_ARG;
        const ProfRec& r = c->prof[i];
        memset(rec, 0, sizeof *rec);
        snprintf(rec->name, sizeof rec->name, "%s", r.name.c_str());
        snprintf(rec->kernel, sizeof rec->kernel, "%s", r.kernel);
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, r.e0, r.e1));
        rec->ms = ms;
        rec->flops = r.flops;
        rec->bytes = r.bytes;
        rec->algo_flops = r.algo_flops;
        return INFUR_OK;
    });
}

int32_t infur_debug_profile_variant(infur_ctx* c, uint32_t i, char* buf, size_t cap) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !buf || !cap || i >= c->prof.size()) return INFUR_E_INVALID_ARG;
        const char* v = c->prof[i].variant ? c->prof[i].variant : "";
        if (strlen(v) >= cap) return fail(c, INFUR_E_CAPACITY, "variant tag needs %zu bytes", strlen(v) + 1);
        memcpy(buf, v, strlen(v) + 1);
        return INFUR_OK;
    });
}

// ---- device memory helpers ----
int32_t infur_dev_alloc(infur_ctx* c, size_t bytes, void** d) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !d) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipMalloc(d, bytes ? bytes : 1));
        return INFUR_OK;
    });
}
int32_t infur_dev_free(infur_ctx* c, void* d) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(d));
        return INFUR_OK;
    });
}
int32_t infur_memcpy_h2d(infur_ctx* c, void* d, const void* s, size_t n) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}
int32_t infur_memcpy_d2h(infur_ctx* c, void* d, const void* s, size_t n) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

}  // extern "C"

namespace infur {
void ctx_model_free(infur_ctx* c) { model_free(c); }
}  // namespace infur

#ifdef KTRACE
namespace infur { hipError_t ktrace_read(unsigned long long* out); }
extern "C" int32_t infur_debug_ktrace(unsigned long long* out) { return infur::ktrace_read(out) == hipSuccess ? 0 : 1; }
#endif
