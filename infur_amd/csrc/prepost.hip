// prepost.hip -- the HBM-bound, bit-exact stages either side of the conv stack.
// Compiled with -ffp-contract=off: every f32 expression here must round exactly like the
// CPU oracle's (oracle/infur_oracle.c), which in turn follows the reference's scalar Rust.
//
//   scale_bgr            Scale::advance resize           infur/src/processing.rs:246-278
//   pack_normalize       ImageSession::forward pre-proc  infur/src/predict_onnx.rs:103-137
//   upsample_planar      the model's final Resize(linear) node (inside session.run, :138)
//   colorcode_planar     ColorCode::advance              infur/src/decode_predict.rs:53-79
//   upsample_argmax_shade  fusion of the last two: reads the 2.7 MB output-stride-8 logits
//                        instead of writing + re-reading 174 MB of full-resolution logits.
#include "kernels.h"
#include "wave_scan.h"

namespace infur {

// ---------------------------------------------------------------------------------------
// Scale.  One thread per output pixel (3 bytes).  Source index rules are the oracle's:
//   nearest : src = trunc(0.5*s + s*dst) in f64, s = src_len/dst_len, clamp to src_len-1
//   bilinear: p = (dst+0.5)*s - 0.5 in f32 clamped to [0,src_len-1]; lerp x then y; round half up
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    scale_nearest_kernel(const uint8_t* __restrict__ in, int W, int H, uint8_t* __restrict__ out,
                         int OW, int OH) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= OW || y >= OH) return;
    const double sx = (double)W / (double)OW, sy = (double)H / (double)OH;
    const double px = sx * 0.5 + sx * (double)x;
    const double py = sy * 0.5 + sy * (double)y;
    unsigned ix = (unsigned)px, iy = (unsigned)py;
    if (ix > (unsigned)W - 1) ix = W - 1;
    if (iy > (unsigned)H - 1) iy = H - 1;
    const uint8_t* s = in + ((size_t)iy * W + ix) * 3;
    uint8_t* d = out + ((size_t)y * OW + x) * 3;
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
}

__device__ __forceinline__ void bilinear_coord(int i, int src, int dst, int& a, int& b, float& f) {
    const float scale = (float)src / (float)dst;
    float p = ((float)i + 0.5f) * scale - 0.5f;
    if (p < 0.0f) p = 0.0f;
    const float lim = (float)(src - 1);
    if (p > lim) p = lim;
    a = (int)p;
    b = a + 1 < src ? a + 1 : src - 1;
    f = p - (float)a;
}

__global__ void __launch_bounds__(256)
    scale_bilinear_kernel(const uint8_t* __restrict__ in, int W, int H, uint8_t* __restrict__ out,
                          int OW, int OH) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= OW || y >= OH) return;
    int x0, x1, y0, y1;
    float fx, fy;
    bilinear_coord(x, W, OW, x0, x1, fx);
    bilinear_coord(y, H, OH, y0, y1, fy);
    const uint8_t* r0 = in + (size_t)y0 * W * 3;
    const uint8_t* r1 = in + (size_t)y1 * W * 3;
    uint8_t* d = out + ((size_t)y * OW + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float p00 = r0[3 * x0 + c], p01 = r0[3 * x1 + c];
        const float p10 = r1[3 * x0 + c], p11 = r1[3 * x1 + c];
        const float top = p00 + (p01 - p00) * fx;
        const float bot = p10 + (p11 - p10) * fx;
        const float v = top + (bot - top) * fy;
        float r = floorf(v + 0.5f);
        r = fminf(fmaxf(r, 0.0f), 255.0f);
        d[c] = (uint8_t)r;
    }
}

hipError_t launch_scale_bgr(const uint8_t* in, int W, int H, uint8_t* out, int OW, int OH,
                            int mode, hipStream_t s) {
    dim3 grid((OW + 63) / 64, (OH + 3) / 4);
    if (mode == 0)
        hipLaunchKernelGGL(scale_nearest_kernel, grid, dim3(256), 0, s, in, W, H, out, OW, OH);
    else
        hipLaunchKernelGGL(scale_bilinear_kernel, grid, dim3(256), 0, s, in, W, H, out, OW, OH);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// pack_normalize: BGR u8 HWC -> RGB f32 CHW through the 3x256 LUT.  One thread = 4 pixels
// (12 input bytes as three aligned dwords, three float4 plane stores).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    pack_normalize_kernel(const uint8_t* __restrict__ bgr, size_t npix, const float* __restrict__ lut,
                          float* __restrict__ chw) {
    __shared__ float slut[768];
    for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
    __syncthreads();
    const size_t nquad = npix >> 2;
    const bool aligned = ((reinterpret_cast<uintptr_t>(bgr) | reinterpret_cast<uintptr_t>(chw)) & 15) == 0 &&
                         (npix & 3) == 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad + (aligned ? 0 : 1);
         q += (size_t)gridDim.x * 256) {
        if (aligned) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(bgr + q * 12);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
            // bytes: b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            float4 R, G, B;
            B.x = slut[512 + (w0 & 255)];
            G.x = slut[256 + ((w0 >> 8) & 255)];
            R.x = slut[(w0 >> 16) & 255];
            B.y = slut[512 + (w0 >> 24)];
            G.y = slut[256 + (w1 & 255)];
            R.y = slut[(w1 >> 8) & 255];
            B.z = slut[512 + ((w1 >> 16) & 255)];
            G.z = slut[256 + (w1 >> 24)];
            R.z = slut[w2 & 255];
            B.w = slut[512 + ((w2 >> 8) & 255)];
            G.w = slut[256 + ((w2 >> 16) & 255)];
            R.w = slut[w2 >> 24];
            *reinterpret_cast<float4*>(chw + q * 4) = R;
            *reinterpret_cast<float4*>(chw + npix + q * 4) = G;
            *reinterpret_cast<float4*>(chw + 2 * npix + q * 4) = B;
        } else {
            // ragged / unaligned sizes: same values, scalar accesses
            const size_t lo = q * 4, hi = lo + 4 < npix ? lo + 4 : npix;
            for (size_t i = lo; i < hi; i++) {
                chw[i] = slut[bgr[3 * i + 2]];
                chw[npix + i] = slut[256 + bgr[3 * i + 1]];
                chw[2 * npix + i] = slut[512 + bgr[3 * i + 0]];
            }
        }
    }
}

hipError_t launch_pack_normalize(const uint8_t* bgr, int W, int H, const float* lut, float* chw,
                                 hipStream_t s) {
    const size_t npix = (size_t)W * H;
    size_t blocks = (npix / 4 + 256) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pack_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bgr, npix, lut, chw);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// display conversion of the (scaled) frame, infur/src/app.rs:132-144:
// Color32::from_rgb(cs[2], cs[1], cs[0]) per pixel -> [r, g, b, 255].  4 pixels per thread.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    bgr_to_rgba_kernel(const uint8_t* __restrict__ bgr, size_t npix, uint32_t* __restrict__ rgba) {
    const size_t nquad = npix >> 2;
    const bool aligned = ((reinterpret_cast<uintptr_t>(bgr) & 3) | (reinterpret_cast<uintptr_t>(rgba) & 15)) == 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad + 1; q += (size_t)gridDim.x * 256) {
        if (aligned && q < nquad) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(bgr + q * 12);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];  // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            uint4 o;
            o.x = 0xff000000u | ((w0 & 0xffu) << 16) | (w0 & 0xff00u) | ((w0 >> 16) & 0xffu);
            o.y = 0xff000000u | ((w0 >> 24) << 16) | ((w1 & 0xffu) << 8) | ((w1 >> 8) & 0xffu);
            o.z = 0xff000000u | (((w1 >> 16) & 0xffu) << 16) | ((w1 >> 24) << 8) | (w2 & 0xffu);
            o.w = 0xff000000u | (((w2 >> 8) & 0xffu) << 16) | (((w2 >> 16) & 0xffu) << 8) | (w2 >> 24);
            *reinterpret_cast<uint4*>(rgba + q * 4) = o;
        } else {
            const size_t lo = q * 4, hi = lo + 4 < npix ? lo + 4 : npix;
            for (size_t i = lo; i < hi; i++)
                rgba[i] = 0xff000000u | ((uint32_t)bgr[3 * i] << 16) | ((uint32_t)bgr[3 * i + 1] << 8) | bgr[3 * i + 2];
        }
    }
}

hipError_t launch_bgr_to_rgba(const uint8_t* bgr, int W, int H, uint32_t* rgba, hipStream_t s) {
    const size_t npix = (size_t)W * H;
    size_t blocks = (npix / 4 + 256) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bgr_to_rgba_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bgr, npix, rgba);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// NHWC -> planar f32 (low-res logits: 21 x 135 x 240 floats; debug read-back of activations)
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void nhwc_to_planar_kernel(const T* __restrict__ in, int HW, int C, float* __restrict__ out) {
    const size_t total = (size_t)HW * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i / HW);
        const size_t p = i - (size_t)c * HW;
        out[i] = (float)in[p * C + c];
    }
}

hipError_t launch_nhwc_to_planar(const void* in, int f16, int H, int W, int C, float* out, hipStream_t s) {
    const size_t total = (size_t)H * W * C;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (f16)
        hipLaunchKernelGGL(nhwc_to_planar_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, (const _Float16*)in, H * W, C, out);
    else
        hipLaunchKernelGGL(nhwc_to_planar_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)in, H * W, C, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Bilinear up-sample.  Coordinates follow the oracle's upsample_table():
//   scale = out_len/in_len; src = out_len > 1 ? (dst+0.5)/scale - 0.5 : 0; clamp [0,in_len-1]
//   i1 = trunc(src), i2 = min(i1+1, in_len-1); d1 = |src-i1|, d2 = |src-i2| (0.5/0.5 if i1==i2)
//   v = dx2*dy2*X11 + dx1*dy2*X21 + dx2*dy1*X12 + dx1*dy1*X22  (left to right, no FMA)
// HIP's f32 division is correctly rounded by default (no -ffast-math here), so the
// coordinates match the host's bit for bit.
// ---------------------------------------------------------------------------------------
struct Lerp {
    int i1, i2;
    float d1, d2;
};

__device__ __forceinline__ Lerp lerp_coord(int i, int in_len, int out_len) {
    const float scale = (float)out_len / (float)in_len;
    float src = out_len > 1 ? ((float)i + 0.5f) / scale - 0.5f : 0.0f;
    if (src < 0.0f) src = 0.0f;
    const float lim = (float)(in_len - 1);
    if (src > lim) src = lim;
    Lerp t;
    t.i1 = (int)src;
    if (t.i1 > in_len - 1) t.i1 = in_len - 1;
    t.i2 = t.i1 + 1 < in_len ? t.i1 + 1 : in_len - 1;
    if (t.i1 == t.i2) {
        t.d1 = 0.5f;
        t.d2 = 0.5f;
    } else {
        t.d1 = fabsf(src - (float)t.i1);
        t.d2 = fabsf(src - (float)t.i2);
    }
    return t;
}

__device__ __forceinline__ float bilerp(float X11, float X21, float X12, float X22, float dx1,
                                        float dx2, float dy1, float dy2) {
    float v = dx2 * dy2 * X11;
    v = v + dx1 * dy2 * X21;
    v = v + dx2 * dy1 * X12;
    v = v + dx1 * dy1 * X22;
    return v;
}

// Quantised models whose file resizes the u8 logits BEFORE it dequantises them (QLinearConv -> Resize -> DequantizeLinear, what
// onnxruntime's QOperator quantiser writes when Resize is on its list): the low-res tensor then holds the u8 CODES as floats, the
// interpolation is ONNX Runtime's UpsampleBilinear<uint8_t> -- the float expression above, static_cast to uint8_t = truncation --
// and DequantizeLinear follows per output value: (trunc(v) - zp) * scale.  on == 0: the interpolated value itself.
__device__ __forceinline__ float up_post(const float v, const UpQuant q) { return q.on ? (truncf(v) - q.zp) * q.scale : v; }

// one thread per output pixel, loops over classes; writes planar [K][OH][OW]
__global__ void __launch_bounds__(256)
    upsample_planar_kernel(const float* __restrict__ low, int LH, int LW, int K, float* __restrict__ out,
                           int OH, int OW, const UpQuant uq) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= OW || y >= OH) return;
    const Lerp tx = lerp_coord(x, LW, OW), ty = lerp_coord(y, LH, OH);
    const float* p11 = low + ((size_t)ty.i1 * LW + tx.i1) * K;
    const float* p21 = low + ((size_t)ty.i1 * LW + tx.i2) * K;
    const float* p12 = low + ((size_t)ty.i2 * LW + tx.i1) * K;
    const float* p22 = low + ((size_t)ty.i2 * LW + tx.i2) * K;
    const size_t plane = (size_t)OH * OW;
    float* o = out + (size_t)y * OW + x;
    for (int k = 0; k < K; k++)
        o[k * plane] = up_post(bilerp(p11[k], p21[k], p12[k], p22[k], tx.d1, tx.d2, ty.d1, ty.d2), uq);
}


// ---------------------------------------------------------------------------------------
// ColorCode.  decode_predict.rs:67-78: k_max = 0, c_max = 0.0, strict '>' in class order;
// alpha = (c_max * 255.0) as u8 (saturating, truncating); colour = LUT[k_max % 20][alpha]
// where the LUT holds epaint's premultiplied bytes (built on the host, infur_capi.cpp).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t shade(int k_max, float c_max, const uint32_t* __restrict__ lut) {
    const float a = c_max * 255.0f;            // c_max >= 0 and never NaN by construction
    const int ai = a >= 255.0f ? 255 : (int)a;  // Rust `as u8`: saturate, truncate
    return lut[(k_max % 20) * 256 + ai];
}

__global__ void __launch_bounds__(256)
    colorcode_planar_kernel(const float* __restrict__ khw, int K, size_t HW, const uint32_t* __restrict__ lut,
                            uint32_t* __restrict__ rgba) {
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
        int k_max = 0;
        float c_max = 0.0f;
        for (int k = 0; k < K; k++) {
            const float c = khw[(size_t)k * HW + p];
            if (c > c_max) {
                k_max = k;
                c_max = c;
            }
        }
        rgba[p] = shade(k_max, c_max, lut);
    }
}

hipError_t launch_colorcode_planar(const float* khw, int K, int H, int W, const uint32_t* lut,
                                   uint32_t* rgba, hipStream_t s) {
    const size_t HW = (size_t)H * W;
    size_t blocks = (HW + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(colorcode_planar_kernel, dim3((unsigned)blocks), dim3(256), 0, s, khw, K, HW, lut, rgba);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// LDS-staged forms of the two up-sampling kernels (the ones that run: the scalar kernels above / below are the
// fallback for class counts > 24 or down-sampling ratios whose footprint does not fit).
//
// A workgroup owns a 64 x 8 tile of OUTPUT pixels.  Bilinear source indices are monotone in the output index, so
// the low-res pixels the tile can touch are the rectangle [i1(first row/col) .. i2(last row/col)]: at the network's
// stride-8 ratio 10 x 3 pixels x 21 classes = 2.5 KB.  The rectangle is staged ONCE, coalesced (a low-res row
// segment is contiguous in NHWC), into LDS as [pixel][24 floats]; every output pixel then reads its four
// neighbours as 6 ds_read_b128 each instead of 84 scalar global loads at stride 21 (the round-1 kernel:
// 331 GB/s, 5.7x the algorithmic HBM reads).  Same expression tree per class, same class order, strict '>' --
// bit-identical to upsample_planar -> colorcode_planar (tests/test_gpu_parity.py).
// ---------------------------------------------------------------------------------------
constexpr int UP_TW = 64, UP_TH = 16, UP_KP = 24;

struct UpTile {
    int r0, c0, nc;
    const Lerp* tx;  // [UP_TW] column coordinates of the tile (LDS)
    const Lerp* ty;  // [UP_TH] row coordinates
    float* pix;      // staged low-res pixels [rows][nc][UP_KP]
};

// The coordinate of every output column / row of the tile is computed ONCE (its two correctly rounded f32 divisions
// are ~25 instructions each) and shared through LDS; staging maps threads as (pixel, class) so it needs no integer
// division, and issues all of a thread's loads before the first LDS store.
__device__ __forceinline__ UpTile stage_lowres_tile(const float* __restrict__ low, int LH, int LW, int K, int OH, int OW,
                                                    float* __restrict__ smem) {
    Lerp* tx = reinterpret_cast<Lerp*>(smem);
    Lerp* ty = tx + UP_TW;
    float* tile = smem + (UP_TW + UP_TH) * (sizeof(Lerp) / sizeof(float));
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * UP_TW, y0 = blockIdx.y * UP_TH;
    if (tid < UP_TW)
        tx[tid] = lerp_coord(min(x0 + tid, OW - 1), LW, OW);
    else if (tid < UP_TW + UP_TH)
        ty[tid - UP_TW] = lerp_coord(min(y0 + tid - UP_TW, OH - 1), LH, OH);
    __syncthreads();
    UpTile t;
    t.tx = tx;
    t.ty = ty;
    t.pix = tile;
    t.c0 = tx[0].i1;
    t.r0 = ty[0].i1;
    t.nc = tx[UP_TW - 1].i2 - t.c0 + 1;  // source indices are monotone: the last column / row bound the rectangle
    const int np = (ty[UP_TH - 1].i2 - t.r0 + 1) * t.nc;
    const int k = tid & 31, pl = tid >> 5;  // 8 low-res pixels per pass, lanes along the classes
    for (int base = 0; base < np; base += 32) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int p = base + 8 * u + pl;
            const int r = p / t.nc, c = p - r * t.nc;  // (nc is small: this is the only division left, once per 8 pixels)
            v[u] = (p < np && k < K) ? low[((size_t)(t.r0 + r) * LW + t.c0 + c) * K + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int p = base + 8 * u + pl;
            if (p < np && k < UP_KP) tile[p * UP_KP + k] = v[u];
        }
    }
    __syncthreads();
    return t;
}

// Both kernels: a wave owns FOUR CONSECUTIVE output rows of the tile.  At the network's 8x ratio consecutive rows
// nearly always share their pair of source rows, so the 4 x NQ neighbour quads (ds_read_b128) stay in registers and are
// re-read only when the (wave-uniform) row pair changes: a quarter of the LDS traffic of the round-2 first form.  NQ =
// ceil(K / 4) is a template argument and every quad is evaluated whole -- the pad classes of a staged slot are zeros,
// their value is +0 and can never pass the strict '>' against c_max >= 0 -- so the body is straight-line code (the
// run-time `k < K` guards of the first form compiled to ds_read_b32 + a branch per class: 22 us at 1080p).  Class pairs
// go through 2-vectors so that the multiplies AND the adds are v_pk_*_f32; per class the expression tree is unchanged.
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int NQ>
__device__ __forceinline__ void load_quads(const float* ra, const float* rb, int ca, int cb, float4 (&v11)[NQ],
                                           float4 (&v21)[NQ], float4 (&v12)[NQ], float4 (&v22)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        v11[q] = *reinterpret_cast<const float4*>(ra + ca + 4 * q);
        v21[q] = *reinterpret_cast<const float4*>(ra + cb + 4 * q);
        v12[q] = *reinterpret_cast<const float4*>(rb + ca + 4 * q);
        v22[q] = *reinterpret_cast<const float4*>(rb + cb + 4 * q);
    }
}

// classes (k, k+1) of one pixel: ((w11*X11 + w21*X21) + w12*X12) + w22*X22 with w11 = dx2*dy2 ... exactly bilerp()
__device__ __forceinline__ f32x2 bilerp2(f32x2 X11, f32x2 X21, f32x2 X12, f32x2 X22, float w11, float w21, float w12,
                                         float w22) {
    f32x2 v = w11 * X11;
    v = v + w21 * X21;
    v = v + w12 * X12;
    v = v + w22 * X22;
    return v;
}

template <int NQ>
__global__ void __launch_bounds__(256)
    upsample_argmax_shade_lds_kernel(const float* __restrict__ low, int LH, int LW, int K,
                                     const uint32_t* __restrict__ lut, uint32_t* __restrict__ rgba, int OH, int OW, const UpQuant uq) {
    extern __shared__ __attribute__((aligned(16))) float up_smem[];
    const UpTile t = stage_lowres_tile(low, LH, LW, K, OH, OW, up_smem);
    const int xl = threadIdx.x & 63;
    const int x = blockIdx.x * UP_TW + xl;
    if (x >= OW) return;
    const Lerp tx = t.tx[xl];
    const int ca = (tx.i1 - t.c0) * UP_KP, cb = (tx.i2 - t.c0) * UP_KP;
    float4 v11[NQ], v21[NQ], v12[NQ], v22[NQ];
    int pi1 = -1, pi2 = -1;
#pragma unroll
    for (int rr = 0; rr < UP_TH / 4; rr++) {
        const int yl = 4 * (threadIdx.x >> 6) + rr;
        const int y = blockIdx.y * UP_TH + yl;
        if (y >= OH) break;
        const Lerp ty = t.ty[yl];
        const int i1 = __builtin_amdgcn_readfirstlane(ty.i1), i2 = __builtin_amdgcn_readfirstlane(ty.i2);
        if (i1 != pi1 || i2 != pi2) {
            load_quads<NQ>(t.pix + (i1 - t.r0) * t.nc * UP_KP, t.pix + (i2 - t.r0) * t.nc * UP_KP, ca, cb, v11, v21, v12, v22);
            pi1 = i1;
            pi2 = i2;
        }
        const float w11 = tx.d2 * ty.d2, w21 = tx.d1 * ty.d2, w12 = tx.d2 * ty.d1, w22 = tx.d1 * ty.d1;
        int k_max = 0;
        float c_max = 0.0f;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const f32x2 lo = bilerp2(f32x2{v11[q].x, v11[q].y}, f32x2{v21[q].x, v21[q].y}, f32x2{v12[q].x, v12[q].y},
                                     f32x2{v22[q].x, v22[q].y}, w11, w21, w12, w22);
            const f32x2 hi = bilerp2(f32x2{v11[q].z, v11[q].w}, f32x2{v21[q].z, v21[q].w}, f32x2{v12[q].z, v12[q].w},
                                     f32x2{v22[q].z, v22[q].w}, w11, w21, w12, w22);
            const float c[4] = {up_post(lo.x, uq), up_post(lo.y, uq), up_post(hi.x, uq), up_post(hi.y, uq)};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (c[e] > c_max) {
                    k_max = 4 * q + e;
                    c_max = c[e];
                }
            }
        }
        rgba[(size_t)y * OW + x] = shade(k_max, c_max, lut);
    }
}

template <int NQ>
__global__ void __launch_bounds__(256)
    upsample_planar_lds_kernel(const float* __restrict__ low, int LH, int LW, int K, float* __restrict__ out, int OH, int OW, const UpQuant uq) {
    extern __shared__ __attribute__((aligned(16))) float up_smem[];
    const UpTile t = stage_lowres_tile(low, LH, LW, K, OH, OW, up_smem);
    const int xl = threadIdx.x & 63;
    const int x = blockIdx.x * UP_TW + xl;
    if (x >= OW) return;
    const Lerp tx = t.tx[xl];
    const int ca = (tx.i1 - t.c0) * UP_KP, cb = (tx.i2 - t.c0) * UP_KP;
    const size_t plane = (size_t)OH * OW;
    float4 v11[NQ], v21[NQ], v12[NQ], v22[NQ];
    int pi1 = -1, pi2 = -1;
#pragma unroll
    for (int rr = 0; rr < UP_TH / 4; rr++) {
        const int yl = 4 * (threadIdx.x >> 6) + rr;
        const int y = blockIdx.y * UP_TH + yl;
        if (y >= OH) break;
        const Lerp ty = t.ty[yl];
        const int i1 = __builtin_amdgcn_readfirstlane(ty.i1), i2 = __builtin_amdgcn_readfirstlane(ty.i2);
        if (i1 != pi1 || i2 != pi2) {
            load_quads<NQ>(t.pix + (i1 - t.r0) * t.nc * UP_KP, t.pix + (i2 - t.r0) * t.nc * UP_KP, ca, cb, v11, v21, v12, v22);
            pi1 = i1;
            pi2 = i2;
        }
        const float w11 = tx.d2 * ty.d2, w21 = tx.d1 * ty.d2, w12 = tx.d2 * ty.d1, w22 = tx.d1 * ty.d1;
        float* o = out + (size_t)y * OW + x;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const f32x2 lo = bilerp2(f32x2{v11[q].x, v11[q].y}, f32x2{v21[q].x, v21[q].y}, f32x2{v12[q].x, v12[q].y},
                                     f32x2{v22[q].x, v22[q].y}, w11, w21, w12, w22);
            const f32x2 hi = bilerp2(f32x2{v11[q].z, v11[q].w}, f32x2{v21[q].z, v21[q].w}, f32x2{v12[q].z, v12[q].w},
                                     f32x2{v22[q].z, v22[q].w}, w11, w21, w12, w22);
            const float c[4] = {up_post(lo.x, uq), up_post(lo.y, uq), up_post(hi.x, uq), up_post(hi.y, uq)};
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (4 * q + e < K) o[(size_t)(4 * q + e) * plane] = c[e];
        }
    }
}

// LDS bytes of the staged rectangle for this geometry, or 0 when the scalar fallback must run (more classes than
// the padded pixel slot holds, or a ratio whose footprint is too big to be worth staging)
static size_t up_tile_lds_bytes(int LH, int LW, int K, int OH, int OW) {
    if (K > UP_KP || K <= 0 || OH <= 0 || OW <= 0) return 0;
    const size_t cols = (size_t)(((long long)UP_TW * LW + OW - 1) / OW) + 3;
    const size_t rows = (size_t)(((long long)UP_TH * LH + OH - 1) / OH) + 3;
    const size_t bytes = (UP_TW + UP_TH) * sizeof(Lerp) + rows * cols * UP_KP * sizeof(float);
    return bytes <= 48 * 1024 ? bytes : 0;
}

// The launch of an up-sampling kernel pair, written once for the three launchers (LH, LW, K, OH, OW and s are theirs): the
// staged kernel's NQ = ceil(K / 4) instantiation on the tile grid where the footprint fits (K <= UP_KP = 24 is checked by
// up_tile_lds_bytes), else the scalar kernel on its 64 x 4 grid
#define UP_LAUNCH(STAGED, SCALAR, ...)                                                                           \
    do {                                                                                                         \
        const size_t lds = up_tile_lds_bytes(LH, LW, K, OH, OW);                                                 \
        const dim3 tiles((OW + UP_TW - 1) / UP_TW, (OH + UP_TH - 1) / UP_TH), rows((OW + 63) / 64, (OH + 3) / 4); \
        switch (lds ? (K + 3) / 4 : 0) {                                                                         \
            case 0: hipLaunchKernelGGL(SCALAR, rows, dim3(256), 0, s, __VA_ARGS__); break;                       \
            case 1: hipLaunchKernelGGL(STAGED<1>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                 \
            case 2: hipLaunchKernelGGL(STAGED<2>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                 \
            case 3: hipLaunchKernelGGL(STAGED<3>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                 \
            case 4: hipLaunchKernelGGL(STAGED<4>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                 \
            case 5: hipLaunchKernelGGL(STAGED<5>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                 \
            default: hipLaunchKernelGGL(STAGED<6>, tiles, dim3(256), lds, s, __VA_ARGS__); break;                \
        }                                                                                                        \
        return hipGetLastError();                                                                                \
    } while (0)

hipError_t launch_upsample_planar(const float* low, int LH, int LW, int K, float* out, int OH,
                                  int OW, hipStream_t s, const UpQuant uq) {
    UP_LAUNCH(upsample_planar_lds_kernel, upsample_planar_kernel, low, LH, LW, K, out, OH, OW, uq);
}

// fused up-sample + argmax + shade, scalar form: same expression tree as upsample_planar -> colorcode
__global__ void __launch_bounds__(256)
    upsample_argmax_shade_kernel(const float* __restrict__ low, int LH, int LW, int K,
                                 const uint32_t* __restrict__ lut, uint32_t* __restrict__ rgba, int OH, int OW, const UpQuant uq) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= OW || y >= OH) return;
    const Lerp tx = lerp_coord(x, LW, OW), ty = lerp_coord(y, LH, OH);
    const float* p11 = low + ((size_t)ty.i1 * LW + tx.i1) * K;
    const float* p21 = low + ((size_t)ty.i1 * LW + tx.i2) * K;
    const float* p12 = low + ((size_t)ty.i2 * LW + tx.i1) * K;
    const float* p22 = low + ((size_t)ty.i2 * LW + tx.i2) * K;
    int k_max = 0;
    float c_max = 0.0f;
    for (int k = 0; k < K; k++) {
        const float c = up_post(bilerp(p11[k], p21[k], p12[k], p22[k], tx.d1, tx.d2, ty.d1, ty.d2), uq);
        if (c > c_max) {
            k_max = k;
            c_max = c;
        }
    }
    rgba[(size_t)y * OW + x] = shade(k_max, c_max, lut);
}

hipError_t launch_upsample_argmax_shade(const float* low, int LH, int LW, int K, const uint32_t* lut,
                                        uint32_t* rgba, int OH, int OW, hipStream_t s, const UpQuant uq) {
    UP_LAUNCH(upsample_argmax_shade_lds_kernel, upsample_argmax_shade_kernel, low, LH, LW, K, lut, rgba, OH, OW, uq);
}

// ---------------------------------------------------------------------------------------
// Segments: ColorCode's sibling for a headless host (the reference's own todo list, README.md:76-77: "softmax if model
// predictions are logits", "class label captions").  Per pixel it produces any subset of
//   class byte k_max | confidence byte | premultiplied RGBA LUT[k_max % 20][conf] | per-class statistics
// in one of two decodes (include/infur_hip.h):
//   RAW      decode_predict.rs:67-78 as shade() above: k_max = 0, c_max = 0.0, strict '>', conf = (c_max * 255) as u8
//   SOFTMAX  the same loop from c_max = -inf (negative logits are legitimate maxima; NaN never wins, the first maximum wins),
//            conf = (p * 255) as u8 with p = 1 / sum_k exp(c_k - c_max) in f32 over the K real classes, NaN terms counting 0;
//            nothing won (all NaN / -inf): class 0, conf 0; c_max = +inf: conf 255
// Three kernels -- fused + LDS-staged, fused scalar fallback, unfused planar -- share seg_decode() and the statistics code, so
// they agree bit for bit.  All three keep a wave on ONE output row (lane = column): y is wave-uniform.
// ---------------------------------------------------------------------------------------
struct SegPix {
    int k, conf;
};

// `cls(k)` is the class value; it is called twice per class in the SOFTMAX decode.  n is a compile-time constant in the staged
// kernel (the loops unroll over registers; its pad classes arrive as -inf, which neither wins nor adds to the sum).
template <class F>
__device__ __forceinline__ SegPix seg_decode(const int n, const int softmax, F&& cls) {
    int k_max = 0;
    float c_max = softmax ? -__builtin_inff() : 0.0f;
#pragma unroll
    for (int k = 0; k < n; k++) {
        const float c = cls(k);
        if (c > c_max) {
            k_max = k;
            c_max = c;
        }
    }
    SegPix r;
    r.k = k_max;
    if (!softmax) {
        const float a = c_max * 255.0f;
        r.conf = a >= 255.0f ? 255 : (int)a;  // Rust `as u8`: saturate, truncate
        return r;
    }
    // exp(d) as exp2(d * log2 e) on v_exp_f32 (1 ulp): with the product's rounding, |d| * 2^-24 relative per term
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < n; k++) {
        const float e = __builtin_amdgcn_exp2f((cls(k) - c_max) * 1.44269504088896341f);
        s = s + (e == e ? e : 0.0f);  // NaN class, or inf - inf under an infinite maximum: no contribution
    }
    const float a = (1.0f / s) * 255.0f;  // finite maximum: its own term is exp2(0) = 1, so s >= 1 and a <= 255
    r.conf = c_max == __builtin_inff() ? 255 : (c_max == -__builtin_inff() ? 0 : (int)a);
    return r;
}

// ---- per-class statistics ----
// Per workgroup an LDS table [class][8] of u32: PIXELS, SUM_X, SUM_Y, SUM_CONF (added), ~MIN_X, ~MIN_Y, MAX_X, MAX_Y (all four
// by max: a minimum is kept as the maximum of the complement, so a zeroed table is the empty one and one ds_max serves both).
// Classes are spatially coherent and a wave is 64 consecutive columns of one row, so a wave-row is folded class by class:
// readlane of the first unfinished lane's class, ballot of equality, and then everything comes out of the 64-bit mask with
// scalar bit operations -- count (popcount), min / max x (ctz / clz), sum x (popcounts of the mask under the six bit-position
// masks).  Sum conf needs no cross-lane adds either: the eight ballots of the confidence's bit planes, taken once per row,
// give sum = sum_b 2^b * popcount(mask & plane_b).  Lanes 0-7 then apply one word each: two LDS instructions per class.
__device__ __forceinline__ unsigned seg_bit_positions(const uint64_t m) {
    return (unsigned)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (unsigned)__popcll(m & 0xCCCCCCCCCCCCCCCCull) +
           4u * (unsigned)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (unsigned)__popcll(m & 0xFF00FF00FF00FF00ull) +
           16u * (unsigned)__popcll(m & 0xFFFF0000FFFF0000ull) + 32u * (unsigned)__popcll(m & 0xFFFFFFFF00000000ull);
}

__device__ __forceinline__ void seg_row_stats(unsigned* __restrict__ sstat, const bool live, const int k, const int conf,
                                              const unsigned x0, const unsigned y) {
    uint64_t todo = __ballot(live);
    if (!todo) return;
    const BitPlanes8 planes((unsigned)conf, live);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int kc = __builtin_amdgcn_readlane(k, __builtin_ctzll(todo));
        const uint64_t m = __ballot(live && k == kc);
        todo &= ~m;
        const unsigned n = (unsigned)__popcll(m);
        const unsigned sconf = planes.sum(m);
        const unsigned lo = x0 + (unsigned)__builtin_ctzll(m), hi = x0 + 63u - (unsigned)__builtin_clzll(m);
        const unsigned word[8] = {n, n * x0 + seg_bit_positions(m), n * y, sconf, ~lo, ~y, hi, y};
        unsigned v = word[0];
#pragma unroll
        for (int i = 1; i < 8; i++) v = lane == i ? word[i] : v;
        if (lane < 4)
            atomicAdd(&sstat[kc * 8 + lane], v);
        else if (lane < 8)
            atomicMax(&sstat[kc * 8 + lane], v);
    }
}

// One atomic per word and workgroup, and only for the classes the workgroup saw, into one of kSegShards copies of the table:
// at 1080p ~2,000 workgroups nearly all hold the dominant class, and one contended word serialises at L2 (~88 returning
// atomics / us) -- sixteen shards of non-returning 64-bit atomics keep that off the kernel's tail.
__device__ __forceinline__ void seg_flush_stats(const unsigned* __restrict__ sstat, const int K, unsigned long long* __restrict__ shards) {
    __syncthreads();
    unsigned long long* g = shards + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) % kSegShards) * K * 8;
    for (int i = threadIdx.x; i < K * 8; i += 256) {
        if (sstat[i & ~7] == 0) continue;
        const unsigned long long v = sstat[i];
        if ((i & 7) < 4)
            atomicAdd(g + i, v);
        else
            atomicMax(g + i, v);
    }
}

// shards -> the caller's K x 8 table, with the empty-class values (MIN_* = UINT64_MAX, everything else 0)
__global__ void __launch_bounds__(256) segments_stats_finalize_kernel(const unsigned long long* __restrict__ shards, int K,
                                                                      unsigned long long* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * 8) return;
    const int w = i & 7;
    unsigned long long acc = 0, n = 0;
    for (int s = 0; s < kSegShards; s++) {
        const unsigned long long v = shards[(size_t)s * K * 8 + i];
        n += shards[(size_t)s * K * 8 + (i & ~7)];
        acc = w < 4 ? acc + v : (v > acc ? v : acc);
    }
    if (w == 4 || w == 5) acc = n ? 0xFFFFFFFFull - acc : ~0ull;
    stats[i] = acc;
}

hipError_t launch_segments_stats_finalize(const unsigned long long* shards, int K, unsigned long long* stats, hipStream_t s) {
    if (K <= 0) return hipSuccess;
    hipLaunchKernelGGL(segments_stats_finalize_kernel, dim3((K * 8 + 255) / 256), dim3(256), 0, s, shards, K, stats);
    return hipGetLastError();
}

__device__ __forceinline__ void seg_store_pixel(const SegOut& o, const uint32_t* __restrict__ lut, const SegPix p, const size_t at) {
    if (o.klass) o.klass[at] = (uint8_t)p.k;
    if (o.conf) o.conf[at] = (uint8_t)p.conf;
    if (o.rgba) o.rgba[at] = lut[(p.k % 20) * 256 + p.conf];
}

// unfused: planar [K][H][W] confidences, as colorcode_planar reads them.  Workgroup = 64 columns x 4 rows, one row per wave.
__global__ void __launch_bounds__(256)
    segments_planar_kernel(const float* __restrict__ khw, int K, int H, int W, int softmax, const uint32_t* __restrict__ lut,
                           const SegOut o) {
    __shared__ unsigned sstat[kSegMaxClasses * 8];
    if (o.shards) {
        for (int i = threadIdx.x; i < K * 8; i += 256) sstat[i] = 0;
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool live = x < W && y < H;
    SegPix p = {0, 0};
    if (live) {
        const size_t HW = (size_t)H * W, at = (size_t)y * W + x;
        p = seg_decode(K, softmax, [&](int k) { return khw[(size_t)k * HW + at]; });
        seg_store_pixel(o, lut, p, at);
    }
    if (o.shards) {
        seg_row_stats(sstat, live, p.k, p.conf, blockIdx.x * 64, y);
        seg_flush_stats(sstat, K, o.shards);
    }
}

hipError_t launch_segments_planar(const float* khw, int K, int H, int W, int softmax, const uint32_t* lut, const SegOut& o,
                                  hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(segments_planar_kernel, grid, dim3(256), 0, s, khw, K, H, W, softmax, lut, o);
    return hipGetLastError();
}

// fused, scalar form (more classes than a staged slot holds, or a ratio that is not staged): upsample_argmax_shade_kernel's loop
__global__ void __launch_bounds__(256)
    upsample_argmax_segments_kernel(const float* __restrict__ low, int LH, int LW, int K, int softmax,
                                    const uint32_t* __restrict__ lut, const SegOut o, int OH, int OW, const UpQuant uq) {
    __shared__ unsigned sstat[kSegMaxClasses * 8];
    if (o.shards) {
        for (int i = threadIdx.x; i < K * 8; i += 256) sstat[i] = 0;
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool live = x < OW && y < OH;
    SegPix p = {0, 0};
    if (live) {
        const Lerp tx = lerp_coord(x, LW, OW), ty = lerp_coord(y, LH, OH);
        const float* p11 = low + ((size_t)ty.i1 * LW + tx.i1) * K;
        const float* p21 = low + ((size_t)ty.i1 * LW + tx.i2) * K;
        const float* p12 = low + ((size_t)ty.i2 * LW + tx.i1) * K;
        const float* p22 = low + ((size_t)ty.i2 * LW + tx.i2) * K;
        p = seg_decode(K, softmax, [&](int k) { return up_post(bilerp(p11[k], p21[k], p12[k], p22[k], tx.d1, tx.d2, ty.d1, ty.d2), uq); });
        seg_store_pixel(o, lut, p, (size_t)y * OW + x);
    }
    if (o.shards) {
        seg_row_stats(sstat, live, p.k, p.conf, blockIdx.x * 64, y);
        seg_flush_stats(sstat, K, o.shards);
    }
}

// A lane of the staged kernel owns one column and FOUR rows, so its four class (or confidence) bytes are one register and a
// wave's natural store would be 64 single bytes per row.  Instead the 4 x 4 bytes of four neighbouring lanes are transposed
// with four quad-broadcast DPP moves: lane j of a quad ends up with row j's four columns and the wave stores 64 dwords
// (16 per row) in one instruction.  Needs OW % 4 == 0 and a dword-aligned plane (then a quad is live or dead as a whole);
// other shapes store bytes.
__device__ __forceinline__ void seg_store_rows4(uint8_t* __restrict__ plane, const uint32_t mine, const bool dwords, const bool live,
                                                const int x, const int y0, const int OH, const int OW) {
    if (!plane) return;
    if (dwords) {
        const uint32_t q0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x00, 0xf, 0xf, false);
        const uint32_t q1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x55, 0xf, 0xf, false);
        const uint32_t q2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xAA, 0xf, 0xf, false);
        const uint32_t q3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xFF, 0xf, 0xf, false);
        const int j = x & 3, sh = 8 * j;
        const uint32_t row = ((q0 >> sh) & 255u) | (((q1 >> sh) & 255u) << 8) | (((q2 >> sh) & 255u) << 16) | ((q3 >> sh) << 24);
        if (live && y0 + j < OH) *reinterpret_cast<uint32_t*>(plane + (size_t)(y0 + j) * OW + (x & ~3)) = row;
    } else if (live) {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (y0 + r < OH) plane[(size_t)(y0 + r) * OW + x] = (uint8_t)(mine >> (8 * r));
    }
}

// fused, LDS-staged: upsample_argmax_shade_lds_kernel's staging, register quads and expression tree; the decode and the
// outputs differ.  No lane leaves early (the statistics end in a barrier): columns beyond OW compute on clamped coordinates
// and are masked at the stores and in the ballots.
template <int NQ>
__global__ void __launch_bounds__(256)
    upsample_argmax_segments_lds_kernel(const float* __restrict__ low, int LH, int LW, int K, int softmax,
                                        const uint32_t* __restrict__ lut, const SegOut o, int OH, int OW, const UpQuant uq) {
    static_assert(UP_TH / 4 == 4, "a lane's rows are packed into one dword");
    extern __shared__ __attribute__((aligned(16))) float up_smem[];
    __shared__ unsigned sstat[UP_KP * 8];
    if (o.shards && threadIdx.x < UP_KP * 8) sstat[threadIdx.x] = 0;  // (published by the barriers of the staging)
    const UpTile t = stage_lowres_tile(low, LH, LW, K, OH, OW, up_smem);
    const int xl = threadIdx.x & 63;
    const int x = blockIdx.x * UP_TW + xl;
    const bool live = x < OW;
    const Lerp tx = t.tx[xl];
    const int ca = (tx.i1 - t.c0) * UP_KP, cb = (tx.i2 - t.c0) * UP_KP;
    float4 v11[NQ], v21[NQ], v12[NQ], v22[NQ];
    int pi1 = -1, pi2 = -1;
    const int y0 = blockIdx.y * UP_TH + 4 * (threadIdx.x >> 6);
    uint32_t kpack = 0, cpack = 0;
#pragma unroll
    for (int rr = 0; rr < UP_TH / 4; rr++) {
        const int y = y0 + rr;
        if (y >= OH) break;
        const Lerp ty = t.ty[y - blockIdx.y * UP_TH];
        const int i1 = __builtin_amdgcn_readfirstlane(ty.i1), i2 = __builtin_amdgcn_readfirstlane(ty.i2);
        if (i1 != pi1 || i2 != pi2) {
            load_quads<NQ>(t.pix + (i1 - t.r0) * t.nc * UP_KP, t.pix + (i2 - t.r0) * t.nc * UP_KP, ca, cb, v11, v21, v12, v22);
            pi1 = i1;
            pi2 = i2;
        }
        const float w11 = tx.d2 * ty.d2, w21 = tx.d1 * ty.d2, w12 = tx.d2 * ty.d1, w22 = tx.d1 * ty.d1;
        float c[4 * NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const f32x2 lo = bilerp2(f32x2{v11[q].x, v11[q].y}, f32x2{v21[q].x, v21[q].y}, f32x2{v12[q].x, v12[q].y},
                                     f32x2{v22[q].x, v22[q].y}, w11, w21, w12, w22);
            const f32x2 hi = bilerp2(f32x2{v11[q].z, v11[q].w}, f32x2{v21[q].z, v21[q].w}, f32x2{v12[q].z, v12[q].w},
                                     f32x2{v22[q].z, v22[q].w}, w11, w21, w12, w22);
            c[4 * q + 0] = up_post(lo.x, uq);
            c[4 * q + 1] = up_post(lo.y, uq);
            c[4 * q + 2] = up_post(hi.x, uq);
            c[4 * q + 3] = up_post(hi.y, uq);
        }
        // the zero pad classes of the staged slot (only the last quad has any: NQ = ceil(K / 4)) must neither win against a
        // negative maximum nor enter the softmax sum
#pragma unroll
        for (int e = 1; e < 4; e++)
            if (4 * (NQ - 1) + e >= K) c[4 * (NQ - 1) + e] = -__builtin_inff();
        const SegPix p = seg_decode(4 * NQ, softmax, [&](int k) { return c[k]; });
        if (live && o.rgba) o.rgba[(size_t)y * OW + x] = lut[(p.k % 20) * 256 + p.conf];
        kpack |= (uint32_t)p.k << (8 * rr);
        cpack |= (uint32_t)p.conf << (8 * rr);
        if (o.shards) seg_row_stats(sstat, live, p.k, p.conf, blockIdx.x * UP_TW, y);
    }
    const bool dwords = (OW & 3) == 0 && ((reinterpret_cast<uintptr_t>(o.klass) | reinterpret_cast<uintptr_t>(o.conf)) & 3) == 0;
    seg_store_rows4(o.klass, kpack, dwords, live, x, y0, OH, OW);
    seg_store_rows4(o.conf, cpack, dwords, live, x, y0, OH, OW);
    if (o.shards) seg_flush_stats(sstat, K, o.shards);
}

hipError_t launch_upsample_argmax_segments(const float* low, int LH, int LW, int K, int softmax, const uint32_t* lut,
                                           const SegOut& o, int OH, int OW, hipStream_t s, const UpQuant uq) {
    UP_LAUNCH(upsample_argmax_segments_lds_kernel, upsample_argmax_segments_kernel, low, LH, LW, K, softmax, lut, o, OH, OW, uq);
}

}  // namespace infur
