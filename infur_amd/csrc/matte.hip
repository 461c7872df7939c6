// matte.hip -- Matte and Composite (include/infur_hip.h).  Matte turns the hard selection of a byte or u32 plane into a
// soft alpha that follows the edges of the packed BGR frame: a joint (cross) bilateral filter of the mask, guided by the picture,
// with a rational range weight, in exact integers.  Composite lays the frame over a colour or a picture with that alpha, or cuts
// it out.
//   0 prepare  the five count words, and the 766 weights (4096 s^2) / (s^2 + d^2) of the call's sigma as u16 (a kernel, not a
//              memset: the call is capturable as launches only)
//   1 tiles    a workgroup of four waves owns 64 columns x 16 rows of the output
//        stage    the tile grown by the radius on every side goes to LDS, one word a pixel: B | G << 8 | R << 16 | m << 24, with
//                 selection, invert and conf resolved here; a wave stages a row in two steps of 64 columns and leaves a word per
//                 row that says whether the row's pixels inside the frame all hold one m (and which) -- one ballot per step.
//                 Pixels outside the frame are staged as zero words.  SELECTED and OUTSIDE are popcounts over the tile's own
//                 pixels
//        quiet    a wave owns four output rows; the 4 + 2r row words above and below them, read by as many lanes, say in three
//                 ballots whether every m its windows can see is the same c: then alpha is c and the wave leaves
//        taps     otherwise a lane is a column and carries four vertically adjacent outputs.  A tap word is read from LDS once
//                 (adjacent lanes, adjacent banks) and serves the outputs whose window holds its row: v_sad_u8 on the three colour
//                 bytes, one u16 read of the weight table in LDS, one add into D and one 24-bit multiply-add into N.  Which of the
//                 four outputs a row serves is a wave-uniform mask (1, 3, 7, 15, 14, 12, 8), and the inner loop is compiled once
//                 per mask.  Rows outside the frame are skipped by the wave; columns outside it exist only in tiles at the left and
//                 right border, which run a second form of the loop that gives those taps weight 0
//        alpha    (2N + D) / (2D); CLEAR, SOFT and OPAQUE from three ballots per wave-row, one add per workgroup and word
//   2 counts   the five words -> the eight counts
// Composite is one pointwise launch: a lane takes four pixels, reads three u32 words of the frame (and of the backdrop) and one of
// alpha where the pointers are aligned, bytes at the ragged end, and reads before it writes, so `out` may be the frame.
// Every output byte is a function of its window alone and has one writer; the counts are integer sums.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace infur {

namespace {

constexpr int kMatBlock = 256;
constexpr unsigned kMatStride = kMatteTileW + 2 * kMatteMaxRadius;  // words a row of the tile in LDS: 96
constexpr unsigned kMatRows = kMatteTileH + 2 * kMatteMaxRadius;    // rows of the tile in LDS: 48
constexpr unsigned kMatWaveRows = kMatteTileH / 4;                  // output rows a wave, and outputs a lane: 4
constexpr unsigned kMatDist = 766;                                  // colour distances 0 .. 765
constexpr unsigned kMatTable = 768;                                 // u16 entries staged (a whole number of words; the last two are 0)
constexpr unsigned kMatOne = 4096;                                  // the centre tap's weight
constexpr unsigned kMatSelLds = 1024;                               // a selection table of at most this many bytes is staged in LDS
constexpr unsigned kRowMixed = 0x100, kRowEmpty = 0x200;            // a row word: one m (0 .. 255), several, or no pixel inside the frame
constexpr size_t kMatAccBytes = 256;                                // in front of the weights: SELECTED, OUTSIDE, CLEAR, SOFT, OPAQUE

constexpr unsigned long long kMatWindow = (2ull * kMatteMaxRadius + 1) * (2ull * kMatteMaxRadius + 1);
// N <= 33^2 * 4096 * 255 and 2N + D <= 2 279 337 984: every sum is a u32 (and not an i32)
static_assert(kMatWindow * kMatOne * 255ull == 1137438720ull && 2ull * kMatWindow * kMatOne * 255ull + kMatWindow * kMatOne == 2279337984ull &&
                  2279337984ull < (1ull << 32),
              "Matte's sums leave 32 bits");
static_assert(kMatOne * 255u * 255u + 765u * 765u < (1ull << 32) && kMatOne <= 65535, "a weight is a u16 and its quotient a u32");
static_assert(kMatWaveRows == 4 && kMatteTileW == 64, "a wave is a row of the tile and carries four of them");

__global__ void __launch_bounds__(kMatBlock) matte_prepare_kernel(unsigned* __restrict__ acc, uint16_t* __restrict__ weights, unsigned sigma) {
    if (threadIdx.x < 8) acc[threadIdx.x] = 0u;
    const unsigned s2 = sigma * sigma;
    for (unsigned d = threadIdx.x; d < kMatTable; d += kMatBlock) weights[d] = d < kMatDist ? (uint16_t)((kMatOne * s2) / (s2 + d * d)) : (uint16_t)0;
}

// one row of taps for the outputs of MASK.  row: the tile row at the lane's leftmost tap; gx0: that tap's column in the frame
template <unsigned MASK, bool EDGE>
__device__ __forceinline__ void tap_row(const unsigned* row, const uint16_t* wt, unsigned taps, int gx0, unsigned W, const unsigned (&pc)[4],
                                        unsigned (&D)[4], unsigned (&N)[4]) {
    for (unsigned i = 0; i < taps; i++) {
        const unsigned q = row[i];
        const unsigned col = q & 0xFFFFFFu, m = q >> 24;
        const bool inside = !EDGE || (unsigned)(gx0 + (int)i) < W;
#pragma unroll
        for (unsigned k = 0; k < kMatWaveRows; k++) {
            if (!((MASK >> k) & 1u)) continue;
            unsigned w = wt[__builtin_amdgcn_sad_u8(pc[k], col, 0u)];
            if (EDGE) w = inside ? w : 0u;
            D[k] += w;
            N[k] += __umul24(w, m);
        }
    }
}

template <class T>
__global__ void __launch_bounds__(kMatBlock)
    matte_tiles_kernel(const uint8_t* __restrict__ frame, const T* __restrict__ plane, unsigned H, unsigned W, const uint8_t* __restrict__ select,
                       unsigned rows, int invert, const uint8_t* __restrict__ conf, unsigned r, const unsigned* __restrict__ weights,
                       uint8_t* __restrict__ alpha, unsigned* __restrict__ acc) {
    __shared__ unsigned tile[kMatRows * kMatStride];
    __shared__ unsigned wt32[kMatTable / 2];
    __shared__ uint8_t lsel[kMatSelLds];
    __shared__ unsigned rowinfo[kMatRows];
    __shared__ unsigned wcnt[kMatBlock / 64][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X0 = (int)(blockIdx.x * kMatteTileW), Y0 = (int)(blockIdx.y * kMatteTileH), R = (int)r;
    const unsigned tw = kMatteTileW + 2 * r, th = kMatteTileH + 2 * r;

    const uint8_t* tab = select;
    if (rows <= kMatSelLds) {  // (uniform)
        for (unsigned i = threadIdx.x; i < rows; i += kMatBlock) lsel[i] = select[i];
        tab = lsel;
    }
    for (unsigned i = threadIdx.x; i < kMatTable / 2; i += kMatBlock) wt32[i] = weights[i];
    __syncthreads();

    // ---- stage: rows wave, wave + 4, .. of the grown tile ----
    unsigned nsel = 0, nout = 0;
    for (unsigned ty = (unsigned)wave; ty < th; ty += kMatBlock / 64) {
        const int gy = Y0 - R + (int)ty;
        const bool rowin = (unsigned)gy < H, ownrow = ty >= r && ty < r + kMatteTileH;
        unsigned info = kRowEmpty;
#pragma unroll
        for (unsigned step = 0; step < 2; step++) {
            const unsigned tx = (unsigned)lane + 64u * step;
            const int gx = X0 - R + (int)tx;
            const bool in = rowin && tx < tw && (unsigned)gx < W;
            unsigned word = 0, m = 0;
            bool sel = false, outside = false;
            if (in) {
                const size_t at = (size_t)gy * W + (unsigned)gx;
                const unsigned v = (unsigned)plane[at];
                outside = v >= rows;
                sel = (outside ? false : tab[v] != 0) != (invert != 0);
                m = sel ? (conf ? (unsigned)conf[at] : 255u) : 0u;
                const uint8_t* p = frame + at * 3;
                word = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | (m << 24);
            }
            if (tx < tw) tile[ty * kMatStride + tx] = word;
            const unsigned long long b = __ballot(in);
            if (b) {  // (uniform)
                const unsigned first = __shfl(m, __ffsll(b) - 1, 64);
                if (info == kRowEmpty) info = first;
                if (__ballot(in && m != info)) info = kRowMixed;
            }
            const bool own = in && ownrow && tx >= r && tx < r + kMatteTileW;
            nsel += (unsigned)__popcll(__ballot(own && sel));
            nout += (unsigned)__popcll(__ballot(own && outside));
        }
        if (lane == 0) rowinfo[ty] = info;
    }
    __syncthreads();

    // ---- the wave's four output rows ----
    unsigned nclear = 0, nsoft = 0, nopaque = 0;
    const int oy0 = Y0 + wave * (int)kMatWaveRows;
    if ((unsigned)oy0 < H) {  // (uniform)
        const unsigned nrows = kMatWaveRows + 2 * r;  // the rows its windows can see: at most 36
        const unsigned v = (unsigned)lane < nrows ? rowinfo[wave * kMatWaveRows + lane] : kRowEmpty;
        const unsigned long long one = __ballot(v < kRowMixed);
        const unsigned c0 = __shfl(v, one ? __ffsll(one) - 1 : 0, 64);
        const bool quiet = one && !__ballot(v == kRowMixed) && !__ballot(v < kRowMixed && v != c0);
        const int gx = X0 + lane;
        unsigned a[kMatWaveRows];
        if (quiet) {
#pragma unroll
            for (unsigned k = 0; k < kMatWaveRows; k++) a[k] = c0;
        } else {
            unsigned pc[kMatWaveRows], D[kMatWaveRows], N[kMatWaveRows];
#pragma unroll
            for (unsigned k = 0; k < kMatWaveRows; k++) {
                pc[k] = tile[(r + wave * kMatWaveRows + k) * kMatStride + r + lane] & 0xFFFFFFu;
                D[k] = N[k] = 0u;
            }
            const bool edge = X0 < R || X0 + (int)kMatteTileW + R > (int)W;  // some tap column of the tile lies outside the frame
            const uint16_t* wt = (const uint16_t*)wt32;
            const unsigned taps = 2 * r + 1;
            for (unsigned j = 0; j < nrows; j++) {  // tile row wave * 4 + j serves output k iff k <= j <= k + 2r
                if ((unsigned)(Y0 - R + wave * (int)kMatWaveRows + (int)j) >= H) continue;  // (uniform) a row outside the frame
                unsigned mask = 0;
#pragma unroll
                for (unsigned k = 0; k < kMatWaveRows; k++) mask |= (j >= k && j <= k + 2 * r) ? 1u << k : 0u;
                const unsigned* row = tile + (wave * kMatWaveRows + j) * kMatStride + lane;
                const int gx0 = gx - R;
#define MATTE_ROW(M)                                                       \
    case M:                                                                \
        if (edge) tap_row<M, true>(row, wt, taps, gx0, W, pc, D, N);       \
        else tap_row<M, false>(row, wt, taps, gx0, W, pc, D, N);           \
        break;
                switch (mask) {  // (uniform)
                    MATTE_ROW(1u) MATTE_ROW(3u) MATTE_ROW(7u) MATTE_ROW(15u) MATTE_ROW(14u) MATTE_ROW(12u) MATTE_ROW(8u)
                    default: break;
                }
#undef MATTE_ROW
            }
#pragma unroll
            for (unsigned k = 0; k < kMatWaveRows; k++) a[k] = D[k] ? (2u * N[k] + D[k]) / (2u * D[k]) : 0u;  // (D = 0: no live output)
        }
#pragma unroll
        for (unsigned k = 0; k < kMatWaveRows; k++) {
            const int oy = oy0 + (int)k;
            const bool live = (unsigned)oy < H && (unsigned)gx < W;
            if (alpha && live) alpha[(size_t)oy * W + (unsigned)gx] = (uint8_t)a[k];
            nclear += (unsigned)__popcll(__ballot(live && a[k] == 0u));
            nopaque += (unsigned)__popcll(__ballot(live && a[k] == 255u));
            nsoft += (unsigned)__popcll(__ballot(live && a[k] != 0u && a[k] != 255u));
        }
    }
    if (!acc) return;  // (uniform)
    if (lane == 0) {
        wcnt[wave][0] = nsel;
        wcnt[wave][1] = nout;
        wcnt[wave][2] = nclear;
        wcnt[wave][3] = nsoft;
        wcnt[wave][4] = nopaque;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned n = 0;
        for (int k = 0; k < kMatBlock / 64; k++) n += wcnt[k][threadIdx.x];
        if (n) atomicAdd(&acc[threadIdx.x], n);
    }
}

__global__ void __launch_bounds__(64) matte_counts_kernel(const unsigned* __restrict__ acc, unsigned* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 5; k++) counts[k] = acc[k];  // SELECTED, OUTSIDE, CLEAR, SOFT, OPAQUE
    counts[5] = counts[6] = 0u;
    counts[7] = acc[0] ? 0u : kMatteNothing;
}

template <class T>
void launch_matte_t(const uint8_t* frame, const T* plane, unsigned H, unsigned W, const uint8_t* select, unsigned rows, int invert,
                    const uint8_t* conf, unsigned radius, unsigned sigma, unsigned* acc, uint16_t* weights, uint8_t* alpha, unsigned* counts,
                    hipStream_t s) {
    const dim3 grid((W + kMatteTileW - 1) / kMatteTileW, (H + kMatteTileH - 1) / kMatteTileH);
    hipLaunchKernelGGL(matte_prepare_kernel, dim3(1), dim3(kMatBlock), 0, s, acc, weights, sigma);
    hipLaunchKernelGGL(matte_tiles_kernel<T>, grid, dim3(kMatBlock), 0, s, frame, plane, H, W, select, rows, invert, conf, radius,
                       (const unsigned*)weights, alpha, counts ? acc : nullptr);
    if (counts) hipLaunchKernelGGL(matte_counts_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)acc, counts);
}

// ---- Composite ----
__device__ __forceinline__ unsigned blend(unsigned a, unsigned f, unsigned b) { return (a * f + (255u - a) * b + 127u) / 255u; }
__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[3], int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 255u; }

// a lane takes the pixels 4g .. 4g + 3.  wide: frame, alpha, back and out are word-aligned.  frame and out may be one buffer
__global__ void __launch_bounds__(kMatBlock) composite_kernel(const uint8_t* frame, const uint8_t* __restrict__ alpha, size_t npix, unsigned mode,
                                                              const uint8_t* back, unsigned colour, uint8_t* out, int wide) {
    const size_t p0 = ((size_t)blockIdx.x * kMatBlock + threadIdx.x) * 4;
    if (p0 >= npix) return;
    if (wide && p0 + 4 <= npix) {
        const unsigned* fw = (const unsigned*)(frame + p0 * 3);
        const unsigned f[3] = {fw[0], fw[1], fw[2]};
        const unsigned a4 = *(const unsigned*)(alpha + p0);
        if (mode == kCompositeCutout) {
            unsigned* ow = (unsigned*)(out + p0 * 4);
#pragma unroll
            for (int k = 0; k < 4; k++)
                ow[k] = byte_of(f, 3 * k) | (byte_of(f, 3 * k + 1) << 8) | (byte_of(f, 3 * k + 2) << 16) | (((a4 >> (8 * k)) & 255u) << 24);
            return;
        }
        unsigned b[3] = {0u, 0u, 0u};
        if (mode == kCompositeImage) {
            const unsigned* bw = (const unsigned*)(back + p0 * 3);
            b[0] = bw[0];
            b[1] = bw[1];
            b[2] = bw[2];
        }
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const unsigned a = (a4 >> ((i / 3) * 8)) & 255u;
            const unsigned under = mode == kCompositeImage ? byte_of(b, i) : (colour >> ((i % 3) * 8)) & 255u;
            o[i >> 2] |= blend(a, byte_of(f, i), under) << ((i & 3) * 8);
        }
        unsigned* ow = (unsigned*)(out + p0 * 3);
        ow[0] = o[0];
        ow[1] = o[1];
        ow[2] = o[2];
        return;
    }
    const size_t p1 = p0 + 4 < npix ? p0 + 4 : npix;
    for (size_t p = p0; p < p1; p++) {
        const unsigned a = alpha[p];
        const unsigned f0 = frame[p * 3], f1 = frame[p * 3 + 1], f2 = frame[p * 3 + 2];
        if (mode == kCompositeCutout) {
            out[p * 4] = (uint8_t)f0;
            out[p * 4 + 1] = (uint8_t)f1;
            out[p * 4 + 2] = (uint8_t)f2;
            out[p * 4 + 3] = (uint8_t)a;
            continue;
        }
        unsigned b0 = colour & 255u, b1 = (colour >> 8) & 255u, b2 = (colour >> 16) & 255u;
        if (mode == kCompositeImage) {
            b0 = back[p * 3];
            b1 = back[p * 3 + 1];
            b2 = back[p * 3 + 2];
        }
        out[p * 3] = (uint8_t)blend(a, f0, b0);
        out[p * 3 + 1] = (uint8_t)blend(a, f1, b1);
        out[p * 3 + 2] = (uint8_t)blend(a, f2, b2);
    }
}

}  // namespace

// [the five count words, 256 bytes][the 768 u16 weights]
size_t matte_scratch_bytes() { return kMatAccBytes + kMatTable * 2; }

hipError_t launch_matte(const uint8_t* frame, const void* plane, int elem_bytes, unsigned H, unsigned W, const uint8_t* select, unsigned select_rows,
                        int invert, const uint8_t* conf, unsigned radius, unsigned sigma, void* scratch, uint8_t* alpha, unsigned* counts,
                        hipStream_t s) {
    if (!H || !W || H > kMatteMaxSide || W > kMatteMaxSide || !radius || radius > kMatteMaxRadius || !sigma || sigma > 255) return hipErrorInvalidValue;
    if (elem_bytes != 1 && elem_bytes != 4) return hipErrorInvalidValue;
    if (!alpha && !counts) return hipSuccess;
    unsigned* acc = (unsigned*)scratch;
    uint16_t* weights = (uint16_t*)((uint8_t*)scratch + kMatAccBytes);
    if (elem_bytes == 1)
        launch_matte_t(frame, (const uint8_t*)plane, H, W, select, select_rows, invert, conf, radius, sigma, acc, weights, alpha, counts, s);
    else
        launch_matte_t(frame, (const uint32_t*)plane, H, W, select, select_rows, invert, conf, radius, sigma, acc, weights, alpha, counts, s);
    return hipGetLastError();
}

hipError_t launch_composite(const uint8_t* frame, const uint8_t* alpha, unsigned H, unsigned W, unsigned mode, const uint8_t* back, unsigned colour,
                            uint8_t* out, hipStream_t s) {
    if (!H || !W || H > kMatteMaxSide || W > kMatteMaxSide || mode > kCompositeCutout || (mode == kCompositeImage && !back)) return hipErrorInvalidValue;
    const size_t npix = (size_t)H * W, lanes = (npix + 3) / 4;
    const uintptr_t bits = (uintptr_t)frame | (uintptr_t)alpha | (uintptr_t)out | (mode == kCompositeImage ? (uintptr_t)back : 0);
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((lanes + kMatBlock - 1) / kMatBlock)), dim3(kMatBlock), 0, s, frame, alpha, npix, mode, back,
                       colour, out, (bits & 3) == 0 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace infur
