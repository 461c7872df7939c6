// redact.hip -- Redact: the selected pixels of a packed BGR frame are filled, pixelated or blurred (include/infur_hip.h).
// The stage that writes the frame.  Selection comes from a byte or u32 plane through a table of bytes; only selected pixels
// contribute to a result and only selected pixels change.  The cost of the two averaging modes does not grow with the cell or the
// radius: a summed-area table of four u32 channels (sel * B, sel * G, sel * R, sel), sixteen bytes a pixel, is built once a pass
// and every pixel reads the four corners of its box from it.
//   0 clear    the two count words (a kernel, not a memset: the call is capturable as launches only)
//   1 rows     one workgroup per row, 256 columns a step.  A lane gathers its three bytes and its selection bit; the wave scans
//              two packed words (B | G << 16, R | n << 16: 64 * 255 < 2^16) with six shuffles each, the four wave totals meet in LDS
//              and a running carry goes from step to step.  One 128-bit store per pixel
//   2 columns  lanes are columns, so every step of a wave is one coalesced line of the table, four in flight:
//        bands    every band of 64 rows is scanned on its own, in place
//        totals   a lane per column walks the last rows of the bands (y = 63 mod 64) and leaves their running sum there
//        add      every other row of band b >= 1 adds the last row of band b - 1
//   3 resolve  one lane per pixel: selection again, the box (the pixel's cell, or its clipped window: the modes share the rest),
//              four corners, three divisions, three bytes.  An unselected pixel copies the frame where out is another buffer.
//              Counts from ballot popcounts, one add per workgroup and word
//   4 counts   the two words -> the eight counts
// Passes 2 and 3 of BLUR run 1 to 3 again from `out` and resolve in place: the resolve reads the table alone.  FILL is the
// resolve alone.  Everything is an integer and a function of the inputs alone; the two sums commute, so the bytes do not depend on
// scheduling.  H * W <= 2^24 in the averaging modes: 255 * H * W < 2^32 and no entry of the table wraps.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kRedBlock = 256;
constexpr unsigned kRedBand = 64;      // rows a band of the column pass
constexpr unsigned kRedSelLds = 1024;  // a selection table of at most this many bytes is staged in LDS
constexpr size_t kRedAccBytes = 256;   // in front of the table: [0] SELECTED, [1] OUTSIDE

__device__ __forceinline__ uint4 add4(const uint4 a, const uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ uint4 sub4(const uint4 a, const uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// -> where to look a value up: the table staged in `lsel` when it is small, the table itself otherwise.  Holds a barrier.
__device__ __forceinline__ const uint8_t* stage_select(const uint8_t* __restrict__ select, unsigned rows, uint8_t* lsel) {
    if (rows > kRedSelLds) return select;  // (uniform)
    for (unsigned i = threadIdx.x; i < rows; i += kRedBlock) lsel[i] = select[i];
    __syncthreads();
    return lsel;
}

// value v is selected: inside the table with a non-zero byte, or the opposite with invert.  *outside: v lies beyond the table
__device__ __forceinline__ bool is_selected(unsigned v, const uint8_t* tab, unsigned rows, bool invert, bool* outside) {
    const bool in = v < rows;
    *outside = !in;
    const bool s = in ? tab[v] != 0 : false;
    return s != invert;
}

__global__ void __launch_bounds__(64) redact_clear_kernel(unsigned* __restrict__ acc) {
    if (threadIdx.x < 2) acc[threadIdx.x] = 0u;
}

template <class T>
__global__ void __launch_bounds__(kRedBlock)
    redact_rows_kernel(const uint8_t* __restrict__ src, const T* __restrict__ plane, unsigned W, const uint8_t* __restrict__ select, unsigned rows,
                       int invert, uint4* __restrict__ table) {
    __shared__ uint8_t lsel[kRedSelLds];
    __shared__ uint4 wtot[kRedBlock / 64];
    const uint8_t* tab = stage_select(select, rows, lsel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = (size_t)blockIdx.x * W;
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (unsigned x0 = 0; x0 < W; x0 += kRedBlock) {  // (uniform)
        const unsigned x = x0 + threadIdx.x;
        const bool in = x < W;
        unsigned bg = 0, rn = 0;
        bool outside;
        if (in && is_selected((unsigned)plane[row0 + x], tab, rows, invert != 0, &outside)) {
            const uint8_t* p = src + (row0 + x) * 3;
            bg = (unsigned)p[0] | ((unsigned)p[1] << 16);
            rn = (unsigned)p[2] | (1u << 16);
        }
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(bg, d, 64), u = __shfl_up(rn, d, 64);
            if (lane >= d) { bg += t; rn += u; }
        }
        const uint4 mine = make_uint4(bg & 0xFFFFu, bg >> 16, rn & 0xFFFFu, rn >> 16);
        if (lane == 63) wtot[wave] = mine;
        __syncthreads();
        uint4 before = carry;
#pragma unroll
        for (int k = 0; k < kRedBlock / 64; k++) {
            const uint4 s = wtot[k];
            if (k < wave) before = add4(before, s);
            carry = add4(carry, s);
        }
        if (in) table[row0 + x] = add4(before, mine);
        __syncthreads();
    }
}

// band blockIdx.y of 64 rows, scanned down its columns in place
__global__ void __launch_bounds__(kRedBlock) redact_bands_kernel(uint4* __restrict__ table, unsigned H, unsigned W) {
    const unsigned x = blockIdx.x * kRedBlock + threadIdx.x;
    if (x >= W) return;
    const unsigned y0 = blockIdx.y * kRedBand, y1 = y0 + kRedBand < H ? y0 + kRedBand : H;
    uint4* col = table + x;
    uint4 run = make_uint4(0, 0, 0, 0);
    for (unsigned y = y0; y < y1; y += 4) {
        uint4 v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) v[k] = y + k < y1 ? col[(size_t)(y + k) * W] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (y + k < y1) { run = add4(run, v[k]); col[(size_t)(y + k) * W] = run; }
    }
}

// the last rows of the full bands, y = 63 mod 64: their running sum down the column
__global__ void __launch_bounds__(kRedBlock) redact_totals_kernel(uint4* __restrict__ table, unsigned H, unsigned W) {
    const unsigned x = blockIdx.x * kRedBlock + threadIdx.x;
    if (x >= W) return;
    uint4* col = table + x;
    uint4 run = make_uint4(0, 0, 0, 0);
    for (unsigned y = kRedBand - 1; y < H; y += 4 * kRedBand) {
        uint4 v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) v[k] = y + k * kRedBand < H ? col[(size_t)(y + k * kRedBand) * W] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (y + k * kRedBand < H) { run = add4(run, v[k]); col[(size_t)(y + k * kRedBand) * W] = run; }
    }
}

// band blockIdx.y + 1: its rows but the last add the last row of the band above
__global__ void __launch_bounds__(kRedBlock) redact_add_kernel(uint4* __restrict__ table, unsigned H, unsigned W) {
    const unsigned x = blockIdx.x * kRedBlock + threadIdx.x;
    if (x >= W) return;
    const unsigned y0 = (blockIdx.y + 1) * kRedBand, y1 = y0 + kRedBand - 1 < H ? y0 + kRedBand - 1 : H;
    uint4* col = table + x;
    const uint4 off = col[(size_t)(y0 - 1) * W];
    for (unsigned y = y0; y < y1; y += 4) {
        uint4 v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) v[k] = y + k < y1 ? col[(size_t)(y + k) * W] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (y + k < y1) col[(size_t)(y + k) * W] = add4(v[k], off);
    }
}

// round half up: (2 S + n) / (2 n) without the 33rd bit
__device__ __forceinline__ unsigned mean_half_up(unsigned S, unsigned n) {
    const unsigned q = S / n, rem = S - q * n;
    return q + (2u * rem >= n ? 1u : 0u);
}

// mode kRedactFill needs no table; out == nullptr: the counts alone.  copy: an unselected pixel copies the frame
template <class T>
__global__ void __launch_bounds__(kRedBlock)
    redact_resolve_kernel(const uint8_t* frame, const T* __restrict__ plane, unsigned H, unsigned W, unsigned tilesX,
                          const uint8_t* __restrict__ select, unsigned rows, int invert, unsigned mode, unsigned size, unsigned colour,
                          const uint4* __restrict__ table, uint8_t* out, int copy, unsigned* __restrict__ acc) {
    __shared__ uint8_t lsel[kRedSelLds];
    __shared__ unsigned wsel[kRedBlock / 64], wout[kRedBlock / 64];
    const uint8_t* tab = stage_select(select, rows, lsel);
    const WaveRow r = wave_row(H, W, tilesX);
    bool outside = false;
    const bool sel = r.live && is_selected((unsigned)plane[r.at], tab, rows, invert != 0, &outside);
    outside = outside && r.live;
    if (out && sel) {
        unsigned b = colour & 255u, g = (colour >> 8) & 255u, rr = (colour >> 16) & 255u;
        if (mode != kRedactFill) {
            unsigned x0, x1, y0, y1;
            if (mode == kRedactPixelate) {
                x0 = r.x - r.x % size;
                y0 = r.y - r.y % size;
                x1 = x0 + size - 1;
                y1 = y0 + size - 1;
            } else {
                x0 = r.x > size ? r.x - size : 0u;
                y0 = r.y > size ? r.y - size : 0u;
                x1 = r.x + size;
                y1 = r.y + size;
            }
            x1 = x1 < W ? x1 : W - 1;
            y1 = y1 < H ? y1 : H - 1;
            uint4 s = table[(size_t)y1 * W + x1];
            if (x0) s = sub4(s, table[(size_t)y1 * W + x0 - 1]);
            if (y0) s = sub4(s, table[(size_t)(y0 - 1) * W + x1]);
            if (x0 && y0) s = add4(s, table[(size_t)(y0 - 1) * W + x0 - 1]);
            b = mean_half_up(s.x, s.w);  // (s.w >= 1: the pixel itself)
            g = mean_half_up(s.y, s.w);
            rr = mean_half_up(s.z, s.w);
        }
        uint8_t* o = out + r.at * 3;
        o[0] = (uint8_t)b;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)rr;
    } else if (out && copy && r.live) {
        const uint8_t* p = frame + r.at * 3;
        uint8_t* o = out + r.at * 3;
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
    }
    if (!acc) return;  // (uniform)
    const unsigned ns = (unsigned)__popcll(__ballot(sel)), no = (unsigned)__popcll(__ballot(outside));
    if ((threadIdx.x & 63) == 0) { wsel[threadIdx.x >> 6] = ns; wout[threadIdx.x >> 6] = no; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, b = 0;
        for (int k = 0; k < kRedBlock / 64; k++) { a += wsel[k]; b += wout[k]; }
        if (a) atomicAdd(&acc[0], a);
        if (b) atomicAdd(&acc[1], b);
    }
}

__global__ void __launch_bounds__(64) redact_counts_kernel(const unsigned* __restrict__ acc, unsigned passes, unsigned* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    counts[0] = acc[0];
    counts[1] = acc[1];
    counts[2] = passes;
    counts[3] = counts[4] = counts[5] = counts[6] = 0u;
    counts[7] = acc[0] ? 0u : kRedactNothing;
}

template <class T>
hipError_t launch_redact_t(const uint8_t* frame, const T* plane, unsigned H, unsigned W, const uint8_t* select, unsigned rows, int invert,
                           unsigned mode, unsigned size, unsigned passes, unsigned colour, unsigned* acc, uint4* table, uint8_t* out,
                           unsigned* counts, hipStream_t s) {
    const unsigned tilesX = (W + 63) / 64, colBlocks = (W + kRedBlock - 1) / kRedBlock, bands = (H + kRedBand - 1) / kRedBand;
    const dim3 pixels((unsigned)(((size_t)H * tilesX + 3) / 4)), block(kRedBlock);
    if (mode != kRedactBlur) passes = mode == kRedactPixelate ? 1u : 0u;
    if (counts) hipLaunchKernelGGL(redact_clear_kernel, dim3(1), dim3(64), 0, s, acc);
    if (!out || mode == kRedactFill) {
        hipLaunchKernelGGL(redact_resolve_kernel<T>, pixels, block, 0, s, frame, plane, H, W, tilesX, select, rows, invert, (unsigned)kRedactFill, 0u,
                           colour, (const uint4*)nullptr, out, out != frame, counts ? acc : nullptr);
    } else {
        for (unsigned p = 0; p < passes; p++) {
            hipLaunchKernelGGL(redact_rows_kernel<T>, dim3(H), block, 0, s, p ? (const uint8_t*)out : frame, plane, W, select, rows, invert, table);
            hipLaunchKernelGGL(redact_bands_kernel, dim3(colBlocks, bands), block, 0, s, table, H, W);
            if (bands > 1) {
                hipLaunchKernelGGL(redact_totals_kernel, dim3(colBlocks), block, 0, s, table, H, W);
                hipLaunchKernelGGL(redact_add_kernel, dim3(colBlocks, bands - 1), block, 0, s, table, H, W);
            }
            hipLaunchKernelGGL(redact_resolve_kernel<T>, pixels, block, 0, s, frame, plane, H, W, tilesX, select, rows, invert, mode, size, colour,
                               (const uint4*)table, out, p == 0 && out != frame, (counts && p == 0) ? acc : nullptr);
        }
    }
    if (counts) hipLaunchKernelGGL(redact_counts_kernel, dim3(1), dim3(64), 0, s, acc, passes, counts);
    return hipGetLastError();
}

}  // namespace

// [the two count words, 256 bytes][the table: sixteen bytes a pixel, in the averaging modes]
size_t redact_scratch_bytes(size_t npix, unsigned mode) { return kRedAccBytes + (mode == kRedactFill ? 0 : npix * 16); }

hipError_t launch_redact(const uint8_t* frame, const void* plane, int elem_bytes, unsigned H, unsigned W, const uint8_t* select, unsigned select_rows,
                         int invert, unsigned mode, unsigned size, unsigned passes, unsigned colour, void* scratch, uint8_t* out, unsigned* counts,
                         hipStream_t s) {
    if (!H || !W || H > kRedactMaxSide || W > kRedactMaxSide || mode > kRedactBlur) return hipErrorInvalidValue;
    if (mode != kRedactFill && ((size_t)H * W > kRedactMaxPixels || !size)) return hipErrorInvalidValue;
    if (!out && !counts) return hipSuccess;
    unsigned* acc = (unsigned*)scratch;
    uint4* table = (uint4*)((uint8_t*)scratch + kRedAccBytes);
    if (elem_bytes == 1)
        return launch_redact_t(frame, (const uint8_t*)plane, H, W, select, select_rows, invert, mode, size, passes, colour, acc, table, out, counts, s);
    if (elem_bytes == 4)
        return launch_redact_t(frame, (const uint32_t*)plane, H, W, select, select_rows, invert, mode, size, passes, colour, acc, table, out, counts, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
