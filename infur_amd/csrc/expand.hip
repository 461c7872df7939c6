// expand.hip -- Expand: every open pixel of a byte or u32 plane takes the value of its exact nearest seed (include/infur_hip.h,
// DESIGN 4q).  The stage that gives a value to pixels that have none: a margin round a mask, expand_labels, "which object is nearest",
// the holes min_pixels leaves.  Separable, and the column pass costs a pixel the same whether its seed is near or far:
//   0 clear    the accumulator rows and the two totals (a kernel, not a memset: the call is capturable as launches only)
//   1 rows     one workgroup per row.  nx(y, x) = the column of the nearest seed of row y, ties to the left, 0xFFFF = the row has
//              none.  Inside 64 columns the nearest seed on either side of a lane is clz / ctz of the masked ballot; each tile
//              leaves its first and last seed column in LDS, and one thread per tile finds the nearest non-empty tile on each side
//   2 columns  S(y, x) = the row y' that minimises (y - y')^2 + (x - nx(y', x))^2, ties to the smallest y'.  That cost matrix is
//              Monge, so S is non-decreasing in y:
//        coarse   rows y = 0 mod 64 walk outward from y, pruned by the best so far (up while dy^2 <= best, down while dy^2 < best)
//        refine   s = 32, 16, .. 1: rows y = s mod 2s search only [S(y - s), S(y + s)]; per column and level the ranges add up to
//                 at most H + H / 2s rows.  Lanes are columns: every step of a wave is one coalesced line of nx, four in flight
//   3 finish   one lane per pixel: q = (S, nx(S, x)), d^2, the source index and the value gathered from the plane; out, dist2,
//              source.  Per run of equal table rows along the wave the counts of SEEDS and GAINED and a segmented maximum of the
//              key (d^2 << 32) | ~index; the runs of one row are merged inside the wave, and its first head issues one atomicAdd
//              each and the key behind Anchors' load-before-atomicMax filter; per workgroup one 64-bit add of
//              (gained << 32) | seeds and one filtered maximum for the counts
//   4 table    accumulators -> the table rows and the eight counts
// Everything is an integer and a function of the plane alone; sums and maxima commute, so the bytes do not depend on scheduling.
// S is defined for every pixel of every plane (a column without a candidate keeps a row inside the plane), so a plane without a seed
// is read through nx alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kExpBlock = 256;
constexpr int kExpMaxTiles = 512;  // 32768 columns in tiles of 64
constexpr unsigned kExpNone = 0xFFFFFFFFu;
constexpr unsigned kExpNoCol = 0xFFFFu;
constexpr unsigned kExpCoarse = 64;   // the coarse rows' step; the refine levels are its halves
constexpr size_t kExpTotWords = 32;   // u64 words in front of the accumulator rows: [0] (gained << 32) | seeds, [1] the largest d^2

__global__ void __launch_bounds__(kExpBlock) expand_clear_kernel(unsigned long long* __restrict__ acc, size_t n) {
    const size_t i = (size_t)blockIdx.x * kExpBlock + threadIdx.x;
    if (i < n) acc[i] = 0ull;
}

template <class T>
__global__ void __launch_bounds__(kExpBlock) expand_rows_kernel(const T* __restrict__ plane, unsigned W, unsigned open_value, uint16_t* __restrict__ nx) {
    // per tile: its first and last seed column, then the nearest seed column left of the tile and right of it (kExpNoCol: none)
    __shared__ uint16_t first[kExpMaxTiles], last[kExpMaxTiles], near_l[kExpMaxTiles], near_r[kExpMaxTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tiles = (W + 63) / 64;
    const size_t row0 = (size_t)blockIdx.x * W;

    for (unsigned t = wave; t < tiles; t += kExpBlock / 64) {
        const unsigned x = t * 64 + lane;
        const bool seed = x < W && (unsigned)plane[row0 + x] != open_value;
        const uint64_t m = __ballot(seed);
        if (lane == 0) {
            first[t] = (uint16_t)(m ? t * 64 + (unsigned)__builtin_ctzll(m) : kExpNoCol);
            last[t] = (uint16_t)(m ? t * 64 + 63u - (unsigned)__builtin_clzll(m) : kExpNoCol);
        }
    }
    __syncthreads();
    for (unsigned t = threadIdx.x; t < tiles; t += kExpBlock) {
        unsigned l = kExpNoCol, r = kExpNoCol;
        for (unsigned u = t; u-- > 0 && l == kExpNoCol;) l = last[u];
        for (unsigned u = t + 1; u < tiles && r == kExpNoCol; u++) r = first[u];
        near_l[t] = (uint16_t)l;
        near_r[t] = (uint16_t)r;
    }
    __syncthreads();
    for (unsigned t = wave; t < tiles; t += kExpBlock / 64) {
        const unsigned x = t * 64 + lane;
        const bool in = x < W;
        const bool seed = in && (unsigned)plane[row0 + x] != open_value;
        const uint64_t m = __ballot(seed);
        const uint64_t ml = m & (~0ull >> (63 - lane)), mr = m & (~0ull << lane);  // the seeds at or left of the lane, at or right of it
        const unsigned xl = ml ? t * 64 + 63u - (unsigned)__builtin_clzll(ml) : near_l[t];
        const unsigned xr = mr ? t * 64 + (unsigned)__builtin_ctzll(mr) : near_r[t];
        unsigned best = xl;
        if (xl == kExpNoCol || (xr != kExpNoCol && xr - x < x - xl)) best = xr;  // ties go left
        if (in) nx[row0 + x] = (uint16_t)best;
    }
}

// the candidate of row yy for column x: (y - yy)^2 + (x - nx)^2, below 2^31; kExpNone where the row has no seed or `in` is false
__device__ __forceinline__ unsigned expand_cand(const uint16_t* __restrict__ nxcol, unsigned W, unsigned x, unsigned y, unsigned yy, bool in) {
    const unsigned c = in ? (unsigned)nxcol[(size_t)yy * W] : kExpNoCol;
    if (c == kExpNoCol) return kExpNone;
    const unsigned dy = y > yy ? y - yy : yy - y, dx = x > c ? x - c : c - x;
    return dy * dy + dx * dx;
}

__global__ void __launch_bounds__(kExpBlock)
    expand_coarse_kernel(const uint16_t* __restrict__ nx, unsigned H, unsigned W, unsigned tilesX, uint16_t* __restrict__ S) {
    const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned y = (unsigned)(u / tilesX) * kExpCoarse, x = (unsigned)(u % tilesX) * 64 + (threadIdx.x & 63);
    if (y >= H || x >= W) return;
    const uint16_t* nxcol = nx + x;
    unsigned best = expand_cand(nxcol, W, x, y, y, true), bs = y;
    // Four rows a step, their loads in flight together.  A row beyond the pruning bound cannot win (its dy^2 alone is too much), so
    // the bound is tested once a step.
    for (unsigned dy = 1; dy <= y && dy * dy <= best; dy += 4) {  // up: an equal candidate higher up has the smaller y'
        unsigned c[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) c[k] = expand_cand(nxcol, W, x, y, y - (dy + k <= y ? dy + k : y), dy + k <= y);
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (c[k] <= best && c[k] != kExpNone) { best = c[k]; bs = y - dy - k; }
    }
    for (unsigned dy = 1; dy < H - y && dy * dy < best; dy += 4) {  // down: only a strictly nearer one
        unsigned c[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) c[k] = expand_cand(nxcol, W, x, y, dy + k < H - y ? y + dy + k : y, dy + k < H - y);
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (c[k] < best) { best = c[k]; bs = y + dy + k; }
    }
    S[(size_t)y * W + x] = (uint16_t)bs;  // (a plane without a seed: the row itself)
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) { const unsigned o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) { const unsigned o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// rows y = s + 2s k: the search of [S(y - s), S(y + s)], h - 1 where y + s lies outside
__global__ void __launch_bounds__(kExpBlock)
    expand_refine_kernel(const uint16_t* __restrict__ nx, unsigned H, unsigned W, unsigned tilesX, unsigned s, uint16_t* __restrict__ S) {
    const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned y = s + 2 * s * (unsigned)(u / tilesX), x = (unsigned)(u % tilesX) * 64 + (threadIdx.x & 63);
    const bool live = y < H && x < W;
    unsigned lo = kExpNone, hi = 0;
    if (live) {
        lo = S[(size_t)(y - s) * W + x];
        hi = y + s < H ? (unsigned)S[(size_t)(y + s) * W + x] : H - 1;
    }
    const unsigned wlo = wave_min(lo), whi = wave_max(hi);  // (a wave without a live lane: wlo > whi)
    const uint16_t* nxcol = nx + x;
    unsigned best = kExpNone, bs = lo;
    for (unsigned y0 = wlo; y0 <= whi; y0 += 4) {  // ascending, strictly nearer only: ties keep the smaller y'
        unsigned c[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const bool in = y0 + k >= lo && y0 + k <= hi;
            c[k] = expand_cand(nxcol, W, x, y, in ? y0 + k : 0u, in);
        }
#pragma unroll
        for (unsigned k = 0; k < 4; k++)
            if (c[k] < best) { best = c[k]; bs = y0 + k; }
    }
    if (live) S[(size_t)y * W + x] = (uint16_t)bs;
}

template <class T>
__global__ void __launch_bounds__(kExpBlock)
    expand_finish_kernel(const T* __restrict__ plane, const uint16_t* __restrict__ nx, const uint16_t* __restrict__ S, unsigned H, unsigned W,
                         unsigned tilesX, unsigned open_value, unsigned long long reach2, T* __restrict__ out, unsigned* __restrict__ dist2,
                         unsigned* __restrict__ source, unsigned long long* __restrict__ keys, unsigned* __restrict__ sums, unsigned rows,
                         unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long bsum[kExpBlock / 64];
    __shared__ unsigned bmax[kExpBlock / 64];
    const WaveRow r = wave_row(H, W, tilesX);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned v = r.live ? (unsigned)plane[r.at] : open_value;
    const bool seed = r.live && v != open_value, open = r.live && !seed;
    unsigned d2 = 0, src = (unsigned)r.at, gv = open_value;
    bool gain = false, has = false;
    if (open) {
        const unsigned sy = S[r.at], sx = nx[(size_t)sy * W + r.x];
        has = sx != kExpNoCol;
        d2 = src = kExpNone;
        if (has) {
            const unsigned dy = r.y > sy ? r.y - sy : sy - r.y, dx = r.x > sx ? r.x - sx : sx - r.x;
            d2 = dy * dy + dx * dx;
            src = sy * W + sx;
            gain = reach2 == 0 || d2 <= reach2;
            if (gain) gv = (unsigned)plane[src];
        }
    }
    if (r.live) {
        if (out) out[r.at] = (T)(seed ? v : gv);
        if (dist2) dist2[r.at] = d2;
        if (source) source[r.at] = src;
    }
    if (keys) {  // (uniform) the table: one set of atomics per run of equal rows along the wave
        const unsigned rv = seed ? v : gv;
        const bool cnt = (seed || gain) && rv < rows;
        const unsigned key32 = cnt ? rv : kExpNone;  // (rv < rows <= 0xFFFFFFFF: a dead lane's key equals no live one)
        bool cont;
        const uint64_t starts = wave_run_starts(key32, cnt, &cont);
        const unsigned s = run_start(starts, lane), e = s + run_length(starts, (int)s) - 1u;
        const uint64_t run = (~0ull >> (63 - e)) & (~0ull << s);
        const unsigned ns = (unsigned)__popcll(__ballot(seed) & run), ng = (unsigned)__popcll(__ballot(gain) & run);
        unsigned long long key = (cnt && gain) ? ((unsigned long long)d2 << 32) | (unsigned long long)(kExpNone - (unsigned)r.at) : 0ull;
        for (int d = 1; d < 64; d <<= 1) {  // lane i: the maximum over [i, min(i + 2d - 1, e)]
            const unsigned long long o = __shfl_down(key, d, 64);
            if ((unsigned)lane + d <= e && o > key) key = o;
        }
        // The heads of one row are merged before they leave the wave: a plane of noise has a run per pixel and two or three rows to
        // send them to, and sums, unlike maxima, cannot be filtered by a load (9.4 ms on the 1080p noise plane with an add per run).
        // One turn of the loop per distinct row among the heads; a row with one head, the usual case on a label plane, costs a ballot.
        const bool head = cnt && (unsigned)lane == s;
        unsigned long long sum = ((unsigned long long)ng << 32) | ns;
        for (uint64_t todo = __ballot(head); todo;) {
            const int lead = __builtin_ctzll(todo);
            const unsigned val = __shfl(rv, lead, 64);
            const bool mine = head && rv == val;
            const uint64_t same = __ballot(mine);
            if (same & (same - 1)) {  // (uniform) several heads: their sums and the largest key go to the first
                unsigned long long a = mine ? sum : 0ull, k = mine ? key : 0ull;
                for (int d = 32; d > 0; d >>= 1) {
                    a += __shfl_xor(a, d, 64);
                    const unsigned long long o = __shfl_xor(k, d, 64);
                    k = o > k ? o : k;
                }
                if (lane == lead) { sum = a; key = k; }
            }
            if (lane == lead) {
                if ((unsigned)sum) atomicAdd(&sums[2 * (size_t)rv], (unsigned)sum);
                if (sum >> 32) atomicAdd(&sums[2 * (size_t)rv + 1], (unsigned)(sum >> 32));
                // a row only grows: a key that does not beat what the row held a moment ago cannot beat what it holds now
                if (key > __hip_atomic_load(&keys[rv], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&keys[rv], key);
            }
            todo &= ~same;
        }
    }
    if (!tot) return;  // (uniform)
    const unsigned long long wsum = ((unsigned long long)__popcll(__ballot(gain)) << 32) | (unsigned long long)__popcll(__ballot(seed));
    const unsigned wmax = wave_max(open && has ? d2 : 0u);
    if (lane == 0) { bsum[wave] = wsum; bmax[wave] = wmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        unsigned mx = 0;
        for (int k = 0; k < kExpBlock / 64; k++) { sum += bsum[k]; mx = bmax[k] > mx ? bmax[k] : mx; }
        if (sum) atomicAdd(&tot[0], sum);
        if ((unsigned long long)mx > __hip_atomic_load(&tot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&tot[1], (unsigned long long)mx);
    }
}

// keys == nullptr: an empty plane, zero rows and zero counts
__global__ void __launch_bounds__(kExpBlock)
    expand_table_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ sums, const unsigned long long* __restrict__ tot,
                        unsigned long long npix, unsigned rows, unsigned* __restrict__ table, unsigned* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * kExpBlock + threadIdx.x;
    if (table && i < rows) {
        const unsigned long long k = keys ? keys[i] : 0ull;  // (a gained pixel has d^2 >= 1: 0 is "nothing gained")
        table[i * kExpandWords + 0] = keys ? sums[2 * i] : 0u;
        table[i * kExpandWords + 1] = keys ? sums[2 * i + 1] : 0u;
        table[i * kExpandWords + 2] = (unsigned)(k >> 32);
        table[i * kExpandWords + 3] = k ? kExpNone - (unsigned)k : kExpNone;
    }
    if (counts && i == 0) {
        const unsigned long long t = tot ? tot[0] : 0ull;
        const unsigned seeds = (unsigned)t, gained = (unsigned)(t >> 32), open = (unsigned)(npix - seeds);
        counts[0] = seeds;
        counts[1] = open;
        counts[2] = gained;
        counts[3] = open - gained;
        counts[4] = tot ? (unsigned)tot[1] : 0u;
        counts[5] = counts[6] = 0u;
        counts[7] = (npix && !seeds) ? kExpandNoSeed : 0u;
    }
}

unsigned exp_blocks(size_t n) { return (unsigned)((n + kExpBlock - 1) / kExpBlock); }

template <class T>
hipError_t launch_expand_t(const T* plane, unsigned H, unsigned W, unsigned open_value, unsigned reach, uint16_t* nx, uint16_t* S, unsigned long long* acc,
                           T* out, unsigned* dist2, unsigned* source, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    const unsigned tilesX = (W + 63) / 64;
    const bool sums = table || counts;
    unsigned long long* keys = acc + kExpTotWords;
    unsigned* sg = (unsigned*)(keys + rows);
    if (sums) hipLaunchKernelGGL(expand_clear_kernel, dim3(exp_blocks(kExpTotWords + 2 * (size_t)rows)), dim3(kExpBlock), 0, s, acc, kExpTotWords + 2 * (size_t)rows);
    hipLaunchKernelGGL(expand_rows_kernel<T>, dim3(H), dim3(kExpBlock), 0, s, plane, W, open_value, nx);
    const size_t coarse = (size_t)((H + kExpCoarse - 1) / kExpCoarse) * tilesX;
    hipLaunchKernelGGL(expand_coarse_kernel, dim3((unsigned)((coarse + 3) / 4)), dim3(kExpBlock), 0, s, nx, H, W, tilesX, S);
    for (unsigned lv = kExpCoarse / 2; lv >= 1; lv >>= 1) {
        if (H <= lv) continue;  // no row y = lv mod 2 lv
        const size_t waves = (size_t)((H - lv + 2 * lv - 1) / (2 * lv)) * tilesX;
        hipLaunchKernelGGL(expand_refine_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(kExpBlock), 0, s, nx, H, W, tilesX, lv, S);
    }
    const size_t waves = (size_t)H * tilesX;
    hipLaunchKernelGGL(expand_finish_kernel<T>, dim3((unsigned)((waves + 3) / 4)), dim3(kExpBlock), 0, s, plane, nx, S, H, W, tilesX, open_value,
                       (unsigned long long)reach * reach, out, dist2, source, table ? keys : nullptr, sg, rows, counts ? acc : nullptr);
    if (sums)
        hipLaunchKernelGGL(expand_table_kernel, dim3(rows ? exp_blocks(rows) : 1u), dim3(kExpBlock), 0, s, keys, sg, acc, (unsigned long long)H * W, rows, table,
                           counts);
    return hipGetLastError();
}

}  // namespace

// [nx: one u16 per pixel][S: one u16 per pixel][the totals][keys: one u64 per row][sums: two u32 per row], on 256-byte boundaries
static size_t expand_plane_bytes(size_t npix) { return (npix * 2 + 255) & ~(size_t)255; }
size_t expand_scratch_bytes(size_t npix, unsigned rows) { return 2 * expand_plane_bytes(npix) + kExpTotWords * 8 + (((size_t)rows * 16 + 255) & ~(size_t)255); }

hipError_t launch_expand(const void* plane, int elem_bytes, unsigned H, unsigned W, unsigned open_value, unsigned reach, void* scratch, void* out,
                         unsigned* dist2, unsigned* source, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    if (!rows) table = nullptr;
    if (!table) rows = 0;
    const size_t npix = (size_t)H * W;
    if (npix == 0) {
        if (table || counts)
            hipLaunchKernelGGL(expand_table_kernel, dim3(rows ? exp_blocks(rows) : 1u), dim3(kExpBlock), 0, s, nullptr, nullptr, nullptr, 0ull, rows, table, counts);
        return hipGetLastError();
    }
    if (W > kExpandMaxSide || H > kExpandMaxSide) return hipErrorInvalidValue;
    uint16_t* nx = (uint16_t*)scratch;
    uint16_t* S = (uint16_t*)((uint8_t*)scratch + expand_plane_bytes(npix));
    unsigned long long* acc = (unsigned long long*)((uint8_t*)scratch + 2 * expand_plane_bytes(npix));
    if (elem_bytes == 1)
        return launch_expand_t((const uint8_t*)plane, H, W, open_value, reach, nx, S, acc, (uint8_t*)out, dist2, source, table, rows, counts, s);
    if (elem_bytes == 4)
        return launch_expand_t((const uint32_t*)plane, H, W, open_value, reach, nx, S, acc, (uint32_t*)out, dist2, source, table, rows, counts, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
