// anchors.hip -- Anchors: the exact squared Euclidean distance transform of a byte or u32 plane by value, and per value the most
// interior pixel (include/infur_hip.h).  The stage behind Regions and Tracks that measures how thick a region is:
// a caption, a click target or a "where is it" answer sits at the anchor, not at a centroid that may lie off the object.
// Separable, one memset and three launches -- the kernel boundaries are the only ordering, no workgroup ever waits for another:
//   1 rows    one workgroup per row.  g(x, y) = the horizontal distance to the nearest differing position of row y, the frame
//             included: min(x - s + 1, e - x + 1) for the row run [s, e] around x, as a u16 plane.  Runs inside 64 columns come
//             from one ballot (wave_scan.h); each tile of 64 leaves its first and last value and the lengths of its leading and
//             trailing run in LDS, and one thread per tile walks its neighbours for what a run has beyond the tile
//   2 columns one lane per pixel, a wave is 64 columns of one row.  dist2 = min over y' of (y - y')^2 + f(y')^2, f = g where the
//             column holds the pixel's value and 0 at the first differing position or the frame: the walk dy = 1, 2, .. up and
//             down stops once dy^2 >= best, so its length is the pixel's own distance.  Then the key (dist2 << 32) | (~index)
//             takes a segmented maximum over each run of equal values of the wave and the run's head lane issues at most one
//             64-bit atomicMax into the scratch row of its value (none when the row already holds more)
//   3 table   key -> (PIXEL, DIST2); a row no pixel reached reads (INFUR_ANCHOR_NONE, 0)
// Everything is an integer and a function of the plane alone; maxima commute, so the bytes do not depend on scheduling.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kAnchBlock = 256;
constexpr int kAnchMaxTiles = 1024;  // 65535 columns in tiles of 64
constexpr unsigned kAnchNone = 0xFFFFFFFFu;

template <class T>
__global__ void __launch_bounds__(kAnchBlock)
    anchors_rows_kernel(const T* __restrict__ plane, unsigned W, int skip, unsigned skip_value, uint16_t* __restrict__ g) {
    // per tile: the values of its first and last column, lead | trail << 8 (the run lengths at its two ends, 0 = not kept), and
    // what the two runs have beyond the tile
    __shared__ unsigned firstv[kAnchMaxTiles], lastv[kAnchMaxTiles], ends[kAnchMaxTiles], more_l[kAnchMaxTiles], more_r[kAnchMaxTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tiles = (W + 63) / 64;
    const size_t row0 = (size_t)blockIdx.x * W;

    for (unsigned t = wave; t < tiles; t += kAnchBlock / 64) {
        const unsigned x = t * 64 + lane, nin = W - t * 64 < 64 ? W - t * 64 : 64;
        const bool in = x < W;
        const unsigned v = in ? (unsigned)plane[row0 + x] : 0u;
        const bool kept = in && !(skip && v == skip_value);
        bool cont;
        const uint64_t starts = wave_run_starts(v, kept, &cont);
        const uint64_t keptm = __ballot(kept);
        const unsigned v0 = __shfl(v, 0, 64), v1 = __shfl(v, (int)nin - 1, 64);
        if (lane == 0) {
            const unsigned lead = (keptm & 1ull) ? run_length(starts, 0) : 0u;
            const unsigned trail = ((keptm >> (nin - 1)) & 1ull) ? nin - run_start(starts, (int)nin - 1) : 0u;
            firstv[t] = v0;
            lastv[t] = v1;
            ends[t] = lead | (trail << 8);
        }
    }
    __syncthreads();
    for (unsigned t = threadIdx.x; t < tiles; t += kAnchBlock) {
        const unsigned lead = ends[t] & 255u, trail = ends[t] >> 8;
        unsigned l = 0, r = 0;
        if (lead)  // (every tile to the left has 64 columns: a trailing run of 64 is the whole tile)
            for (unsigned u = t; u-- > 0;) {
                const unsigned n = ends[u] >> 8;
                if (!n || lastv[u] != firstv[t]) break;
                l += n;
                if (n < 64) break;
            }
        if (trail)
            for (unsigned u = t + 1; u < tiles; u++) {
                const unsigned n = ends[u] & 255u;
                if (!n || firstv[u] != lastv[t]) break;
                r += n;
                if (n < 64) break;
            }
        more_l[t] = l;
        more_r[t] = r;
    }
    __syncthreads();
    for (unsigned t = wave; t < tiles; t += kAnchBlock / 64) {
        const unsigned x = t * 64 + lane, nin = W - t * 64 < 64 ? W - t * 64 : 64;
        const bool in = x < W;
        const unsigned v = in ? (unsigned)plane[row0 + x] : 0u;
        const bool kept = in && !(skip && v == skip_value);
        bool cont;
        const uint64_t starts = wave_run_starts(v, kept, &cont);
        const unsigned s = run_start(starts, lane), e = s + run_length(starts, (int)s) - 1u;
        const unsigned left = (unsigned)lane - s + 1u + (s == 0 ? more_l[t] : 0u);
        const unsigned right = e - (unsigned)lane + 1u + (e == nin - 1 ? more_r[t] : 0u);
        if (in) g[row0 + x] = kept ? (uint16_t)(left < right ? left : right) : (uint16_t)0;  // (at most 32768)
    }
}

template <class T>
__global__ void __launch_bounds__(kAnchBlock)
    anchors_cols_kernel(const T* __restrict__ plane, const uint16_t* __restrict__ g, unsigned H, unsigned W, unsigned tilesX, int skip,
                        unsigned skip_value, unsigned* __restrict__ dist2, unsigned long long* __restrict__ keys, unsigned rows) {
    const WaveRow r = wave_row(H, W, tilesX);
    const int lane = threadIdx.x & 63;
    const unsigned v = r.live ? (unsigned)plane[r.at] : 0u;
    const bool kept = r.live && !(skip && v == skip_value);
    unsigned best = 0;
    if (kept) {
        const unsigned g0 = g[r.at];
        best = g0 * g0;  // (at most 2^30; below, dy^2 < best before f^2 <= 2^30 is added)
        const T* col = plane + r.x;
        const uint16_t* gcol = g + r.x;
        for (unsigned dy = 1;; dy++) {  // up
            const unsigned d2 = dy * dy;
            if (d2 >= best) break;
            if (dy > r.y) { best = d2; break; }
            const size_t at = (size_t)(r.y - dy) * W;
            if ((unsigned)col[at] != v) { best = d2; break; }
            const unsigned f = gcol[at], cand = d2 + f * f;
            best = cand < best ? cand : best;
        }
        for (unsigned dy = 1;; dy++) {  // down
            const unsigned d2 = dy * dy;
            if (d2 >= best) break;
            if (dy >= H - r.y) { best = d2; break; }
            const size_t at = (size_t)(r.y + dy) * W;
            if ((unsigned)col[at] != v) { best = d2; break; }
            const unsigned f = gcol[at], cand = d2 + f * f;
            best = cand < best ? cand : best;
        }
    }
    if (dist2 && r.live) dist2[r.at] = best;
    if (!keys) return;  // (uniform)
    unsigned long long key = kept ? ((unsigned long long)best << 32) | (unsigned long long)(kAnchNone - (unsigned)r.at) : 0ull;
    bool cont;
    const uint64_t starts = wave_run_starts(v, kept, &cont);
    const unsigned s = run_start(starts, lane), e = s + run_length(starts, (int)s) - 1u;
    for (int d = 1; d < 64; d <<= 1) {  // lane i: the maximum over [i, min(i + 2d - 1, e)]
        const unsigned long long o = __shfl_down(key, d, 64);
        if ((unsigned)lane + d <= e && o > key) key = o;
    }
    // A row only grows, so a key that does not beat what the row held a moment ago cannot beat what it holds now: most heads
    // skip the atomic (a plane of noise has a head per pixel and three rows to send them to), and the row ends the same.
    if (kept && (unsigned)lane == s && v < rows && key > __hip_atomic_load(&keys[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&keys[v], key);
}

// keys == nullptr: every row reads NONE (an empty plane)
__global__ void __launch_bounds__(kAnchBlock) anchors_table_kernel(const unsigned long long* __restrict__ keys, unsigned rows, unsigned* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kAnchBlock + threadIdx.x;
    if (i >= rows) return;
    const unsigned long long k = keys ? keys[i] : 0ull;  // (a kept pixel has dist2 >= 1: 0 is "no pixel")
    out[i * kAnchorWords + 0] = k ? kAnchNone - (unsigned)k : kAnchNone;
    out[i * kAnchorWords + 1] = (unsigned)(k >> 32);
}

template <class T>
hipError_t launch_anchors_t(const T* plane, unsigned H, unsigned W, int skip, unsigned skip_value, uint16_t* g, unsigned long long* keys, unsigned* dist2,
                            unsigned* anchors, unsigned rows, hipStream_t s) {
    const unsigned tilesX = (W + 63) / 64;
    const size_t waves = (size_t)H * tilesX;
    if (anchors) {
        const hipError_t e = hipMemsetAsync(keys, 0, (size_t)rows * 8, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(anchors_rows_kernel<T>, dim3(H), dim3(kAnchBlock), 0, s, plane, W, skip, skip_value, g);
    hipLaunchKernelGGL(anchors_cols_kernel<T>, dim3((unsigned)((waves + 3) / 4)), dim3(kAnchBlock), 0, s, plane, g, H, W, tilesX, skip, skip_value, dist2,
                       anchors ? keys : nullptr, rows);
    if (anchors)
        hipLaunchKernelGGL(anchors_table_kernel, dim3((rows + kAnchBlock - 1) / kAnchBlock), dim3(kAnchBlock), 0, s, keys, rows, anchors);
    return hipGetLastError();
}

}  // namespace

// [g: one u16 per pixel][keys: one u64 per row], on 256-byte boundaries
size_t anchors_keys_offset(size_t npix) { return (npix * 2 + 255) & ~(size_t)255; }
size_t anchors_scratch_bytes(size_t npix, unsigned rows) { return anchors_keys_offset(npix) + (((size_t)rows * 8 + 255) & ~(size_t)255); }

hipError_t launch_anchors(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, void* scratch, unsigned* dist2,
                          unsigned* anchors, unsigned rows, hipStream_t s) {
    if (!rows) anchors = nullptr;
    if ((size_t)H * W == 0) {
        if (anchors) hipLaunchKernelGGL(anchors_table_kernel, dim3((rows + kAnchBlock - 1) / kAnchBlock), dim3(kAnchBlock), 0, s, nullptr, rows, anchors);
        return hipGetLastError();
    }
    if (W > 65535u || H > 65535u) return hipErrorInvalidValue;
    uint16_t* g = (uint16_t*)scratch;
    unsigned long long* keys = (unsigned long long*)((uint8_t*)scratch + anchors_keys_offset((size_t)H * W));
    if (elem_bytes == 1) return launch_anchors_t((const uint8_t*)plane, H, W, skip, skip_value, g, keys, dist2, anchors, rows, s);
    if (elem_bytes == 4) return launch_anchors_t((const uint32_t*)plane, H, W, skip, skip_value, g, keys, dist2, anchors, rows, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
