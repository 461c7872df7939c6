// regions.hip -- Regions: connected components of the class plane (include/infur_hip.h).  The third decode stage
// behind Segments: from the class bytes (and optionally the confidence bytes) a u32 label plane, a per-region table and the
// region count.  A block-based union-find over parent[h*w] (u32; a root is the smallest linear index of its set), in separate
// launches -- the kernel boundaries are the only ordering between the phases, no workgroup ever waits for another:
//   1 tile      64 x 32 tiles labelled in LDS: horizontal runs from one ballot per wave-row (wave_run_starts), vertical /
//               diagonal links as unions between run heads, one flatten pass that stores each pixel's tile root as a global index
//   2 seam      one lane per pixel on a tile border: find + union-by-min over the global array, relaxed agent-scope atomics only
//   3 flatten   every pixel finds its root; per-root pixel counts, one atomic per run of a wave-row
//   4 scan      kept roots (count >= min_pixels, not class 0 under the skip flag) flagged, exclusive prefix sum in raster order
//               = dense ids in ascending order of the root index: flag_block_sum, scan_block_sums, flag_rank
//   5 relabel   label plane (dword stores) and the table rows (64-bit integer atomics, one set per run of a wave-row)
// The scan, the wave-row (wave_row) and its runs are wave_scan.h's.  Everything is an integer and every id is a function of the
// partition alone, so the bytes do not depend on the order in which atomics arrive, on the tile shape or on the device.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kRegTW = 64, kRegTH = 32;  // tile: one wave-row wide, eight rows per wave
constexpr unsigned kRegNone = 0xFFFFFFFFu;

// ---- union-find in LDS (tile-local indices r * 64 + lane; the parent of a node is never larger than the node) ----
__device__ __forceinline__ unsigned lds_find(unsigned* lp, unsigned a) {
    unsigned p;  // (an atomic load: other waves unite concurrently, and the compiler must re-read the word)
    while ((p = __hip_atomic_load(lp + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a) a = p;
    return a;
}

// lock-free union by minimum: when the atomicMin displaced another link (old != a), the displaced parent is united next
__device__ __forceinline__ void lds_union(unsigned* lp, unsigned a, unsigned b) {
    for (;;) {
        a = lds_find(lp, a);
        b = lds_find(lp, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = atomicMin(&lp[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(256)
    regions_tile_kernel(const uint8_t* __restrict__ klass, unsigned H, unsigned W, unsigned tilesX, int conn8, unsigned* __restrict__ parent) {
    __shared__ unsigned lp[kRegTH * kRegTW];
    __shared__ short cls[kRegTH * kRegTW];  // -1: outside the image
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned x0 = (blockIdx.x % tilesX) * kRegTW, y0 = (blockIdx.x / tilesX) * kRegTH;
    const unsigned x = x0 + lane;
    // horizontal runs: the run start is the label, no per-pixel union
    for (int r = wave; r < kRegTH; r += 4) {
        const unsigned y = y0 + r;
        const bool live = x < W && y < H;
        const int c = live ? (int)klass[(size_t)y * W + x] : -1;
        bool cont;
        const uint64_t starts = wave_run_starts(c, live, &cont);
        lp[r * kRegTW + lane] = (unsigned)(r * kRegTW) + run_start(starts, lane);
        cls[r * kRegTW + lane] = (short)c;
    }
    __syncthreads();
    // vertical (and diagonal) links, once per pair of touching runs
    for (int r = wave ? wave : 4; r < kRegTH; r += 4) {
        const int i = r * kRegTW + lane;
        const int c = cls[i];
        if (c < 0) continue;
        const bool left = lane > 0 && cls[i - 1] == c, upleft = lane > 0 && cls[i - kRegTW - 1] == c;
        if (cls[i - kRegTW] == c) {
            if (!(left && upleft)) lds_union(lp, i, i - kRegTW);  // else the pixel to the left links the same two runs
        } else if (conn8) {
            if (upleft && !left) lds_union(lp, i, i - kRegTW - 1);  // (left: its own vertical link covers this one)
            if (lane < 63 && cls[i - kRegTW + 1] == c && cls[i + 1] != c) lds_union(lp, i, i - kRegTW + 1);
        }
    }
    __syncthreads();
    for (int r = wave; r < kRegTH; r += 4) {
        const int i = r * kRegTW + lane;
        if (cls[i] < 0) continue;
        const unsigned root = lds_find(lp, i);
        parent[(size_t)(y0 + r) * W + x] = (unsigned)((size_t)(y0 + root / kRegTW) * W + x0 + root % kRegTW);
    }
}

// ---- union-find over the global array, across workgroups: every access a relaxed agent-scope atomic (a plain load may be
// served from a line another XCD's L2 has since rewritten) ----
__device__ __forceinline__ unsigned g_find(unsigned* parent, unsigned a) {
    unsigned p;
    while ((p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = p;
    return a;
}

__device__ __forceinline__ void g_union(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = g_find(parent, a);
        b = g_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// items [0, nV): pixel (y, 64 k) of vertical seam k, every row; items [nV, total): pixel (32 j, x) of horizontal seam j.
// Each unites the pairs that cross its seam (pairs at a tile corner are seen from both seams: a second union is a no-op).
__global__ void __launch_bounds__(256) regions_seam_kernel(const uint8_t* __restrict__ klass, unsigned H, unsigned W, int conn8, size_t nV,
                                                           size_t total, unsigned* parent) {
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    if (it < nV) {
        const unsigned y = (unsigned)(it % H), x = (unsigned)(it / H + 1) * kRegTW;
        const unsigned i = (unsigned)((size_t)y * W + x);
        const uint8_t c = klass[i], cw = klass[i - 1];
        if (cw == c) g_union(parent, i, i - 1);
        if (conn8 && y > 0) {
            if (klass[i - W - 1] == c) g_union(parent, i, i - W - 1);
            if (klass[i - W] == cw) g_union(parent, i - 1, i - W);
        }
    } else {
        const size_t j = it - nV;
        const unsigned x = (unsigned)(j % W), y = (unsigned)(j / W + 1) * kRegTH;
        const unsigned i = (unsigned)((size_t)y * W + x);
        const uint8_t c = klass[i];
        if (klass[i - W] == c) g_union(parent, i, i - W);
        if (conn8) {
            if (x > 0 && klass[i - W - 1] == c) g_union(parent, i, i - W - 1);
            if (x + 1 < W && klass[i - W + 1] == c) g_union(parent, i, i - W + 1);
        }
    }
}

// every pixel finds its root (whatever a racing store of this pass has left in a word is an ancestor too); the pixel count of
// a root is pre-aggregated per run of equal roots in the wave-row: one atomic per run
__global__ void __launch_bounds__(256) regions_flatten_count_kernel(unsigned H, unsigned W, unsigned tilesX, unsigned* parent, unsigned* cnt) {
    const WaveRow p = wave_row(H, W, tilesX);
    const int lane = threadIdx.x & 63;
    unsigned root = kRegNone;
    if (p.live) {
        unsigned a = parent[p.at], q;
        while ((q = parent[a]) != a) a = q;
        parent[p.at] = root = a;
    }
    bool cont;
    const uint64_t starts = wave_run_starts(root, p.live, &cont);
    if (p.live && !cont) atomicAdd(&cnt[root], run_length(starts, lane));
}

__device__ __forceinline__ bool reg_keep(const size_t i, const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt,
                                         const uint8_t* __restrict__ klass, const unsigned min_pixels, const int skip_bg) {
    return parent[i] == (unsigned)i && cnt[i] >= min_pixels && !(skip_bg && klass[i] == 0);
}

// ---- the three-launch exclusive scan of the kept-root flags (wave_scan.h) ----
__global__ void __launch_bounds__(kScanBlock) regions_scan_sums_kernel(const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt,
                                                                       const uint8_t* __restrict__ klass, size_t N, unsigned min_pixels, int skip_bg,
                                                                       unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(i < N && reg_keep(i, parent, cnt, klass, min_pixels, skip_bg), wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: partial[] -> its exclusive prefix sums in place, the total to total[0] and, when wanted, to the caller's word
__global__ void __launch_bounds__(kScanBlock) regions_scan_partials_kernel(unsigned* __restrict__ partial, size_t NB, unsigned* __restrict__ total,
                                                                           unsigned* __restrict__ d_n) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) {
        total[0] = n;
        if (d_n) d_n[0] = n;
    }
}

// ids[i] = dense id of a kept root, INFUR_REGION_NONE for every other pixel
__global__ void __launch_bounds__(kScanBlock) regions_scan_apply_kernel(const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt,
                                                                        const uint8_t* __restrict__ klass, size_t N, unsigned min_pixels, int skip_bg,
                                                                        const unsigned* __restrict__ partial, unsigned* __restrict__ ids) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const bool keep = i < N && reg_keep(i, parent, cnt, klass, min_pixels, skip_bg);
    const unsigned id = flag_rank(keep, partial[blockIdx.x], wsum);
    if (i < N) ids[i] = keep ? id : kRegNone;
}

// rows [0, min(n, rows)) of the caller's table get the empty-row values; rows at or beyond n are left alone
__global__ void __launch_bounds__(256) regions_table_init_kernel(unsigned long long* __restrict__ table, unsigned rows, const unsigned* __restrict__ total) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned n = total[0] < rows ? total[0] : rows;
    if (r >= n) return;
    unsigned long long* row = table + r * kRegWords;
    row[0] = row[1] = row[2] = row[3] = row[6] = row[7] = 0ull;
    row[4] = row[5] = ~0ull;
}

// label plane + table.  Per run of equal roots in a wave-row its head lane applies the eight statistics words; the sum of the
// confidence bytes over the run comes from the eight ballots of their bit planes (BitPlanes8).
__global__ void __launch_bounds__(256)
    regions_relabel_kernel(const uint8_t* __restrict__ klass, const uint8_t* __restrict__ conf, unsigned H, unsigned W, unsigned tilesX,
                           const unsigned* __restrict__ parent, const unsigned* __restrict__ ids, unsigned* __restrict__ labels,
                           unsigned long long* __restrict__ table, unsigned rows) {
    const WaveRow p = wave_row(H, W, tilesX);
    const int lane = threadIdx.x & 63;
    const unsigned root = p.live ? parent[p.at] : kRegNone;
    const unsigned id = p.live ? ids[root] : kRegNone;
    if (labels && p.live) labels[p.at] = id;
    if (!table) return;
    const unsigned cf = (conf && p.live) ? conf[p.at] : 0u;
    const BitPlanes8 planes(cf, true);
    bool cont;
    const uint64_t starts = wave_run_starts(root, p.live, &cont);
    if (!p.live || id >= rows) return;
    unsigned long long* row = table + (size_t)id * kRegWords;
    if (!cont) {
        const unsigned long long n = run_length(starts, lane);
        const uint64_t run = (n == 64 ? ~0ull : ((1ull << n) - 1ull)) << lane;
        const unsigned long long sconf = planes.sum(run);
        atomicAdd(row + 0, n);
        atomicAdd(row + 1, n * p.x + n * (n - 1) / 2);
        atomicAdd(row + 2, n * p.y);
        if (sconf) atomicAdd(row + 3, sconf);
        atomicMin(row + 4, (unsigned long long)p.x);
        atomicMin(row + 5, (unsigned long long)p.y);
        atomicMax(row + 6, (unsigned long long)p.x + n - 1);
        atomicMax(row + 7, (unsigned long long)p.y);
    }
    if (root == (unsigned)p.at) {  // the root pixel's lane: no other lane writes these two words
        row[8] = klass[p.at];
        row[9] = p.at;
    }
}

inline size_t reg_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// parent, counts, ids (u32 per pixel each) + the scan's block sums + the total
size_t regions_scratch_bytes(size_t npix) { return 3 * reg_align(npix * 4) + reg_align(scan_blocks(npix) * 4) + 256; }

hipError_t launch_regions(const uint8_t* klass, const uint8_t* conf, unsigned H, unsigned W, int conn8, unsigned min_pixels, int skip_bg,
                          void* scratch, unsigned* labels, unsigned long long* table, unsigned rows, unsigned* d_n, hipStream_t s) {
    const size_t N = (size_t)H * W, NB = scan_blocks(N);
    const unsigned tilesX = (W + kRegTW - 1) / kRegTW, tilesY = (H + kRegTH - 1) / kRegTH;
    const size_t tiles = (size_t)tilesX * tilesY, rowBlocks = ((size_t)tilesX * H + 3) / 4;
    const size_t nV = (size_t)(tilesX - 1) * H, nSeam = nV + (size_t)(tilesY - 1) * W;
    if (tiles > 0x7FFFFFFFull || rowBlocks > 0x7FFFFFFFull || (nSeam + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint8_t* base = (uint8_t*)scratch;
    unsigned* parent = (unsigned*)base;
    unsigned* cnt = (unsigned*)(base + reg_align(N * 4));
    unsigned* ids = (unsigned*)(base + 2 * reg_align(N * 4));
    unsigned* partial = (unsigned*)(base + 3 * reg_align(N * 4));
    unsigned* total = (unsigned*)(base + 3 * reg_align(N * 4) + reg_align(NB * 4));
    hipError_t e = hipMemsetAsync(cnt, 0, N * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(regions_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, s, klass, H, W, tilesX, conn8, parent);
    if (nSeam)
        hipLaunchKernelGGL(regions_seam_kernel, dim3((unsigned)((nSeam + 255) / 256)), dim3(256), 0, s, klass, H, W, conn8, nV, nSeam, parent);
    hipLaunchKernelGGL(regions_flatten_count_kernel, dim3((unsigned)rowBlocks), dim3(256), 0, s, H, W, tilesX, parent, cnt);
    hipLaunchKernelGGL(regions_scan_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, parent, cnt, klass, N, min_pixels, skip_bg, partial);
    hipLaunchKernelGGL(regions_scan_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, partial, NB, total, d_n);
    if (labels || (table && rows)) {
        hipLaunchKernelGGL(regions_scan_apply_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, parent, cnt, klass, N, min_pixels, skip_bg, partial, ids);
        if (table && rows) {
            const size_t cap = rows < N ? rows : N;  // there are at most N regions
            hipLaunchKernelGGL(regions_table_init_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, table, rows, total);
        }
        hipLaunchKernelGGL(regions_relabel_kernel, dim3((unsigned)rowBlocks), dim3(256), 0, s, klass, conf, H, W, tilesX, parent, ids, labels,
                           (table && rows) ? table : nullptr, rows);
    }
    return hipGetLastError();
}

}  // namespace infur
