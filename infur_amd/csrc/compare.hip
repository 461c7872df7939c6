// compare.hip -- Compare: the confusion matrix and the per-value best partner between two planes (include/infur_hip.h).
// The stage that says how good a result is: a class plane against ground truth (pixel accuracy, IoU per class), two arithmetic
// modes against each other, a label plane against ground-truth instances (IoU per object, panoptic quality).  The planes are
// H x W of 1- or 4-byte elements each; a pixel is ignored, outside (a >= rows_a or b >= rows_b) or inside, and only inside pixels
// reach the matrix and the rows.  Two forms, chosen by rows_a * rows_b alone; the kernel boundaries are the only ordering, no
// workgroup ever waits for another:
//   dense (rows_a * rows_b <= 4096)   one memset, four launches
//     1 dense    a bounded grid; a workgroup walks wave-rows (64 columns of one row per wave), one ballot of "the (i, j) key
//                differs from the left lane's" (wave_run_starts), the head lane of each run adds the run length to the
//                workgroup's matrix in LDS; at the end the non-zero entries go to the scratch matrix with global adds
//     2 lines    one wave per row and per column of the scratch matrix: its sum (PIXELS), its largest entry with the smallest
//                index (the partner), PAIRS; the caller's matrix
//     3 rows, 4 counts   as below
//   table (everything larger)         two memsets (a third for a wanted matrix), five launches
//     1 count    R = the runs of equal inside pairs along wave-rows, and the pixel classes.  2 R > slots is the overflow rule
//     2 insert   the head lane of each run: one add of the run length to PIXELS of i and of j (and to the matrix, when wanted),
//                then -- unless the table overflows -- a 64-bit CAS of (i << 32) | j into an open-addressing table and one
//                non-returning add of the run length.  Inside this kernel the table is touched by atomics only
//     3 choose   one lane per slot: atomicMax of (inter << 32) | (0xFFFFFFFF - partner) into best_a[i] and best_b[j]; PAIRS
//     4 rows     one lane per row of either side: (PIXELS, PARTNER, INTER, UNION); MATCHED from one ballot per wave
//     5 counts   the eight words
// The slot a pair lands in depends on timing and never reaches an output; everything else is a sum or a maximum of integers,
// which commute: the bytes written do not depend on the order in which atomics arrive.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kCmpBlock = 256;
constexpr unsigned kCmpNone = 0xFFFFFFFFu;
constexpr unsigned long long kCmpDead = ~0ull;
constexpr unsigned kCmpDenseGrid = 2048;  // eight workgroups of 16 KB on each of 256 CUs

// the accumulators at the head of the scratch, cleared by the call's memset
enum { kAccIgnored = 0, kAccOutside, kAccEqual, kAccRuns, kAccPairs, kAccMatched, kAccWords = 8 };

struct CmpIn {
    const void *a, *b;
    unsigned H, W, tilesX;
    unsigned ign_a, ign_b, ignore_a, ignore_b;  // ign_*: the side has an ignored value
    unsigned rows_a, rows_b;
};

// The scratch of a call, u32 words unless noted: [acc 8][pix_a rows_a][pix_b rows_b][best_a rows_a u64][best_b rows_b u64], then
// the dense form's matrix [rows_a * rows_b] or the table's [cnts slots][keys slots u64].  Everything in front of keys is cleared
// to 0 by one memset, keys to all ones by a second.
struct CmpMem {
    unsigned *acc, *pix_a, *pix_b;
    unsigned long long *best_a, *best_b;
    unsigned* mat;  // dense
    unsigned* cnts;  // table
    unsigned long long* keys;
    unsigned slots;
    size_t zero_bytes, bytes;
};

__host__ CmpMem cmp_layout(void* scratch, unsigned rows_a, unsigned rows_b, bool dense, unsigned slots) {
    CmpMem m{};
    uint8_t* p = (uint8_t*)scratch;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return p + o;
    };
    m.acc = (unsigned*)take(kAccWords * 4);
    m.pix_a = (unsigned*)take((size_t)rows_a * 4);
    m.pix_b = (unsigned*)take((size_t)rows_b * 4);
    m.best_a = (unsigned long long*)take((size_t)rows_a * 8);
    m.best_b = (unsigned long long*)take((size_t)rows_b * 8);
    if (dense) {
        m.mat = (unsigned*)take((size_t)rows_a * rows_b * 4);
        m.zero_bytes = at;
    } else {
        m.cnts = (unsigned*)take((size_t)slots * 4);
        m.zero_bytes = at;
        m.keys = (unsigned long long*)take((size_t)slots * 8);
        m.slots = slots;
    }
    m.bytes = at;
    return m;
}

// wave-row u of the plane (wave_scan.h's wave_row numbers them by blockIdx; the dense form walks several per workgroup)
__device__ __forceinline__ WaveRow cmp_wave_row(const size_t u, unsigned H, unsigned W, unsigned tilesX) {
    WaveRow r;
    r.y = (unsigned)(u / tilesX);
    r.x = (unsigned)(u % tilesX) * 64 + (threadIdx.x & 63);
    r.live = r.y < H && r.x < W;
    r.at = (size_t)r.y * W + r.x;
    return r;
}

// What one lane sees of its pixel: the pair key (i << 32) | j of an inside pixel, else kCmpDead; the pixel's class as ballots.
struct CmpPixel {
    unsigned long long key;
    uint64_t ignored, outside, equal, starts;  // wave masks
    bool head;                                 // this lane starts a run of an inside pair
};
template <class TA, class TB>
__device__ __forceinline__ CmpPixel cmp_pixel(const CmpIn& in, const WaveRow& r) {
    unsigned va = 0, vb = 0;
    if (r.live) {
        va = (unsigned)((const TA*)in.a)[r.at];
        vb = (unsigned)((const TB*)in.b)[r.at];
    }
    const bool ign = r.live && ((in.ign_a && va == in.ignore_a) || (in.ign_b && vb == in.ignore_b));
    const bool cmp = r.live && !ign;
    const bool inside = cmp && va < in.rows_a && vb < in.rows_b;
    CmpPixel p;
    p.key = inside ? ((unsigned long long)va << 32) | vb : kCmpDead;
    p.ignored = __ballot(ign);
    p.outside = __ballot(cmp && !inside);
    p.equal = __ballot(inside && va == vb);
    bool cont;
    p.starts = wave_run_starts(p.key, inside, &cont);
    p.head = inside && !cont;
    return p;
}

// ---- dense form ----
template <class TA, class TB>
__global__ void __launch_bounds__(kCmpBlock) compare_dense_kernel(CmpIn in, CmpMem m, size_t waveRows) {
    __shared__ unsigned lmat[kCmpDenseMax];
    __shared__ unsigned lacc[4];
    const unsigned entries = in.rows_a * in.rows_b;
    for (unsigned e = threadIdx.x; e < entries; e += kCmpBlock) lmat[e] = 0u;
    if (threadIdx.x < 4) lacc[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // (u is the same in all lanes of a wave: the ballots below are taken by whole waves)
    for (size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < waveRows; u += (size_t)gridDim.x * 4) {
        const WaveRow r = cmp_wave_row(u, in.H, in.W, in.tilesX);
        const CmpPixel p = cmp_pixel<TA, TB>(in, r);
        if (p.head) atomicAdd(&lmat[(unsigned)(p.key >> 32) * in.rows_b + (unsigned)p.key], run_length(p.starts, lane));
        const uint64_t heads = __ballot(p.head);
        if (lane == 0) {
            if (p.ignored) atomicAdd(&lacc[kAccIgnored], (unsigned)__popcll(p.ignored));
            if (p.outside) atomicAdd(&lacc[kAccOutside], (unsigned)__popcll(p.outside));
            if (p.equal) atomicAdd(&lacc[kAccEqual], (unsigned)__popcll(p.equal));
            if (heads) atomicAdd(&lacc[kAccRuns], (unsigned)__popcll(heads));
        }
    }
    __syncthreads();
    for (unsigned e = threadIdx.x; e < entries; e += kCmpBlock) {
        const unsigned n = lmat[e];
        if (n) atomicAdd(&m.mat[e], n);
    }
    if (threadIdx.x < 4 && lacc[threadIdx.x]) atomicAdd(&m.acc[threadIdx.x], lacc[threadIdx.x]);
}

// one wave per line of the scratch matrix: wave l < rows_a is row l, the others are the columns
__global__ void __launch_bounds__(kCmpBlock) compare_lines_kernel(CmpMem m, unsigned rows_a, unsigned rows_b, unsigned* __restrict__ matrix) {
    const size_t l = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (l >= (size_t)rows_a + rows_b) return;  // (by whole waves)
    const bool row = l < rows_a;
    const unsigned at = row ? (unsigned)l : (unsigned)(l - rows_a), len = row ? rows_b : rows_a;
    const size_t first = row ? (size_t)at * rows_b : at, step = row ? 1 : rows_b;
    unsigned sum = 0, pairs = 0;
    unsigned long long best = 0ull;
    for (unsigned k = lane; k < len; k += 64) {
        const unsigned n = m.mat[first + k * step];
        if (row && matrix) matrix[first + k] = n;
        if (!n) continue;
        sum += n;
        pairs++;
        const unsigned long long key = ((unsigned long long)n << 32) | (kCmpNone - k);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        pairs += __shfl_xor(pairs, d, 64);
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if (lane) return;
    (row ? m.pix_a : m.pix_b)[at] = sum;
    (row ? m.best_a : m.best_b)[at] = best;
    if (row && pairs) atomicAdd(&m.acc[kAccPairs], pairs);
}

// ---- table form ----
__device__ __forceinline__ unsigned cmp_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}

__device__ __forceinline__ bool cmp_overflow(const CmpMem& m) { return 2ull * m.acc[kAccRuns] > (unsigned long long)m.slots; }

template <class TA, class TB>
__global__ void __launch_bounds__(kCmpBlock) compare_count_kernel(CmpIn in, CmpMem m) {
    __shared__ unsigned lacc[4];
    if (threadIdx.x < 4) lacc[threadIdx.x] = 0u;
    __syncthreads();
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const CmpPixel p = cmp_pixel<TA, TB>(in, r);
    const uint64_t heads = __ballot(p.head);
    if ((threadIdx.x & 63) == 0) {
        if (p.ignored) atomicAdd(&lacc[kAccIgnored], (unsigned)__popcll(p.ignored));
        if (p.outside) atomicAdd(&lacc[kAccOutside], (unsigned)__popcll(p.outside));
        if (p.equal) atomicAdd(&lacc[kAccEqual], (unsigned)__popcll(p.equal));
        if (heads) atomicAdd(&lacc[kAccRuns], (unsigned)__popcll(heads));
    }
    __syncthreads();
    if (threadIdx.x < 4 && lacc[threadIdx.x]) atomicAdd(&m.acc[threadIdx.x], lacc[threadIdx.x]);
}

template <class TA, class TB>
__global__ void __launch_bounds__(kCmpBlock) compare_insert_kernel(CmpIn in, CmpMem m, unsigned* __restrict__ matrix) {
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const CmpPixel p = cmp_pixel<TA, TB>(in, r);
    if (!p.head) return;
    const unsigned n = run_length(p.starts, threadIdx.x & 63), i = (unsigned)(p.key >> 32), j = (unsigned)p.key;
    (void)__hip_atomic_fetch_add(m.pix_a + i, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(m.pix_b + j, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (matrix) (void)__hip_atomic_fetch_add(matrix + (size_t)i * in.rows_b + j, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cmp_overflow(m)) return;
    const unsigned mask = m.slots - 1;
    unsigned s = cmp_hash(p.key, mask);
    for (unsigned it = 0; it < m.slots; it++) {  // at most half the slots are ever taken: the loop ends long before its bound
        unsigned long long old = kCmpDead;
        __hip_atomic_compare_exchange_strong(m.keys + s, &old, p.key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kCmpDead || old == p.key) {
            (void)__hip_atomic_fetch_add(m.cnts + s, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        s = (s + 1) & mask;
    }
}

__global__ void __launch_bounds__(kCmpBlock) compare_choose_kernel(CmpMem m) {
    const size_t s = (size_t)blockIdx.x * kCmpBlock + threadIdx.x;
    const bool full = s < m.slots && !cmp_overflow(m) && m.keys[s] != kCmpDead;
    if (full) {
        const unsigned long long key = m.keys[s];
        const unsigned i = (unsigned)(key >> 32), j = (unsigned)key;
        const unsigned long long inter = (unsigned long long)m.cnts[s] << 32;
        atomicMax(m.best_a + i, inter | (kCmpNone - j));
        atomicMax(m.best_b + j, inter | (kCmpNone - i));
    }
    const uint64_t any = __ballot(full);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&m.acc[kAccPairs], (unsigned)__popcll(any));
}

// ---- both forms ----
// One lane per row: lane t < rows_a writes row t of a's table, the others b's.  pix == nullptr (an empty plane): every row NONE.
__global__ void __launch_bounds__(kCmpBlock) compare_rows_kernel(CmpMem m, unsigned rows_a, unsigned rows_b, unsigned* __restrict__ out_a,
                                                                 unsigned* __restrict__ out_b) {
    const size_t t = (size_t)blockIdx.x * kCmpBlock + threadIdx.x;
    const bool live = t < (size_t)rows_a + rows_b, side_a = t < rows_a;
    const size_t at = side_a ? t : t - rows_a;
    unsigned pix = 0, partner = kCmpNone, inter = 0, uni = 0;
    if (live && m.pix_a) {
        pix = (side_a ? m.pix_a : m.pix_b)[at];
        const unsigned long long best = (side_a ? m.best_a : m.best_b)[at];
        if (best) {  // (an inside pixel and no partner: the table overflowed)
            partner = kCmpNone - (unsigned)best;
            inter = (unsigned)(best >> 32);
            uni = pix + (side_a ? m.pix_b : m.pix_a)[partner] - inter;
        }
    }
    unsigned* out = side_a ? out_a : out_b;
    if (live && out) {
        out[at * kCompareWords + 0] = pix;
        out[at * kCompareWords + 1] = partner;
        out[at * kCompareWords + 2] = inter;
        out[at * kCompareWords + 3] = uni;
    }
    const uint64_t matched = __ballot(live && side_a && 2ull * inter > uni);
    if (m.acc && (threadIdx.x & 63) == 0 && matched) atomicAdd(&m.acc[kAccMatched], (unsigned)__popcll(matched));
}

__global__ void compare_counts_kernel(CmpMem m, unsigned long long npix, int table, unsigned* __restrict__ counts) {
    const unsigned ignored = m.acc[kAccIgnored];
    counts[0] = (unsigned)(npix - ignored);
    counts[1] = m.acc[kAccEqual];
    counts[2] = ignored;
    counts[3] = m.acc[kAccOutside];
    counts[4] = m.acc[kAccPairs];
    counts[5] = m.acc[kAccMatched];
    counts[6] = m.acc[kAccRuns];
    counts[7] = table ? (kCmpTable | (cmp_overflow(m) ? kCmpOverflow : 0u)) : 0u;
}

template <class TA, class TB>
hipError_t launch_compare_t(const CmpIn& in, const CmpMem& m, bool dense, unsigned* matrix, unsigned* rows_a_out, unsigned* rows_b_out, unsigned* counts,
                            hipStream_t s) {
    const size_t waveRows = (size_t)in.H * in.tilesX, rowBlocks = (waveRows + 3) / 4;
    const size_t lines = (size_t)in.rows_a + in.rows_b;
    if (rowBlocks > 0x7FFFFFFFull || (lines + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m.acc, 0, m.zero_bytes, s);
    if (e != hipSuccess) return e;
    if (dense) {
        const unsigned grid = rowBlocks < kCmpDenseGrid ? (unsigned)rowBlocks : kCmpDenseGrid;
        hipLaunchKernelGGL((compare_dense_kernel<TA, TB>), dim3(grid), dim3(kCmpBlock), 0, s, in, m, waveRows);
        if (lines) hipLaunchKernelGGL(compare_lines_kernel, dim3((unsigned)((lines + 3) / 4)), dim3(kCmpBlock), 0, s, m, in.rows_a, in.rows_b, matrix);
    } else {
        e = hipMemsetAsync(m.keys, 0xFF, (size_t)m.slots * 8, s);
        if (e == hipSuccess && matrix) e = hipMemsetAsync(matrix, 0, (size_t)in.rows_a * in.rows_b * 4, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((compare_count_kernel<TA, TB>), dim3((unsigned)rowBlocks), dim3(kCmpBlock), 0, s, in, m);
        hipLaunchKernelGGL((compare_insert_kernel<TA, TB>), dim3((unsigned)rowBlocks), dim3(kCmpBlock), 0, s, in, m, matrix);
        hipLaunchKernelGGL(compare_choose_kernel, dim3((m.slots + kCmpBlock - 1) / kCmpBlock), dim3(kCmpBlock), 0, s, m);
    }
    if (lines)
        hipLaunchKernelGGL(compare_rows_kernel, dim3((unsigned)((lines + kCmpBlock - 1) / kCmpBlock)), dim3(kCmpBlock), 0, s, m, in.rows_a, in.rows_b,
                           rows_a_out, rows_b_out);
    if (counts) hipLaunchKernelGGL(compare_counts_kernel, dim3(1), dim3(1), 0, s, m, (unsigned long long)in.H * in.W, dense ? 0 : 1, counts);
    return hipGetLastError();
}

}  // namespace

bool compare_dense(unsigned rows_a, unsigned rows_b) { return (unsigned long long)rows_a * rows_b <= (unsigned long long)kCmpDenseMax; }

size_t compare_scratch_bytes(unsigned rows_a, unsigned rows_b, unsigned pair_slots) {
    return cmp_layout(nullptr, rows_a, rows_b, compare_dense(rows_a, rows_b), pair_slots).bytes;
}

hipError_t launch_compare(const void* a, int elem_a, const void* b, int elem_b, unsigned H, unsigned W, int ign_a, unsigned ignore_a, int ign_b,
                          unsigned ignore_b, unsigned rows_a, unsigned rows_b, void* scratch, unsigned pair_slots, unsigned* matrix, unsigned* rows_a_out,
                          unsigned* rows_b_out, unsigned* counts, hipStream_t s) {
    if (W > 65535u || H > 65535u) return hipErrorInvalidValue;
    if (!rows_a || !rows_b) matrix = nullptr;
    if (!rows_a) rows_a_out = nullptr;
    if (!rows_b) rows_b_out = nullptr;
    if ((size_t)H * W == 0) {  // zeros and NONE rows, and nothing else: no scratch
        hipError_t e = hipSuccess;
        if (matrix) e = hipMemsetAsync(matrix, 0, (size_t)rows_a * rows_b * 4, s);
        if (e == hipSuccess && counts) e = hipMemsetAsync(counts, 0, kCompareCountWords * 4, s);
        if (e != hipSuccess) return e;
        const size_t lines = (size_t)(rows_a_out ? rows_a : 0) + (rows_b_out ? rows_b : 0);
        if (lines)
            hipLaunchKernelGGL(compare_rows_kernel, dim3((unsigned)((lines + kCmpBlock - 1) / kCmpBlock)), dim3(kCmpBlock), 0, s, CmpMem{},
                               rows_a_out ? rows_a : 0u, rows_b_out ? rows_b : 0u, rows_a_out, rows_b_out);
        return hipGetLastError();
    }
    const bool dense = compare_dense(rows_a, rows_b);
    if (!dense && (pair_slots < 64 || (pair_slots & (pair_slots - 1)))) return hipErrorInvalidValue;
    const CmpMem m = cmp_layout(scratch, rows_a, rows_b, dense, pair_slots);
    const CmpIn in{a, b, H, W, (W + 63) / 64, ign_a ? 1u : 0u, ign_b ? 1u : 0u, ignore_a, ignore_b, rows_a, rows_b};
    if (elem_a == 1 && elem_b == 1) return launch_compare_t<uint8_t, uint8_t>(in, m, dense, matrix, rows_a_out, rows_b_out, counts, s);
    if (elem_a == 1 && elem_b == 4) return launch_compare_t<uint8_t, uint32_t>(in, m, dense, matrix, rows_a_out, rows_b_out, counts, s);
    if (elem_a == 4 && elem_b == 1) return launch_compare_t<uint32_t, uint8_t>(in, m, dense, matrix, rows_a_out, rows_b_out, counts, s);
    if (elem_a == 4 && elem_b == 4) return launch_compare_t<uint32_t, uint32_t>(in, m, dense, matrix, rows_a_out, rows_b_out, counts, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
