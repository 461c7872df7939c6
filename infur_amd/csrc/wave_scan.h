// wave_scan.h -- the two device idioms the decode stages behind Segments share (regions.hip, tracks.hip, runs.hip):
//   the flag scan  the exclusive prefix sum of one flag per element in three launches of kScanBlock lanes: block sums
//                  (flag_block_sum), one workgroup over the sums (scan_block_sums), rank of every element (flag_rank)
//   the wave-row   a wave is 64 consecutive columns of one row (wave_row); runs of equal keys along it from one ballot
//                  (wave_run_starts, run_start, run_length); sums of a byte over any lane mask from eight more (BitPlanes8)
// Device functions and constants only: every stage keeps its own thin kernels, so the names in a profile are the stage's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace infur {

constexpr int kScanBlock = 1024;  // elements per workgroup of the scan launches
__host__ __device__ constexpr size_t scan_blocks(const size_t n) { return (n + kScanBlock - 1) / kScanBlock; }

// -> the number of set flags in the workgroup of kBlock lanes, valid in thread 0.  wsum: kBlock / 64 words of LDS
template <int kBlock = kScanBlock>
__device__ __forceinline__ unsigned flag_block_sum(const bool flag, unsigned* wsum) {
    const uint64_t m = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kBlock / 64; k++) s += wsum[k];
    return s;
}

// -> block_base + the number of set flags before this lane in its workgroup: with the scanned block sum as block_base, the
// number before this element in the whole array.  Holds a barrier: call it before any divergent return.
__device__ __forceinline__ unsigned flag_rank(const bool flag, const unsigned block_base, unsigned* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = block_base;
    for (int k = 0; k < wave; k++) before += wsum[k];
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// One workgroup of kScanBlock lanes: partial[0, NB) -> its exclusive prefix sums in place; -> the total, in every thread.
// More than kScanBlock sums take further passes of the loop: Runs' test_more_than_1024_block_sums, Regions' 1080p planes,
// Outlines' million-edge checkerboard and Simplify's comb execute them with sums in every pass; tests/test_gpu_stage_limits.py
// executes them for Shapes' vertex scan and Coverage's scan over the augmented rows with zeros beyond the first pass (the carry
// into the total).  They stand in for Tracks too, which no test can give the million regions its own second pass would need
// (tests/stage_limits.py lists every such crossing and the test that reaches it).
__device__ __forceinline__ unsigned scan_block_sums(unsigned* __restrict__ partial, const size_t NB, unsigned* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;
    for (size_t base = 0; base < NB; base += kScanBlock) {
        const size_t i = base + threadIdx.x;
        const unsigned v = i < NB ? partial[i] : 0u;
        unsigned inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int k = 0; k < kScanBlock / 64; k++) {
            const unsigned s = wsum[k];
            before += k < wave ? s : 0u;
            all += s;
        }
        __syncthreads();
        if (i < NB) partial[i] = carry + before + inc - v;
        carry += all;
    }
    return carry;
}

// A wave is 64 consecutive columns of one row (four wave-rows per workgroup of 256, numbered in raster order).
struct WaveRow {
    unsigned x, y;
    bool live;
    size_t at;
};
__device__ __forceinline__ WaveRow wave_row(unsigned H, unsigned W, unsigned tilesX) {
    const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    WaveRow r;
    r.y = (unsigned)(u / tilesX);
    r.x = (unsigned)(u % tilesX) * 64 + (threadIdx.x & 63);
    r.live = r.y < H && r.x < W;
    r.at = (size_t)r.y * W + r.x;
    return r;
}

// -> the mask of the lanes that start a run of equal keys along the wave; *cont: this lane continues its left neighbour's run.
// A dead lane (outside the image, or a key that is not to be counted) is always a start.  A stage that lets dead lanes
// continue each other gets the same answers from this: it asks only live heads, a dead key never equals a live one, so the
// first dead lane behind a live run is a start under either convention and the run's length is the same.
template <class K>
__device__ __forceinline__ uint64_t wave_run_starts(const K key, const bool live, bool* cont) {
    const K left = __shfl_up(key, 1, 64);
    *cont = live && (threadIdx.x & 63) > 0 && key == left;
    return ~__ballot(*cont);
}

// start of the run lane `lane` belongs to, from the mask of run starts (bit 0 is always set)
__device__ __forceinline__ unsigned run_start(const uint64_t starts, const int lane) {
    return 63u - (unsigned)__builtin_clzll(starts & (~0ull >> (63 - lane)));
}

// length of the run that starts at `lane` (dead lanes count as starts, so a run ends at the image edge)
__device__ __forceinline__ unsigned run_length(const uint64_t starts, const int lane) {
    const uint64_t above = lane == 63 ? 0ull : (starts >> (lane + 1));
    return above ? (unsigned)__builtin_ctzll(above) + 1u : 64u - (unsigned)lane;
}

// The eight ballots of a byte's bit planes over the live lanes, taken once per wave-row: the sum of the byte over any lane
// mask then needs no cross-lane adds, sum = sum_b 2^b * popcount(mask & plane_b)  
struct BitPlanes8 {
    uint64_t plane[8];
    __device__ __forceinline__ BitPlanes8(const unsigned byte, const bool live) {
#pragma unroll
        for (int b = 0; b < 8; b++) plane[b] = __ballot(live && ((byte >> b) & 1u));
    }
    __device__ __forceinline__ unsigned sum(const uint64_t mask) const {
        unsigned s = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) s += (unsigned)__popcll(mask & plane[b]) << b;
        return s;
    }
};

}  // namespace infur
