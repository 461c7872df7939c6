// runs.hip -- Runs: a byte or u32 plane as raster-ordered runs (include/infur_hip.h).  The egress stage behind
// Segments, Regions and Tracks: records (START, END, VALUE), a per-row index and the count, so that a host fetches 12 bytes
// per run and not the dense plane.  One lane per pixel over the linear index, the flag scan of wave_scan.h, three launches -- the
// kernel boundaries are the only ordering, no workgroup ever waits for another:
//   1 sums      head(i) = the pixel starts a run that is emitted; flag_block_sum of it
//   2 partials  scan_block_sums: one workgroup, the block sums -> their exclusive prefix sums; the total
//   3 emit      the exclusive head count at a pixel (flag_rank) is its record's index: the head lane stores START and VALUE, the
//               TAIL lane stores END into record (inclusive count - 1) -- a run may span many waves and workgroups, and neither
//               end ever looks for the other; a lane in column 0 stores row_start[y], the last pixel's lane row_start[h]
// The left / right neighbour comes from a lane shuffle, except on the first / last lane of a wave, which loads it.  Everything is
// an integer and a function of the plane alone, and every output word has exactly one writer: identical bytes from run to run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

// What one lane knows about its pixel.  Dead lanes (i >= N) are neither head nor tail.
struct RunPix {
    unsigned v, x;
    bool live, head, tail;
};

template <class T>
__device__ __forceinline__ RunPix run_pixel(const T* __restrict__ plane, const size_t i, const size_t N, const unsigned W, const int skip,
                                            const unsigned skip_value) {
    const int lane = threadIdx.x & 63;
    RunPix p;
    p.live = i < N;
    p.v = p.live ? (unsigned)plane[i] : 0u;
    p.x = p.live ? (unsigned)i % W : 0u;  // (a live index is below 2^32 - 2)
    unsigned vl = __shfl_up(p.v, 1, 64), vr = __shfl_down(p.v, 1, 64);
    const bool first = p.x == 0, last = p.x + 1 == W;         // of the row: a run never crosses into the next one
    if (lane == 0 && p.live && !first) vl = (unsigned)plane[i - 1];   // (x > 0: i - 1 is in this row)
    if (lane == 63 && p.live && !last) vr = (unsigned)plane[i + 1];   // (x + 1 < W: i + 1 is in this row, so below N)
    const bool kept = p.live && !(skip && p.v == skip_value);
    p.head = kept && (first || p.v != vl);
    p.tail = kept && (last || p.v != vr);
    return p;
}

template <class T>
__global__ void __launch_bounds__(kScanBlock) runs_sums_kernel(const T* __restrict__ plane, size_t N, unsigned W, int skip, unsigned skip_value,
                                                               unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(run_pixel(plane, i, N, W, skip, skip_value).head, wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: partial[0, NB) -> its exclusive prefix sums in place, the total to partial[NB] and, when wanted, to the caller's word
__global__ void __launch_bounds__(kScanBlock) runs_partials_kernel(unsigned* __restrict__ partial, size_t NB, unsigned* __restrict__ d_n) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) {
        partial[NB] = n;
        if (d_n) d_n[0] = n;
    }
}

template <class T>
__global__ void __launch_bounds__(kScanBlock)
    runs_emit_kernel(const T* __restrict__ plane, size_t N, unsigned H, unsigned W, int skip, unsigned skip_value, const unsigned* __restrict__ partial,
                     unsigned* __restrict__ runs, unsigned rows, unsigned* __restrict__ row_start) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const RunPix p = run_pixel(plane, i, N, W, skip, skip_value);
    const unsigned excl = flag_rank(p.head, partial[blockIdx.x], wsum);  // emitted runs that start before this pixel
    const unsigned incl = excl + (p.head ? 1u : 0u);
    if (!p.live) return;
    if (runs) {
        if (p.head && excl < rows) {
            runs[(size_t)excl * kRunWords + 0] = (unsigned)i;
            runs[(size_t)excl * kRunWords + 2] = p.v;
        }
        // the run this pixel ends began at the latest emitted head at or before it: a break in between would have ended it sooner
        if (p.tail && incl - 1 < rows) runs[(size_t)(incl - 1) * kRunWords + 1] = (unsigned)i + 1u;
    }
    if (row_start) {
        if (p.x == 0) row_start[(unsigned)i / W] = excl;
        if (i == N - 1) row_start[H] = incl;
    }
}

template <class T>
hipError_t launch_runs_t(const T* plane, unsigned H, unsigned W, int skip, unsigned skip_value, unsigned* partial, unsigned* runs, unsigned rows,
                         unsigned* row_start, unsigned* d_n, hipStream_t s) {
    const size_t N = (size_t)H * W, NB = scan_blocks(N);
    hipLaunchKernelGGL(runs_sums_kernel<T>, dim3((unsigned)NB), dim3(kScanBlock), 0, s, plane, N, W, skip, skip_value, partial);
    hipLaunchKernelGGL(runs_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, partial, NB, d_n);
    if ((runs && rows) || row_start)
        hipLaunchKernelGGL(runs_emit_kernel<T>, dim3((unsigned)NB), dim3(kScanBlock), 0, s, plane, N, H, W, skip, skip_value, partial,
                           rows ? runs : nullptr, rows, row_start);
    return hipGetLastError();
}

}  // namespace

// the block sums and the total
size_t runs_scratch_bytes(size_t npix) { return (scan_blocks(npix) + 1) * 4; }

hipError_t launch_runs(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, void* scratch, unsigned* runs,
                       unsigned rows, unsigned* row_start, unsigned* d_n, hipStream_t s) {
    if (elem_bytes == 1) return launch_runs_t((const uint8_t*)plane, H, W, skip, skip_value, (unsigned*)scratch, runs, rows, row_start, d_n, s);
    if (elem_bytes == 4) return launch_runs_t((const uint32_t*)plane, H, W, skip, skip_value, (unsigned*)scratch, runs, rows, row_start, d_n, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
