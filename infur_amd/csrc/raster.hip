// raster.hip -- Raster: polygon loops, or run-length records, filled back into a dense plane (include/infur_hip.h).  The
// one stage that goes from the small representation to the large one.  Everything is an exact integer function of the input.
//   0 clear   the head words and one 64-bit accumulator word per pixel = 0 (one memset node)
//   1 edges   one wave per loop (dealt round-robin to at most 32 Ki waves), lanes strided over its segments.  A segment a -> b with
//             y_a != y_b crosses the centre line of every row min(y) <= y < max(y) at the CROSSING COLUMN c, the smallest x whose
//             pixel centre lies at or to the right of the segment; the crossing adds +-(VALUE << 32 | 1) to word (y, c), + when the
//             segment heads north.  A lane walks the rows of its own segment while |dy| <= kRasterLaneRows; longer segments are
//             handed to the whole wave (a ballot of the long ones, the ends broadcast by __shfl, lanes strided over the rows).
//      runs   (the other front end) one lane per record: + at START, - at END unless END ends its row
//   2 rows    one workgroup per row: an inclusive 64-bit prefix sum along the row, 1024 columns a step with a carry, after which the
//             low word of a pixel is its winding k and the high word its value sum S; the resolve (OUTSIDE: the word is 0; PAINTED:
//             k == 1 and S fits the plane; CONFLICT: anything else) and the plane store; PAINTED and CONFLICT counted per thread in
//             one 64-bit register, summed across the wave once and added with one atomic add per wave
//   3 finish  counts_out
// Addition modulo 2^64 commutes and the counters are integers: identical bytes from run to run.  The numbers of loops, vertices
// and records are device words: the grids come from the caller's rows.  Truncated input makes every launch see nothing and
// leaves the plane alone.  Every index a record holds is compared with the counts, and the counts with the rows, before it
// addresses anything; a crossing is stored only when its row is below H and its column below W.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace infur {

namespace {

// A lane walks its own segment's rows up to this many; the wave takes the longer ones.  While one lane walks, the other 63 wait for
// it, so a batch of 64 segments costs the longest lane walk: at most 16 row steps here.  A segment handed to the wave costs the
// broadcast (four __shfl and the ballot's bit loop, about three row steps) plus one row step per 64 rows, with 64 - |dy| lanes
// idle for |dy| < 64.  Pixel staircases (|dy| = 1) and the chords a tolerance of one or two pixels leaves (|dy| of 2 to about
// 12) stay in the lanes, where a batch of them costs less than one wave hand-off each; a rectangle side or a long chord, where
// the lane walk would serialise thousands of rows, goes to the wave.
constexpr int kRasterLaneRows = 16;

constexpr int kLoopBlock = 256;       // four waves, each with a loop of its own, per workgroup of the edges launch
constexpr unsigned kLoopGrid = 8192;  // at most: 32 workgroups for each of 256 compute units, so that uneven loops even out
constexpr int kRunsBlock = 256;
constexpr int kRowBlock = 256;  // the workgroup of a row
constexpr int kRowCols = 4;     // consecutive columns per thread and step: kRowBlock * kRowCols = 1024 columns a step

using u64 = unsigned long long;

// the head of the scratch: {PAINTED | CONFLICT << 32 (one 64-bit counter), status}; the accumulator follows at kHeadBytes
constexpr size_t kHeadBytes = 256;

struct RasterIn {
    const unsigned* loops;     // loops: records (OFFSET, COUNT, VALUE, START); runs: records (START, END, VALUE)
    const unsigned* vertices;  // loops only
    const unsigned* counts;    // loops: {n_loops, n_vertices}; runs: {n_runs}
    unsigned rows0, rows1;     // the rows declared for the records and the vertices
    unsigned count_words;      // 2: loops, 1: runs
    unsigned H, W;
};

// -> the numbers of records and vertices there are to read: both 0 when either exceeds its rows
__device__ __forceinline__ bool input_counts(const RasterIn& in, unsigned* n0, unsigned* n1) {
    const unsigned c0 = in.counts[0], c1 = in.count_words > 1 ? in.counts[1] : 0u;
    const bool truncated = c0 > in.rows0 || c1 > in.rows1;
    *n0 = truncated ? 0u : c0;
    *n1 = truncated ? 0u : c1;
    return truncated;
}

struct Pt {
    int x, y;
};

// a vertex id on the lattice of (W + 1) x (H + 1) points; a Y above H is clamped onto it and reported
__device__ __forceinline__ Pt point_of(const unsigned id, const RasterIn& in, unsigned* status) {
    const unsigned w1 = in.W + 1u;
    unsigned y = id / w1;
    const unsigned x = id - y * w1;
    if (y > in.H) {
        y = in.H;
        *status |= kRasterOutside;
    }
    return {(int)x, (int)y};
}

// The crossing column of the segment (x0, y0) -> (x1, y1), y0 < y1, with the centre line of row y in [y0, y1): the smallest x
// with x + 1/2 >= x*, as ceil((num - dy) / (2 dy)), clamped to 0 from below.  Every term is below 2^28 and the sum below 2^30.
__device__ __forceinline__ int crossing(const int x0, const int y0, const int x1, const int y1, const int y) {
    const int dy = y1 - y0, dx = x1 - x0;
    if (dx == 0) return x0;
    const int a = 2 * x0 * dy + dx * (2 * y + 1 - 2 * y0) - dy;
    return a <= 0 ? 0 : (a + 2 * dy - 1) / (2 * dy);
}

// one crossing: row y is below H by construction (y < max(y_a, y_b) <= H); a column at or beyond W has no effect
__device__ __forceinline__ void cross(u64* __restrict__ acc, const RasterIn& in, const int y, const int c, const u64 delta) {
    if ((unsigned)y < in.H && (unsigned)c < in.W)
        __hip_atomic_fetch_add(acc + (size_t)y * in.W + c, delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kLoopBlock) raster_edges_kernel(RasterIn in, u64* __restrict__ acc, unsigned* __restrict__ status_word) {
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const unsigned lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kLoopBlock / 64);
    unsigned status = 0;
    for (size_t loop = (size_t)blockIdx.x * (kLoopBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) {
        const unsigned* r = in.loops + loop * kLoopWords;
        const unsigned off = r[0], n = r[1], value = r[2];
        if (n < 2u || (uint64_t)off + n > nv) {  // (uniform across the wave)
            status |= kRasterMalformed;
            continue;
        }
        const u64 word = (u64)value << 32 | 1ull;
        for (uint64_t base = 0; base < n; base += 64u) {  // (64 bits: no COUNT makes the walk wrap)
            const uint64_t i = base + lane;
            const bool active = i < n;
            // the segment of this lane, oriented downwards: (x0, y0) is its upper end
            int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
            u64 delta = 0;
            if (active) {
                const Pt a = point_of(in.vertices[off + i], in, &status), b = point_of(in.vertices[off + (i + 1u == n ? 0u : i + 1u)], in, &status);
                const bool north = b.y < a.y;
                x0 = north ? b.x : a.x, y0 = north ? b.y : a.y;
                x1 = north ? a.x : b.x, y1 = north ? a.y : b.y;
                delta = north ? word : 0ull - word;
            }
            const int dy = y1 - y0;  // 0: horizontal, or no segment
            if (dy > 0 && dy <= kRasterLaneRows)
                for (int y = y0; y < y1; y++) cross(acc, in, y, crossing(x0, y0, x1, y1, y), delta);
            u64 todo = __ballot(dy > kRasterLaneRows);
            while (todo) {
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sx1 = __shfl(x1, src, 64), sy1 = __shfl(y1, src, 64);
                const u64 sdelta = __shfl(delta, src, 64);
                for (int y = sy0 + (int)lane; y < sy1; y += 64) cross(acc, in, y, crossing(sx0, sy0, sx1, sy1, y), sdelta);
            }
        }
    }
    if (status) atomicOr(status_word, status);
}

__global__ void __launch_bounds__(kRunsBlock) raster_runs_kernel(RasterIn in, u64* __restrict__ acc, unsigned* __restrict__ status_word) {
    unsigned n, unused;
    input_counts(in, &n, &unused);
    const size_t i = (size_t)blockIdx.x * kRunsBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned* r = in.loops + i * kRunWords;
    const unsigned start = r[0], end = r[1], value = r[2];
    const uint64_t npix = (uint64_t)in.H * in.W;
    if (!(start < end && end <= npix && start / in.W == (end - 1u) / in.W)) {
        atomicOr(status_word, kRasterMalformed);
        return;
    }
    const u64 word = (u64)value << 32 | 1ull;
    __hip_atomic_fetch_add(acc + start, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (end % in.W != 0u) __hip_atomic_fetch_add(acc + end, 0ull - word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 wave_inclusive(u64 v, const unsigned lane) {
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        const u64 o = __shfl_up(v, step, 64);
        if (lane >= (unsigned)step) v += o;
    }
    return v;
}

// One workgroup per row (grid.x = H).  The row is walked kRowBlock * kRowCols columns a step; the sum of everything to the left
// is carried in a register every thread keeps alike.  The wave sums of a step go through LDS, in one of two buffers by the
// step's parity, so that one barrier a step is enough: a thread that writes buffer p again has passed the barrier of the step
// between, which every thread reaches only after it has read buffer p.
template <typename T>
__global__ void __launch_bounds__(kRowBlock)
    raster_rows_kernel(RasterIn in, const u64* __restrict__ acc, T* __restrict__ plane, const unsigned fill, u64* __restrict__ counter) {
    __shared__ u64 wsum[2][kRowBlock / 64];
    unsigned n0, n1;
    if (input_counts(in, &n0, &n1)) return;  // truncated input: the plane is left alone
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * in.W;
    u64 carry = 0;
    u64 mine = 0;  // this thread's pixels: PAINTED in the low word, CONFLICT in the high
    unsigned parity = 0;
    for (unsigned left = 0; left < in.W; left += kRowBlock * kRowCols, parity ^= 1u) {
        const unsigned col = left + threadIdx.x * kRowCols;
        u64 v[kRowCols];
#pragma unroll
        for (int j = 0; j < kRowCols; j++) v[j] = col + j < in.W ? acc[row + col + j] : 0ull;
#pragma unroll
        for (int j = 1; j < kRowCols; j++) v[j] += v[j - 1];
        const u64 incl = wave_inclusive(v[kRowCols - 1], lane);
        if (lane == 63) wsum[parity][wave] = incl;
        __syncthreads();
        u64 before = carry + (incl - v[kRowCols - 1]);
#pragma unroll
        for (int k = 0; k < kRowBlock / 64; k++) {
            const u64 s = wsum[parity][k];
            before += (unsigned)k < wave ? s : 0ull;
            carry += s;
        }
        unsigned out[kRowCols];
#pragma unroll
        for (int j = 0; j < kRowCols; j++) {
            const u64 word = before + v[j];
            const unsigned k = (unsigned)word, sum = (unsigned)(word >> 32);
            const bool inside = col + j < in.W;
            const bool is_painted = inside && k == 1u && (sizeof(T) == 4 || sum <= 255u);
            const bool is_conflict = inside && word != 0ull && !is_painted;
            out[j] = is_painted ? sum : fill;
            mine += (u64)is_painted | (u64)is_conflict << 32;
        }
        if (plane) {
            T* p = plane + row + col;
            if (sizeof(T) == 1 && col + kRowCols <= in.W && ((uintptr_t)p & 3u) == 0) {
                *(unsigned*)p = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < kRowCols; j++)
                    if (col + j < in.W) p[j] = (T)out[j];
            }
        }
    }
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) mine += __shfl_xor(mine, step, 64);
    if (lane == 0 && mine) atomicAdd(counter, mine);
}

__global__ void raster_finish_kernel(RasterIn in, const u64* __restrict__ counter, const unsigned* __restrict__ status_word,
                                     unsigned* __restrict__ counts_out) {
    unsigned n0, n1;
    const bool truncated = input_counts(in, &n0, &n1);
    const u64 c = *counter;
    counts_out[0] = in.counts[0];
    counts_out[1] = truncated ? 0u : (unsigned)c;
    counts_out[2] = truncated ? 0u : (unsigned)(c >> 32);
    counts_out[3] = truncated ? kRasterTruncated : *status_word;
}

hipError_t launch_common(const RasterIn& in, const bool runs, void* scratch, const int elem_bytes, const unsigned fill, void* plane,
                         unsigned* counts_out, hipStream_t s) {
    uint8_t* base = (uint8_t*)scratch;
    u64* counter = (u64*)base;
    unsigned* status_word = (unsigned*)(base + 8);
    u64* acc = (u64*)(base + kHeadBytes);
    const size_t npix = (size_t)in.H * in.W;
    const hipError_t e = hipMemsetAsync(base, 0, kHeadBytes + npix * 8, s);
    if (e != hipSuccess) return e;
    if (in.rows0) {
        if (runs) {
            hipLaunchKernelGGL(raster_runs_kernel, dim3((unsigned)(((size_t)in.rows0 + kRunsBlock - 1) / kRunsBlock)), dim3(kRunsBlock), 0, s, in, acc,
                               status_word);
        } else {
            const size_t blocks = ((size_t)in.rows0 + 3) / 4;
            hipLaunchKernelGGL(raster_edges_kernel, dim3((unsigned)(blocks < kLoopGrid ? blocks : kLoopGrid)), dim3(kLoopBlock), 0, s, in, acc, status_word);
        }
    }
    if (elem_bytes == 1)
        hipLaunchKernelGGL(raster_rows_kernel<uint8_t>, dim3(in.H), dim3(kRowBlock), 0, s, in, acc, (uint8_t*)plane, fill, counter);
    else
        hipLaunchKernelGGL(raster_rows_kernel<unsigned>, dim3(in.H), dim3(kRowBlock), 0, s, in, acc, (unsigned*)plane, fill, counter);
    if (counts_out) hipLaunchKernelGGL(raster_finish_kernel, dim3(1), dim3(1), 0, s, in, counter, status_word, counts_out);
    return hipGetLastError();
}

}  // namespace

size_t raster_scratch_bytes(size_t npix) { return kHeadBytes + npix * 8; }

hipError_t launch_raster(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                         unsigned H, unsigned W, int elem_bytes, unsigned fill_value, void* scratch, void* plane, unsigned* counts_out, hipStream_t s) {
    const RasterIn in = {loops, vertices, counts, loops_rows_in, vertex_rows_in, 2u, H, W};
    return launch_common(in, false, scratch, elem_bytes, fill_value, plane, counts_out, s);
}

hipError_t launch_raster_runs(const unsigned* runs, unsigned runs_rows_in, const unsigned* d_n, unsigned H, unsigned W, int elem_bytes,
                              unsigned fill_value, void* scratch, void* plane, unsigned* counts_out, hipStream_t s) {
    const RasterIn in = {runs, nullptr, d_n, runs_rows_in, 0u, 1u, H, W};
    return launch_common(in, true, scratch, elem_bytes, fill_value, plane, counts_out, s);
}

}  // namespace infur
