// simplify.hip -- Simplify: Douglas-Peucker on the loops Outlines leaves on the device (include/infur_hip.h).  A loop's
// kept set is a function of the loop alone, so one wave owns one loop and the order in which it visits the segments is free; the
// kept vertices of all loops are then ordered by the flag scan of wave_scan.h over the whole vertex array, because loops lie back
// to back.  The kernel boundaries are the only ordering: no workgroup ever waits for another and there is no atomic.
//   0 clear     keep[0, vertex_rows_in) = 0 (a memset node)
//   1 keep      one wave per loop (the loops dealt round-robin to at most 32 Ki waves): anchor B from a strided argmax of |v_i - v_0|^2, then an explicit stack of segments (a, c):
//               strided argmax of D, keep[m] = 1 when it exceeds the tolerance, the larger half waits on the stack and the smaller
//               is next.  The stack is one entry per lane, in registers: at most log2(n) + 2 <= 34 of the 64 are ever used
//   2 sums      over the positions 0 .. vertex_rows_in: flag_block_sum of "p < n_vertices and keep[p]"
//   3 partials  scan_block_sums: the block sums -> their exclusive prefix sums; the total n_vertices'
//   4 rank      rank[p] = the number of kept vertices below p, for p <= n_vertices; a kept vertex stores its id at its rank
//   5 records   one lane per loop: OFFSET' = rank[OFFSET], COUNT' = rank[OFFSET + COUNT] - rank[OFFSET]; block sums of "COUNT' < 3"
//               and of "malformed"
//   6 counts    one workgroup adds those block sums and writes counts_out
// The number of loops and of vertices are device words: the grids come from the caller's rows, and workgroups beyond the counts
// have nothing to do.  Truncated input (a count above its rows) makes every launch see no loop and no vertex.  Every index a record
// holds is compared with the counts, and the counts with the rows, before it addresses anything.  Everything is an integer and
// every output word has exactly one writer.
// Cost: a segment of k vertices is read once per level of the recursion below it, 64 vertices per step of the wave that owns the
// loop: O(n * depth / 64) steps for a loop of n vertices, O(n^2 / 64) when every split is lopsided.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kKeepBlock = 256;      // four waves, each with a loop of its own, per workgroup of the keep launch
constexpr unsigned kKeepGrid = 8192;  // at most: 32 workgroups for each of 256 compute units, so that uneven loops even out
constexpr unsigned kMaxCoord = 8191;

struct SimplifyIn {
    const unsigned* loops;
    const unsigned* vertices;
    const unsigned* counts;
    unsigned loops_rows, vertex_rows, w1;  // w1: the lattice's width, w + 1
};

// -> the numbers of loops and vertices there are to read: both 0 when either exceeds its rows
__device__ __forceinline__ bool input_counts(const SimplifyIn& in, unsigned* nl, unsigned* nv) {
    const unsigned c0 = in.counts[0], c1 = in.counts[1];
    const bool truncated = c0 > in.loops_rows || c1 > in.vertex_rows;
    *nl = truncated ? 0u : c0;
    *nv = truncated ? 0u : c1;
    return truncated;
}

// record i < nl -> its OFFSET and COUNT; false when it is malformed (COUNT < 2 or its vertices end beyond nv)
__device__ __forceinline__ bool loop_range(const SimplifyIn& in, const unsigned i, const unsigned nv, unsigned* off, unsigned* cnt) {
    const unsigned* r = in.loops + (size_t)i * kLoopWords;
    *off = r[0];
    *cnt = r[1];
    return *cnt >= 2u && (uint64_t)*off + *cnt <= nv;
}

struct Pt {
    int x, y;
};
// vertex k of the loop at `off` with n vertices; k == n is vertex 0 again.  A Y above 8191 reads as 8191
__device__ __forceinline__ Pt vertex(const SimplifyIn& in, const unsigned off, const unsigned n, const unsigned k) {
    const unsigned id = in.vertices[off + (k == n ? 0u : k)];
    const unsigned y = id / in.w1;
    return {(int)(id - y * in.w1), (int)(y < kMaxCoord ? y : kMaxCoord)};
}

// the wave-wide maximum of the key (d, -i): the larger d, on a tie the smaller i; every lane gets the answer
__device__ __forceinline__ void wave_argmax(uint64_t* d, unsigned* i) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const uint64_t od = __shfl_xor((unsigned long long)*d, step, 64);
        const unsigned oi = __shfl_xor(*i, step, 64);
        if (od > *d || (od == *d && oi < *i)) {
            *d = od;
            *i = oi;
        }
    }
}

// one wave, one loop
__device__ __forceinline__ void keep_loop(const SimplifyIn& in, const unsigned loop, const unsigned nv, const unsigned lane, const uint64_t t2,
                                          uint8_t* __restrict__ keep) {
    unsigned off, n;
    if (!loop_range(in, loop, nv, &off, &n)) return;

    // the anchors: vertex 0 and the farthest from it
    const Pt v0 = vertex(in, off, n, 0);
    uint64_t best = 0;
    unsigned at = 0xFFFFFFFFu;
    for (unsigned i = 1u + lane; i < n; i += 64u) {
        const Pt p = vertex(in, off, n, i);
        const int64_t dx = p.x - v0.x, dy = p.y - v0.y;
        const uint64_t d = (uint64_t)(dx * dx + dy * dy);
        if (at == 0xFFFFFFFFu || d > best) {
            best = d;
            at = i;
        }
    }
    wave_argmax(&best, &at);
    const unsigned B = at;  // (n >= 2: lane 0 had vertex 1)
    if (lane == 0) {
        keep[off] = 1;
        keep[off + B] = 1;
    }

    // the segments that wait: entry k lives in lane k
    unsigned stack_a = B, stack_c = n;  // entry 0 = (B, n), in every lane: only lane 0's counts
    unsigned sp = 1, a = 0, c = B;
    for (;;) {
        if (c - a < 2u) {
            if (sp == 0) break;
            sp--;
            a = __shfl(stack_a, (int)sp, 64);
            c = __shfl(stack_c, (int)sp, 64);
            continue;
        }
        const Pt pa = vertex(in, off, n, a), pc = vertex(in, off, n, c);
        const int64_t ex = pc.x - pa.x, ey = pc.y - pa.y;
        uint64_t len = (uint64_t)(ex * ex + ey * ey);
        const bool closed = len == 0;  // the ends coincide: the distance from the point takes the chord's place
        if (closed) len = 1;
        best = 0;
        at = 0xFFFFFFFFu;
        for (unsigned i = a + 1u + lane; i < c; i += 64u) {
            const Pt p = vertex(in, off, n, i);
            const int64_t dx = p.x - pa.x, dy = p.y - pa.y;
            const int64_t cross = ex * dy - ey * dx;
            const uint64_t d = (uint64_t)(closed ? dx * dx + dy * dy : cross * cross);
            if (at == 0xFFFFFFFFu || d > best) {
                best = d;
                at = i;
            }
        }
        wave_argmax(&best, &at);
        const unsigned m = at;  // a < m < c
        if (256u * best > t2 * len && sp < 64u) {  // (sp < 64 cannot fail: the waiting segments at least double from the top down)
            if (lane == 0) keep[off + m] = 1;
            const bool left_waits = m - a >= c - m;
            if (lane == sp) {
                stack_a = left_waits ? a : m;
                stack_c = left_waits ? m : c;
            }
            sp++;
            if (left_waits)
                a = m;
            else
                c = m;
        } else {
            c = a;  // nothing between a and c is kept
        }
    }
}

// The loops are dealt to the waves of a grid that fills the machine and no more: a grid of one wave per row of capacity would
// mostly launch waves that find no loop (the rows are the caller's worst case), and launching them is what costs
__global__ void __launch_bounds__(kKeepBlock) simplify_keep_kernel(SimplifyIn in, unsigned tol16, uint8_t* __restrict__ keep) {
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const unsigned lane = threadIdx.x & 63;
    const uint64_t t2 = (uint64_t)tol16 * tol16;
    const size_t waves = (size_t)gridDim.x * (kKeepBlock / 64);
    for (size_t loop = (size_t)blockIdx.x * (kKeepBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) keep_loop(in, (unsigned)loop, nv, lane, t2, keep);
}

// the flag of position p of the scan: a kept vertex
__device__ __forceinline__ bool kept_at(const uint8_t* __restrict__ keep, const size_t p, const unsigned nv) { return p < nv && keep[p] != 0; }

__global__ void __launch_bounds__(kScanBlock) simplify_sums_kernel(SimplifyIn in, const uint8_t* __restrict__ keep, unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(kept_at(keep, p, nv), wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: partial[0, NB) -> its exclusive prefix sums in place, the total (n_vertices') to partial[NB]
__global__ void __launch_bounds__(kScanBlock) simplify_partials_kernel(unsigned* __restrict__ partial, size_t NB) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) partial[NB] = n;
}

__global__ void __launch_bounds__(kScanBlock)
    simplify_rank_kernel(SimplifyIn in, const uint8_t* __restrict__ keep, const unsigned* __restrict__ partial, unsigned* __restrict__ rank,
                         unsigned* __restrict__ vertices_out, unsigned vertex_rows_out) {
    __shared__ unsigned wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;  // p <= vertex_rows_in has a word of rank[]
    const bool flag = kept_at(keep, p, nv);
    const unsigned r = flag_rank(flag, partial[blockIdx.x], wsum);
    if (p <= nv) rank[p] = r;
    if (flag && vertices_out && r < vertex_rows_out) vertices_out[r] = in.vertices[p];
}

__global__ void __launch_bounds__(kScanBlock)
    simplify_records_kernel(SimplifyIn in, const unsigned* __restrict__ rank, unsigned* __restrict__ loops_out, unsigned loops_rows_out,
                            unsigned* __restrict__ thin_partial, unsigned* __restrict__ bad_partial) {
    __shared__ unsigned wsum[kScanBlock / 64], bsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    bool thin = false, bad = false;
    if (i < nl) {
        unsigned off, cnt;
        bad = !loop_range(in, (unsigned)i, nv, &off, &cnt);
        const unsigned first = rank[off < nv ? off : nv];
        const unsigned kept = bad ? 0u : rank[off + cnt] - first;
        thin = kept < 3u;
        if (loops_out && i < loops_rows_out) {
            const unsigned* src = in.loops + i * kLoopWords;
            unsigned* r = loops_out + i * kLoopWords;
            r[0] = first;
            r[1] = kept;
            r[2] = src[2];
            r[3] = src[3];
        }
    }
    const unsigned t = flag_block_sum(thin, wsum), b = flag_block_sum(bad, bsum);
    if (threadIdx.x == 0) {
        thin_partial[blockIdx.x] = t;
        bad_partial[blockIdx.x] = b;
    }
}

// one workgroup: counts_out = {n_loops, n_vertices', n_degenerate, status}.  NL: the block sums of the records launch
__global__ void __launch_bounds__(kScanBlock)
    simplify_counts_kernel(SimplifyIn in, const unsigned* __restrict__ n_kept, const unsigned* __restrict__ thin_partial,
                           const unsigned* __restrict__ bad_partial, size_t NL, unsigned* __restrict__ counts_out) {
    __shared__ unsigned tsum[kScanBlock / 64], bsum[kScanBlock / 64];
    unsigned t = 0, b = 0;
    for (size_t k = threadIdx.x; k < NL; k += kScanBlock) {
        t += thin_partial[k];
        b += bad_partial[k];
    }
    for (int d = 32; d > 0; d >>= 1) {
        t += __shfl_down(t, d, 64);
        b += __shfl_down(b, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        tsum[threadIdx.x >> 6] = t;
        bsum[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kScanBlock / 64; k++) {
        t += tsum[k];
        b += bsum[k];
    }
    unsigned nl, nv;
    const bool truncated = input_counts(in, &nl, &nv);
    counts_out[0] = in.counts[0];
    counts_out[1] = *n_kept;
    counts_out[2] = t;
    counts_out[3] = (truncated ? 1u : 0u) | (b ? 2u : 0u);
}

// the scratch, on 256-byte boundaries: [vertex block sums + total][thin sums][bad sums][rank][keep]
struct Layout {
    size_t partial, thin, bad, rank, keep, bytes;
    Layout(const size_t loops_rows, const size_t vertex_rows) {
        const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        partial = 0;
        thin = up((scan_blocks(vertex_rows + 1) + 1) * 4);
        bad = thin + up((scan_blocks(loops_rows) + 1) * 4);
        rank = bad + up((scan_blocks(loops_rows) + 1) * 4);
        keep = rank + up((vertex_rows + 1) * 4);
        bytes = keep + up(vertex_rows + 1);
    }
};

}  // namespace

size_t simplify_scratch_bytes(size_t loops_rows, size_t vertex_rows) { return Layout(loops_rows, vertex_rows).bytes; }

hipError_t launch_simplify(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                           unsigned W, unsigned tol16, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out,
                           unsigned vertex_rows_out, unsigned* counts_out, hipStream_t s) {
    const Layout at(loops_rows_in, vertex_rows_in);
    uint8_t* base = (uint8_t*)scratch;
    unsigned* partial = (unsigned*)(base + at.partial);
    unsigned* thin = (unsigned*)(base + at.thin);
    unsigned* bad = (unsigned*)(base + at.bad);
    unsigned* rank = (unsigned*)(base + at.rank);
    uint8_t* keep = base + at.keep;
    const SimplifyIn in = {loops, vertices, counts, loops_rows_in, vertex_rows_in, W + 1u};
    const size_t NB = scan_blocks((size_t)vertex_rows_in + 1), NL = scan_blocks(loops_rows_in);
    const size_t keep_blocks = ((size_t)loops_rows_in + 3) / 4;
    hipError_t e = hipMemsetAsync(keep, 0, (size_t)vertex_rows_in + 1, s);
    if (e != hipSuccess) return e;
    if (loops_rows_in)
        hipLaunchKernelGGL(simplify_keep_kernel, dim3((unsigned)(keep_blocks < kKeepGrid ? keep_blocks : kKeepGrid)), dim3(kKeepBlock), 0, s, in, tol16,
                           keep);
    hipLaunchKernelGGL(simplify_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, keep, partial);
    hipLaunchKernelGGL(simplify_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, partial, NB);
    hipLaunchKernelGGL(simplify_rank_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, keep, partial, rank, vertices_out, vertex_rows_out);
    if (loops_rows_in)
        hipLaunchKernelGGL(simplify_records_kernel, dim3((unsigned)NL), dim3(kScanBlock), 0, s, in, rank, loops_out, loops_rows_out, thin, bad);
    if (counts_out) hipLaunchKernelGGL(simplify_counts_kernel, dim3(1), dim3(kScanBlock), 0, s, in, partial + NB, thin, bad, NL, counts_out);
    return hipGetLastError();
}

}  // namespace infur
