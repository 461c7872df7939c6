// outlines.hip -- Outlines: the boundaries of the value-regions of a byte or u32 plane as closed loops of lattice vertices
// (include/infur_hip.h).  Every boundary edge (pixel, side) knows its predecessor from the 2 x 2 pixels around its
// tail, so the edges are a set of disjoint cycles given as a linked list; pointer doubling along the predecessors finds each
// cycle's start and every corner's place in it, and two scans order the loops.  The kernel boundaries are the only ordering: no
// workgroup ever waits for another and there is no atomic.
//   1 edge sums     one lane per (pixel, side) over the edge id 4*i + s; flag_block_sum of "is an edge"
//   2 edge partials scan_block_sums: the block sums -> their exclusive prefix sums; n_edges
//   3 base          flag_rank at the lane of side N: base[i] = the dense index of the pixel's first edge, so that an edge id maps
//                   to its dense index as base[i] + popcount(the pixel's lower sides)
//   4 init          per edge: the predecessor's dense index and the corner flag from the local rule; state[e] = (ptr, m, n, cnt) =
//                   (predecessor, own dense index if a corner else ~0, corner, corner), pred[e] = predecessor.  The dense index
//                   stands for the edge id in m: both ascend together
//   5 K rounds      B = state[ptr]; if B.m < m then (m, n) = (B.m, B.n + cnt); cnt += B.cnt; ptr = B.ptr -- double-buffered.  After
//                   K = ceil(log2(capacity)) rounds every window spans its cycle: m is the loop's start, n - 1 a corner's index
//                   among the loop's vertices, n[pred(start)] the loop's number of vertices
//   6 loop sums     over the dense edges: block sums of "is a start" (m == own index) and of the starts' vertex counts
//   7 loop partials both sums scanned; the counts {n_loops, n_vertices, n_edges} -- or {0, 0, n_edges} on overflow
//   8 loop rank     a start leaves (loop index, vertex offset, vertex count) in the buffer the last round read from, now free
//   9 emit          one lane per (pixel, side) again: a corner stores its tail vertex at offset[start] + n - 1, a start its record
// Workgroups beyond n_edges return at once, and so does everything behind the scan when n_edges exceeds the capacity.
// Everything is an integer and a function of the plane alone, and every output word has exactly one writer.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kRoundBlock = 256;
constexpr unsigned kNoEdge = 0xFFFFFFFFu;

struct Plane {
    unsigned H, W;
    int skip, conn8;
    unsigned skip_value;
};

// the value at (x, y) equals v; false outside the plane.  v is a kept value, so an equal pixel is kept too.  Unsigned wrap-around
// makes x = -1 and y = -1 fail the bounds test.
template <class T>
__device__ __forceinline__ bool is_v(const T* __restrict__ plane, const Plane& g, const unsigned x, const unsigned y, const unsigned v) {
    return x < g.W && y < g.H && (unsigned)plane[(size_t)y * g.W + x] == v;
}

// -> the mask of the sides N, E, S, W of pixel (x, y) (inside the plane) that are edges; *v: its value
template <class T>
__device__ __forceinline__ unsigned edge_mask(const T* __restrict__ plane, const Plane& g, const unsigned x, const unsigned y, unsigned* v) {
    *v = (unsigned)plane[(size_t)y * g.W + x];
    if (g.skip && *v == g.skip_value) return 0u;
    return (is_v(plane, g, x, y - 1u, *v) ? 0u : 1u) | (is_v(plane, g, x + 1u, y, *v) ? 0u : 2u) | (is_v(plane, g, x, y + 1u, *v) ? 0u : 4u) |
           (is_v(plane, g, x - 1u, y, *v) ? 0u : 8u);
}

// What one lane of the launches over the edge ids knows.  Dead lanes (t >= 4 * H * W) are no edge.
struct EdgeLane {
    unsigned i, x, y, d, v, mask;
    bool live, edge;
};

template <class T>
__device__ __forceinline__ EdgeLane edge_lane(const T* __restrict__ plane, const Plane& g, const size_t t, const size_t N4) {
    EdgeLane e;
    e.v = 0u;
    e.live = t < N4;
    e.i = e.live ? (unsigned)(t >> 2) : 0u;
    e.d = (unsigned)t & 3u;
    e.x = e.i % g.W;
    e.y = e.i / g.W;
    e.mask = e.live ? edge_mask(plane, g, e.x, e.y, &e.v) : 0u;
    e.edge = (e.mask >> e.d) & 1u;
    return e;
}

__device__ __forceinline__ int step_x(const unsigned d) { return d == 0 ? 1 : d == 2 ? -1 : 0; }
__device__ __forceinline__ int step_y(const unsigned d) { return d == 1 ? 1 : d == 3 ? -1 : 0; }

// The predecessor of edge (pixel e, heading d): the mirror image of the header's successor rule, on the pixel behind on the right
// (Rb) and behind on the left (Lb) of the edge's tail.  -> the predecessor's pixel and side; *corner: its heading is another.
struct Pred {
    unsigned x, y, side;
    bool corner, same_pixel;
};
template <class T>
__device__ __forceinline__ Pred predecessor(const T* __restrict__ plane, const Plane& g, const EdgeLane& e) {
    const unsigned d = e.d, left = (d + 3u) & 3u;
    const unsigned rbx = e.x - (unsigned)step_x(d), rby = e.y - (unsigned)step_y(d);
    const unsigned lbx = rbx + (unsigned)step_x(left), lby = rby + (unsigned)step_y(left);
    const bool rb = is_v(plane, g, rbx, rby, e.v), lb = is_v(plane, g, lbx, lby, e.v);
    if (rb && !lb) return {rbx, rby, d, false, false};                             // it went straight
    if (lb && (rb || g.conn8)) return {lbx, lby, (d + 1u) & 3u, true, false};      // it turned left (the saddle under CONN8 too)
    return {e.x, e.y, left, true, true};                                           // it turned right, around this pixel's corner
}

template <class T>
__global__ void __launch_bounds__(kScanBlock) outlines_edge_sums_kernel(const T* __restrict__ plane, Plane g, size_t N4, unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t t = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(edge_lane(plane, g, t, N4).edge, wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: partial[0, NB) -> its exclusive prefix sums in place, the total (n_edges) to partial[NB]
__global__ void __launch_bounds__(kScanBlock) outlines_edge_partials_kernel(unsigned* __restrict__ partial, size_t NB) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) partial[NB] = n;
}

template <class T>
__global__ void __launch_bounds__(kScanBlock)
    outlines_base_kernel(const T* __restrict__ plane, Plane g, size_t N4, const unsigned* __restrict__ partial, unsigned* __restrict__ base) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t t = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const EdgeLane e = edge_lane(plane, g, t, N4);
    const unsigned rank = flag_rank(e.edge, partial[blockIdx.x], wsum);
    if (e.live && e.d == 0) base[e.i] = rank;
}

template <class T>
__global__ void __launch_bounds__(kRoundBlock)
    outlines_init_kernel(const T* __restrict__ plane, Plane g, size_t N4, const unsigned* __restrict__ n_edges, unsigned cap,
                         const unsigned* __restrict__ base, uint4* __restrict__ state, unsigned* __restrict__ pred) {
    const unsigned n = *n_edges;
    if (n > cap) return;
    const size_t t = (size_t)blockIdx.x * kRoundBlock + threadIdx.x;
    const EdgeLane e = edge_lane(plane, g, t, N4);
    if (!e.edge) return;
    const unsigned self = base[e.i] + (unsigned)__popc(e.mask & ((1u << e.d) - 1u));
    const Pred p = predecessor(plane, g, e);
    unsigned pv, pmask = e.mask;
    if (!p.same_pixel) pmask = edge_mask(plane, g, p.x, p.y, &pv);
    unsigned ptr = base[(size_t)p.y * g.W + p.x] + (unsigned)__popc(pmask & ((1u << p.side) - 1u));
    if (self >= n) return;      // (cannot be: the ranks are below their total)
    if (ptr >= n) ptr = self;   // (cannot be: a predecessor is an edge; no later read leaves the state for it)
    state[self] = make_uint4(ptr, p.corner ? self : kNoEdge, p.corner ? 1u : 0u, p.corner ? 1u : 0u);
    pred[self] = ptr;
}

__global__ void __launch_bounds__(kRoundBlock)
    outlines_round_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const unsigned* __restrict__ n_edges, unsigned cap) {
    const unsigned n = *n_edges;
    const size_t e = (size_t)blockIdx.x * kRoundBlock + threadIdx.x;
    if (n > cap || e >= n) return;
    uint4 a = src[e];
    const uint4 b = src[a.x];
    if (b.y < a.y) {
        a.y = b.y;
        a.z = b.z + a.w;
    }
    a.w += b.w;
    a.x = b.x;
    dst[e] = a;
}

// the sum of v over the workgroup of kScanBlock lanes, valid in thread 0: flag_block_sum's sibling for values
__device__ __forceinline__ unsigned value_block_sum(unsigned v, unsigned* wsum) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kScanBlock / 64; k++) s += wsum[k];
    return s;
}

// -> block_base + the sum of v over the lanes before this one in its workgroup: flag_rank's sibling for values.  Holds a barrier.
__device__ __forceinline__ unsigned value_rank(const unsigned v, const unsigned block_base, unsigned* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = block_base;
    for (int k = 0; k < wave; k++) before += wsum[k];
    return before + inc - v;
}

// is dense edge e the start of its loop, and if so, how many vertices has the loop
__device__ __forceinline__ bool loop_start(const uint4* __restrict__ state, const unsigned* __restrict__ pred, const size_t e, const unsigned n,
                                           unsigned* count) {
    *count = 0;
    if (e >= n || state[e].y != (unsigned)e) return false;
    *count = state[pred[e]].z;
    return true;
}

__global__ void __launch_bounds__(kScanBlock)
    outlines_loop_sums_kernel(const uint4* __restrict__ state, const unsigned* __restrict__ pred, const unsigned* __restrict__ n_edges, unsigned cap,
                              unsigned* __restrict__ loop_partial, unsigned* __restrict__ vert_partial) {
    __shared__ unsigned wsum[kScanBlock / 64], vsum[kScanBlock / 64];
    const unsigned n = *n_edges <= cap ? *n_edges : 0u;  // overflow: no loops
    unsigned count;
    const bool start = loop_start(state, pred, (size_t)blockIdx.x * kScanBlock + threadIdx.x, n, &count);
    const unsigned s = flag_block_sum(start, wsum), v = value_block_sum(count, vsum);
    if (threadIdx.x == 0) {
        loop_partial[blockIdx.x] = s;
        vert_partial[blockIdx.x] = v;
    }
}

__global__ void __launch_bounds__(kScanBlock)
    outlines_loop_partials_kernel(unsigned* __restrict__ loop_partial, unsigned* __restrict__ vert_partial, size_t NB, const unsigned* __restrict__ n_edges,
                                  unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n_loops = scan_block_sums(loop_partial, NB, wsum);
    __syncthreads();
    const unsigned n_vertices = scan_block_sums(vert_partial, NB, wsum);
    if (threadIdx.x == 0 && counts) {
        counts[0] = n_loops;
        counts[1] = n_vertices;
        counts[2] = *n_edges;
    }
}

__global__ void __launch_bounds__(kScanBlock)
    outlines_loop_rank_kernel(const uint4* __restrict__ state, const unsigned* __restrict__ pred, const unsigned* __restrict__ n_edges, unsigned cap,
                              const unsigned* __restrict__ loop_partial, const unsigned* __restrict__ vert_partial, uint4* __restrict__ loop_of) {
    __shared__ unsigned wsum[kScanBlock / 64], vsum[kScanBlock / 64];
    const unsigned n = *n_edges <= cap ? *n_edges : 0u;
    const size_t e = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    unsigned count;
    const bool start = loop_start(state, pred, e, n, &count);
    const unsigned index = flag_rank(start, loop_partial[blockIdx.x], wsum), offset = value_rank(count, vert_partial[blockIdx.x], vsum);
    if (start) loop_of[e] = make_uint4(index, offset, count, 0u);
}

template <class T>
__global__ void __launch_bounds__(kRoundBlock)
    outlines_emit_kernel(const T* __restrict__ plane, Plane g, size_t N4, const unsigned* __restrict__ n_edges, unsigned cap,
                         const unsigned* __restrict__ base, const uint4* __restrict__ state, const uint4* __restrict__ loop_of,
                         unsigned* __restrict__ loops, unsigned loops_rows, unsigned* __restrict__ vertices, unsigned vertex_rows) {
    const unsigned n = *n_edges;
    if (n > cap) return;
    const size_t t = (size_t)blockIdx.x * kRoundBlock + threadIdx.x;
    const EdgeLane e = edge_lane(plane, g, t, N4);
    if (!e.edge) return;
    const unsigned self = base[e.i] + (unsigned)__popc(e.mask & ((1u << e.d) - 1u));
    if (self >= n) return;
    const uint4 s = state[self];
    if (s.y >= n) return;  // (cannot be: every loop has a corner)
    const uint4 l = loop_of[s.y];
    if (vertices && predecessor(plane, g, e).corner) {
        const unsigned at = l.y + s.z - 1u;  // tail vertex: N (x, y), E (x+1, y), S (x+1, y+1), W (x, y+1)
        const unsigned X = e.x + (e.d == 1 || e.d == 2 ? 1u : 0u), Y = e.y + (e.d >= 2 ? 1u : 0u);
        if (s.z >= 1u && at < vertex_rows) vertices[at] = Y * (g.W + 1u) + X;
    }
    if (loops && s.y == self && l.x < loops_rows) {
        unsigned* r = loops + (size_t)l.x * kLoopWords;
        r[0] = l.y;
        r[1] = l.z;
        r[2] = e.v;
        r[3] = (unsigned)t;
    }
}

unsigned rounds_for(const size_t cap) {
    unsigned k = 0;
    while (((size_t)1 << k) < cap) k++;
    return k;
}

// the scratch, on 256-byte boundaries: [edge block sums + n_edges][loop sums][vertex sums][base][pred][state A][state B]
struct Layout {
    size_t edge_partial, loop_partial, vert_partial, base, pred, state_a, state_b, bytes;
    Layout(const size_t npix, const size_t cap) {
        const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        edge_partial = 0;
        loop_partial = up((scan_blocks(npix * 4) + 1) * 4);
        vert_partial = loop_partial + up((scan_blocks(cap) + 1) * 4);
        base = vert_partial + up((scan_blocks(cap) + 1) * 4);
        pred = base + up(npix * 4);
        state_a = pred + up(cap * 4);
        state_b = state_a + up(cap * 16);
        bytes = state_b + up(cap * 16);
    }
};

template <class T>
hipError_t launch_outlines_t(const T* plane, unsigned H, unsigned W, int skip, int conn8, unsigned skip_value, size_t cap, uint8_t* scratch,
                             unsigned* loops, unsigned loops_rows, unsigned* vertices, unsigned vertex_rows, unsigned* counts, hipStream_t s) {
    const size_t npix = (size_t)H * W, N4 = npix * 4, NB = scan_blocks(N4), NC = scan_blocks(cap);
    const Layout at(npix, cap);
    const Plane g = {H, W, skip, conn8, skip_value};
    unsigned* edge_partial = (unsigned*)(scratch + at.edge_partial);
    unsigned* loop_partial = (unsigned*)(scratch + at.loop_partial);
    unsigned* vert_partial = (unsigned*)(scratch + at.vert_partial);
    unsigned* base = (unsigned*)(scratch + at.base);
    unsigned* pred = (unsigned*)(scratch + at.pred);
    uint4* a = (uint4*)(scratch + at.state_a);
    uint4* b = (uint4*)(scratch + at.state_b);
    const unsigned* n_edges = edge_partial + NB;
    const unsigned ucap = (unsigned)cap;  // (cap <= 4 * H * W < 2^32 - 1)
    const dim3 lanes4((unsigned)((N4 + kRoundBlock - 1) / kRoundBlock)), dense((unsigned)((cap + kRoundBlock - 1) / kRoundBlock));
    hipLaunchKernelGGL(outlines_edge_sums_kernel<T>, dim3((unsigned)NB), dim3(kScanBlock), 0, s, plane, g, N4, edge_partial);
    hipLaunchKernelGGL(outlines_edge_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, edge_partial, NB);
    hipLaunchKernelGGL(outlines_base_kernel<T>, dim3((unsigned)NB), dim3(kScanBlock), 0, s, plane, g, N4, edge_partial, base);
    hipLaunchKernelGGL(outlines_init_kernel<T>, lanes4, dim3(kRoundBlock), 0, s, plane, g, N4, n_edges, ucap, base, a, pred);
    const unsigned K = rounds_for(cap);
    for (unsigned k = 0; k < K; k++) {
        hipLaunchKernelGGL(outlines_round_kernel, dense, dim3(kRoundBlock), 0, s, a, b, n_edges, ucap);
        uint4* t = a;
        a = b;
        b = t;
    }  // a: the final state; b: free
    hipLaunchKernelGGL(outlines_loop_sums_kernel, dim3((unsigned)NC), dim3(kScanBlock), 0, s, a, pred, n_edges, ucap, loop_partial, vert_partial);
    hipLaunchKernelGGL(outlines_loop_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, loop_partial, vert_partial, NC, n_edges, counts);
    if ((loops && loops_rows) || (vertices && vertex_rows)) {
        hipLaunchKernelGGL(outlines_loop_rank_kernel, dim3((unsigned)NC), dim3(kScanBlock), 0, s, a, pred, n_edges, ucap, loop_partial, vert_partial, b);
        hipLaunchKernelGGL(outlines_emit_kernel<T>, lanes4, dim3(kRoundBlock), 0, s, plane, g, N4, n_edges, ucap, base, a, b, loops_rows ? loops : nullptr,
                           loops_rows, vertex_rows ? vertices : nullptr, vertex_rows);
    }
    return hipGetLastError();
}

}  // namespace

size_t outlines_scratch_bytes(size_t npix, size_t cap) { return Layout(npix, cap).bytes; }

hipError_t launch_outlines(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, int conn8, unsigned skip_value, size_t cap,
                           void* scratch, unsigned* loops, unsigned loops_rows, unsigned* vertices, unsigned vertex_rows, unsigned* counts,
                           hipStream_t s) {
    if (elem_bytes == 1)
        return launch_outlines_t((const uint8_t*)plane, H, W, skip, conn8, skip_value, cap, (uint8_t*)scratch, loops, loops_rows, vertices,
                                 vertex_rows, counts, s);
    if (elem_bytes == 4)
        return launch_outlines_t((const uint32_t*)plane, H, W, skip, conn8, skip_value, cap, (uint8_t*)scratch, loops, loops_rows, vertices,
                                 vertex_rows, counts, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
