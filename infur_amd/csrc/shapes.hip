// shapes.hip -- Shapes: per outline loop its area, perimeter and moments, its convex hull and the smallest rectangle around it; per
// value the sums (include/infur_hip.h).  Everything is an exact integer function of a loop, so one wave owns one loop,
// as in simplify.hip, and the hull vertices of all loops are ordered by the flag scan of wave_scan.h over the whole vertex array.
// The kernel boundaries are the only ordering between workgroups; the per-value table is built from 64-bit atomic adds and one
// atomicMax per outer loop, which commute: identical bytes from run to run.
//   0 clear     the two header words and keep[0, vertex_rows_in] = 0 (one memset node); the per-value table = 0 (another)
//   1 hull      one wave per loop (dealt round-robin to at most 32 Ki waves): the seven measures from a strided sum with a cross-lane
//               reduction; the anchors (lexicographic minimum and maximum by (Y, X)) from a strided argmin / argmax; then an
//               explicit stack of cyclic index ranges (a, c): strided argmax of the distance on the outer side of the chord,
//               keep[m] = 1 when it is strictly positive, the larger half waits on the stack (one entry per lane, in registers);
//               last a walk over the kept flags that drops any kept vertex collinear with its kept neighbours
//   2 sums      over the positions 0 .. vertex_rows_in: flag_block_sum of "p < n_vertices and keep[p]"
//   3 partials  scan_block_sums: the block sums -> their exclusive prefix sums; the total n_hull_vertices
//   4 rank      rank[p] = the number of kept vertices below p; a kept vertex stores its id at its rank (scratch and vertices_out)
//   5 rect      one wave per loop: its record (OFFSET', COUNT', VALUE, START), HULL_AREA2 and the minimum rectangle over the hull's
//               edges, lanes strided over the edges, every lane over all hull vertices: O(k^2 / 64) for a hull of k vertices
//   6 finish    the per-value LOOP words from their keys; counts_out
// The number of loops and of vertices are device words: the grids come from the caller's rows.  Truncated input makes every launch
// see no loop and no vertex.  Every index a record holds is compared with the counts, and the counts with the rows, before it
// addresses anything.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kLoopBlock = 256;       // four waves, each with a loop of its own, per workgroup of the hull and rect launches
constexpr unsigned kLoopGrid = 8192;  // at most: 32 workgroups for each of 256 compute units, so that uneven loops even out
constexpr unsigned kMaxCoord = 8191;
constexpr unsigned kNone = 0xFFFFFFFFu;
// the words of a per-loop record and of a per-value row (the header's INFUR_SHAPE_*)
constexpr int kHullArea2 = 7, kRectEdge = 8, kRectW = 9, kRectH = 10, kRectL = 11, kOuter = 8, kHoles = 9, kLoopWord = 10;

using u64 = unsigned long long;
using u128 = unsigned __int128;

struct ShapesIn {
    const unsigned* loops;
    const unsigned* vertices;
    const unsigned* counts;
    unsigned loops_rows, vertex_rows, w1;  // w1: the lattice's width, w + 1
};

// -> the numbers of loops and vertices there are to read: both 0 when either exceeds its rows
__device__ __forceinline__ bool input_counts(const ShapesIn& in, unsigned* nl, unsigned* nv) {
    const unsigned c0 = in.counts[0], c1 = in.counts[1];
    const bool truncated = c0 > in.loops_rows || c1 > in.vertex_rows;
    *nl = truncated ? 0u : c0;
    *nv = truncated ? 0u : c1;
    return truncated;
}

// record i < nl -> its OFFSET and COUNT; false when it is malformed (COUNT < 2 or its vertices end beyond nv)
__device__ __forceinline__ bool loop_range(const ShapesIn& in, const unsigned i, const unsigned nv, unsigned* off, unsigned* cnt) {
    const unsigned* r = in.loops + (size_t)i * kLoopWords;
    *off = r[0];
    *cnt = r[1];
    return *cnt >= 2u && (uint64_t)*off + *cnt <= nv;
}

struct Pt {
    int x, y;
};
__device__ __forceinline__ Pt point_of(const unsigned id, const unsigned w1) {
    const unsigned y = id / w1;
    return {(int)(id - y * w1), (int)(y < kMaxCoord ? y : kMaxCoord)};  // a Y above 8191 reads as 8191
}
// vertex k of the loop at `off` with n vertices, k below 2n: the indices are cyclic
__device__ __forceinline__ Pt vertex(const ShapesIn& in, const unsigned off, const unsigned n, const unsigned k) {
    return point_of(in.vertices[off + (k >= n ? k - n : k)], in.w1);
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step, 64);
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const u64 o = __shfl_xor(v, step, 64);
        v = o > v ? o : v;
    }
    return v;
}

// the wave-wide maximum of the key (d, -i): the larger d, on a tie the smaller i; every lane gets the answer
__device__ __forceinline__ void wave_argmax(uint64_t* d, unsigned* i) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const uint64_t od = __shfl_xor((u64)*d, step, 64);
        const unsigned oi = __shfl_xor(*i, step, 64);
        if (od > *d || (od == *d && oi < *i)) {
            *d = od;
            *i = oi;
        }
    }
}

// (b - a) x (c - b)
__device__ __forceinline__ int64_t turn(const Pt a, const Pt b, const Pt c) {
    return (int64_t)(b.x - a.x) * (c.y - b.y) - (int64_t)(b.y - a.y) * (c.x - b.x);
}

// one wave, one loop: its measures (to `m`, in every lane) and the keep flags of its hull
__device__ __forceinline__ void hull_loop(const ShapesIn& in, const unsigned off, const unsigned n, const unsigned lane, u64 m[kShapeMeasures],
                                          uint8_t* __restrict__ keep) {
    // the measures, modulo 2^64, and the anchors
    u64 s[kShapeMeasures] = {};
    u64 lo_key = ~0ull, hi_key = 0;
    for (unsigned i = lane; i < n; i += 64u) {
        const Pt p = vertex(in, off, n, i), q = vertex(in, off, n, i + 1u);
        const int64_t xi = p.x, yi = p.y, xj = q.x, yj = q.y;
        const u64 c = (u64)(xi * yj - xj * yi);
        s[0] += c;
        s[1] += (u64)((xj > xi ? xj - xi : xi - xj) + (yj > yi ? yj - yi : yi - yj));
        s[2] += c * (u64)(xi + xj);
        s[3] += c * (u64)(yi + yj);
        s[4] += c * (u64)(xi * xi + xi * xj + xj * xj);
        s[5] += c * (u64)(yi * yi + yi * yj + yj * yj);
        s[6] += c * (u64)(xi * yj + 2 * xi * yi + 2 * xj * yj + xj * yi);
        const u64 yx = ((u64)p.y << 14 | (u64)p.x) << 32;
        const u64 lk = yx | i, hk = yx | (kNone - i);  // on equal (Y, X) the smallest index, both times
        lo_key = lk < lo_key ? lk : lo_key;
        hi_key = hk > hi_key ? hk : hi_key;
    }
#pragma unroll
    for (int k = 0; k < kShapeMeasures; k++) m[k] = wave_sum(s[k]);
    const unsigned lo = (unsigned)~wave_max(~lo_key), hi = kNone - (unsigned)wave_max(hi_key);
    if (lane == 0) keep[off + lo] = 1;
    if (lo != hi) {  // (otherwise every vertex is one point)
        if (lane == 0) keep[off + hi] = 1;
        const int64_t sgn = (int64_t)m[0] < 0 ? -1 : 1;
        // the ranges run over the indices lo .. lo + n, taken modulo n: a loop whose start is not a hull vertex wraps
        const unsigned H = hi > lo ? hi : hi + n;
        unsigned stack_a = H, stack_c = lo + n;  // entry 0 = (H, lo + n); entry k lives in lane k
        unsigned sp = 1, a = lo, c = H;
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
            uint64_t best = 0;
            unsigned at = kNone;
            for (unsigned i = a + 1u + lane; i < c; i += 64u) {
                const Pt p = vertex(in, off, n, i);
                const int64_t o = sgn * (ey * (p.x - pa.x) - ex * (p.y - pa.y));  // positive on the outer side of the chord
                const uint64_t d = o > 0 ? (uint64_t)o : 0u;
                if (at == kNone || d > best) {
                    best = d;
                    at = i;
                }
            }
            wave_argmax(&best, &at);
            const unsigned mid = at;  // a < mid < c
            if (best > 0 && sp < 64u) {  // (sp < 64 cannot fail: the waiting ranges at least double from the top down)
                if (lane == 0) keep[off + (mid >= n ? mid - n : mid)] = 1;
                const bool left_waits = mid - a >= c - mid;
                if (lane == sp) {
                    stack_a = left_waits ? a : mid;
                    stack_c = left_waits ? mid : c;
                }
                sp++;
                if (left_waits)
                    a = mid;
                else
                    c = mid;
            } else {
                c = a;  // nothing between a and c is on the hull
            }
        }
    }
    // The last pass: a kept vertex that is collinear with its kept neighbours goes.  Every test reads the flags as the recursion
    // left them: a chunk's flags are in the ballot before any of its vertices is dropped, and a drop only reaches backwards.
    __threadfence_block();
    unsigned c1 = kNone, c2 = kNone, f0 = kNone, f1 = kNone, total = 0;  // the last two and the first two kept so far, from lo on
    for (unsigned b = 0; b < n; b += 64u) {
        const unsigned t = b + lane;
        const bool flag = t < n && keep[off + (lo + t >= n ? lo + t - n : lo + t)] != 0;
        const uint64_t mask = __ballot(flag);
        if (flag) {
            const uint64_t below = mask & ((1ull << lane) - 1ull);
            unsigned p1 = c1, p2 = c2;
            if (below) {
                const unsigned h1 = 63u - (unsigned)__builtin_clzll(below);
                const uint64_t below2 = below & ~(1ull << h1);
                p1 = b + h1;
                p2 = below2 ? b + 63u - (unsigned)__builtin_clzll(below2) : c1;
            }
            if (p2 != kNone && turn(vertex(in, off, n, lo + p2), vertex(in, off, n, lo + p1), vertex(in, off, n, lo + t)) == 0)
                keep[off + (lo + p1 >= n ? lo + p1 - n : lo + p1)] = 0;
        }
        const unsigned cnt = (unsigned)__popcll(mask);
        if (cnt) {
            const unsigned top = 63u - (unsigned)__builtin_clzll(mask), bot = (unsigned)__builtin_ctzll(mask);
            const uint64_t rest = mask & (mask - 1ull);
            if (f0 == kNone) {
                f0 = b + bot;
                if (rest) f1 = b + (unsigned)__builtin_ctzll(rest);
            } else if (f1 == kNone) {
                f1 = b + bot;
            }
            c2 = cnt >= 2u ? b + 63u - (unsigned)__builtin_clzll(mask & ~(1ull << top)) : c1;
            c1 = b + top;
            total += cnt;
        }
    }
    if (total >= 3u && lane == 0) {  // the two triples that close the ring
        const Pt pl2 = vertex(in, off, n, lo + c2), pl1 = vertex(in, off, n, lo + c1), p0 = vertex(in, off, n, lo + f0), p1 = vertex(in, off, n, lo + f1);
        if (turn(pl2, pl1, p0) == 0) keep[off + (lo + c1 >= n ? lo + c1 - n : lo + c1)] = 0;
        if (turn(pl1, p0, p1) == 0) keep[off + (lo + f0 >= n ? lo + f0 - n : lo + f0)] = 0;
    }
}

// The loops are dealt to the waves of a grid that fills the machine and no more (simplify.hip).  sign[i]: 1 an outer loop
// (AREA2 > 0), 2 a hole (AREA2 < 0), else 0
__global__ void __launch_bounds__(kLoopBlock)
    shapes_hull_kernel(ShapesIn in, uint8_t* __restrict__ keep, uint8_t* __restrict__ sign, long long* __restrict__ shapes, unsigned shape_rows,
                       u64* __restrict__ values, unsigned value_rows) {
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const unsigned lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kLoopBlock / 64);
    for (size_t loop = (size_t)blockIdx.x * (kLoopBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) {
        unsigned off, n;
        u64 m[kShapeMeasures] = {};
        const bool well = loop_range(in, (unsigned)loop, nv, &off, &n);
        if (well) hull_loop(in, off, n, lane, m, keep);
        if (lane != 0) continue;
        const long long area2 = (long long)m[0];
        sign[loop] = !well || area2 == 0 ? 0 : area2 > 0 ? 1 : 2;
        if (shapes && loop < shape_rows)
            for (int k = 0; k < kShapeMeasures; k++) shapes[loop * kShapeWords + k] = (long long)m[k];
        const unsigned value = in.loops[loop * kLoopWords + 2];
        if (!well || !values || value >= value_rows) continue;
        u64* row = values + (size_t)value * kShapeWords;
        for (int k = 0; k < kShapeMeasures; k++) atomicAdd(row + k, m[k]);
        if (area2 > 0) {  // the value's outer loop with the largest AREA2 (below 2^28), on a tie the smallest index
            atomicAdd(row + kOuter, 1ull);
            atomicMax(row + kLoopWord, (u64)area2 << 32 | (u64)(kNone - (unsigned)loop));
        } else if (area2 < 0) {
            atomicAdd(row + kHoles, 1ull);
        }
    }
}

// the flag of position p of the scan: a kept vertex
__device__ __forceinline__ bool kept_at(const uint8_t* __restrict__ keep, const size_t p, const unsigned nv) { return p < nv && keep[p] != 0; }

__global__ void __launch_bounds__(kScanBlock) shapes_sums_kernel(ShapesIn in, const uint8_t* __restrict__ keep, unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(kept_at(keep, p, nv), wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: partial[0, NB) -> its exclusive prefix sums in place, the total (n_hull_vertices) to partial[NB]
__global__ void __launch_bounds__(kScanBlock) shapes_partials_kernel(unsigned* __restrict__ partial, size_t NB) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) partial[NB] = n;
}

__global__ void __launch_bounds__(kScanBlock)
    shapes_rank_kernel(ShapesIn in, const uint8_t* __restrict__ keep, const unsigned* __restrict__ partial, unsigned* __restrict__ rank,
                       unsigned* __restrict__ hull, unsigned* __restrict__ vertices_out, unsigned vertex_rows_out) {
    __shared__ unsigned wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;  // p <= vertex_rows_in has a word of rank[]
    const bool flag = kept_at(keep, p, nv);
    const unsigned r = flag_rank(flag, partial[blockIdx.x], wsum);
    if (p <= nv) rank[p] = r;
    if (flag) {  // (r < nv <= vertex_rows_in: inside hull[])
        const unsigned id = in.vertices[p];
        hull[r] = id;
        if (vertices_out && r < vertex_rows_out) vertices_out[r] = id;
    }
}

// A candidate rectangle: wh = W << 32 | H, lj = L << 32 | j; j == kNone: no edge yet.  Two words that are always replaced
// together by selects.
struct Rect {
    u64 wh, lj;
};
// a before b: the smaller W * H / L, compared exactly (the products reach 2^83); on a tie the smaller j
__device__ __forceinline__ bool rect_before(const Rect a, const Rect b) {
    const unsigned aj = (unsigned)a.lj, bj = (unsigned)b.lj;
    const u128 x = (u128)((a.wh >> 32) * (a.wh & kNone)) * (b.lj >> 32), y = (u128)((b.wh >> 32) * (b.wh & kNone)) * (a.lj >> 32);
    const bool both = aj != kNone && bj != kNone;
    return both ? x < y || (x == y && aj < bj) : aj != kNone;
}
__device__ __forceinline__ Rect rect_first(const Rect a, const Rect b) {
    const bool take = rect_before(a, b);
    return {take ? a.wh : b.wh, take ? a.lj : b.lj};
}

// one wave per loop: the record, HULL_AREA2 and the rectangle.  head[0]: a malformed record was seen; head[1]: the largest COUNT'
__global__ void __launch_bounds__(kLoopBlock)
    shapes_rect_kernel(ShapesIn in, const unsigned* __restrict__ rank, const unsigned* __restrict__ hull, const uint8_t* __restrict__ sign,
                       unsigned* __restrict__ head, unsigned* __restrict__ loops_out, unsigned loops_rows_out, long long* __restrict__ shapes,
                       unsigned shape_rows, u64* __restrict__ values, unsigned value_rows) {
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const unsigned lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kLoopBlock / 64);
    for (size_t loop = (size_t)blockIdx.x * (kLoopBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) {
        unsigned off, cnt;
        const bool well = loop_range(in, (unsigned)loop, nv, &off, &cnt);
        const unsigned first = rank[off < nv ? off : nv];
        const unsigned k = well ? rank[off + cnt] - first : 0u;
        const unsigned* h = hull + first;  // k ids
        u64 area = 0;
        Rect best = {0, kNone};
        for (unsigned j = lane; j < k; j += 64u) {
            const Pt v = point_of(h[j], in.w1), u = point_of(h[j + 1u < k ? j + 1u : 0u], in.w1);
            area += (u64)((int64_t)v.x * u.y - (int64_t)u.x * v.y);
            const int64_t ex = u.x - v.x, ey = u.y - v.y;
            int64_t lo = INT64_MAX, hi = INT64_MIN, far = 0;
            for (unsigned q = 0; q < k; q++) {
                const Pt p = point_of(h[q], in.w1);
                const int64_t dot = ex * p.x + ey * p.y, cr = ex * (p.y - v.y) - ey * (p.x - v.x);
                lo = dot < lo ? dot : lo;
                hi = dot > hi ? dot : hi;
                far = (cr < 0 ? -cr : cr) > far ? (cr < 0 ? -cr : cr) : far;
            }
            best = rect_first({(u64)(hi - lo) << 32 | (u64)far, (u64)(ex * ex + ey * ey) << 32 | j}, best);  // (each of W, H, L below 2^28)
        }
        area = wave_sum(area);
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) best = rect_first({__shfl_xor(best.wh, step, 64), __shfl_xor(best.lj, step, 64)}, best);
        if (lane != 0) continue;
        if (!well) atomicOr(head, 1u);
        atomicMax(head + 1, k);
        const unsigned* src = in.loops + loop * kLoopWords;
        if (loops_out && loop < loops_rows_out) {
            unsigned* r = loops_out + loop * kLoopWords;
            r[0] = first;
            r[1] = k;
            r[2] = src[2];
            r[3] = src[3];
        }
        if (shapes && loop < shape_rows) {
            long long* r = shapes + loop * kShapeWords;
            r[kHullArea2] = (long long)area;
            r[kRectEdge] = k ? (long long)(best.lj & kNone) : 0;
            r[kRectW] = k ? (long long)(best.wh >> 32) : 0;
            r[kRectH] = k ? (long long)(best.wh & kNone) : 0;
            r[kRectL] = k ? (long long)(best.lj >> 32) : 0;
        }
        if (values && sign[loop] == 1 && src[2] < value_rows) atomicAdd(values + (size_t)src[2] * kShapeWords + kHullArea2, area);
    }
}

// the per-value LOOP words from their keys (0: the value has no outer loop); thread 0 writes counts_out
__global__ void __launch_bounds__(256) shapes_finish_kernel(ShapesIn in, const unsigned* __restrict__ n_kept, const unsigned* __restrict__ head,
                                                            long long* __restrict__ values, unsigned value_rows, unsigned* __restrict__ counts_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (values && i < value_rows) {
        const u64 key = (u64)values[i * kShapeWords + kLoopWord];
        values[i * kShapeWords + kLoopWord] = key ? (long long)(kNone - (unsigned)key) : -1ll;
    }
    if (i != 0 || !counts_out) return;
    unsigned nl, nv;
    const bool truncated = input_counts(in, &nl, &nv);
    counts_out[0] = in.counts[0];
    counts_out[1] = *n_kept;
    counts_out[2] = (truncated ? kShapesTruncated : 0u) | (head[0] ? kShapesMalformed : 0u);
    counts_out[3] = head[1];
}

// the scratch, on 256-byte boundaries: [vertex block sums + total][rank][hull ids][sign][head][keep]; head and keep are cleared together
struct Layout {
    size_t partial, rank, hull, sign, head, keep, bytes;
    Layout(const size_t loops_rows, const size_t vertex_rows) {
        const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        partial = 0;
        rank = up((scan_blocks(vertex_rows + 1) + 1) * 4);
        hull = rank + up((vertex_rows + 1) * 4);
        sign = hull + up((vertex_rows + 1) * 4);
        head = sign + up(loops_rows + 1);
        keep = head + 256;
        bytes = keep + up(vertex_rows + 1);
    }
};

}  // namespace

size_t shapes_scratch_bytes(size_t loops_rows, size_t vertex_rows) { return Layout(loops_rows, vertex_rows).bytes; }

hipError_t launch_shapes(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                         unsigned W, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out, unsigned vertex_rows_out,
                         long long* shapes, unsigned shape_rows, long long* values, unsigned value_rows, unsigned* counts_out, hipStream_t s) {
    const Layout at(loops_rows_in, vertex_rows_in);
    uint8_t* base = (uint8_t*)scratch;
    unsigned* partial = (unsigned*)(base + at.partial);
    unsigned* rank = (unsigned*)(base + at.rank);
    unsigned* hull = (unsigned*)(base + at.hull);
    uint8_t* sign = base + at.sign;
    unsigned* head = (unsigned*)(base + at.head);
    uint8_t* keep = base + at.keep;
    const ShapesIn in = {loops, vertices, counts, loops_rows_in, vertex_rows_in, W + 1u};
    const size_t NB = scan_blocks((size_t)vertex_rows_in + 1);
    const size_t loop_blocks = ((size_t)loops_rows_in + 3) / 4;
    const dim3 loop_grid((unsigned)(loop_blocks < kLoopGrid ? loop_blocks : kLoopGrid));
    hipError_t e = hipMemsetAsync(head, 0, 256 + (size_t)vertex_rows_in + 1, s);
    if (e != hipSuccess) return e;
    if (values) {
        e = hipMemsetAsync(values, 0, (size_t)value_rows * kShapeWords * 8, s);
        if (e != hipSuccess) return e;
    }
    if (loops_rows_in)
        hipLaunchKernelGGL(shapes_hull_kernel, loop_grid, dim3(kLoopBlock), 0, s, in, keep, sign, shapes, shape_rows, (u64*)values, value_rows);
    hipLaunchKernelGGL(shapes_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, keep, partial);
    hipLaunchKernelGGL(shapes_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, partial, NB);
    hipLaunchKernelGGL(shapes_rank_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, keep, partial, rank, hull, vertices_out, vertex_rows_out);
    if (loops_rows_in)
        hipLaunchKernelGGL(shapes_rect_kernel, loop_grid, dim3(kLoopBlock), 0, s, in, rank, hull, sign, head, loops_out, loops_rows_out, shapes, shape_rows,
                           (u64*)values, value_rows);
    if (values || counts_out) {
        const unsigned blocks = values && value_rows ? (value_rows + 255u) / 256u : 1u;
        hipLaunchKernelGGL(shapes_finish_kernel, dim3(blocks), dim3(256), 0, s, in, partial + NB, head, values, value_rows, counts_out);
    }
    return hipGetLastError();
}

}  // namespace infur
