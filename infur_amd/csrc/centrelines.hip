// centrelines.hip -- Centrelines (include/infur_hip.h): the one-pixel centrelines Skeleton leaves, traced into polyline
// branches.  Every link of a kept pixel is two DARTS (pixel, direction); a dart knows its predecessor from its tail pixel alone -- a
// path pixel hands on its other link, a node starts a branch -- so the darts are disjoint chains that end at nodes, and cycles where a
// ring has no node.  Pointer doubling along the predecessors ranks both at once; the kernel boundaries are the only ordering, no
// workgroup waits for another, and every scratch and output word has one writer per launch (the one exception is the word a round
// raises so that the rounds behind a finished one leave at once).
//   1 links     a wave per row segment of kClCore columns and the column on either side: three rows of values and kept flags per
//               lane, E and W from shuffles and ballots -> link[p]: the link bits N, NE, E, SE, S, SW, W, NW and, in bit 8, "kept"
//   2 sums      per scan block of pixels: the darts, nodes, ends and diagonal darts
//   3 partials  the dart sums scanned, the others added up -> hdr = {n_darts, nodes, ends, diagonal darts}; clears the round words
//   4 base      base[p] = the dense index of p's first dart; dart (p, k) is base[p] + popcount(link[p] below k): ascending with 8p + k
//   5 init      per dart the record Dart of 48 bytes: its predecessor, itself as the window's minimum, and what it adds to a branch
//   6 K rounds  a = state[e], b = state[a.ptr]: the window [e .. ptr) takes in b's.  A chain is DONE once the window holds its start
//               (the start points at itself and is done from the beginning); a ring keeps, Outlines' way, the strict minimum m of
//               the window and the sums SINCE m, and is done once b's minimum is its own: the two windows then cover the cycle.  A
//               dart cannot know which of the two it is on, so both rules run on the one record.  Double-buffered; a round copies
//               what is done, so behind a round that met only done darts both buffers agree and the later rounds exit on its word
//   7 ends      the last dart of a chain (its head is a node) writes the branch's totals and "canonical" -- the start lies below
//               the reverse of this dart -- into the start's slot of the free buffer; a ring's start (m == itself) reads the
//               totals at its predecessor and is canonical when it runs along its pixel's lowest link
//   8 sums      per scan block of pixels: canonical starts and isolated pixels, their vertices, canonical rings
//   9 partials  scanned -> counts
//  10 rank      a start's pixel writes the record, the last vertex and (index, offset) into the slot; isolated pixels likewise
//  11 emit      every dart of a canonical branch stores its tail pixel at offset + (links or kept vertices behind it)
// Launches 10 and 11 are left out when neither records nor vertices are wanted.  Everything is an integer and a function of the
// inputs alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kClBlock = 256;
constexpr int kClCore = 62;         // columns a wave of the links launch owns; lanes 0 and 63 hold the column on either side
constexpr unsigned kClHdrWords = 64;  // n_darts, nodes, ends, diagonal darts, then the round words
constexpr unsigned kClLive = 4;       // hdr[kClLive + k]: round k met a dart that was not done
constexpr unsigned kChain = 1u, kRing = 2u;

// a dart's record, moved as three 128-bit words
struct Dart {
    uint4 a;  // ptr, m (the smallest dense index in the window), done (0, kChain, kRing), the window's MIN_H
    uint4 w;  // over the window [e .. ptr): links, kept vertices, diagonal links, MIN_H since m
    uint4 n;  // since m, inclusive: links, kept vertices, diagonal links, (unused)
};
static_assert(sizeof(Dart) == 48, "three 128-bit words");

// a start's slot in the buffer the last round left free: the same 48 bytes
//   a = (vertices, links, diagonal links, MIN_H)   w = (canonical, last pixel B, branch index, vertex offset)

struct Geo {
    unsigned H, W;
    size_t npix;
    int skip, corners;
    unsigned skip_value;
    unsigned cap2;  // the dart capacity, 2 * max_links
};

__device__ __forceinline__ size_t head_of(const size_t p, const unsigned k, const unsigned W) {
    const int dx = (k >= 1 && k <= 3) ? 1 : (k >= 5 ? -1 : 0), dy = (k == 7 || k <= 1) ? -1 : ((k >= 3 && k <= 5) ? 1 : 0);
    return p + (size_t)((ptrdiff_t)dy * (ptrdiff_t)W + dx);
}
__device__ __forceinline__ unsigned below(const unsigned link, const unsigned k) { return (unsigned)__popc(link & ((1u << k) - 1u)); }
// the tail vertex of dart (p, k) stays under CORNERS: p is a node, or the branch turns at p
__device__ __forceinline__ bool turns(const unsigned link, const unsigned k) { return link != ((1u << k) | (1u << (k ^ 4u))); }

// the sum of v over the workgroup of kScanBlock lanes, valid in thread 0
__device__ __forceinline__ unsigned value_block_sum(unsigned v, unsigned* wsum) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kScanBlock / 64; k++) s += wsum[k];
    return s;
}

// -> block_base + the sum of v over the lanes before this one in its workgroup.  Holds a barrier.
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

template <class T>
__global__ void __launch_bounds__(kClBlock)
    cl_links_kernel(const T* __restrict__ plane, const uint8_t* __restrict__ kind, Geo g, unsigned tilesX, uint16_t* __restrict__ link) {
    const size_t u = (size_t)blockIdx.x * (kClBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const unsigned y = (unsigned)(u / tilesX);
    if (y >= g.H) return;  // (the whole wave)
    const unsigned c = (unsigned)(u % tilesX) * kClCore + (unsigned)lane - 1u;  // wraps to a column outside the frame in lane 0 of tile 0
    unsigned v[3];
    uint64_t kept[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const unsigned yy = y + (unsigned)r - 1u;
        const bool in = c < g.W && yy < g.H;
        const size_t at = in ? (size_t)yy * g.W + c : 0;
        v[r] = in ? (unsigned)plane[at] : 0u;
        kept[r] = __ballot(in && !(g.skip && v[r] == g.skip_value) && (!kind || kind[at] != 0));
    }
    const unsigned me = v[1];
    unsigned set = 0;  // bit k: neighbour k is inside the frame, kept and holds this pixel's value
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const unsigned e = __shfl_down(v[r], 1, 64), wv = __shfl_up(v[r], 1, 64);
        const bool ke = lane < 63 && ((kept[r] >> (lane + 1)) & 1ull), kw = lane > 0 && ((kept[r] >> (lane - 1)) & 1ull), km = (kept[r] >> lane) & 1ull;
        const unsigned be = ke && e == me, bw = kw && wv == me, bm = km && v[r] == me;
        if (r == 0) set |= bm | (be << 1) | (bw << 7);
        if (r == 1) set |= (be << 2) | (bw << 6);
        if (r == 2) set |= (bm << 4) | (be << 3) | (bw << 5);
    }
    if (lane == 0 || lane == 63 || c >= g.W) return;
    unsigned out = 0;
    if ((kept[1] >> lane) & 1ull) {
        out = (set & 0x55u) | 0x100u;
#pragma unroll
        for (unsigned k = 1; k < 8; k += 2)
            if (((set >> k) & 1u) && !((set >> (k - 1u)) & 1u) && !((set >> ((k + 1u) & 7u)) & 1u)) out |= 1u << k;
    }
    link[(size_t)y * g.W + c] = (uint16_t)out;
}

__global__ void __launch_bounds__(kScanBlock) cl_dart_sums_kernel(const uint16_t* __restrict__ link, size_t npix, size_t NB, unsigned* __restrict__ part) {
    __shared__ unsigned ws[4][kScanBlock / 64];
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned l = p < npix ? link[p] : 0u, d = (unsigned)__popc(l & 255u);
    const unsigned darts = value_block_sum(d, ws[0]), nodes = flag_block_sum((l >> 8) && d != 2, ws[1]), ends = flag_block_sum(d == 1, ws[2]),
                   diag = value_block_sum((unsigned)__popc(l & 0xAAu), ws[3]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = darts;
        part[(NB + 1) + blockIdx.x] = nodes;
        part[(NB + 1) + NB + blockIdx.x] = ends;
        part[(NB + 1) + 2 * NB + blockIdx.x] = diag;
    }
}

// the total of t[0, NB) in thread 0 of one workgroup of kScanBlock lanes
__device__ __forceinline__ unsigned total_of(const unsigned* __restrict__ t, const size_t NB, unsigned* wsum) {
    unsigned v = 0;
    for (size_t i = threadIdx.x; i < NB; i += kScanBlock) v += t[i];
    __syncthreads();  // (wsum is free again)
    return value_block_sum(v, wsum);
}

__global__ void __launch_bounds__(kScanBlock) cl_dart_partials_kernel(unsigned* __restrict__ part, size_t NB, unsigned* __restrict__ hdr) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(part, NB, wsum);
    const unsigned nodes = total_of(part + (NB + 1), NB, wsum), ends = total_of(part + (NB + 1) + NB, NB, wsum),
                   diag = total_of(part + (NB + 1) + 2 * NB, NB, wsum);
    if (threadIdx.x == 0) {
        hdr[0] = n;
        hdr[1] = nodes;
        hdr[2] = ends;
        hdr[3] = diag;
    }
    if (threadIdx.x >= kClLive && threadIdx.x < kClHdrWords) hdr[threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(kScanBlock)
    cl_base_kernel(const uint16_t* __restrict__ link, size_t npix, const unsigned* __restrict__ part, unsigned* __restrict__ base) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned rank = value_rank(p < npix ? (unsigned)__popc(link[p] & 255u) : 0u, part[blockIdx.x], wsum);
    if (p < npix) base[p] = rank;
}

// the dense index of the dart that precedes (p, k) on a path pixel p: the dart into p along p's other link
__device__ __forceinline__ unsigned pred_of(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, const Geo& g, const size_t p,
                                            const unsigned l, const unsigned k, const unsigned self) {
    const unsigned other = l & ~(1u << k) & 255u;
    if (!other) return self;  // (cannot be: a path pixel has two links)
    const unsigned k2 = (unsigned)__ffs((int)other) - 1u;
    const size_t q = head_of(p, k2, g.W);
    if (q >= g.npix) return self;  // (cannot be: a link stays inside the frame)
    return base[q] + below(link[q] & 255u, k2 ^ 4u);
}

__global__ void __launch_bounds__(kClBlock)
    cl_init_kernel(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, const unsigned* __restrict__ height, Geo g,
                   const unsigned* __restrict__ hdr, Dart* __restrict__ state) {
    const unsigned n = hdr[0];
    const size_t p = (size_t)blockIdx.x * kClBlock + threadIdx.x;
    if (n > g.cap2 || p >= g.npix) return;
    const unsigned l = link[p] & 255u;
    if (!l) return;
    const bool node = __popc(l) != 2;
    const unsigned hg = height ? height[p] : 0u;
    unsigned self = base[p];
    for (unsigned rest = l; rest; rest &= rest - 1u, self++) {
        const unsigned k = (unsigned)__ffs((int)rest) - 1u;
        if (self >= n) return;  // (cannot be: the ranks are below their total)
        unsigned ptr = node ? self : pred_of(link, base, g, p, l, k, self);
        if (ptr >= n) ptr = self;  // (cannot be: a predecessor is a dart; no later read leaves the state for it)
        const unsigned kept = (node || turns(l, k)) ? 1u : 0u, dg = k & 1u;
        Dart d;
        d.a = make_uint4(ptr, self, ptr == self ? kChain : 0u, hg);
        d.w = make_uint4(1u, kept, dg, hg);
        d.n = make_uint4(1u, kept, dg, 0u);
        state[self] = d;
    }
}

__global__ void __launch_bounds__(kClBlock)
    cl_round_kernel(const Dart* __restrict__ src, Dart* __restrict__ dst, unsigned* __restrict__ hdr, unsigned cap2, unsigned round) {
    const unsigned n = hdr[0];
    const size_t e = (size_t)blockIdx.x * kClBlock + threadIdx.x;
    if (n > cap2 || (round && !hdr[kClLive + round - 1u])) return;  // overflow, or the round before met only done darts: both buffers agree
    const bool live = e < n;
    Dart a;
    if (live) a = src[e];
    const bool open = live && !a.a.z;
    if (__ballot(open) && (threadIdx.x & 63) == 0) __hip_atomic_store(&hdr[kClLive + round], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!live) return;
    if (open) {
        const Dart b = src[a.a.x];
        if (b.a.y < a.a.y) {  // the strict minimum moves on: what a held lies behind it
            a.a.y = b.a.y;
            a.n = make_uint4(b.n.x + a.w.x, b.n.y + a.w.y, b.n.z + a.w.z, 0u);
            a.w.w = min(b.w.w, a.a.w);
        } else if (b.a.y == a.a.y) {
            a.a.z = kRing;  // both windows hold the same minimum: together they cover the cycle
        }
        if (b.a.z) a.a.z = b.a.z;
        a.w.x += b.w.x;
        a.w.y += b.w.y;
        a.w.z += b.w.z;
        a.a.w = min(a.a.w, b.a.w);
        a.a.x = b.a.x;
    }
    dst[e] = a;
}

__global__ void __launch_bounds__(kClBlock)
    cl_ends_kernel(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, const unsigned* __restrict__ height, Geo g,
                   const unsigned* __restrict__ hdr, const Dart* __restrict__ state, Dart* __restrict__ slot) {
    const unsigned n = hdr[0];
    const size_t p = (size_t)blockIdx.x * kClBlock + threadIdx.x;
    if (n > g.cap2 || p >= g.npix) return;
    const unsigned l = link[p] & 255u;
    if (!l) return;
    const bool path = __popc(l) == 2;
    unsigned self = base[p];
    for (unsigned rest = l; rest; rest &= rest - 1u, self++) {
        const unsigned k = (unsigned)__ffs((int)rest) - 1u;
        if (self >= n) return;
        const size_t q = head_of(p, k, g.W);
        if (q >= g.npix) continue;  // (cannot be)
        const unsigned lq = link[q] & 255u;
        const Dart d = state[self];
        if (__popc(lq) != 2) {  // the last dart of a chain
            const unsigned s = d.a.x < n ? d.a.x : self, rev = base[q] + below(lq, k ^ 4u);
            const unsigned mh = min(d.a.w, height ? height[q] : 0u);
            slot[s].a = make_uint4((g.corners ? d.w.y : d.w.x) + 1u, d.w.x, d.w.z, mh);
            slot[s].w = make_uint4(s < rev ? 1u : 0u, (unsigned)q, 0u, 0u);
        } else if (path && d.a.z == kRing && d.a.y == self) {  // a ring's start: the totals since it stand at its predecessor
            const unsigned pm = pred_of(link, base, g, p, l, k, self);
            const Dart t = state[pm < n ? pm : self];
            slot[self].a = make_uint4((g.corners ? t.n.y : t.n.x) + 1u, t.n.x, t.n.z, t.w.w);
            slot[self].w = make_uint4(k == (unsigned)__ffs((int)l) - 1u ? 1u : 0u, (unsigned)p, 0u, 0u);
        }
    }
}

// what the pixel's lane of launches 8 and 10 knows: the canonical starts among its darts (bit i: its i-th dart), the rings among
// them, their vertices; an isolated kept pixel is a branch of one vertex
struct Starts {
    unsigned l, first, mask, rings, branches, vertices;
    bool isolated;
};
__device__ __forceinline__ Starts starts_of(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, const size_t npix, const unsigned n,
                                            const Dart* __restrict__ state, const Dart* __restrict__ slot, const size_t p) {
    Starts s = {0u, 0u, 0u, 0u, 0u, 0u, false};
    if (p >= npix) return s;
    const unsigned l16 = link[p];
    s.l = l16 & 255u;
    s.isolated = l16 == 0x100u;
    if (s.isolated) s.branches = s.vertices = 1u;
    if (!s.l) return s;
    const bool node = __popc(s.l) != 2;
    s.first = base[p];
    for (unsigned i = 0, e = s.first; i < (unsigned)__popc(s.l) && e < n; i++, e++) {
        bool start = node;
        if (!node) {
            const uint4 a = state[e].a;
            start = a.z == kRing && a.y == e;
        }
        if (start && slot[e].w.x) {
            s.mask |= 1u << i;
            s.rings += node ? 0u : 1u;
            s.branches++;
            s.vertices += slot[e].a.x;
        }
    }
    return s;
}

__global__ void __launch_bounds__(kScanBlock)
    cl_branch_sums_kernel(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, size_t npix, size_t NB, const unsigned* __restrict__ hdr,
                          unsigned cap2, const Dart* __restrict__ state, const Dart* __restrict__ slot, unsigned* __restrict__ part) {
    __shared__ unsigned ws[3][kScanBlock / 64];
    const unsigned n = hdr[0];
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    Starts s = {0u, 0u, 0u, 0u, 0u, 0u, false};
    if (n <= cap2) s = starts_of(link, base, npix, n, state, slot, p);  // overflow: no branches
    const unsigned b = value_block_sum(s.branches, ws[0]), v = value_block_sum(s.vertices, ws[1]), r = value_block_sum(s.rings, ws[2]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = b;
        part[(NB + 1) + blockIdx.x] = v;
        part[2 * (NB + 1) + blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(kScanBlock)
    cl_branch_partials_kernel(unsigned* __restrict__ part, size_t NB, const unsigned* __restrict__ hdr, unsigned cap2, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned branches = scan_block_sums(part, NB, wsum);
    __syncthreads();
    const unsigned vertices = scan_block_sums(part + (NB + 1), NB, wsum);
    const unsigned rings = total_of(part + 2 * (NB + 1), NB, wsum);
    if (threadIdx.x == 0 && counts) {
        counts[0] = branches;
        counts[1] = vertices;
        counts[2] = hdr[0] / 2u;
        counts[3] = hdr[1];
        counts[4] = hdr[2];
        counts[5] = rings;
        counts[6] = hdr[3] / 2u;
        counts[7] = hdr[0] > cap2 ? kCentrelinesOverflow : 0u;
    }
}

__device__ __forceinline__ void put_record(unsigned* __restrict__ records, const unsigned rows, const unsigned index, const unsigned offset, const unsigned count,
                                           const unsigned value, const unsigned a, const unsigned b, const unsigned links, const unsigned diag,
                                           const unsigned min_h) {
    if (!records || index >= rows) return;
    unsigned* r = records + (size_t)index * kCentrelineWords;  // (a caller's u32 array: word stores, no 128-bit alignment assumed)
    r[0] = offset;
    r[1] = count;
    r[2] = value;
    r[3] = a;
    r[4] = b;
    r[5] = links - diag;
    r[6] = diag;
    r[7] = min_h;
}

template <class T>
__global__ void __launch_bounds__(kScanBlock)
    cl_rank_kernel(const T* __restrict__ plane, const uint16_t* __restrict__ link, const unsigned* __restrict__ base, const unsigned* __restrict__ height,
                   size_t npix, size_t NB, const unsigned* __restrict__ hdr, unsigned cap2, const Dart* __restrict__ state, Dart* __restrict__ slot,
                   const unsigned* __restrict__ part, unsigned* __restrict__ records, unsigned rows, unsigned* __restrict__ vertices, unsigned vertex_rows) {
    __shared__ unsigned ws[2][kScanBlock / 64];
    const unsigned n = hdr[0];
    if (n > cap2) return;  // (the whole launch)
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const Starts s = starts_of(link, base, npix, n, state, slot, p);
    unsigned index = value_rank(s.branches, part[blockIdx.x], ws[0]), offset = value_rank(s.vertices, part[(NB + 1) + blockIdx.x], ws[1]);
    if (!s.branches) return;
    const unsigned value = (unsigned)plane[p];
    if (s.isolated) {
        put_record(records, rows, index, offset, 1u, value, (unsigned)p, (unsigned)p, 0u, 0u, height ? height[p] : 0u);
        if (vertices && offset < vertex_rows) vertices[offset] = (unsigned)p;
        return;
    }
    for (unsigned i = 0; i < 4; i++) {
        if (!((s.mask >> i) & 1u)) continue;
        const unsigned e = s.first + i;
        const uint4 t = slot[e].a, c = slot[e].w;
        put_record(records, rows, index, offset, t.x, value, (unsigned)p, c.y, t.y, t.z, t.w);
        if (vertices && t.x && offset + t.x - 1u < vertex_rows) vertices[offset + t.x - 1u] = c.y;
        slot[e].w = make_uint4(1u, c.y, index, offset);
        index++;
        offset += t.x;
    }
}

__global__ void __launch_bounds__(kClBlock)
    cl_emit_kernel(const uint16_t* __restrict__ link, const unsigned* __restrict__ base, Geo g, const unsigned* __restrict__ hdr,
                   const Dart* __restrict__ state, const Dart* __restrict__ slot, unsigned* __restrict__ vertices, unsigned vertex_rows) {
    const unsigned n = hdr[0];
    const size_t p = (size_t)blockIdx.x * kClBlock + threadIdx.x;
    if (n > g.cap2 || p >= g.npix) return;
    const unsigned l = link[p] & 255u;
    if (!l) return;
    const bool node = __popc(l) != 2;
    unsigned self = base[p];
    for (unsigned rest = l; rest; rest &= rest - 1u, self++) {
        const unsigned k = (unsigned)__ffs((int)rest) - 1u;
        if (self >= n) return;
        const Dart d = state[self];
        const unsigned s = d.a.z == kRing ? d.a.y : d.a.x;  // the branch's start
        if (!d.a.z || s >= n) continue;                     // (cannot be: K rounds finish every dart)
        const uint4 c = slot[s].w;
        if (!c.x) continue;  // the branch is listed from its other end
        if (g.corners && !(node || turns(l, k))) continue;
        const unsigned behind = d.a.z == kRing ? (g.corners ? d.n.y : d.n.x) : (g.corners ? d.w.y : d.w.x);
        const unsigned at = c.w + behind - 1u;
        if (behind && at < vertex_rows) vertices[at] = (unsigned)p;
    }
}

__global__ void cl_empty_kernel(unsigned* __restrict__ counts) {
    if (threadIdx.x < kCentrelinesCountWords) counts[threadIdx.x] = 0u;
}

// the scratch, on 256-byte boundaries: [hdr][dart partials: 4 arrays][branch partials: 3 arrays][link][base][state A][state B]
struct Layout {
    size_t hdr, dart_part, branch_part, link, base, state_a, state_b, bytes;
    Layout(const size_t npix, const size_t cap2) {
        const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        const size_t NB = scan_blocks(npix);
        hdr = 0;
        dart_part = up(kClHdrWords * 4);
        branch_part = dart_part + up(((NB + 1) + 3 * NB) * 4);
        link = branch_part + up(3 * (NB + 1) * 4);
        base = link + up(npix * 2);
        state_a = base + up(npix * 4);
        state_b = state_a + up(cap2 * sizeof(Dart));
        bytes = state_b + up(cap2 * sizeof(Dart));
    }
};

template <class T>
hipError_t launch_centrelines_t(const T* plane, const uint8_t* kind, const unsigned* height, unsigned H, unsigned W, int skip, int corners,
                                unsigned skip_value, size_t max_links, uint8_t* scratch, unsigned* records, unsigned rows, unsigned* vertices,
                                unsigned vertex_rows, unsigned* counts, hipStream_t s) {
    const size_t npix = (size_t)H * W, NB = scan_blocks(npix), cap2 = 2 * max_links;
    const Layout at(npix, cap2);
    const Geo g = {H, W, npix, skip, corners, skip_value, (unsigned)cap2};  // (cap2 <= 4 * H * W < 2^32)
    unsigned* hdr = (unsigned*)(scratch + at.hdr);
    unsigned* dart_part = (unsigned*)(scratch + at.dart_part);
    unsigned* branch_part = (unsigned*)(scratch + at.branch_part);
    uint16_t* link = (uint16_t*)(scratch + at.link);
    unsigned* base = (unsigned*)(scratch + at.base);
    Dart* a = (Dart*)(scratch + at.state_a);
    Dart* b = (Dart*)(scratch + at.state_b);
    const unsigned tilesX = (W + kClCore - 1) / kClCore;
    const dim3 rows4((unsigned)(((size_t)H * tilesX + 3) / 4)), pixels((unsigned)((npix + kClBlock - 1) / kClBlock)), dense((unsigned)((cap2 + kClBlock - 1) / kClBlock));
    hipLaunchKernelGGL(cl_links_kernel<T>, rows4, dim3(kClBlock), 0, s, plane, kind, g, tilesX, link);
    hipLaunchKernelGGL(cl_dart_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, link, npix, NB, dart_part);
    hipLaunchKernelGGL(cl_dart_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, dart_part, NB, hdr);
    hipLaunchKernelGGL(cl_base_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, link, npix, dart_part, base);
    hipLaunchKernelGGL(cl_init_kernel, pixels, dim3(kClBlock), 0, s, link, base, height, g, hdr, a);
    const unsigned K = centrelines_rounds(max_links);
    for (unsigned k = 0; k < K; k++) {
        hipLaunchKernelGGL(cl_round_kernel, dense, dim3(kClBlock), 0, s, a, b, hdr, g.cap2, k);
        Dart* t = a;
        a = b;
        b = t;
    }  // a: the final state; b: free, the starts' slots
    hipLaunchKernelGGL(cl_ends_kernel, pixels, dim3(kClBlock), 0, s, link, base, height, g, hdr, a, b);
    hipLaunchKernelGGL(cl_branch_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, link, base, npix, NB, hdr, g.cap2, a, b, branch_part);
    hipLaunchKernelGGL(cl_branch_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, branch_part, NB, hdr, g.cap2, counts);
    if (records || vertices) {
        hipLaunchKernelGGL(cl_rank_kernel<T>, dim3((unsigned)NB), dim3(kScanBlock), 0, s, plane, link, base, height, npix, NB, hdr, g.cap2, a, b, branch_part,
                           records, rows, vertices, vertex_rows);
        if (vertices) hipLaunchKernelGGL(cl_emit_kernel, pixels, dim3(kClBlock), 0, s, link, base, g, hdr, a, b, vertices, vertex_rows);
    }
    return hipGetLastError();
}

}  // namespace

size_t centrelines_scratch_bytes(size_t npix, size_t max_links) { return Layout(npix, 2 * max_links).bytes; }

unsigned centrelines_rounds(size_t max_links) {
    unsigned k = 0;
    while (((size_t)1 << k) < 2 * max_links) k++;
    return k + 1;  // a ring's last dart needs one round more than its window: the window behind it must reach the start again
}

hipError_t launch_centrelines(const void* plane, int elem_bytes, const uint8_t* kind, const unsigned* height, unsigned H, unsigned W, int skip, int corners,
                              unsigned skip_value, size_t max_links, void* scratch, unsigned* records, unsigned rows, unsigned* vertices,
                              unsigned vertex_rows, unsigned* counts, hipStream_t s) {
    if ((size_t)H * W == 0) {
        if (counts) hipLaunchKernelGGL(cl_empty_kernel, dim3(1), dim3(64), 0, s, counts);
        return hipGetLastError();
    }
    if (!rows) records = nullptr;
    if (!vertex_rows) vertices = nullptr;
    if (elem_bytes == 1)
        return launch_centrelines_t((const uint8_t*)plane, kind, height, H, W, skip, corners, skip_value, max_links, (uint8_t*)scratch, records, rows, vertices,
                                    vertex_rows, counts, s);
    if (elem_bytes == 4)
        return launch_centrelines_t((const uint32_t*)plane, kind, height, H, W, skip, corners, skip_value, max_links, (uint8_t*)scratch, records, rows, vertices,
                                    vertex_rows, counts, s);
    return hipErrorInvalidValue;
}

}  // namespace infur
