// coverage.hip -- Coverage: Outlines' loops simplified so that neighbouring polygons still fit (include/infur_hip.h).
// A border between two regions is walked by two loops, in opposite directions.  The loops are cut at the plane's junctions (lattice
// vertices where three or four borders meet) into arcs, and an arc's kept set is a function of its vertex sequence that does not
// change when the sequence is reversed: both neighbours keep the same vertices.  One wave owns one arc.  The kernel boundaries are
// the only ordering: no workgroup ever waits for another and there is no atomic.
//   0 clear      keep[0, aug_rows] = 0 (a memset node)
//   1 junctions  one lane per lattice vertex, four cell loads, one ballot per wave: a bitmap in 64-bit words along the rows
//   2 junctions  the same along the columns, so that a vertical edge reads words too
//   3 measure    one wave per loop, a lane per edge: 1 + the junction bits strictly inside the edge (whole words: a long straight
//                edge costs length / 64); the loop's augmented length, its junction count, whether it is malformed
//   4 loop sums, 5 loop partials, 6 loop offsets: the exclusive prefix sums of the augmented lengths and of the arc counts over
//                the loops, in 64 bits and stored saturated, so that no hand-made input can wrap a sum below the capacity
//   7 emit       one wave per loop: the augmented ids, a junction byte each, and the arc table (head position, loop)
//   8 arcs       one wave per arc or ring (dealt round-robin to at most 32 Ki waves): Simplify's strided argmax and register stack,
//                with the key (D, -id) and indices modulo the loop; a ring first finds its two anchors
//   9 sums, 10 partials, 11 rank: the flag scan of wave_scan.h over the keep flags; a kept vertex stores its id at its rank
//  12 records    one lane per loop: OFFSET' = rank[first], COUNT' = rank[end] - rank[first]; block sums of "COUNT' < 3" and "malformed"
//  13 counts     one workgroup adds those block sums and writes counts_out
// The numbers of loops and vertices are device words: the grids come from the caller's rows, and waves beyond the counts have
// nothing to do.  Truncated input makes every launch see no loop; more augmented vertices than aug_rows makes every launch after
// the loop scan see none.  Every index a record or a vertex holds is compared with the counts, the rows and the lattice before it
// addresses anything, and every store into the augmented arrays is compared with aug_rows.  Integers only, one writer per word.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kWaveBlock = 256;       // four waves, each with a loop or an arc of its own
constexpr unsigned kWaveGrid = 8192;  // at most: 32 workgroups for each of 256 compute units, so that uneven work evens out
constexpr uint64_t kNoCell = 1ull << 32;  // outside the plane or skipped: no 32-bit value
constexpr unsigned kIdle = 0xFFFFFFFFu;

struct CovIn {
    const void* plane;
    const unsigned* loops;
    const unsigned* vertices;
    const unsigned* counts;
    unsigned elem_bytes, H, W, skip, skip_value;
    unsigned loops_rows, vertex_rows, aug_rows;
    unsigned w1, h1, wordsX, wordsY;  // the lattice (W + 1) x (H + 1); 64-bit words per lattice row and per lattice column
};

// the scratch, on 256-byte boundaries
struct Layout {
    size_t jrow, jcol, loop_n, loop_j, loop_bad, part_n, part_a, aug_off, arc_off, aug, jf, arc_pos, arc_loop, keep, rank, partial, thin, bad, bytes;
    Layout(const size_t H, const size_t W, const size_t loops_rows, const size_t aug_rows) {
        const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        size_t at = 0;
        const auto take = [&](size_t n) {
            const size_t here = at;
            at += up(n);
            return here;
        };
        jrow = take((H + 1) * ((W + 64) / 64) * 8);
        jcol = take((W + 1) * ((H + 64) / 64) * 8);
        loop_n = take((loops_rows + 1) * 4);
        loop_j = take((loops_rows + 1) * 4);
        loop_bad = take(loops_rows + 1);
        part_n = take((scan_blocks(loops_rows + 1) + 1) * 8);
        part_a = take((scan_blocks(loops_rows + 1) + 1) * 8);
        aug_off = take((loops_rows + 1) * 4);
        arc_off = take((loops_rows + 1) * 4);
        aug = take(aug_rows * 4);
        jf = take(aug_rows);
        arc_pos = take(aug_rows * 4);
        arc_loop = take(aug_rows * 4);
        keep = take(aug_rows + 1);
        rank = take((aug_rows + 1) * 4);
        partial = take((scan_blocks(aug_rows + 1) + 1) * 4);
        thin = take((scan_blocks(loops_rows) + 1) * 4);
        bad = take((scan_blocks(loops_rows) + 1) * 4);
        bytes = at;
    }
};

struct CovScratch {
    uint64_t *jrow, *jcol, *part_n, *part_a;
    unsigned *loop_n, *loop_j, *aug_off, *arc_off, *aug, *arc_pos, *arc_loop, *rank, *partial, *thin, *bad;
    uint8_t *loop_bad, *jf, *keep;
    unsigned NBL;  // the workgroups of the loop scan: part_n[NBL] and part_a[NBL] hold the totals
};

// -> the numbers of loops and vertices there are to read: both 0 when either exceeds its rows
__device__ __forceinline__ bool input_counts(const CovIn& in, unsigned* nl, unsigned* nv) {
    const unsigned c0 = in.counts[0], c1 = in.counts[1];
    const bool truncated = c0 > in.loops_rows || c1 > in.vertex_rows;
    *nl = truncated ? 0u : c0;
    *nv = truncated ? 0u : c1;
    return truncated;
}

// record i < nl -> its OFFSET and COUNT; false when it is malformed (COUNT < 2 or its vertices end beyond nv)
__device__ __forceinline__ bool loop_range(const CovIn& in, const unsigned i, const unsigned nv, unsigned* off, unsigned* cnt) {
    const unsigned* r = in.loops + (size_t)i * kLoopWords;
    *off = r[0];
    *cnt = r[1];
    return *cnt >= 2u && (uint64_t)*off + *cnt <= nv;
}

__device__ __forceinline__ unsigned sat32(const uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)v; }

// the totals the loop scan left: the augmented vertices (saturated) and whether they exceed the capacity
__device__ __forceinline__ bool aug_total(const CovIn& in, const CovScratch& sc, unsigned* n_aug) {
    const uint64_t n = sc.part_n[sc.NBL];
    *n_aug = sat32(n);
    return n > in.aug_rows;
}

// ---------------------------------------------------------------- junction bits
__device__ __forceinline__ uint64_t cell(const CovIn& in, const int x, const int y) {
    if (x < 0 || y < 0 || x >= (int)in.W || y >= (int)in.H) return kNoCell;
    const size_t i = (size_t)y * in.W + (size_t)x;
    const unsigned v = in.elem_bytes == 1 ? (unsigned)((const uint8_t*)in.plane)[i] : ((const unsigned*)in.plane)[i];
    return in.skip && v == in.skip_value ? kNoCell : (uint64_t)v;
}

// kCol = false: a wave is 64 consecutive X of one lattice row, word Y * wordsX + X / 64; true: 64 consecutive Y of one lattice
// column, word X * wordsY + Y / 64.  Bits beyond the lattice are 0
template <bool kCol>
__global__ void __launch_bounds__(kWaveBlock) coverage_junction_kernel(CovIn in, uint64_t* __restrict__ bits) {
    const size_t u = (size_t)blockIdx.x * (kWaveBlock / 64) + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    const unsigned words = kCol ? in.wordsY : in.wordsX, lines = kCol ? in.w1 : in.h1;
    const unsigned line = (unsigned)(u / words), along = (unsigned)(u % words) * 64u + lane;
    if (line >= lines) return;  // (the whole wave)
    const int X = (int)(kCol ? line : along), Y = (int)(kCol ? along : line);
    bool junction = false;
    if (X < (int)in.w1 && Y < (int)in.h1) {
        const uint64_t ul = cell(in, X - 1, Y - 1), ur = cell(in, X, Y - 1), ll = cell(in, X - 1, Y), lr = cell(in, X, Y);
        junction = (int)(ul != ur) + (int)(ll != lr) + (int)(ul != ll) + (int)(ur != lr) >= 3;
    }
    const uint64_t m = __ballot(junction);
    if (lane == 0) bits[u] = m;
}

// ---------------------------------------------------------------- edges of a loop
// word wi of a bitmap line, cut to the bits lo .. hi (inclusive, lo <= hi, wi between their words)
__device__ __forceinline__ uint64_t cut(uint64_t m, const unsigned wi, const unsigned lo, const unsigned hi) {
    if (wi == (lo >> 6)) m &= ~0ull << (lo & 63u);
    if (wi == (hi >> 6)) m &= ~0ull >> (63u - (hi & 63u));
    return m;
}

struct Edge {
    bool bad, head;        // malformed; the tail vertex is a junction
    const uint64_t* line;  // the bitmap line the edge lies on
    unsigned lo, hi;       // the positions strictly inside it, inclusive: none when lo > hi
    bool forward;          // travelled towards larger positions
    unsigned step, origin;  // the vertex at position t of the line has the id origin + t * step
};

// the edge from vertex id a to vertex id b
__device__ __forceinline__ Edge edge_of(const CovIn& in, const CovScratch& sc, const unsigned a, const unsigned b) {
    Edge e = {true, false, nullptr, 1u, 0u, true, 0u, 0u};
    const unsigned lattice = in.w1 * in.h1;  // at most 2^26
    if (a >= lattice || b >= lattice) return e;
    const unsigned ya = a / in.w1, xa = a - ya * in.w1, yb = b / in.w1, xb = b - yb * in.w1;
    if ((xa == xb) == (ya == yb)) return e;  // a diagonal, or no length
    e.bad = false;
    e.head = (sc.jrow[(size_t)ya * in.wordsX + (xa >> 6)] >> (xa & 63u)) & 1ull;
    unsigned from, to;
    if (ya == yb) {
        e.line = sc.jrow + (size_t)ya * in.wordsX;
        from = xa, to = xb, e.step = 1u, e.origin = ya * in.w1;
    } else {
        e.line = sc.jcol + (size_t)xa * in.wordsY;
        from = ya, to = yb, e.step = in.w1, e.origin = xa;
    }
    e.forward = to > from;
    e.lo = (e.forward ? from : to) + 1u;
    e.hi = (e.forward ? to : from) - 1u;  // (from != to: no wrap)
    return e;
}

__device__ __forceinline__ unsigned inside_count(const Edge& e) {
    unsigned n = 0;
    if (e.lo <= e.hi)
        for (unsigned wi = e.lo >> 6; wi <= (e.hi >> 6); wi++) n += (unsigned)__popcll(cut(e.line[wi], wi, e.lo, e.hi));
    return n;
}

// vertex k of the record at `off` with cnt vertices, cyclically
__device__ __forceinline__ unsigned loop_vertex(const CovIn& in, const unsigned off, const unsigned cnt, const unsigned k) {
    return in.vertices[(size_t)off + (k == cnt ? 0u : k)];
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) v += __shfl_xor((unsigned long long)v, step, 64);
    return v;
}

__global__ void __launch_bounds__(kWaveBlock) coverage_measure_kernel(CovIn in, CovScratch sc) {
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const unsigned lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kWaveBlock / 64);
    for (size_t loop = (size_t)blockIdx.x * (kWaveBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) {
        unsigned off, cnt;
        bool bad = !loop_range(in, (unsigned)loop, nv, &off, &cnt);
        uint64_t n = 0, j = 0;
        if (!bad) {
            for (unsigned i = lane; i < cnt; i += 64u) {
                const Edge e = edge_of(in, sc, loop_vertex(in, off, cnt, i), loop_vertex(in, off, cnt, i + 1u));
                if (e.bad) {
                    bad = true;
                    break;
                }
                const unsigned k = inside_count(e);
                n += 1u + k;
                j += (e.head ? 1u : 0u) + k;
            }
        }
        bad = __ballot(bad) != 0ull;
        n = wave_sum64(n);
        j = wave_sum64(j);
        if (lane == 0) {
            sc.loop_n[loop] = bad ? 0u : sat32(n);
            sc.loop_j[loop] = bad ? 0u : sat32(j);
            sc.loop_bad[loop] = bad ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------- the scan over the loops (values, in 64 bits)
// what loop i adds: its augmented vertices, and its arcs (a loop without a junction is one ring)
__device__ __forceinline__ void loop_adds(const CovScratch& sc, const size_t i, const unsigned nl, uint64_t* n, uint64_t* a) {
    *n = *a = 0;
    if (i < nl) {
        const unsigned ln = sc.loop_n[i], lj = sc.loop_j[i];
        *n = ln;
        *a = ln ? (lj ? lj : 1u) : 0u;
    }
}

// -> the sum over the workgroup before this lane; *all: over the whole workgroup.  wsum: kScanBlock / 64 words of LDS, free again
// on return
__device__ __forceinline__ uint64_t block_exclusive64(const uint64_t v, uint64_t* wsum, uint64_t* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int k = 0; k < kScanBlock / 64; k++) {
        const uint64_t s = wsum[k];
        before += k < wave ? s : 0ull;
        total += s;
    }
    __syncthreads();
    *all = total;
    return before + inc - v;
}

__global__ void __launch_bounds__(kScanBlock) coverage_loop_sums_kernel(CovIn in, CovScratch sc) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    uint64_t n, a, all_n, all_a;
    loop_adds(sc, (size_t)blockIdx.x * kScanBlock + threadIdx.x, nl, &n, &a);
    block_exclusive64(n, wsum, &all_n);
    block_exclusive64(a, wsum, &all_a);
    if (threadIdx.x == 0) {
        sc.part_n[blockIdx.x] = all_n;
        sc.part_a[blockIdx.x] = all_a;
    }
}

// one workgroup: part[0, NB) -> its exclusive prefix sums in place, the total to part[NB] (scan_block_sums of wave_scan.h in 64 bits)
__device__ __forceinline__ void scan_sums64(uint64_t* __restrict__ part, const size_t NB, uint64_t* wsum) {
    uint64_t carry = 0;
    for (size_t base = 0; base < NB; base += kScanBlock) {
        const size_t i = base + threadIdx.x;
        uint64_t all;
        const uint64_t before = block_exclusive64(i < NB ? part[i] : 0ull, wsum, &all);
        if (i < NB) part[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) part[NB] = carry;
}

__global__ void __launch_bounds__(kScanBlock) coverage_loop_partials_kernel(CovScratch sc) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    scan_sums64(sc.part_n, sc.NBL, wsum);
    scan_sums64(sc.part_a, sc.NBL, wsum);
}

// aug_off[i], arc_off[i] for i <= n_loops: where loop i's augmented vertices and arcs begin; [n_loops] holds the totals
__global__ void __launch_bounds__(kScanBlock) coverage_loop_offsets_kernel(CovIn in, CovScratch sc) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    unsigned nl, nv;
    input_counts(in, &nl, &nv);
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint64_t n, a, all;
    loop_adds(sc, i, nl, &n, &a);
    const uint64_t bn = block_exclusive64(n, wsum, &all), ba = block_exclusive64(a, wsum, &all);
    if (i <= nl) {
        sc.aug_off[i] = sat32(sc.part_n[blockIdx.x] + bn);
        sc.arc_off[i] = sat32(sc.part_a[blockIdx.x] + ba);
    }
}

// ---------------------------------------------------------------- the augmented loops and the arc table
__device__ __forceinline__ unsigned wave_inclusive(unsigned v, const unsigned lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d, 64);
        if (lane >= (unsigned)d) v += t;
    }
    return v;
}

__global__ void __launch_bounds__(kWaveBlock) coverage_emit_kernel(CovIn in, CovScratch sc) {
    unsigned nl, nv, n_aug;
    input_counts(in, &nl, &nv);
    if (aug_total(in, sc, &n_aug)) return;
    const unsigned lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kWaveBlock / 64);
    for (size_t loop = (size_t)blockIdx.x * (kWaveBlock / 64) + (threadIdx.x >> 6); loop < nl; loop += waves) {
        if (sc.loop_n[loop] == 0u) continue;  // malformed
        unsigned off, cnt;
        loop_range(in, (unsigned)loop, nv, &off, &cnt);
        unsigned pos = sc.aug_off[loop], arc = sc.arc_off[loop];
        if (sc.loop_j[loop] == 0u && lane == 0 && arc < in.aug_rows) {  // a ring: one entry, at its first vertex
            sc.arc_pos[arc] = pos;
            sc.arc_loop[arc] = (unsigned)loop;
        }
        for (unsigned c = 0; c < cnt; c += 64u) {  // (cnt is the wave's: every lane takes every step)
            const unsigned i = c + lane;
            const bool active = i < cnt;
            unsigned a = 0;
            Edge e = {true, false, nullptr, 1u, 0u, true, 0u, 0u};
            if (active) {
                a = loop_vertex(in, off, cnt, i);
                e = edge_of(in, sc, a, loop_vertex(in, off, cnt, i + 1u));
            }
            const unsigned k = active && !e.bad ? inside_count(e) : 0u;
            const unsigned mine = active ? 1u + k : 0u, heads = active ? (e.head ? 1u : 0u) + k : 0u;
            const unsigned inc_n = wave_inclusive(mine, lane), inc_j = wave_inclusive(heads, lane);
            size_t p = (size_t)pos + inc_n - mine, q = (size_t)arc + inc_j - heads;
            if (active) {
                const auto put = [&](const unsigned id, const bool head) {
                    if (p < in.aug_rows) {
                        sc.aug[p] = id;
                        sc.jf[p] = head ? 1 : 0;
                    }
                    if (head) {
                        if (q < in.aug_rows) {
                            sc.arc_pos[q] = (unsigned)p;
                            sc.arc_loop[q] = (unsigned)loop;
                        }
                        q++;
                    }
                    p++;
                };
                put(a, e.head);
                if (k) {
                    if (e.forward) {
                        for (unsigned wi = e.lo >> 6; wi <= (e.hi >> 6); wi++)
                            for (uint64_t m = cut(e.line[wi], wi, e.lo, e.hi); m; m &= m - 1ull)
                                put(e.origin + (wi * 64u + (unsigned)__builtin_ctzll(m)) * e.step, true);
                    } else {
                        for (unsigned wi = e.hi >> 6; wi + 1u > (e.lo >> 6); wi--) {
                            for (uint64_t m = cut(e.line[wi], wi, e.lo, e.hi); m;) {
                                const unsigned b = 63u - (unsigned)__builtin_clzll(m);
                                put(e.origin + (wi * 64u + b) * e.step, true);
                                m &= ~(1ull << b);
                            }
                            if (wi == 0u) break;
                        }
                    }
                }
            }
            pos += __shfl(inc_n, 63, 64);
            arc += __shfl(inc_j, 63, 64);
        }
    }
}

// ---------------------------------------------------------------- one wave, one arc
struct Pt {
    int x, y;
};

// one arc or ring of a loop whose augmented vertices are aug[base, base + n): position t of the arc is vertex (s + t) mod n
struct Arc {
    const unsigned* aug;
    unsigned base, n, s, w1;
    __device__ __forceinline__ unsigned at(const unsigned t) const { return base + (t >= n - s ? t - (n - s) : s + t); }  // t <= n
    __device__ __forceinline__ unsigned id(const unsigned t) const { return aug[at(t)]; }
    __device__ __forceinline__ Pt pt(const unsigned v) const {
        const unsigned y = v / w1;
        return {(int)(v - y * w1), (int)y};
    }
};

// the wave-wide maximum of the key (d, -id, -t): the larger d, on a tie the smaller vertex id, then the earlier position
__device__ __forceinline__ void wave_argmax(uint64_t* d, unsigned* id, unsigned* t) {
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const uint64_t od = __shfl_xor((unsigned long long)*d, step, 64);
        const unsigned oi = __shfl_xor(*id, step, 64), ot = __shfl_xor(*t, step, 64);
        if (od > *d || (od == *d && (oi < *id || (oi == *id && ot < *t)))) {
            *d = od;
            *id = oi;
            *t = ot;
        }
    }
}

__device__ __forceinline__ void keep_arc(Arc arc, const bool ring, unsigned len, const unsigned lane, const uint64_t t2, uint8_t* __restrict__ keep) {
    uint64_t best;
    unsigned bid, at;
    unsigned stack_a = 0, stack_c = 0, sp = 0, a = 0, c = len;
    if (ring) {
        // anchor A: the smallest id (the key (0, -id, -t) of the same reduction)
        best = 0, bid = kIdle, at = kIdle;
        for (unsigned t = lane; t < arc.n; t += 64u) {
            const unsigned v = arc.id(t);
            if (v < bid) bid = v, at = t;
        }
        wave_argmax(&best, &bid, &at);
        arc.s = at;  // (s was 0: positions now count from A)
        // anchor B: the farthest from A
        const Pt pa = arc.pt(bid);
        best = 0, bid = kIdle, at = kIdle;
        for (unsigned t = 1u + lane; t < arc.n; t += 64u) {
            const unsigned v = arc.id(t);
            const Pt p = arc.pt(v);
            const int64_t dx = p.x - pa.x, dy = p.y - pa.y;
            const uint64_t d = (uint64_t)(dx * dx + dy * dy);
            if (at == kIdle || d > best || (d == best && v < bid)) best = d, bid = v, at = t;
        }
        wave_argmax(&best, &bid, &at);
        const unsigned B = at;  // (n >= 2: lane 0 had position 1)
        if (lane == 0) keep[arc.at(B)] = 1;
        stack_a = B, stack_c = arc.n, sp = 1;  // entry 0 = (B, n), in every lane: only lane 0's counts
        c = B;
    }
    if (lane == 0) keep[arc.at(0)] = 1;
    for (;;) {
        if (c - a < 2u) {
            if (sp == 0) break;
            sp--;
            a = __shfl(stack_a, (int)sp, 64);
            c = __shfl(stack_c, (int)sp, 64);
            continue;
        }
        const Pt pa = arc.pt(arc.id(a)), pc = arc.pt(arc.id(c));
        const int64_t ex = pc.x - pa.x, ey = pc.y - pa.y;
        uint64_t length = (uint64_t)(ex * ex + ey * ey);
        const bool closed = length == 0;  // the ends coincide: the distance from the point takes the chord's place
        if (closed) length = 1;
        best = 0, bid = kIdle, at = kIdle;
        for (unsigned t = a + 1u + lane; t < c; t += 64u) {
            const unsigned v = arc.id(t);
            const Pt p = arc.pt(v);
            const int64_t dx = p.x - pa.x, dy = p.y - pa.y;
            const int64_t cross = ex * dy - ey * dx;
            const uint64_t d = (uint64_t)(closed ? dx * dx + dy * dy : cross * cross);
            if (at == kIdle || d > best || (d == best && v < bid)) best = d, bid = v, at = t;
        }
        wave_argmax(&best, &bid, &at);
        const unsigned m = at;  // a < m < c
        if (256u * best > t2 * length && sp < 64u) {  // (sp < 64 cannot fail: the waiting segments at least double from the top down)
            if (lane == 0) keep[arc.at(m)] = 1;
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

__global__ void __launch_bounds__(kWaveBlock) coverage_arcs_kernel(CovIn in, CovScratch sc, unsigned tol16) {
    unsigned nl, nv, n_aug;
    input_counts(in, &nl, &nv);
    if (aug_total(in, sc, &n_aug)) return;
    const unsigned n_arcs = sc.arc_off[nl];  // at most n_aug <= aug_rows
    const unsigned lane = threadIdx.x & 63;
    const uint64_t t2 = (uint64_t)tol16 * tol16;
    const size_t waves = (size_t)gridDim.x * (kWaveBlock / 64);
    for (size_t k = (size_t)blockIdx.x * (kWaveBlock / 64) + (threadIdx.x >> 6); k < n_arcs && k < in.aug_rows; k += waves) {
        const unsigned pos = sc.arc_pos[k], loop = sc.arc_loop[k];
        if (loop >= nl) continue;
        const unsigned base = sc.aug_off[loop], n = sc.aug_off[loop + 1u] - base;
        const unsigned first = sc.arc_off[loop], arcs = sc.arc_off[loop + 1u] - first;
        if (pos < base || pos - base >= n || (uint64_t)base + n > n_aug || k < first || k - first >= arcs) continue;  // (the table is the emit launch's)
        const bool ring = sc.jf[pos] == 0;
        unsigned len = n;
        if (!ring) {
            const unsigned next = sc.arc_pos[k + 1u - first < arcs ? k + 1u : first];
            if (next < base || next - base >= n) continue;
            len = next > pos ? next - pos : n - (pos - next);
        }
        const Arc arc = {sc.aug, base, n, ring ? 0u : pos - base, in.w1};
        keep_arc(arc, ring, len, lane, t2, sc.keep);
    }
}

// ---------------------------------------------------------------- the flag scan over the keep flags, records, counts
__device__ __forceinline__ bool kept_at(const uint8_t* __restrict__ keep, const size_t p, const unsigned n) { return p < n && keep[p] != 0; }

// the augmented vertices there are to rank: none when they exceed the capacity
__device__ __forceinline__ unsigned aug_count(const CovIn& in, const CovScratch& sc) {
    unsigned n_aug;
    return aug_total(in, sc, &n_aug) ? 0u : n_aug;
}

__global__ void __launch_bounds__(kScanBlock) coverage_sums_kernel(CovIn in, CovScratch sc) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = aug_count(in, sc);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(kept_at(sc.keep, p, n), wsum);
    if (threadIdx.x == 0) sc.partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kScanBlock) coverage_partials_kernel(unsigned* __restrict__ partial, size_t NB) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = scan_block_sums(partial, NB, wsum);
    if (threadIdx.x == 0) partial[NB] = n;
}

__global__ void __launch_bounds__(kScanBlock) coverage_rank_kernel(CovIn in, CovScratch sc, unsigned* __restrict__ vertices_out, unsigned vertex_rows_out) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned n = aug_count(in, sc);
    const size_t p = (size_t)blockIdx.x * kScanBlock + threadIdx.x;  // p <= aug_rows has a word of rank[]
    const bool flag = kept_at(sc.keep, p, n);
    const unsigned r = flag_rank(flag, sc.partial[blockIdx.x], wsum);
    if (p <= n) sc.rank[p] = r;
    if (flag && vertices_out && r < vertex_rows_out) vertices_out[r] = sc.aug[p];
}

__global__ void __launch_bounds__(kScanBlock) coverage_records_kernel(CovIn in, CovScratch sc, unsigned* __restrict__ loops_out, unsigned loops_rows_out) {
    __shared__ unsigned wsum[kScanBlock / 64], bsum[kScanBlock / 64];
    unsigned nl, nv, n_aug;
    input_counts(in, &nl, &nv);
    if (aug_total(in, sc, &n_aug)) nl = 0;
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    bool thin = false, bad = false;
    if (i < nl) {
        bad = sc.loop_bad[i] != 0;
        const unsigned from = sc.aug_off[i], to = sc.aug_off[i + 1];  // from <= to <= n_aug
        const unsigned first = sc.rank[from < n_aug ? from : n_aug];
        const unsigned kept = sc.rank[to < n_aug ? to : n_aug] - first;
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
        sc.thin[blockIdx.x] = t;
        sc.bad[blockIdx.x] = b;
    }
}

// one workgroup: counts_out = {n_loops, n_vertices', n_degenerate, status, n_aug, n_arcs}.  NL: the block sums of the records launch
__global__ void __launch_bounds__(kScanBlock) coverage_counts_kernel(CovIn in, CovScratch sc, size_t NB, size_t NL, unsigned* __restrict__ counts_out) {
    __shared__ unsigned tsum[kScanBlock / 64], bsum[kScanBlock / 64];
    unsigned t = 0, b = 0;
    for (size_t k = threadIdx.x; k < NL; k += kScanBlock) {
        t += sc.thin[k];
        b += sc.bad[k];
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
    unsigned nl, nv, n_aug;
    const bool truncated = input_counts(in, &nl, &nv);
    const bool overflow = aug_total(in, sc, &n_aug);
    counts_out[0] = in.counts[0];
    counts_out[1] = sc.partial[NB];
    counts_out[2] = t;
    counts_out[3] = truncated ? 1u : overflow ? 4u : b ? 2u : 0u;
    counts_out[4] = n_aug;
    counts_out[5] = overflow ? 0u : sat32(sc.part_a[sc.NBL]);
}

unsigned wave_grid(const size_t items) {
    const size_t blocks = (items + 3) / 4;
    return (unsigned)(blocks < kWaveGrid ? blocks : kWaveGrid);
}

}  // namespace

size_t coverage_scratch_bytes(size_t H, size_t W, size_t loops_rows, size_t aug_rows) { return Layout(H, W, loops_rows, aug_rows).bytes; }

hipError_t launch_coverage(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, const unsigned* loops,
                           unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts, unsigned tol16,
                           unsigned aug_rows, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out,
                           unsigned vertex_rows_out, unsigned* counts_out, hipStream_t s) {
    const Layout at(H, W, loops_rows_in, aug_rows);
    uint8_t* base = (uint8_t*)scratch;
    CovIn in;
    in.plane = plane, in.loops = loops, in.vertices = vertices, in.counts = counts;
    in.elem_bytes = (unsigned)elem_bytes, in.H = H, in.W = W, in.skip = skip ? 1u : 0u, in.skip_value = skip_value;
    in.loops_rows = loops_rows_in, in.vertex_rows = vertex_rows_in, in.aug_rows = aug_rows;
    in.w1 = W + 1u, in.h1 = H + 1u, in.wordsX = (W + 64u) / 64u, in.wordsY = (H + 64u) / 64u;
    CovScratch sc;
    sc.jrow = (uint64_t*)(base + at.jrow), sc.jcol = (uint64_t*)(base + at.jcol);
    sc.part_n = (uint64_t*)(base + at.part_n), sc.part_a = (uint64_t*)(base + at.part_a);
    sc.loop_n = (unsigned*)(base + at.loop_n), sc.loop_j = (unsigned*)(base + at.loop_j), sc.loop_bad = base + at.loop_bad;
    sc.aug_off = (unsigned*)(base + at.aug_off), sc.arc_off = (unsigned*)(base + at.arc_off);
    sc.aug = (unsigned*)(base + at.aug), sc.jf = base + at.jf;
    sc.arc_pos = (unsigned*)(base + at.arc_pos), sc.arc_loop = (unsigned*)(base + at.arc_loop);
    sc.keep = base + at.keep, sc.rank = (unsigned*)(base + at.rank), sc.partial = (unsigned*)(base + at.partial);
    sc.thin = (unsigned*)(base + at.thin), sc.bad = (unsigned*)(base + at.bad);
    const size_t NBL = scan_blocks((size_t)loops_rows_in + 1), NB = scan_blocks((size_t)aug_rows + 1), NL = scan_blocks(loops_rows_in);
    sc.NBL = (unsigned)NBL;
    hipError_t e = hipMemsetAsync(sc.keep, 0, (size_t)aug_rows + 1, s);
    if (e != hipSuccess) return e;
    const size_t row_waves = (size_t)in.h1 * in.wordsX, col_waves = (size_t)in.w1 * in.wordsY;
    hipLaunchKernelGGL(coverage_junction_kernel<false>, dim3((unsigned)((row_waves + 3) / 4)), dim3(kWaveBlock), 0, s, in, sc.jrow);
    hipLaunchKernelGGL(coverage_junction_kernel<true>, dim3((unsigned)((col_waves + 3) / 4)), dim3(kWaveBlock), 0, s, in, sc.jcol);
    if (loops_rows_in) hipLaunchKernelGGL(coverage_measure_kernel, dim3(wave_grid(loops_rows_in)), dim3(kWaveBlock), 0, s, in, sc);
    hipLaunchKernelGGL(coverage_loop_sums_kernel, dim3((unsigned)NBL), dim3(kScanBlock), 0, s, in, sc);
    hipLaunchKernelGGL(coverage_loop_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, sc);
    hipLaunchKernelGGL(coverage_loop_offsets_kernel, dim3((unsigned)NBL), dim3(kScanBlock), 0, s, in, sc);
    if (loops_rows_in && aug_rows) {
        hipLaunchKernelGGL(coverage_emit_kernel, dim3(wave_grid(loops_rows_in)), dim3(kWaveBlock), 0, s, in, sc);
        hipLaunchKernelGGL(coverage_arcs_kernel, dim3(wave_grid(aug_rows)), dim3(kWaveBlock), 0, s, in, sc, tol16);
    }
    hipLaunchKernelGGL(coverage_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, sc);
    hipLaunchKernelGGL(coverage_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, sc.partial, NB);
    hipLaunchKernelGGL(coverage_rank_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, in, sc, vertices_out, vertex_rows_out);
    if (loops_rows_in) hipLaunchKernelGGL(coverage_records_kernel, dim3((unsigned)NL), dim3(kScanBlock), 0, s, in, sc, loops_out, loops_rows_out);
    if (counts_out) hipLaunchKernelGGL(coverage_counts_kernel, dim3(1), dim3(kScanBlock), 0, s, in, sc, NB, NL, counts_out);
    return hipGetLastError();
}

}  // namespace infur
