// skeleton.hip -- Skeleton (include/infur_hip.h): every value of a plane thinned to one-pixel centrelines by Guo and Hall's
// two-sub-iteration rule, and the measures of what is kept.  The state is a bitmap, and a bitmap word is one row of a tile's CORE:
// kSkCoreW = 48 columns in the low bits of a 64-bit word, word (tx, y) at tx * H + y.  A workgroup that thins loads an EXTENDED
// block -- its core and a halo of kSkK = 8 pixels on every side, 64 columns by kSkRows = 128 rows, one word and one lane per row --
// builds each extended word from the core words of three tiles, and writes back only words that are its own: no two workgroups
// ever write one word, so the ping-pong between the two alive bitmaps needs no atomics.
//   1 prepare    a wave per core row: one ballot each for "alive" (inside the frame and not skipped) and for "holds the same value
//                as its E / S / SE / SW neighbour, both alive".  The relation is symmetric, so the four planes give all eight
//                directions by shifts, nothing outside the frame is ever related to anything, and the value plane is not read again
//                before the measures.  Clears the accumulators and tile flags and lays the empty rows into the table.
//   2 thin       ceil(max_rounds / 8) launches, a workgroup per tile, 8 sub-iterations each between two LDS row buffers with one
//                barrier per sub-iteration.  A lane evaluates C, N and m as a boolean network on whole words, 64 pixels at once.
//                After j sub-iterations the outer j rings of the extended block are stale; the core lies 8 inside and is exact.
//                A tile whose 3 x 3 tiles removed nothing in the launch before copies its core words and leaves; a launch behind one
//                that removed nothing anywhere exits on the ROUNDS word at its first instruction (both bitmaps agree from then on).
//   3 measures   a wave per core row over the final bitmap: kind_out, the totals, and the per-value rows with one atomic per run of
//                equal values along the wave
//   4 counts     the eight counts, and MIN_H of the rows no kept pixel touched
// Determinism: what leaves is a function of the bitmaps, which are exact, and sums, minima and maxima of integers, which commute.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

typedef unsigned long long u64;

constexpr int kSkBlock = 256;  // prepare, measures, counts: four wave-rows
constexpr int kSkK = 8;        // the halo, and the sub-iterations of a thin launch: even, so every launch starts on an odd one
constexpr int kSkCoreW = 48, kSkRows = 128, kSkCoreH = kSkRows - 2 * kSkK;
constexpr u64 kSkCoreBits = (1ull << kSkCoreW) - 1ull, kSkCoreMask = kSkCoreBits << kSkK;
constexpr unsigned kSkNone = 0xFFFFFFFFu;
constexpr u64 kSkDead = ~0ull;
static_assert(kSkK % 2 == 0 && kSkCoreW + 2 * kSkK == 64 && kSkK <= kSkCoreW && kSkK <= kSkCoreH && kSkK == kSkeletonK, "the tile");

// the accumulators at the head of the scratch
enum { kSkRounds = 0, kSkRemoved, kSkKept, kSkEnds, kSkJunctions, kSkOrtho, kSkDiag, kSkAccWords = 8 };

struct SkelIn {
    const void* plane;
    const unsigned* height;  // or null
    unsigned H, W, tilesX, tilesY;
    unsigned skip, skip_value;
    unsigned max_rounds;  // the effective one
};

struct SkelMem {
    unsigned* acc;      // kSkAccWords
    unsigned* flag[2];  // per tile: the last launch of that parity in which the tile removed a core pixel
    u64* alive[2];      // tilesX * H words each
    u64 *relE, *relS, *relSE, *relSW;
    size_t clear_words, bytes;  // [acc, flag[1]] is cleared by prepare
};

__host__ SkelMem skel_layout(void* scratch, unsigned H, unsigned W) {
    const size_t tilesX = (W + kSkCoreW - 1) / kSkCoreW, tilesY = (H + kSkCoreH - 1) / kSkCoreH, words = tilesX * H, tiles = tilesX * tilesY;
    uint8_t* p = (uint8_t*)scratch;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        uint8_t* q = p + at;
        at += (bytes + 255) & ~(size_t)255;
        return q;
    };
    SkelMem m{};
    m.acc = (unsigned*)take(kSkAccWords * 4 + 2 * tiles * 4);
    m.flag[0] = m.acc + kSkAccWords;
    m.flag[1] = m.flag[0] + tiles;
    m.clear_words = kSkAccWords + 2 * tiles;
    m.alive[0] = (u64*)take(words * 8);
    m.alive[1] = (u64*)take(words * 8);
    m.relE = (u64*)take(words * 8);
    m.relS = (u64*)take(words * 8);
    m.relSE = (u64*)take(words * 8);
    m.relSW = (u64*)take(words * 8);
    m.bytes = at;
    return m;
}

// the value of pixel (x, y) as a key, kSkDead when it lies outside the frame or is skipped
template <class T>
__device__ __forceinline__ u64 sk_key(const SkelIn& in, long x, unsigned y) {
    if (x < 0 || x >= (long)in.W || y >= in.H) return kSkDead;
    const unsigned v = (unsigned)((const T*)in.plane)[(size_t)y * in.W + (size_t)x];
    return (in.skip && v == in.skip_value) ? kSkDead : (u64)v;
}

// four wave-rows per workgroup, a wave-row is one core row of a tile
struct CoreRow {
    unsigned y, tx;
    int lane;
    bool row;  // the row exists
};
__device__ __forceinline__ CoreRow core_row(unsigned H, unsigned tilesX) {
    const size_t u = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    CoreRow r;
    r.y = (unsigned)(u / tilesX);
    r.tx = (unsigned)(u % tilesX);
    r.lane = threadIdx.x & 63;
    r.row = r.y < H;
    return r;
}

template <class T>
__global__ void __launch_bounds__(kSkBlock) skel_prepare_kernel(SkelIn in, SkelMem m, unsigned* __restrict__ table, unsigned rows) {
    const size_t gid = (size_t)blockIdx.x * kSkBlock + threadIdx.x, stride = (size_t)gridDim.x * kSkBlock;
    for (size_t i = gid; i < m.clear_words; i += stride) m.acc[i] = 0u;
    if (table)  // the row of a value no kept pixel holds; MIN_H starts at the top and is put right by the counts launch
        for (size_t i = gid; i < (size_t)rows * kSkeletonWords; i += stride) table[i] = (i & 7) == 5 || (i & 7) == 6 ? kSkNone : 0u;
    const CoreRow r = core_row(in.H, in.tilesX);
    if (!r.row) return;
    // lane l looks at column tx * 48 + l - 1: the core's 48 columns are lanes 1 .. 48, lanes 0 and 49 their neighbours
    const long x = (long)r.tx * kSkCoreW + r.lane - 1;
    const bool mine = r.lane >= 1 && r.lane <= kSkCoreW;
    const u64 k0 = r.lane <= kSkCoreW + 1 ? sk_key<T>(in, x, r.y) : kSkDead, k1 = r.lane <= kSkCoreW + 1 ? sk_key<T>(in, x, r.y + 1u) : kSkDead;
    const u64 e0 = __shfl_down(k0, 1, 64), e1 = __shfl_down(k1, 1, 64), w1 = __shfl_up(k1, 1, 64);
    const bool own = mine && k0 != kSkDead;
    const u64 alive = __ballot(own) >> 1, E = __ballot(own && k0 == e0) >> 1, S = __ballot(own && k0 == k1) >> 1, SE = __ballot(own && k0 == e1) >> 1,
              SW = __ballot(own && k0 == w1) >> 1;
    if (r.lane == 0) {
        const size_t at = (size_t)r.tx * in.H + r.y;
        m.alive[0][at] = alive;
        m.relE[at] = E;
        m.relS[at] = S;
        m.relSE[at] = SE;
        m.relSW[at] = SW;
    }
}

// the extended word of row y of tile tx: the last 8 columns of the tile to the left, the tile's 48, the first 8 of the tile to the
// right; nothing where there is no row or no tile
__device__ __forceinline__ u64 sk_ext(const u64* __restrict__ plane, unsigned H, unsigned tilesX, unsigned tx, long y) {
    if (y < 0 || y >= (long)H) return 0ull;
    const u64 own = plane[(size_t)tx * H + (size_t)y];
    const u64 lf = tx > 0 ? plane[(size_t)(tx - 1) * H + (size_t)y] : 0ull;
    const u64 rt = tx + 1 < tilesX ? plane[(size_t)(tx + 1) * H + (size_t)y] : 0ull;
    return (lf >> (kSkCoreW - kSkK)) | (own << kSkK) | (rt << (kSkCoreW + kSkK));
}

// The eight neighbours of every pixel of a row at once, "set for p": alive and of p's value.  U, M, D: the alive words of the row
// above, the row itself and the row below; the masks say which neighbour holds the pixel's own value.
struct SkMasks {
    u64 n, ne, e, se, s, sw, w, nw;
};
__device__ __forceinline__ SkMasks sk_masks(u64 eRow, u64 sRow, u64 seRow, u64 swRow, u64 sUp, u64 seUp, u64 swUp) {
    return SkMasks{sUp, swUp >> 1, eRow, seRow, sRow, swRow, eRow << 1, seUp << 1};
}
struct SkNbrs {
    u64 p2, p3, p4, p5, p6, p7, p8, p9;
};
__device__ __forceinline__ SkNbrs sk_nbrs(const SkMasks& k, u64 U, u64 M, u64 D) {
    return SkNbrs{U & k.n, (U >> 1) & k.ne, (M >> 1) & k.e, (D >> 1) & k.se, D & k.s, (D << 1) & k.sw, (M << 1) & k.w, (U << 1) & k.nw};
}

__device__ __forceinline__ u64 sk_ge2(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// the pixels of M that die in a sub-iteration: C == 1, 2 <= min(N1, N2) <= 3 and !m
__device__ __forceinline__ u64 sk_dies(const SkNbrs& p, u64 M, bool odd) {
    const u64 a = p.p9 | p.p2, b = p.p3 | p.p4, c = p.p5 | p.p6, d = p.p7 | p.p8;  // N1's terms
    const u64 e = p.p2 | p.p3, f = p.p4 | p.p5, g = p.p6 | p.p7, h = p.p8 | p.p9;  // N2's terms
    const u64 t1 = ~p.p2 & b, t2 = ~p.p4 & c, t3 = ~p.p6 & d, t4 = ~p.p8 & a;      // C's terms
    const u64 c1 = (t1 | t2 | t3 | t4) & ~sk_ge2(t1, t2, t3, t4);
    // min(N1, N2) in [2, 3]: both at least 2 and not both 4
    const u64 n23 = sk_ge2(a, b, c, d) & sk_ge2(e, f, g, h) & ~(a & b & c & d & e & f & g & h);
    const u64 mm = odd ? (p.p6 | p.p7 | ~p.p9) & p.p8 : (p.p2 | p.p3 | ~p.p5) & p.p4;
    return M & c1 & n23 & ~mm;
}

// Launch L (1-based) runs sub-iterations 8 (L - 1) + 1 .. 8 (L - 1) + steps from src to dst.
__global__ void __launch_bounds__(kSkRows) skel_thin_kernel(SkelIn in, SkelMem m, const u64* __restrict__ src, u64* __restrict__ dst, unsigned L,
                                                            unsigned steps) {
    // nothing was removed in launch L - 1: nothing will be, and both bitmaps hold the final state.  (A workgroup of this launch can
    // only raise the word, so every workgroup decides alike.)
    if (L > 1 && __hip_atomic_load(m.acc + kSkRounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)kSkK * (L - 2)) return;
    __shared__ u64 rowbuf[2][kSkRows + 2];                                         // [.][r + 1]; [.][0] and [.][kSkRows + 1] stay 0
    __shared__ u64 upS[kSkRows + 1], upSE[kSkRows + 1], upSW[kSkRows + 1];  // [r + 1]: the relation rows, read by the row below
    __shared__ unsigned removed[2];                                                // the last step that removed a core pixel; how many
    const unsigned tx = blockIdx.x, ty = blockIdx.y, r = threadIdx.x;
    const long y = (long)ty * kSkCoreH - kSkK + (long)r;
    const bool core = r >= (unsigned)kSkK && r < (unsigned)(kSkRows - kSkK) && y < (long)in.H;
    const size_t at = (size_t)tx * in.H + (size_t)(core ? y : 0);
    // the dependence cone of the core over 8 sub-iterations lies inside the 3 x 3 tiles around it
    bool active = L == 1;
    if (!active) {
        const unsigned* prev = m.flag[(L - 1) & 1];
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const long ny = (long)ty + dy, nx = (long)tx + dx;
                if (ny >= 0 && ny < (long)in.tilesY && nx >= 0 && nx < (long)in.tilesX && prev[(size_t)ny * in.tilesX + (size_t)nx] == L - 1) active = true;
            }
    }
    if (!active) {  // the other bitmap must still hold the core
        if (core) dst[at] = src[at];
        return;
    }
    u64 M = sk_ext(src, in.H, in.tilesX, tx, y);
    const u64 eRow = sk_ext(m.relE, in.H, in.tilesX, tx, y), sRow = sk_ext(m.relS, in.H, in.tilesX, tx, y);
    const u64 seRow = sk_ext(m.relSE, in.H, in.tilesX, tx, y), swRow = sk_ext(m.relSW, in.H, in.tilesX, tx, y);
    upS[r + 1] = sRow;
    upSE[r + 1] = seRow;
    upSW[r + 1] = swRow;
    rowbuf[0][r + 1] = M;
    if (r == 0) {
        upS[0] = upSE[0] = upSW[0] = 0ull;
        rowbuf[0][0] = rowbuf[1][0] = rowbuf[0][kSkRows + 1] = rowbuf[1][kSkRows + 1] = 0ull;
        removed[0] = removed[1] = 0u;
    }
    __syncthreads();
    const SkMasks k = sk_masks(eRow, sRow, seRow, swRow, upS[r], upSE[r], upSW[r]);
    unsigned last = 0, gone = 0;
    for (unsigned j = 1; j <= steps; j++) {
        const unsigned cur = (j - 1) & 1;
        const u64 die = sk_dies(sk_nbrs(k, rowbuf[cur][r], M, rowbuf[cur][r + 2]), M, (j & 1) != 0);
        M &= ~die;
        rowbuf[cur ^ 1][r + 1] = M;
        if (core && (die & kSkCoreMask)) last = j, gone += (unsigned)__popcll(die & kSkCoreMask);
        __syncthreads();
    }
    if (core) dst[at] = (M >> kSkK) & kSkCoreBits;
    if (last) {
        atomicMax(&removed[0], last);
        atomicAdd(&removed[1], gone);
    }
    __syncthreads();
    if (r == 0 && removed[0]) {
        (void)__hip_atomic_fetch_max(m.acc + kSkRounds, (unsigned)kSkK * (L - 1) + removed[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(m.acc + kSkRemoved, removed[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        m.flag[L & 1][(size_t)ty * in.tilesX + tx] = L;
    }
}

template <class T>
__global__ void __launch_bounds__(kSkBlock) skel_measure_kernel(SkelIn in, SkelMem m, const u64* __restrict__ fin, uint8_t* __restrict__ kind,
                                                                unsigned* __restrict__ table, unsigned rows) {
    __shared__ unsigned lacc[5];
    if (threadIdx.x < 5) lacc[threadIdx.x] = 0u;
    __syncthreads();
    const CoreRow r = core_row(in.H, in.tilesX);
    const unsigned x = r.tx * kSkCoreW + (unsigned)r.lane;
    const bool live = r.row && r.lane < kSkCoreW && x < in.W;
    const size_t at = (size_t)r.y * in.W + x;
    const u64 M = r.row ? sk_ext(fin, in.H, in.tilesX, r.tx, (long)r.y) : 0ull;
    if (M & kSkCoreMask) {  // (uniform over the wave)
        const long y = (long)r.y;
        const SkMasks k = sk_masks(sk_ext(m.relE, in.H, in.tilesX, r.tx, y), sk_ext(m.relS, in.H, in.tilesX, r.tx, y), sk_ext(m.relSE, in.H, in.tilesX, r.tx, y),
                                   sk_ext(m.relSW, in.H, in.tilesX, r.tx, y), sk_ext(m.relS, in.H, in.tilesX, r.tx, y - 1),
                                   sk_ext(m.relSE, in.H, in.tilesX, r.tx, y - 1), sk_ext(m.relSW, in.H, in.tilesX, r.tx, y - 1));
        const SkNbrs p = sk_nbrs(k, sk_ext(fin, in.H, in.tilesX, r.tx, y - 1), M, sk_ext(fin, in.H, in.tilesX, r.tx, y + 1));
        const int bit = r.lane + kSkK;
        const bool kept = live && ((M >> bit) & 1ull);
        const unsigned n = (unsigned)(((p.p2 >> bit) & 1ull) + ((p.p3 >> bit) & 1ull) + ((p.p4 >> bit) & 1ull) + ((p.p5 >> bit) & 1ull) + ((p.p6 >> bit) & 1ull) +
                                      ((p.p7 >> bit) & 1ull) + ((p.p8 >> bit) & 1ull) + ((p.p9 >> bit) & 1ull));
        if (live && kind) kind[at] = kept ? (uint8_t)(1u + n) : (uint8_t)0;
        // as words whose bit l is lane l: the kept pixels, ends and junctions, and the links counted at their pixel of smaller index
        const u64 wK = (M >> kSkK) & kSkCoreBits, wE = __ballot(kept && n == 1u), wJ = __ballot(kept && n >= 3u);
        const u64 wO1 = ((M & p.p4) >> kSkK) & kSkCoreBits, wO2 = ((M & p.p6) >> kSkK) & kSkCoreBits;
        const u64 wD1 = ((M & p.p5 & ~p.p4 & ~p.p6) >> kSkK) & kSkCoreBits, wD2 = ((M & p.p7 & ~p.p8 & ~p.p6) >> kSkK) & kSkCoreBits;
        if (r.lane == 0) {
            atomicAdd(&lacc[0], (unsigned)__popcll(wK));
            if (wE) atomicAdd(&lacc[1], (unsigned)__popcll(wE));
            if (wJ) atomicAdd(&lacc[2], (unsigned)__popcll(wJ));
            if (wO1 | wO2) atomicAdd(&lacc[3], (unsigned)(__popcll(wO1) + __popcll(wO2)));
            if (wD1 | wD2) atomicAdd(&lacc[4], (unsigned)(__popcll(wD1) + __popcll(wD2)));
        }
        if (table && rows) {
            const u64 key = kept ? (u64)((const T*)in.plane)[at] : kSkDead;
            bool cont;
            const u64 starts = wave_run_starts(key, kept, &cont);
            unsigned lo = 0, hi = 0;
            if (in.height) {  // the segmented minimum and maximum of the run, as Split's saddles
                lo = hi = kept ? in.height[at] : 0u;
                const unsigned head = run_start(starts, r.lane), end = head + run_length(starts, (int)head) - 1u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned tl = __shfl_down(lo, d, 64), th = __shfl_down(hi, d, 64);
                    if ((unsigned)r.lane + d <= end) lo = min(lo, tl), hi = max(hi, th);
                }
            }
            if (kept && !cont && key < (u64)rows) {
                const unsigned len = run_length(starts, r.lane);
                const u64 run = (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << r.lane;
                unsigned* row = table + (size_t)key * kSkeletonWords;
                const unsigned ne = (unsigned)__popcll(wE & run), nj = (unsigned)__popcll(wJ & run);
                const unsigned no = (unsigned)(__popcll(wO1 & run) + __popcll(wO2 & run)), nd = (unsigned)(__popcll(wD1 & run) + __popcll(wD2 & run));
                atomicAdd(row + 0, len);
                if (ne) atomicAdd(row + 1, ne);
                if (nj) atomicAdd(row + 2, nj);
                if (no) atomicAdd(row + 3, no);
                if (nd) atomicAdd(row + 4, nd);
                atomicMin(row + 5, (unsigned)at);
                if (in.height) {
                    atomicMin(row + 6, lo);
                    atomicMax(row + 7, hi);
                }
            }
        }
    } else if (live && kind) {
        kind[at] = 0;
    }
    __syncthreads();
    if (threadIdx.x < 5 && lacc[threadIdx.x]) atomicAdd(m.acc + kSkKept + threadIdx.x, lacc[threadIdx.x]);
}

__global__ void __launch_bounds__(kSkBlock) skel_counts_kernel(SkelIn in, SkelMem m, unsigned* __restrict__ table, unsigned rows,
                                                               unsigned* __restrict__ counts) {
    const size_t gid = (size_t)blockIdx.x * kSkBlock + threadIdx.x, stride = (size_t)gridDim.x * kSkBlock;
    if (table)
        for (size_t v = gid; v < rows; v += stride)
            if (!in.height || !table[v * kSkeletonWords]) table[v * kSkeletonWords + 6] = 0u;
    if (counts && gid == 0) {
        const unsigned rounds = m.acc[kSkRounds];
        counts[0] = m.acc[kSkKept];
        counts[1] = m.acc[kSkRemoved];
        counts[2] = rounds;
        counts[3] = m.acc[kSkEnds];
        counts[4] = m.acc[kSkJunctions];
        counts[5] = m.acc[kSkOrtho];
        counts[6] = m.acc[kSkDiag];
        counts[7] = in.max_rounds < rounds + 2u ? kSkeletonUnfinished : 0u;
    }
}

__global__ void __launch_bounds__(kSkBlock) skel_empty_kernel(unsigned* __restrict__ table, unsigned rows, unsigned* __restrict__ counts) {
    const size_t gid = (size_t)blockIdx.x * kSkBlock + threadIdx.x, stride = (size_t)gridDim.x * kSkBlock;
    if (table)
        for (size_t i = gid; i < (size_t)rows * kSkeletonWords; i += stride) table[i] = (i & 7) == 5 ? kSkNone : 0u;
    if (counts && gid < (size_t)kSkeletonCountWords) counts[gid] = 0u;
}

unsigned row_blocks(size_t words, unsigned cap = 65536) {
    const size_t b = (words + kSkBlock - 1) / kSkBlock;
    return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

template <class T>
hipError_t launch_skeleton_t(const SkelIn& in, const SkelMem& m, uint8_t* kind, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    const size_t waveRows = (size_t)in.H * in.tilesX, rowBlocks = (waveRows + 3) / 4;
    if (rowBlocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((skel_prepare_kernel<T>), dim3((unsigned)rowBlocks), dim3(kSkBlock), 0, s, in, m, table, rows);
    const unsigned launches = skeleton_thin_launches(in.max_rounds);
    for (unsigned L = 1; L <= launches; L++) {
        const unsigned steps = L < launches ? (unsigned)kSkK : in.max_rounds - (unsigned)kSkK * (launches - 1);
        hipLaunchKernelGGL(skel_thin_kernel, dim3(in.tilesX, in.tilesY), dim3(kSkRows), 0, s, in, m, (const u64*)m.alive[(L - 1) & 1], m.alive[L & 1], L, steps);
    }
    hipLaunchKernelGGL((skel_measure_kernel<T>), dim3((unsigned)rowBlocks), dim3(kSkBlock), 0, s, in, m, (const u64*)m.alive[launches & 1], kind, table, rows);
    hipLaunchKernelGGL(skel_counts_kernel, dim3(table ? row_blocks(rows, 4096) : 1u), dim3(kSkBlock), 0, s, in, m, table, rows, counts);
    return hipGetLastError();
}

}  // namespace

unsigned skeleton_thin_launches(unsigned max_rounds) { return (max_rounds + (unsigned)kSkK - 1u) / (unsigned)kSkK; }

size_t skeleton_scratch_bytes(unsigned H, unsigned W) { return skel_layout(nullptr, H, W).bytes; }

hipError_t launch_skeleton(const void* plane, int elem_bytes, const unsigned* height, unsigned H, unsigned W, int skip, unsigned skip_value,
                           unsigned max_rounds, void* scratch, uint8_t* kind, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    if (!rows) table = nullptr;
    if ((size_t)H * W == 0) {  // no pixel: the empty rows and zero counts, and no scratch
        if (table || counts) hipLaunchKernelGGL(skel_empty_kernel, dim3(row_blocks((size_t)rows * kSkeletonWords)), dim3(kSkBlock), 0, s, table, rows, counts);
        return hipGetLastError();
    }
    if (H > 65535u || W > 65535u || max_rounds == 0 || max_rounds > kSkeletonMaxRounds) return hipErrorInvalidValue;
    const SkelMem m = skel_layout(scratch, H, W);
    const SkelIn in{plane, height, H, W, (W + kSkCoreW - 1) / kSkCoreW, (H + kSkCoreH - 1) / kSkCoreH, skip ? 1u : 0u, skip_value, max_rounds};
    return elem_bytes == 1   ? launch_skeleton_t<uint8_t>(in, m, kind, table, rows, counts, s)
           : elem_bytes == 4 ? launch_skeleton_t<uint32_t>(in, m, kind, table, rows, counts, s)
                             : hipErrorInvalidValue;
}

}  // namespace infur
