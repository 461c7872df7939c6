// split.hip -- Split (include/infur_hip.h): touching objects of one value separated at their necks, a marker watershed of
// a u32 height plane (typically Anchors' dist2) as a maximum spanning forest rooted in the basins whose peak reaches `core`.
// Pixels are ordered by K = (height << 32) | (0xFFFFFFFF - index).  The kernel boundaries are the only ordering, no workgroup ever
// waits for another, and nothing is read back inside the call:
//   1 clear      the accumulators, flags and per-root words to 0, the table's keys and first edge ids to all ones
//   2 ascent     one lane per pixel, a wave is 64 columns of a row: up[i] = the largest same-valued 4-neighbour when it is larger
//                than the pixel, else i (a peak); a skipped pixel kSpNone
//   3 doubling   ceil(log2(h w)) launches, up <- up[up] between two buffers; a launch behind one that changed nothing exits on a
//                device flag (both buffers are then equal, so the buffer the last launch would have written is valid either way)
//   4 count      RUNS (a run head needs the pair one column to the left, or one row up, to differ) and BASINS; parent[i] = i
//   5 insert     unless 2 RUNS > slots: edges towards y+1 as runs along the wave-row (one ballot of "the (basin above, basin below)
//                key differs from the left lane's"; the head lane does the 64-bit CAS, one atomicMax of the run's largest
//                min-height -- a segmented wave maximum -- and one atomicMin of its first edge id); edges towards x+1 one per edge
//   6 phase 1    one lane per slot: SADDLE >= core unites its two basins by atomicMin hooking (regions.hip's seam union); PAIRS
//   7 roots      every peak finds its root; a peak of height >= core marks its root; MARKED
//   8 rounds     ceil(log2(min(h w, slots))) + 1 times (choose over the slots, hook and flatten over the pixels): Boruvka's steps
//                with the marked components as the forest's roots.  Rounds behind one that hooked nothing exit on a device flag
//   9 measure    per final root: first pixel, PIXELS, highest peak; per slot: NECK
//  10 number     the flag scan of wave_scan.h over "this pixel is its segment's first", the table rows, the label plane, the counts;
//                the first launch of the scan also counts the segments per VALUE in a second open-addressing table (one CAS and
//                one add per segment): the add that finds 1 has found a value with more than one segment, SPLIT_VALUES
// Determinism: the slot a pair lands in and every interim root stay inside the scratch; what leaves is the partition (unique, because
// the order on pairs is strict), numbered by first pixels, and sums, minima and maxima of integers, which commute.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kSpBlock = 256;
constexpr unsigned kSpNone = 0xFFFFFFFFu;
constexpr unsigned long long kSpDead = ~0ull;
constexpr int kSpMaxRounds = 34;  // of either loop: h w < 2^31

// the accumulators at the head of the scratch
enum { kSpRuns = 0, kSpBasins, kSpPairs, kSpMarked, kSpSplitValues, kSpSegments, kSpAccWords = 8 };

struct SplitIn {
    const void* plane;
    const unsigned* height;
    unsigned H, W, tilesX;
    unsigned skip, skip_value;
    unsigned core;
    size_t npix;
};

// The scratch of a call.  [acc, best) .. pk is cleared to 0 and [first, keys] to all ones by the clear launch; the rest is written
// before it is read.
struct SplitMem {
    unsigned* acc;             // kSpAccWords
    unsigned *dflag, *rflag;   // [t]: doubling launch t changed a pointer; round t hooked something ([0]: go).  kSpMaxRounds + 2 each
    unsigned* mark;            // per root: the component holds a peak of height >= core
    unsigned* pix;             // per final root: PIXELS
    unsigned* neck;            // per final root: NECK
    unsigned* saddle;          // per slot: SADDLE
    unsigned long long* best;  // per root: the round's (SADDLE << 32) | (0xFFFFFFFF - FIRST); 0 between rounds
    unsigned long long* pk;    // per final root: (HEIGHT << 32) | (0xFFFFFFFF - PEAK) of its highest peak
    unsigned long long* vkeys;  // per value slot: VALUE + 1, 0 while the slot is free
    unsigned* vcnt;             // per value slot: the segments of that value
    unsigned* first;           // per slot: FIRST
    unsigned* firstpix;        // per final root: its first pixel
    unsigned long long* keys;  // per slot: (A << 32) | B, A < B
    unsigned *up0, *up1;       // the ascent pointers; after the doubling one of them is the basin plane, the other is free
    unsigned* parent;          // per peak: union-find over basins; flattened (parent = root) between launches from `roots` on
    unsigned* partial;         // the block sums of the flag scan
    unsigned slots, vslots;
    size_t zero_words, ones_words, bytes;
};

struct Taker {
    uint8_t* p;
    size_t at = 0;
    uint8_t* take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return p + o;
    }
};

// the slots of the value table: twice the values there can be (a byte holds 256, a segment needs a pixel), a power of two
__host__ unsigned split_value_slots(size_t npix, int elem_bytes) {
    const size_t most = (elem_bytes == 1 && npix > 256) ? 256 : npix;
    unsigned v = 64;
    while (v < 2 * most && v < (1u << 31)) v <<= 1;
    return v;
}

__host__ SplitMem split_layout(void* scratch, size_t npix, unsigned slots, int elem_bytes) {
    SplitMem m{};
    Taker t{(uint8_t*)scratch};
    m.acc = (unsigned*)t.take(kSpAccWords * 4);
    m.dflag = (unsigned*)t.take((kSpMaxRounds + 2) * 4);
    m.rflag = (unsigned*)t.take((kSpMaxRounds + 2) * 4);
    m.mark = (unsigned*)t.take(npix * 4);
    m.pix = (unsigned*)t.take(npix * 4);
    m.neck = (unsigned*)t.take(npix * 4);
    m.saddle = (unsigned*)t.take((size_t)slots * 4);
    m.best = (unsigned long long*)t.take(npix * 8);
    m.pk = (unsigned long long*)t.take(npix * 8);
    m.vslots = split_value_slots(npix, elem_bytes);
    m.vkeys = (unsigned long long*)t.take((size_t)m.vslots * 8);
    m.vcnt = (unsigned*)t.take((size_t)m.vslots * 4);
    m.zero_words = t.at / 4;
    m.first = (unsigned*)t.take((size_t)slots * 4);
    m.firstpix = (unsigned*)t.take(npix * 4);
    m.keys = (unsigned long long*)t.take((size_t)slots * 8);
    m.ones_words = t.at / 4 - m.zero_words;
    m.up0 = (unsigned*)t.take(npix * 4);
    m.up1 = (unsigned*)t.take(npix * 4);
    m.parent = (unsigned*)t.take(npix * 4);
    m.partial = (unsigned*)t.take(scan_blocks(npix) * 4);
    m.slots = slots;
    m.bytes = t.at;
    return m;
}

__global__ void __launch_bounds__(kSpBlock) split_clear_kernel(SplitMem m) {
    const size_t stride = (size_t)gridDim.x * kSpBlock, total = m.zero_words + m.ones_words;
    for (size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x; i < total; i += stride) m.acc[i] = i < m.zero_words ? 0u : kSpNone;
}

// "this launch changed something": thousands of waves would store to the one word, and stores to one address queue up behind each
// other, so a wave first looks whether the word is set already
__device__ __forceinline__ void sp_raise(unsigned* flag) {
    if (!__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long sp_key(unsigned height, unsigned index) { return ((unsigned long long)height << 32) | (kSpNone - index); }

// the value of pixel (x, y), which must lie in the frame; *kept: it is not skipped
template <class T>
__device__ __forceinline__ unsigned sp_value(const SplitIn& in, size_t at, bool* kept) {
    const unsigned v = (unsigned)((const T*)in.plane)[at];
    *kept = !(in.skip && v == in.skip_value);
    return v;
}

template <class T>
__global__ void __launch_bounds__(kSpBlock) split_ascent_kernel(SplitIn in, SplitMem m) {
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    if (blockIdx.x == 0 && threadIdx.x == 0) m.dflag[0] = 1u;
    if (!r.live) return;
    bool kept, k2;
    const unsigned v = sp_value<T>(in, r.at, &kept);
    unsigned up = kSpNone;
    if (kept) {
        const unsigned i = (unsigned)r.at;
        unsigned long long top = sp_key(in.height[r.at], i);
        up = i;
        // every neighbour is looked at only inside the frame; the largest key wins and keys are distinct
        if (r.y > 0 && sp_value<T>(in, r.at - in.W, &k2) == v && k2) {
            const unsigned long long k = sp_key(in.height[r.at - in.W], i - in.W);
            if (k > top) top = k, up = i - in.W;
        }
        if (r.x > 0 && sp_value<T>(in, r.at - 1, &k2) == v && k2) {
            const unsigned long long k = sp_key(in.height[r.at - 1], i - 1u);
            if (k > top) top = k, up = i - 1u;
        }
        if (r.x + 1 < in.W && sp_value<T>(in, r.at + 1, &k2) == v && k2) {
            const unsigned long long k = sp_key(in.height[r.at + 1], i + 1u);
            if (k > top) top = k, up = i + 1u;
        }
        if (r.y + 1 < in.H && sp_value<T>(in, r.at + in.W, &k2) == v && k2) {
            const unsigned long long k = sp_key(in.height[r.at + in.W], i + in.W);
            if (k > top) top = k, up = i + in.W;
        }
    }
    m.up0[r.at] = up;
}

// up <- up[up]: after launch t a pointer spans 2^t steps of the ascent, or has reached its peak
__global__ void __launch_bounds__(kSpBlock) split_double_kernel(SplitMem m, const unsigned* __restrict__ src, unsigned* __restrict__ dst, size_t npix,
                                                                unsigned t) {
    if (!m.dflag[t - 1]) return;
    const size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    bool changed = false;
    if (i < npix) {
        const unsigned u = src[i];
        unsigned n = u;
        if (u != kSpNone) n = src[u];
        dst[i] = n;
        changed = n != u;
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) sp_raise(m.dflag + t);
}

// What one lane sees of its pixel once the basins are known: its basin, the basins to the right and below, and whether the edges
// towards them join two basins of one value.
struct SplitPixel {
    unsigned b, right, down;
    bool eh, ev;  // the edge to (x+1, y), the edge to (x, y+1)
};
template <class T>
__device__ __forceinline__ SplitPixel sp_pixel(const SplitIn& in, const unsigned* __restrict__ basin, const WaveRow& r) {
    SplitPixel p{kSpNone, kSpNone, kSpNone, false, false};
    if (r.live) {
        bool kept, k2;
        const unsigned v = sp_value<T>(in, r.at, &kept);
        p.b = basin[r.at];
        if (r.x + 1 < in.W) {
            p.right = basin[r.at + 1];
            p.eh = kept && sp_value<T>(in, r.at + 1, &k2) == v && k2 && p.right != p.b;
        }
        if (r.y + 1 < in.H) {
            p.down = basin[r.at + in.W];
            p.ev = kept && sp_value<T>(in, r.at + in.W, &k2) == v && k2 && p.down != p.b;
        }
    }
    return p;
}

__device__ __forceinline__ bool sp_overflow(const SplitMem& m) { return 2ull * m.acc[kSpRuns] > (unsigned long long)m.slots; }

template <class T>
__global__ void __launch_bounds__(kSpBlock) split_count_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin) {
    __shared__ unsigned lacc[2];
    if (threadIdx.x < 2) lacc[threadIdx.x] = 0u;
    __syncthreads();
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const SplitPixel p = sp_pixel<T>(in, basin, r);
    if (r.live) m.parent[r.at] = (unsigned)r.at;
    // a run head: an edge whose (basin, basin) differs from that of the edge one column to the left (edges between rows) or one row
    // up (edges between columns).  Equal basins mean equal values, so the neighbouring edge needs no look at the plane.
    unsigned heads = 0;
    if (p.ev && !(r.x > 0 && basin[r.at - 1] == p.b && basin[r.at + in.W - 1] == p.down)) heads++;
    if (p.eh && !(r.y > 0 && basin[r.at - in.W] == p.b && basin[r.at - in.W + 1] == p.right)) heads++;
    const uint64_t h1 = __ballot(heads & 1u), h2 = __ballot(heads & 2u), pk = __ballot(r.live && p.b == (unsigned)r.at);
    if ((threadIdx.x & 63) == 0) {
        const unsigned nh = (unsigned)__popcll(h1) + 2u * (unsigned)__popcll(h2);
        if (nh) atomicAdd(&lacc[0], nh);
        if (pk) atomicAdd(&lacc[1], (unsigned)__popcll(pk));
    }
    __syncthreads();
    if (threadIdx.x == 0 && lacc[0]) atomicAdd(&m.acc[kSpRuns], lacc[0]);
    if (threadIdx.x == 1 && lacc[1]) atomicAdd(&m.acc[kSpBasins], lacc[1]);
}

__device__ __forceinline__ unsigned sp_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}

// edges between the basins a and b: the largest min-height of them `saddle`, the smallest of their ids `edge`
__device__ __forceinline__ void sp_insert(const SplitMem& m, unsigned a, unsigned b, unsigned saddle, unsigned edge) {
    const unsigned long long key = a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
    const unsigned mask = m.slots - 1;
    unsigned s = sp_hash(key, mask);
    for (unsigned it = 0; it < m.slots; it++) {  // at most half the slots are ever taken: the loop ends long before its bound
        unsigned long long old = kSpDead;
        __hip_atomic_compare_exchange_strong(m.keys + s, &old, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kSpDead || old == key) {
            (void)__hip_atomic_fetch_max(m.saddle + s, saddle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_min(m.first + s, edge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        s = (s + 1) & mask;
    }
}

template <class T>
__global__ void __launch_bounds__(kSpBlock) split_insert_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin) {
    if (sp_overflow(m)) return;
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const SplitPixel p = sp_pixel<T>(in, basin, r);
    const int lane = threadIdx.x & 63;
    const unsigned here = r.live ? in.height[r.at] : 0u;
    unsigned hv = 0, hh = 0;
    if (p.ev) hv = min(here, in.height[r.at + in.W]);
    if (p.eh) hh = min(here, in.height[r.at + 1]);
    const unsigned long long key = p.ev ? ((unsigned long long)p.b << 32) | p.down : kSpDead;
    bool cont;
    const uint64_t starts = wave_run_starts(key, p.ev, &cont);
    // the segmented maximum: after the step of distance d a lane holds the maximum over [lane, lane + 2d) of its own run
    const unsigned head = run_start(starts, lane), last = head + run_length(starts, (int)head) - 1u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_down(hv, d, 64);
        if ((unsigned)lane + d <= last) hv = max(hv, t);
    }
    const unsigned edge = 2u * (unsigned)r.at;
    if (p.ev && !cont) sp_insert(m, p.b, p.down, hv, edge + 1u);
    if (p.eh) sp_insert(m, p.b, p.right, hh, edge);
}

// ---- union-find over the basins: every access of a launch that unites is a relaxed agent-scope atomic, as at Regions' seams ----
__device__ __forceinline__ unsigned sp_find(unsigned* parent, unsigned a) {
    unsigned p;
    while ((p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = p;  // a parent is below its child
    return a;
}

__device__ __forceinline__ void sp_union(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = sp_find(parent, a);
        b = sp_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        const unsigned old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kSpBlock) split_phase1_kernel(SplitMem m, unsigned core) {
    if (sp_overflow(m)) return;
    const size_t s = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    const bool full = s < m.slots && m.keys[s] != kSpDead;
    if (full && m.saddle[s] >= core) {
        const unsigned long long key = m.keys[s];
        sp_union(m.parent, (unsigned)(key >> 32), (unsigned)key);
    }
    const uint64_t any = __ballot(full);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&m.acc[kSpPairs], (unsigned)__popcll(any));
}

__global__ void __launch_bounds__(kSpBlock) split_roots_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin) {
    if (sp_overflow(m)) return;
    const size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    bool marked = false;
    if (i < in.npix && basin[i] == (unsigned)i) {
        // (whatever a racing store of this launch has left in a word is an ancestor too)
        const unsigned root = sp_find(m.parent, (unsigned)i);
        __hip_atomic_store(m.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        marked = in.height[i] >= in.core;
        if (marked) __hip_atomic_store(m.mark + root, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t any = __ballot(marked);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&m.acc[kSpMarked], (unsigned)__popcll(any));
    if (i == 0) m.rflag[0] = 1u;
}

// ---- phase 2: Boruvka's rounds.  Between launches parent[b] is the root of basin b ----
__global__ void __launch_bounds__(kSpBlock) split_choose_kernel(SplitMem m, unsigned t) {
    if (!m.rflag[t - 1]) return;
    const size_t s = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    if (s >= m.slots || m.keys[s] == kSpDead) return;
    const unsigned long long key = m.keys[s];
    const unsigned ra = m.parent[(unsigned)(key >> 32)], rb = m.parent[(unsigned)key];
    if (ra == rb) return;
    const bool ma = m.mark[ra] != 0u, mb = m.mark[rb] != 0u;
    if (ma && mb) return;
    const unsigned long long word = ((unsigned long long)m.saddle[s] << 32) | (kSpNone - m.first[s]);  // never 0: an edge id is below 2^32 - 1
    if (!ma) atomicMax(m.best + ra, word);
    if (!mb) atomicMax(m.best + rb, word);
}

// one lane per root with a word: the partner is found again from FIRST, edge id -> two pixels -> basins -> roots.  Two roots that
// chose each other hold the same word (FIRST names one pair); the smaller stays.  next[r], the root's own word, is the only store.
__global__ void __launch_bounds__(kSpBlock) split_hook_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin, unsigned* __restrict__ next,
                                                              unsigned t) {
    if (!m.rflag[t - 1]) return;
    const size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    bool hooked = false;
    if (i < in.npix && basin[i] == (unsigned)i && m.parent[i] == (unsigned)i) {
        const unsigned self = (unsigned)i;
        unsigned to = self;
        const unsigned long long word = m.best[i];
        if (word) {
            const unsigned edge = kSpNone - (unsigned)word;
            const size_t p = edge >> 1, q = (edge & 1u) ? p + in.W : p + 1;
            if (q < in.npix) {  // (always: the id came from an edge of the plane)
                const unsigned rp = m.parent[basin[p]], rq = m.parent[basin[q]];
                const unsigned partner = rp == self ? rq : rp;
                if (!(m.best[partner] == word && self < partner)) to = partner;
            }
        }
        next[i] = to;
        hooked = to != self;
    }
    if (__ballot(hooked) && (threadIdx.x & 63) == 0) sp_raise(m.rflag + t);
}

// every peak follows the hooks of its old root to the new one.  The hooks form a forest (the order on pairs is strict, so the only
// cycle of choices is the mutual one, which hook has broken); the bound on the walk is never reached.
__global__ void __launch_bounds__(kSpBlock) split_flatten_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin,
                                                                 const unsigned* __restrict__ next, unsigned t) {
    if (!m.rflag[t - 1]) return;
    const size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    if (i >= in.npix || basin[i] != (unsigned)i) return;
    unsigned r = m.parent[i];
    for (size_t it = 0; it < in.npix; it++) {
        const unsigned n = next[r];
        if (n == r) break;
        r = n;
    }
    m.parent[i] = r;
    m.best[i] = 0ull;
}

// ---- measure and number ----
template <class T>
__global__ void __launch_bounds__(kSpBlock) split_measure_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin) {
    if (sp_overflow(m)) return;
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const int lane = threadIdx.x & 63;
    unsigned root = kSpNone;
    bool kept = false;
    if (r.live) {
        const unsigned b = basin[r.at];
        kept = b != kSpNone;
        if (kept) {
            root = m.parent[b];
            if (b == (unsigned)r.at) atomicMax(m.pk + root, sp_key(in.height[r.at], b));
        }
    }
    bool cont;
    const uint64_t starts = wave_run_starts(root, kept, &cont);
    if (kept && !cont) {  // the head of a run is its smallest index
        (void)__hip_atomic_fetch_add(m.pix + root, run_length(starts, lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_min(m.firstpix + root, (unsigned)r.at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(kSpBlock) split_neck_kernel(SplitMem m) {
    if (sp_overflow(m)) return;
    const size_t s = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    if (s >= m.slots || m.keys[s] == kSpDead) return;
    const unsigned long long key = m.keys[s];
    const unsigned ra = m.parent[(unsigned)(key >> 32)], rb = m.parent[(unsigned)key];
    if (ra == rb) return;
    const unsigned sd = m.saddle[s];
    (void)__hip_atomic_fetch_max(m.neck + ra, sd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(m.neck + rb, sd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one more segment of `value`.  Whichever add finds 1 in the slot has found a value with more than one segment, and no other add of
// that slot finds 1: SPLIT_VALUES does not depend on who comes when.
__device__ __forceinline__ void sp_count_value(const SplitMem& m, unsigned value) {
    const unsigned long long key = (unsigned long long)value + 1ull;
    const unsigned mask = m.vslots - 1;
    unsigned s = sp_hash(key, mask);
    for (unsigned it = 0; it < m.vslots; it++) {  // at most half the slots are ever taken: the loop ends long before its bound
        unsigned long long old = 0ull;
        __hip_atomic_compare_exchange_strong(m.vkeys + s, &old, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0ull || old == key) {
            if (__hip_atomic_fetch_add(m.vcnt + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u)
                (void)__hip_atomic_fetch_add(m.acc + kSpSplitValues, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        s = (s + 1) & mask;
    }
}

// this pixel is the first of its segment
__device__ __forceinline__ bool sp_first(const SplitMem& m, const unsigned* __restrict__ basin, size_t i, size_t npix, unsigned* root) {
    if (i >= npix) return false;
    const unsigned b = basin[i];
    if (b == kSpNone) return false;
    *root = m.parent[b];
    return m.firstpix[*root] == (unsigned)i;
}

template <class T>
__global__ void __launch_bounds__(kScanBlock) split_block_sums_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin) {
    __shared__ unsigned wsum[kScanBlock / 64];
    unsigned root;
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const bool first = !sp_overflow(m) && sp_first(m, basin, i, in.npix, &root);
    const unsigned s = flag_block_sum(first, wsum);
    if (threadIdx.x == 0) m.partial[blockIdx.x] = s;
    if (first) sp_count_value(m, (unsigned)((const T*)in.plane)[i]);
}

__global__ void __launch_bounds__(kScanBlock) split_scan_kernel(SplitMem m, size_t npix) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned total = scan_block_sums(m.partial, scan_blocks(npix), wsum);
    if (threadIdx.x == 0) m.acc[kSpSegments] = total;
}

// the first pixel of a segment gives it its number and writes its row; segid[root] has that one writer
template <class T>
__global__ void __launch_bounds__(kScanBlock) split_rank_kernel(SplitIn in, SplitMem m, const unsigned* __restrict__ basin, unsigned* __restrict__ segid,
                                                                unsigned* __restrict__ table, unsigned rows) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    unsigned root = 0;
    const bool over = sp_overflow(m);
    const bool first = !over && sp_first(m, basin, i, in.npix, &root);
    const unsigned rank = flag_rank(first, m.partial[blockIdx.x], wsum);
    if (!first) return;
    segid[root] = rank;
    if (table && rank < rows) {
        const unsigned long long pk = m.pk[root];
        unsigned* o = table + (size_t)rank * kSplitWords;
        o[0] = (unsigned)((const T*)in.plane)[i];
        o[1] = m.pix[root];
        o[2] = (unsigned)i;
        o[3] = kSpNone - (unsigned)pk;
        o[4] = (unsigned)(pk >> 32);
        o[5] = m.neck[root];
    }
}

__global__ void __launch_bounds__(kSpBlock) split_labels_kernel(SplitMem m, const unsigned* __restrict__ basin, const unsigned* __restrict__ segid,
                                                                size_t npix, unsigned* __restrict__ labels) {
    if (sp_overflow(m)) return;
    const size_t i = (size_t)blockIdx.x * kSpBlock + threadIdx.x;
    if (i >= npix) return;
    const unsigned b = basin[i];
    labels[i] = b == kSpNone ? kSpNone : segid[m.parent[b]];
}

__global__ void split_counts_kernel(SplitMem m, unsigned* __restrict__ counts) {
    const bool over = sp_overflow(m);
    counts[0] = over ? 0u : m.acc[kSpSegments];
    counts[1] = m.acc[kSpBasins];
    counts[2] = m.acc[kSpPairs];
    counts[3] = m.acc[kSpRuns];
    counts[4] = m.acc[kSpMarked];
    counts[5] = m.acc[kSpSplitValues];
    unsigned rounds = 0;  // the rounds that hooked something are the first ones
    while (rounds < kSpMaxRounds && m.rflag[rounds + 1]) rounds++;
    counts[6] = rounds;
    counts[7] = over ? kSplitOverflow : 0u;
}

__global__ void split_empty_counts_kernel(unsigned* __restrict__ counts) {
    if (threadIdx.x < kSplitCountWords) counts[threadIdx.x] = 0u;
}

unsigned ceil_log2(size_t n) {
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

template <class T>
hipError_t launch_split_t(const SplitIn& in, const SplitMem& m, unsigned* labels, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    const size_t npix = in.npix;
    const size_t rowBlocks = ((size_t)in.H * in.tilesX + 3) / 4, pixBlocks = (npix + kSpBlock - 1) / kSpBlock, scanBlocks = scan_blocks(npix);
    if (rowBlocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 rowGrid((unsigned)rowBlocks), pixGrid((unsigned)pixBlocks), slotGrid((m.slots + kSpBlock - 1) / kSpBlock), blk(kSpBlock);
    const size_t clearWords = m.zero_words + m.ones_words;
    const size_t clearBlocks = (clearWords + kSpBlock * 16 - 1) / (kSpBlock * 16);
    hipLaunchKernelGGL(split_clear_kernel, dim3((unsigned)(clearBlocks < 65536 ? clearBlocks : 65536)), blk, 0, s, m);
    hipLaunchKernelGGL((split_ascent_kernel<T>), rowGrid, blk, 0, s, in, m);
    const unsigned doublings = ceil_log2(npix);
    unsigned *src = m.up0, *dst = m.up1;
    for (unsigned t = 1; t <= doublings; t++) {
        hipLaunchKernelGGL(split_double_kernel, pixGrid, blk, 0, s, m, (const unsigned*)src, dst, npix, t);
        unsigned* const x = src;
        src = dst;
        dst = x;
    }
    const unsigned* basin = src;  // what the last doubling wrote; dst is free: the hooks of the rounds, then the segment ids
    unsigned* spare = dst;
    hipLaunchKernelGGL((split_count_kernel<T>), rowGrid, blk, 0, s, in, m, basin);
    hipLaunchKernelGGL((split_insert_kernel<T>), rowGrid, blk, 0, s, in, m, basin);
    hipLaunchKernelGGL(split_phase1_kernel, slotGrid, blk, 0, s, m, in.core);
    hipLaunchKernelGGL(split_roots_kernel, pixGrid, blk, 0, s, in, m, basin);
    const unsigned rounds = split_rounds(npix, m.slots);
    for (unsigned t = 1; t <= rounds; t++) {
        hipLaunchKernelGGL(split_choose_kernel, slotGrid, blk, 0, s, m, t);
        hipLaunchKernelGGL(split_hook_kernel, pixGrid, blk, 0, s, in, m, basin, spare, t);
        hipLaunchKernelGGL(split_flatten_kernel, pixGrid, blk, 0, s, in, m, basin, (const unsigned*)spare, t);
    }
    hipLaunchKernelGGL((split_measure_kernel<T>), rowGrid, blk, 0, s, in, m, basin);
    hipLaunchKernelGGL(split_neck_kernel, slotGrid, blk, 0, s, m);
    hipLaunchKernelGGL((split_block_sums_kernel<T>), dim3((unsigned)scanBlocks), dim3(kScanBlock), 0, s, in, m, basin);
    hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, m, npix);
    if (labels || (table && rows)) {
        hipLaunchKernelGGL((split_rank_kernel<T>), dim3((unsigned)scanBlocks), dim3(kScanBlock), 0, s, in, m, basin, spare, table, rows);
        if (labels) hipLaunchKernelGGL(split_labels_kernel, pixGrid, blk, 0, s, m, basin, (const unsigned*)spare, npix, labels);
    }
    if (counts) hipLaunchKernelGGL(split_counts_kernel, dim3(1), dim3(1), 0, s, m, counts);
    return hipGetLastError();
}

}  // namespace

unsigned split_rounds(size_t npix, unsigned pair_slots) { return ceil_log2(npix < pair_slots ? npix : (size_t)pair_slots) + 1u; }

unsigned split_launches(size_t npix, unsigned pair_slots, bool labels, bool table, bool counts) {
    if (!npix) return counts ? 1u : 0u;
    return 10u + ceil_log2(npix) + 3u * split_rounds(npix, pair_slots) + ((labels || table) ? 1u : 0u) + (labels ? 1u : 0u) + (counts ? 1u : 0u);
}

size_t split_scratch_bytes(size_t npix, unsigned pair_slots, int elem_bytes) { return split_layout(nullptr, npix, pair_slots, elem_bytes).bytes; }

hipError_t launch_split(const void* plane, int elem_bytes, const unsigned* height, unsigned H, unsigned W, int skip, unsigned skip_value, unsigned core,
                        void* scratch, unsigned pair_slots, unsigned* labels, unsigned* table, unsigned rows, unsigned* counts, hipStream_t s) {
    const size_t npix = (size_t)H * W;
    if (npix == 0) {  // no pixel, no segment: zeros, and no scratch
        if (counts) hipLaunchKernelGGL(split_empty_counts_kernel, dim3(1), dim3(64), 0, s, counts);
        return hipGetLastError();
    }
    if (npix >= (1ull << 31) || pair_slots < 64 || (pair_slots & (pair_slots - 1))) return hipErrorInvalidValue;
    if (elem_bytes != 1 && elem_bytes != 4) return hipErrorInvalidValue;
    const SplitMem m = split_layout(scratch, npix, pair_slots, elem_bytes);
    const SplitIn in{plane, height, H, W, (W + 63) / 64, skip ? 1u : 0u, skip_value, core, npix};
    return elem_bytes == 1   ? launch_split_t<uint8_t>(in, m, labels, table, rows, counts, s)
           : elem_bytes == 4 ? launch_split_t<uint32_t>(in, m, labels, table, rows, counts, s)
                             : hipErrorInvalidValue;
}

}  // namespace infur
