// sieve.hip -- Adjacency and Sieve (include/infur_hip.h): which values of a plane touch along how many pixel edges, and
// the merger of every region below a size threshold into the neighbour it shares the longest border with.  A pixel is inside when
// its value is below `rows` and is not the skipped value; a border edge is a pixel edge between two inside 4-neighbours of
// different values.  The edge between (x, y) and (x+1, y) has id 2 (y W + x), the edge between (x, y) and (x, y+1) id 2 (y W + x) + 1.
// The kernel boundaries are the only ordering, no workgroup ever waits for another:
//   adjacency   two memsets, up to nine launches
//     1 count    R = the border runs (a run head needs the pair one column to the left, or one row up), the pixel classes, and
//                -- for a wanted row table -- PERIMETER: one ballot of run starts of the value per wave-row, one add per run
//     2 insert   unless 2 R > slots: borders between rows y and y+1 as runs along the wave-row (one ballot of "the (top, bottom)
//                key differs from the left lane's", one 64-bit CAS of (A << 32) | B, one add of the run length and one atomicMin
//                of the edge id per run); borders between columns x and x+1 one per edge
//     3 slots    one lane per slot: DEGREE adds, atomicMax of (border << 32) | (0xFFFFFFFF - neighbour) per side, PAIRS, EDGES,
//                and the pair's bit in the bitmap of first edge ids
//     4-6 rank   popcounts of the bitmap words per workgroup, scan_block_sums over them, the exclusive prefix per word
//     7 records  one lane per slot: the record at the rank of its FIRST
//     8 rows, 9 counts
//   sieve       1 count and 2 insert of the label plane with rows = min(*n_regions, table_rows), then init, max_rounds x (choose
//               over the slots, apply over the regions), relabel, rows, counts.  A round behind one that resolved nothing exits
//               on a device flag.
// The slot a pair lands in depends on timing and never reaches an output: the records are placed by FIRST, everything else is a
// sum, a minimum or a maximum of integers, which commute.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kAdjBlock = 256;
constexpr unsigned kAdjNone = 0xFFFFFFFFu;
constexpr unsigned long long kAdjDead = ~0ull;

// the accumulators at the head of the scratch, cleared by the call's memset
enum { kAccRuns = 0, kAccSkipped, kAccOutside, kAccPairs, kAccEdges, kAccWords = 8 };
// the sieve's own
enum { kSvSmall = 0, kSvAbsorbed, kSvRounds, kSvChanged, kSvWords = 8 };

struct AdjIn {
    const void* plane;
    unsigned H, W, tilesX;
    unsigned skip, skip_value;
    unsigned rows;
    const unsigned* d_n;  // Sieve: the device word n_regions, rows = min(*d_n, rows)
};

// The scratch of a call.  Everything in front of `first` is cleared to 0 by one memset, first and keys to all ones by a second;
// wbase needs no initialisation.
struct AdjMem {
    unsigned* acc;
    unsigned *deg, *perim;     // per row; null when no row table is wanted
    unsigned long long* best;  // per row
    unsigned* cnts;            // per slot: BORDER
    unsigned *bits, *partial;  // the bitmap of first edge ids and its block sums; null when no records are wanted
    unsigned* first;           // per slot: FIRST
    unsigned long long* keys;  // per slot: (A << 32) | B
    unsigned* wbase;           // per bitmap word: the set bits in front of it
    unsigned slots;
    size_t words;  // of the bitmap
    size_t zero_bytes, ones_bytes, bytes;
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

__host__ AdjMem adj_layout(void* scratch, size_t npix, unsigned rows, unsigned slots, bool want_rows, bool want_pairs) {
    AdjMem m{};
    Taker t{(uint8_t*)scratch};
    m.acc = (unsigned*)t.take(kAccWords * 4);
    if (want_rows) {
        m.deg = (unsigned*)t.take((size_t)rows * 4);
        m.perim = (unsigned*)t.take((size_t)rows * 4);
        m.best = (unsigned long long*)t.take((size_t)rows * 8);
    }
    m.cnts = (unsigned*)t.take((size_t)slots * 4);
    m.words = want_pairs ? (2 * npix + 31) / 32 : 0;
    if (want_pairs) {
        m.bits = (unsigned*)t.take(m.words * 4);
        m.partial = (unsigned*)t.take(scan_blocks(m.words) * 4);
    }
    m.zero_bytes = t.at;
    m.first = (unsigned*)t.take((size_t)slots * 4);
    m.keys = (unsigned long long*)t.take((size_t)slots * 8);
    m.ones_bytes = t.at - m.zero_bytes;
    if (want_pairs) m.wbase = (unsigned*)t.take(m.words * 4);
    m.slots = slots;
    m.bytes = t.at;
    return m;
}

__device__ __forceinline__ unsigned adj_rows(const AdjIn& in) {
    if (!in.d_n) return in.rows;
    const unsigned n = *in.d_n;
    return n < in.rows ? n : in.rows;
}

// the value of pixel (x, y) when it is inside, else kAdjNone; (x, y) must lie in the frame
template <class T>
__device__ __forceinline__ unsigned adj_inside(const AdjIn& in, unsigned x, unsigned y, unsigned rows) {
    const unsigned v = (unsigned)((const T*)in.plane)[(size_t)y * in.W + x];
    return (v < rows && !(in.skip && v == in.skip_value)) ? v : kAdjNone;
}

__device__ __forceinline__ bool adj_border(unsigned a, unsigned b) { return a != kAdjNone && b != kAdjNone && a != b; }

// What one lane sees of its pixel: its inside value, the neighbours to the right and below (kAdjNone beyond the frame), and whether
// the edges towards them are border edges.
struct AdjPixel {
    unsigned v, right, down;
    bool bh, bv;  // the edge to (x+1, y), the edge to (x, y+1)
};
template <class T>
__device__ __forceinline__ AdjPixel adj_pixel(const AdjIn& in, const WaveRow& r, unsigned rows) {
    AdjPixel p{kAdjNone, kAdjNone, kAdjNone, false, false};
    if (r.live) {
        p.v = adj_inside<T>(in, r.x, r.y, rows);
        if (r.x + 1 < in.W) p.right = adj_inside<T>(in, r.x + 1, r.y, rows);
        if (r.y + 1 < in.H) p.down = adj_inside<T>(in, r.x, r.y + 1, rows);
        p.bh = adj_border(p.v, p.right);
        p.bv = adj_border(p.v, p.down);
    }
    return p;
}

__device__ __forceinline__ bool adj_overflow(const AdjMem& m) { return 2ull * m.acc[kAccRuns] > (unsigned long long)m.slots; }

template <class T>
__global__ void __launch_bounds__(kAdjBlock) adj_count_kernel(AdjIn in, AdjMem m) {
    __shared__ unsigned lacc[3];
    if (threadIdx.x < 3) lacc[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned rows = adj_rows(in);
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const int lane = threadIdx.x & 63;
    const AdjPixel p = adj_pixel<T>(in, r, rows);
    unsigned raw = 0;
    if (r.live) raw = (unsigned)((const T*)in.plane)[r.at];
    const bool skipped = r.live && in.skip && raw == in.skip_value;
    // a run head: a border edge whose pair differs from the pair one column to the left (edges between rows) or one row up
    unsigned heads = 0;
    if (p.bv && !(r.x > 0 && adj_inside<T>(in, r.x - 1, r.y, rows) == p.v && adj_inside<T>(in, r.x - 1, r.y + 1, rows) == p.down)) heads++;
    if (p.bh && !(r.y > 0 && adj_inside<T>(in, r.x, r.y - 1, rows) == p.v && adj_inside<T>(in, r.x + 1, r.y - 1, rows) == p.right)) heads++;
    const uint64_t h1 = __ballot(heads & 1u), h2 = __ballot(heads & 2u), sk = __ballot(skipped), out = __ballot(r.live && !skipped && raw >= rows);
    if (lane == 0) {
        const unsigned nh = (unsigned)__popcll(h1) + 2u * (unsigned)__popcll(h2);
        if (nh) atomicAdd(&lacc[0], nh);
        if (sk) atomicAdd(&lacc[1], (unsigned)__popcll(sk));
        if (out) atomicAdd(&lacc[2], (unsigned)__popcll(out));
    }
    if (m.perim) {  // (uniform)
        // the sides of the pixel that face anything but its value, the frame included; summed per run of the value along the wave
        unsigned sides = 0;
        const bool in_v = p.v != kAdjNone;
        if (in_v) {
            sides += (r.x + 1 >= in.W || p.right != p.v) ? 1u : 0u;
            sides += (r.y + 1 >= in.H || p.down != p.v) ? 1u : 0u;
            sides += (r.x == 0 || adj_inside<T>(in, r.x - 1, r.y, rows) != p.v) ? 1u : 0u;
            sides += (r.y == 0 || adj_inside<T>(in, r.x, r.y - 1, rows) != p.v) ? 1u : 0u;
        }
        bool cont;
        const uint64_t starts = wave_run_starts(p.v, in_v, &cont);
        const uint64_t b0 = __ballot(sides & 1u), b1 = __ballot(sides & 2u), b2 = __ballot(sides & 4u);
        if (in_v && !cont) {
            const unsigned len = run_length(starts, lane);
            const uint64_t mask = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
            const unsigned sum = (unsigned)__popcll(mask & b0) + 2u * (unsigned)__popcll(mask & b1) + 4u * (unsigned)__popcll(mask & b2);
            if (sum) (void)__hip_atomic_fetch_add(m.perim + p.v, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && lacc[threadIdx.x]) atomicAdd(&m.acc[threadIdx.x], lacc[threadIdx.x]);
}

__device__ __forceinline__ unsigned adj_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}

// n border edges between the values a and b, the smallest of them `edge`
__device__ __forceinline__ void adj_insert(const AdjMem& m, unsigned a, unsigned b, unsigned n, unsigned edge) {
    const unsigned long long key = a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
    const unsigned mask = m.slots - 1;
    unsigned s = adj_hash(key, mask);
    for (unsigned it = 0; it < m.slots; it++) {  // at most half the slots are ever taken: the loop ends long before its bound
        unsigned long long old = kAdjDead;
        __hip_atomic_compare_exchange_strong(m.keys + s, &old, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kAdjDead || old == key) {
            (void)__hip_atomic_fetch_add(m.cnts + s, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_min(m.first + s, edge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        s = (s + 1) & mask;
    }
}

template <class T>
__global__ void __launch_bounds__(kAdjBlock) adj_insert_kernel(AdjIn in, AdjMem m) {
    if (adj_overflow(m)) return;
    const WaveRow r = wave_row(in.H, in.W, in.tilesX);
    const AdjPixel p = adj_pixel<T>(in, r, adj_rows(in));
    const unsigned long long key = p.bv ? ((unsigned long long)p.v << 32) | p.down : kAdjDead;
    bool cont;
    const uint64_t starts = wave_run_starts(key, p.bv, &cont);
    const unsigned edge = 2u * (unsigned)r.at;
    if (p.bv && !cont) adj_insert(m, p.v, p.down, run_length(starts, threadIdx.x & 63), edge + 1u);
    if (p.bh) adj_insert(m, p.v, p.right, 1u, edge);
}

__global__ void __launch_bounds__(kAdjBlock) adj_slots_kernel(AdjMem m) {
    const size_t s = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    const bool full = s < m.slots && !adj_overflow(m) && m.keys[s] != kAdjDead;
    unsigned border = 0;
    if (full) {
        const unsigned long long key = m.keys[s];
        const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
        border = m.cnts[s];
        if (m.deg) {
            (void)__hip_atomic_fetch_add(m.deg + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(m.deg + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMax(m.best + a, ((unsigned long long)border << 32) | (kAdjNone - b));
            atomicMax(m.best + b, ((unsigned long long)border << 32) | (kAdjNone - a));
        }
        if (m.bits) {
            const unsigned f = m.first[s];
            atomicOr(m.bits + (f >> 5), 1u << (f & 31u));
        }
    }
    const uint64_t any = __ballot(full);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) border += __shfl_xor(border, d, 64);
    if ((threadIdx.x & 63) == 0 && any) {
        atomicAdd(&m.acc[kAccPairs], (unsigned)__popcll(any));
        atomicAdd(&m.acc[kAccEdges], border);
    }
}

// ---- the rank of a first edge id: the set bits of the bitmap in front of it ----
__global__ void __launch_bounds__(kScanBlock) adj_word_sums_kernel(AdjMem m) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    unsigned n = i < m.words ? (unsigned)__popc(m.bits[i]) : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int k = 0; k < kScanBlock / 64; k++) s += wsum[k];
        m.partial[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kScanBlock) adj_scan_kernel(AdjMem m) {
    __shared__ unsigned wsum[kScanBlock / 64];
    (void)scan_block_sums(m.partial, scan_blocks(m.words), wsum);
}

__global__ void __launch_bounds__(kScanBlock) adj_word_base_kernel(AdjMem m) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = i < m.words ? (unsigned)__popc(m.bits[i]) : 0u;
    unsigned inc = n;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = m.partial[blockIdx.x];
    for (int k = 0; k < wave; k++) before += wsum[k];
    if (i < m.words) m.wbase[i] = before + inc - n;
}

__global__ void __launch_bounds__(kAdjBlock) adj_records_kernel(AdjMem m, unsigned* __restrict__ pairs, unsigned pair_rows) {
    const size_t s = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (s >= m.slots || adj_overflow(m) || m.keys[s] == kAdjDead) return;
    const unsigned f = m.first[s];
    const unsigned rank = m.wbase[f >> 5] + (unsigned)__popc(m.bits[f >> 5] & ((1u << (f & 31u)) - 1u));
    if (rank >= pair_rows) return;
    const unsigned long long key = m.keys[s];
    unsigned* o = pairs + (size_t)rank * kAdjPairWords;
    o[0] = (unsigned)(key >> 32);
    o[1] = (unsigned)key;
    o[2] = m.cnts[s];
    o[3] = f;
}

__global__ void __launch_bounds__(kAdjBlock) adj_rows_kernel(AdjMem m, unsigned rows, unsigned* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (t >= rows) return;
    const unsigned long long best = m.best[t];
    out[t * kAdjRowWords + 0] = m.deg[t];
    out[t * kAdjRowWords + 1] = best ? kAdjNone - (unsigned)best : kAdjNone;
    out[t * kAdjRowWords + 2] = (unsigned)(best >> 32);
    out[t * kAdjRowWords + 3] = m.perim[t];
}

// an empty plane: no value has a pixel
__global__ void __launch_bounds__(kAdjBlock) adj_empty_rows_kernel(unsigned rows, unsigned* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (t >= rows) return;
    out[t * kAdjRowWords + 0] = 0u;
    out[t * kAdjRowWords + 1] = kAdjNone;
    out[t * kAdjRowWords + 2] = 0u;
    out[t * kAdjRowWords + 3] = 0u;
}

__global__ void adj_counts_kernel(AdjMem m, unsigned pair_rows, int want_pairs, unsigned* __restrict__ counts) {
    const bool over = adj_overflow(m);
    const unsigned pairs = m.acc[kAccPairs];
    const unsigned written = want_pairs ? (pairs < pair_rows ? pairs : pair_rows) : 0u;
    counts[0] = pairs;
    counts[1] = m.acc[kAccEdges];
    counts[2] = m.acc[kAccSkipped];
    counts[3] = m.acc[kAccOutside];
    counts[4] = m.acc[kAccRuns];
    counts[5] = written;
    counts[6] = 0u;
    counts[7] = (over ? kAdjOverflow : 0u) | ((want_pairs && pairs > pair_rows) ? kAdjTruncated : 0u);
}

template <class T>
hipError_t launch_adj_table(const AdjIn& in, const AdjMem& m, hipStream_t s) {
    const size_t rowBlocks = ((size_t)in.H * in.tilesX + 3) / 4;
    if (rowBlocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m.acc, 0, m.zero_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(m.first, 0xFF, m.ones_bytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((adj_count_kernel<T>), dim3((unsigned)rowBlocks), dim3(kAdjBlock), 0, s, in, m);
    hipLaunchKernelGGL((adj_insert_kernel<T>), dim3((unsigned)rowBlocks), dim3(kAdjBlock), 0, s, in, m);
    return hipGetLastError();
}

// ---- Sieve ----
struct SieveMem {
    unsigned* sacc;            // kSvWords
    unsigned* flags;           // [t]: round t resolved something ([0]: the table did not overflow); 66 words
    unsigned long long* best;  // per region: the round's winning (border << 32) | (0xFFFFFFFF - q); stays 0 while unresolved
    unsigned *cls, *into, *round, *border;  // per region, written by init; cls == kAdjNone: unresolved
    size_t zero_bytes, bytes;
};

__host__ SieveMem sieve_layout(void* scratch, unsigned table_rows) {
    SieveMem v{};
    Taker t{(uint8_t*)scratch};
    v.sacc = (unsigned*)t.take(kSvWords * 4);
    v.flags = (unsigned*)t.take(66 * 4);
    v.best = (unsigned long long*)t.take((size_t)table_rows * 8);
    v.zero_bytes = t.at;
    v.cls = (unsigned*)t.take((size_t)table_rows * 4);
    v.into = (unsigned*)t.take((size_t)table_rows * 4);
    v.round = (unsigned*)t.take((size_t)table_rows * 4);
    v.border = (unsigned*)t.take((size_t)table_rows * 4);
    v.bytes = t.at;
    return v;
}

struct SieveIn {
    const uint8_t* klass;
    const unsigned* labels;
    const unsigned long long* table;
    const unsigned* d_n;
    unsigned table_rows, min_pixels, max_rounds;
    size_t npix;
};

__device__ __forceinline__ unsigned sieve_n(const SieveIn& in) {
    const unsigned n = *in.d_n;
    return n < in.table_rows ? n : in.table_rows;
}

__global__ void __launch_bounds__(kAdjBlock) sieve_init_kernel(SieveIn in, AdjMem m, SieveMem v) {
    const size_t r = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    const bool live = r < sieve_n(in);
    bool small = false;
    if (live) {
        small = in.table[r * kRegWords + 0] < (unsigned long long)in.min_pixels;
        v.cls[r] = small ? kAdjNone : (unsigned)in.table[r * kRegWords + 8];
        v.into[r] = (unsigned)r;
        v.round[r] = small ? kAdjNone : 0u;
        v.border[r] = 0u;
    }
    const uint64_t any = __ballot(small);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&v.sacc[kSvSmall], (unsigned)__popcll(any));
    if (r == 0 && !adj_overflow(m)) v.flags[0] = 1u;
}

__global__ void __launch_bounds__(kAdjBlock) sieve_choose_kernel(AdjMem m, SieveMem v, unsigned t) {
    if (!v.flags[t - 1]) return;
    const size_t s = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (s >= m.slots || m.keys[s] == kAdjDead) return;
    const unsigned long long key = m.keys[s];
    const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
    const bool ra = v.cls[a] != kAdjNone, rb = v.cls[b] != kAdjNone;
    if (ra == rb) return;
    const unsigned long long border = (unsigned long long)m.cnts[s] << 32;
    if (ra) atomicMax(v.best + b, border | (kAdjNone - a));
    else atomicMax(v.best + a, border | (kAdjNone - b));
}

__global__ void __launch_bounds__(kAdjBlock) sieve_apply_kernel(SieveIn in, SieveMem v, unsigned t) {
    if (!v.flags[t - 1]) return;
    const size_t r = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    unsigned changed = 0;
    bool won = false;
    if (r < sieve_n(in) && v.cls[r] == kAdjNone && v.best[r]) {
        // q was resolved before this round: nothing of it is written in this launch
        const unsigned long long best = v.best[r];
        const unsigned q = kAdjNone - (unsigned)best, k = v.cls[q];
        v.cls[r] = k;
        v.into[r] = v.into[q];
        v.round[r] = t;
        v.border[r] = (unsigned)(best >> 32);
        won = true;
        if (k != (unsigned)in.table[r * kRegWords + 8]) changed = (unsigned)in.table[r * kRegWords + 0];
    }
    const uint64_t any = __ballot(won);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) changed += __shfl_xor(changed, d, 64);
    if ((threadIdx.x & 63) == 0 && any) {
        atomicAdd(&v.sacc[kSvAbsorbed], (unsigned)__popcll(any));
        if (changed) atomicAdd(&v.sacc[kSvChanged], changed);
        atomicMax(&v.sacc[kSvRounds], t);
        v.flags[t] = 1u;
    }
}

__global__ void __launch_bounds__(kAdjBlock) sieve_relabel_kernel(SieveIn in, SieveMem v, uint8_t* __restrict__ klass_out) {
    const size_t i = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (i >= in.npix) return;
    const unsigned l = in.labels[i];
    uint8_t k = in.klass[i];
    if (l < sieve_n(in)) {  // (INFUR_REGION_NONE is above every n)
        const unsigned to = v.cls[l];
        if (to != kAdjNone) k = (uint8_t)to;
    }
    klass_out[i] = k;
}

__global__ void __launch_bounds__(kAdjBlock) sieve_rows_kernel(SieveIn in, SieveMem v, unsigned* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * kAdjBlock + threadIdx.x;
    if (r >= sieve_n(in)) return;
    const unsigned k = v.cls[r];
    out[r * kSieveRowWords + 0] = k != kAdjNone ? k : (unsigned)in.table[r * kRegWords + 8];
    out[r * kSieveRowWords + 1] = v.into[r];
    out[r * kSieveRowWords + 2] = v.round[r];
    out[r * kSieveRowWords + 3] = v.border[r];
}

__global__ void sieve_counts_kernel(SieveIn in, AdjMem m, SieveMem v, unsigned* __restrict__ counts) {
    const bool over = adj_overflow(m);
    const unsigned small = v.sacc[kSvSmall], absorbed = v.sacc[kSvAbsorbed], stranded = small - absorbed;
    // the pairs: the full slots were not counted by a launch of their own
    counts[0] = sieve_n(in);
    counts[1] = small;
    counts[2] = absorbed;
    counts[3] = stranded;
    counts[4] = v.sacc[kSvRounds];
    counts[5] = v.sacc[kSvChanged];
    counts[6] = m.acc[kAccPairs];
    counts[7] = (over ? kSieveOverflow : 0u) | ((v.flags[in.max_rounds] && stranded) ? kSieveRoundsExhausted : 0u) |
                (*in.d_n > in.table_rows ? kSieveTableShort : 0u);
}

}  // namespace

size_t adjacency_scratch_bytes(size_t npix, unsigned rows, unsigned pair_slots, bool want_rows, bool want_pairs) {
    return adj_layout(nullptr, npix, rows, pair_slots, want_rows, want_pairs).bytes;
}

hipError_t launch_adjacency(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, unsigned rows, void* scratch,
                            unsigned pair_slots, unsigned* pairs, unsigned pair_rows, unsigned* rows_out, unsigned* counts, hipStream_t s) {
    const size_t npix = (size_t)H * W;
    if (!rows) rows_out = nullptr;
    if (npix == 0) {  // zeros and NONE rows, and nothing else: no scratch
        if (counts) {
            const hipError_t e = hipMemsetAsync(counts, 0, kAdjCountWords * 4, s);
            if (e != hipSuccess) return e;
        }
        if (rows_out) hipLaunchKernelGGL(adj_empty_rows_kernel, dim3((rows + kAdjBlock - 1) / kAdjBlock), dim3(kAdjBlock), 0, s, rows, rows_out);
        return hipGetLastError();
    }
    if (npix >= (1ull << 31) || pair_slots < 64 || (pair_slots & (pair_slots - 1))) return hipErrorInvalidValue;
    const bool want_pairs = pairs != nullptr;
    if (!want_pairs) pair_rows = 0;
    const bool ranked = want_pairs && pair_rows;
    const AdjMem m = adj_layout(scratch, npix, rows, pair_slots, rows_out != nullptr, ranked);
    const AdjIn in{plane, H, W, (W + 63) / 64, skip ? 1u : 0u, skip_value, rows, nullptr};
    hipError_t e = elem_bytes == 1 ? launch_adj_table<uint8_t>(in, m, s) : elem_bytes == 4 ? launch_adj_table<uint32_t>(in, m, s) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    const unsigned slotBlocks = (pair_slots + kAdjBlock - 1) / kAdjBlock;
    hipLaunchKernelGGL(adj_slots_kernel, dim3(slotBlocks), dim3(kAdjBlock), 0, s, m);
    if (ranked) {
        const size_t nb = scan_blocks(m.words);
        if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(adj_word_sums_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, s, m);
        hipLaunchKernelGGL(adj_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, m);
        hipLaunchKernelGGL(adj_word_base_kernel, dim3((unsigned)nb), dim3(kScanBlock), 0, s, m);
        hipLaunchKernelGGL(adj_records_kernel, dim3(slotBlocks), dim3(kAdjBlock), 0, s, m, pairs, pair_rows);
    }
    if (rows_out) hipLaunchKernelGGL(adj_rows_kernel, dim3((rows + kAdjBlock - 1) / kAdjBlock), dim3(kAdjBlock), 0, s, m, rows, rows_out);
    if (counts) hipLaunchKernelGGL(adj_counts_kernel, dim3(1), dim3(1), 0, s, m, pair_rows, want_pairs ? 1 : 0, counts);
    return hipGetLastError();
}

size_t sieve_scratch_bytes(size_t npix, unsigned table_rows, unsigned pair_slots) {
    const size_t a = adj_layout(nullptr, npix, 0, pair_slots, false, false).bytes;
    return a + sieve_layout(nullptr, table_rows).bytes;
}

hipError_t launch_sieve(const uint8_t* klass, const unsigned* labels, const unsigned long long* table, unsigned table_rows, const unsigned* d_n, unsigned H,
                        unsigned W, unsigned min_pixels, unsigned max_rounds, void* scratch, unsigned pair_slots, uint8_t* klass_out, unsigned* rows_out,
                        unsigned* counts, hipStream_t s) {
    const size_t npix = (size_t)H * W;
    if (npix == 0 || npix >= (1ull << 31) || pair_slots < 64 || (pair_slots & (pair_slots - 1)) || max_rounds < 1 || max_rounds > 64)
        return hipErrorInvalidValue;
    const AdjMem m = adj_layout(scratch, npix, 0, pair_slots, false, false);
    const SieveMem v = sieve_layout((uint8_t*)scratch + m.bytes, table_rows);
    const AdjIn ain{labels, H, W, (W + 63) / 64, 0u, 0u, table_rows, d_n};
    const SieveIn in{klass, labels, table, d_n, table_rows, min_pixels, max_rounds, npix};
    hipError_t e = launch_adj_table<uint32_t>(ain, m, s);
    if (e == hipSuccess) e = hipMemsetAsync(v.sacc, 0, v.zero_bytes, s);
    if (e != hipSuccess) return e;
    const unsigned slotBlocks = (pair_slots + kAdjBlock - 1) / kAdjBlock;
    const unsigned regBlocks = table_rows ? (table_rows + kAdjBlock - 1) / kAdjBlock : 1u;
    hipLaunchKernelGGL(adj_slots_kernel, dim3(slotBlocks), dim3(kAdjBlock), 0, s, m);  // (no rows, no bitmap: PAIRS alone)
    hipLaunchKernelGGL(sieve_init_kernel, dim3(regBlocks), dim3(kAdjBlock), 0, s, in, m, v);
    for (unsigned t = 1; t <= max_rounds; t++) {
        hipLaunchKernelGGL(sieve_choose_kernel, dim3(slotBlocks), dim3(kAdjBlock), 0, s, m, v, t);
        hipLaunchKernelGGL(sieve_apply_kernel, dim3(regBlocks), dim3(kAdjBlock), 0, s, in, v, t);
    }
    if (klass_out) {
        const size_t blocks = (npix + kAdjBlock - 1) / kAdjBlock;
        hipLaunchKernelGGL(sieve_relabel_kernel, dim3((unsigned)blocks), dim3(kAdjBlock), 0, s, in, v, klass_out);
    }
    if (rows_out && table_rows) hipLaunchKernelGGL(sieve_rows_kernel, dim3(regBlocks), dim3(kAdjBlock), 0, s, in, v, rows_out);
    if (counts) hipLaunchKernelGGL(sieve_counts_kernel, dim3(1), dim3(1), 0, s, in, m, v, counts);
    return hipGetLastError();
}

}  // namespace infur
