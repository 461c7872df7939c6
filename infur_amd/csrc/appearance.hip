// appearance.hip -- Appearance: what every value of a plane looks like in the packed BGR frame (include/infur_hip.h).
// A reduction of the frame keyed by a byte or u32 plane: per value the pixel count, the three colour sums, their six second moments
// and the joint histogram on the top two bits of each channel, with its mode.  Three launches, no memset, nothing read back; the
// kernel boundaries are the only ordering and no workgroup waits for another:
//   1 clear    zeroes the table, the histogram (the caller's, or the scratch one when the caller wants none) and the eight count words
//   2 tiles    a workgroup owns a tile of 64 columns x kAppTileRows rows, a wave kAppWaveRows consecutive rows of it, a lane a
//              column.  Per wave-row: one ballot finds the runs of equal value (wave_scan.h); the lanes of a run that fall in the
//              same bin find each other by six more ballots and their leader adds the popcount; the nine sums are reduced inside
//              the wave, segmented by run, as three packed 64-bit words, and the last lane of a run adds them.  Where the whole
//              wave-row is one run the lanes only add into registers, and the wave reduces once when the value changes or its
//              rows end.  All adds go to a slot of the tile's value -> slot table in LDS; a run that finds no slot adds to global
//              memory itself.  At the end every (slot, non-zero word) is one global add: 64-bit into the table, 32-bit into the
//              histogram, and the three pixel classes one add each into the count words
//   3 finish   a wave per row, a lane per bin: PIXELS (the sum of the bins), MODE_BIN and MODE_COUNT by a cross-lane maximum of
//              (count << 6) | (63 - bin); VALUES from a count per workgroup; workgroup 0 writes STATUS
// The slot a value lands in and the order of the adds depend on timing and never reach an output: everything written is a sum of
// integers, which commute, or a maximum of them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr int kAppBlock = 256;
constexpr int kAppWaves = kAppBlock / 64;
constexpr int kAppWaveRows = 8;                           // consecutive rows of the tile one wave walks
constexpr int kAppTileRows = kAppWaves * kAppWaveRows;    // 32
constexpr int kAppTilePixels = 64 * kAppTileRows;         // 2048
constexpr int kAppSlots = 16;                             // distinct values a tile keeps in LDS; a power of two
constexpr int kAppSums = 9;                               // B G R BB GG RR BG BR GR: the table's words 1..9
constexpr unsigned kAppEmpty = 0xFFFFFFFFu;               // never a counted value: those are below table_rows
constexpr unsigned kAppFinishGrid = 2048;

// every 32-bit sum a slot holds in LDS is at most tile pixels x 255^2; a lane's registers hold kAppWaveRows x 255^2
static_assert((unsigned long long)kAppTilePixels * 65025ull < (1ull << 32), "a tile's sums must fit 32 bits");
static_assert((kAppSlots & (kAppSlots - 1)) == 0, "the slot probe wraps by a mask");

struct AppIn {
    const uint8_t* frame;
    const void* plane;
    unsigned H, W, tilesX;
    unsigned skip, skip_value, rows;
};

// where the adds of one call go: table and hist may be null (hist is the scratch one when the caller wants none and rows > 0)
struct AppOut {
    unsigned long long* table;
    unsigned* hist;
    unsigned* counts;  // the caller's eight words, or the scratch ones
};

// ---- 1 clear ----
__global__ void __launch_bounds__(kAppBlock) appearance_clear_kernel(unsigned* __restrict__ table, size_t table_words, unsigned* __restrict__ hist,
                                                                     size_t hist_words, unsigned* __restrict__ counts) {
    const size_t step = (size_t)gridDim.x * kAppBlock, t = (size_t)blockIdx.x * kAppBlock + threadIdx.x;
    for (size_t i = t; i < table_words; i += step) table[i] = 0u;
    for (size_t i = t; i < hist_words; i += step) hist[i] = 0u;
    if (t < (size_t)kAppearanceCountWords) counts[t] = 0u;
}

// ---- 2 tiles ----
// the tile's accumulators: a slot is a value, its nine sums and its 64 bins
struct AppTile {
    unsigned key[kAppSlots];
    unsigned sum[kAppSlots][kAppSums];
    unsigned bin[kAppSlots][kAppearanceBins];
    unsigned acc[3];  // COUNTED, SKIPPED, OUTSIDE
};

// -> the slot of value v, claimed if need be; -1 where kAppSlots other values hold every slot (they never leave: -1 stays -1)
__device__ __forceinline__ int app_slot(AppTile& t, const unsigned v) {
    unsigned s = (v * 0x9E3779B1u) >> 28;
    static_assert(kAppSlots == 16, "the hash keeps the top four bits");
    for (int it = 0; it < kAppSlots; it++) {
        unsigned old = t.key[s];
        if (old == kAppEmpty) old = atomicCAS(&t.key[s], kAppEmpty, v);
        if (old == kAppEmpty || old == v) return (int)s;
        s = (s + 1) & (kAppSlots - 1);
    }
    return -1;
}

// one of the nine sums of value v: to its slot, or straight to the table where the tile had no slot left
__device__ __forceinline__ void app_add_sum(AppTile& t, const AppOut& o, const int slot, const unsigned v, const int k, const unsigned n) {
    if (!n) return;
    if (slot >= 0)
        atomicAdd(&t.sum[slot][k], n);
    else
        (void)__hip_atomic_fetch_add(o.table + (size_t)v * kAppearanceWords + 1 + k, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The registers of a wave whose rows are one run each: a lane adds its own pixel and nothing crosses lanes until the value changes.
struct AppPending {
    unsigned v;
    int slot;
    bool any;
    unsigned s[kAppSums];
};

// (by whole waves) the pending sums reduced over the wave; lane k < 9 adds word k
__device__ __forceinline__ void app_flush_pending(AppTile& t, const AppOut& o, AppPending& p, const int lane) {
    if (!p.any) return;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < kAppSums; k++) {
        unsigned x = p.s[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
        mine = lane == k ? x : mine;
        p.s[k] = 0u;
    }
    if (lane < kAppSums) app_add_sum(t, o, p.slot, p.v, lane, mine);
    p.any = false;
}

template <class T>
__global__ void __launch_bounds__(kAppBlock) appearance_tiles_kernel(AppIn in, AppOut o) {
    __shared__ AppTile t;
    for (unsigned e = threadIdx.x; e < sizeof(AppTile) / 4; e += kAppBlock) ((unsigned*)&t)[e] = 0u;
    __syncthreads();  // (key is cleared to 0 with the rest and set to empty here: two passes keep the first a flat loop)
    if (threadIdx.x < kAppSlots) t.key[threadIdx.x] = kAppEmpty;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tx = blockIdx.x % in.tilesX, ty = blockIdx.x / in.tilesX;
    const unsigned x = tx * 64 + lane;
    const unsigned y0 = ty * kAppTileRows + wave * kAppWaveRows;
    const bool sums = o.table != nullptr;
    unsigned n_counted = 0, n_skipped = 0, n_outside = 0;  // the same in every lane
    AppPending pend;
    pend.v = kAppEmpty, pend.slot = -1, pend.any = false;
#pragma unroll
    for (int k = 0; k < kAppSums; k++) pend.s[k] = 0u;

    for (int j = 0; j < kAppWaveRows; j++) {
        const unsigned y = y0 + j;
        if (y >= in.H) break;  // (by whole waves)
        const bool live = x < in.W;
        const size_t at = (size_t)y * in.W + x;
        unsigned v = kAppEmpty, b = 0, g = 0, r = 0;
        if (live) {
            v = (unsigned)((const T*)in.plane)[at];
            const uint8_t* px = in.frame + 3 * at;  // bytes 3 at .. 3 at + 2 of H * W * 3: the last pixel ends the frame
            b = px[0], g = px[1], r = px[2];
        }
        const bool counted = live && !(in.skip && v == in.skip_value);
        const bool inside = counted && v < in.rows;
        n_counted += (unsigned)__popcll(__ballot(inside));
        n_skipped += (unsigned)__popcll(__ballot(live && !counted));
        n_outside += (unsigned)__popcll(__ballot(counted && !inside));

        bool cont;
        const uint64_t starts = wave_run_starts(v, inside, &cont);
        const bool head = inside && !cont;
        const uint64_t heads = __ballot(head), in_mask = __ballot(inside);
        if (!heads) continue;  // nothing of this row is counted in a row
        const bool one_run = (heads & (heads - 1)) == 0;  // the common case on label planes

        // the slot of every run: the pending one where the row goes on with the pending value, else the head lane looks it up
        const unsigned s0 = run_start(starts, lane);
        int slot = -1;
        uint64_t run_mask;
        if (one_run) {
            const unsigned hv = __shfl(v, __builtin_ctzll(heads), 64);
            if (pend.v != hv) {
                app_flush_pending(t, o, pend, lane);
                if (head) slot = app_slot(t, v);
                pend.v = hv;
                pend.slot = __shfl(slot, __builtin_ctzll(heads), 64);
            }
            slot = pend.slot;
            run_mask = in_mask;
        } else {
            app_flush_pending(t, o, pend, lane);
            pend.v = kAppEmpty;
            if (head) slot = app_slot(t, v);
            slot = __shfl(slot, (int)s0, 64);
            const unsigned len = run_length(starts, (int)s0);
            run_mask = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << s0;
        }

        // the histogram: the lanes of one run in one bin elect their lowest lane, which adds their number
        const unsigned bin = ((r >> 6) << 4) | ((g >> 6) << 2) | (b >> 6);
        uint64_t peers = run_mask;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint64_t set = __ballot(inside && ((bin >> k) & 1u));
            peers &= ((bin >> k) & 1u) ? set : ~set;
        }
        if (inside && (peers & ((1ull << lane) - 1ull)) == 0) {
            const unsigned n = (unsigned)__popcll(peers);
            if (slot >= 0)
                atomicAdd(&t.bin[slot][bin], n);
            else
                (void)__hip_atomic_fetch_add(o.hist + (size_t)v * kAppearanceBins + bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!sums) continue;

        if (one_run) {  // registers only: at most kAppWaveRows x 255^2 a lane
            if (inside) {
                pend.s[0] += b, pend.s[1] += g, pend.s[2] += r;
                pend.s[3] += b * b, pend.s[4] += g * g, pend.s[5] += r * r;
                pend.s[6] += b * g, pend.s[7] += b * r, pend.s[8] += g * r;
            }
            pend.any = true;
            continue;
        }
        // Several runs: an inclusive scan along the wave that does not cross a run start.  A run has at most 64 lanes, so a sum of
        // bytes fits 14 bits and a sum of products 22: three words of 22 + 22 + 14 bits carry the nine sums.
        unsigned long long p0 = 0, p1 = 0, p2 = 0;
        if (inside) {
            p0 = (unsigned long long)(b * b) | ((unsigned long long)(g * g) << 22) | ((unsigned long long)b << 44);
            p1 = (unsigned long long)(r * r) | ((unsigned long long)(b * g) << 22) | ((unsigned long long)g << 44);
            p2 = (unsigned long long)(b * r) | ((unsigned long long)(g * r) << 22) | ((unsigned long long)r << 44);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long q0 = __shfl_up(p0, d, 64), q1 = __shfl_up(p1, d, 64), q2 = __shfl_up(p2, d, 64);
            if (lane >= (int)s0 + d) p0 += q0, p1 += q1, p2 += q2;
        }
        const bool tail = inside && (lane == 63 || ((starts >> (lane + 1)) & 1ull));
        if (tail) {
            constexpr unsigned m22 = (1u << 22) - 1u, m14 = (1u << 14) - 1u;
            app_add_sum(t, o, slot, v, 0, (unsigned)(p0 >> 44) & m14);
            app_add_sum(t, o, slot, v, 1, (unsigned)(p1 >> 44) & m14);
            app_add_sum(t, o, slot, v, 2, (unsigned)(p2 >> 44) & m14);
            app_add_sum(t, o, slot, v, 3, (unsigned)p0 & m22);
            app_add_sum(t, o, slot, v, 4, (unsigned)(p0 >> 22) & m22);
            app_add_sum(t, o, slot, v, 5, (unsigned)p1 & m22);
            app_add_sum(t, o, slot, v, 6, (unsigned)(p1 >> 22) & m22);
            app_add_sum(t, o, slot, v, 7, (unsigned)p2 & m22);
            app_add_sum(t, o, slot, v, 8, (unsigned)(p2 >> 22) & m22);
        }
    }
    app_flush_pending(t, o, pend, lane);
    if (lane == 0) {
        if (n_counted) atomicAdd(&t.acc[0], n_counted);
        if (n_skipped) atomicAdd(&t.acc[1], n_skipped);
        if (n_outside) atomicAdd(&t.acc[2], n_outside);
    }
    __syncthreads();

    // the flush: one global add per (slot, non-zero word)
    if (threadIdx.x < 3 && t.acc[threadIdx.x]) atomicAdd(&o.counts[threadIdx.x], t.acc[threadIdx.x]);
    constexpr unsigned per_slot = kAppSums + kAppearanceBins;
    for (unsigned e = threadIdx.x; e < kAppSlots * per_slot; e += kAppBlock) {
        const unsigned s = e / per_slot, k = e % per_slot;
        const unsigned v = t.key[s];
        if (v == kAppEmpty) continue;
        if (k < (unsigned)kAppSums) {
            const unsigned n = t.sum[s][k];
            if (n) (void)__hip_atomic_fetch_add(o.table + (size_t)v * kAppearanceWords + 1 + k, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned n = t.bin[s][k - kAppSums];
            if (n) (void)__hip_atomic_fetch_add(o.hist + (size_t)v * kAppearanceBins + (k - kAppSums), n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- 3 finish ----
// One wave per row, a lane per bin.  The maximum of (count << 6) | (63 - bin) is the largest count at the smallest bin.
__global__ void __launch_bounds__(kAppBlock) appearance_finish_kernel(AppOut o, unsigned rows) {
    __shared__ unsigned values[kAppWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;  // rows of this wave with pixels; the same in every lane
    for (size_t row = (size_t)blockIdx.x * kAppWaves + wave; row < rows; row += (size_t)gridDim.x * kAppWaves) {
        const unsigned n = o.hist[row * kAppearanceBins + lane];
        unsigned pixels = n;
        unsigned long long best = ((unsigned long long)n << 6) | (unsigned)(63 - lane);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            pixels += __shfl_xor(pixels, d, 64);
            const unsigned long long other = __shfl_xor(best, d, 64);
            best = other > best ? other : best;
        }
        mine += pixels ? 1u : 0u;
        if (o.table && lane == 0) {
            unsigned long long* out = o.table + row * kAppearanceWords;
            out[0] = pixels;
            out[10] = pixels ? 63u - (unsigned)(best & 63ull) : 0u;
            out[11] = best >> 6;
        }
    }
    if (lane == 0) values[wave] = mine;
    __syncthreads();
    if (threadIdx.x) return;
    unsigned all = 0;
    for (int k = 0; k < kAppWaves; k++) all += values[k];
    if (all) atomicAdd(&o.counts[3], all);
    if (blockIdx.x == 0) o.counts[7] = o.counts[0] ? 0u : kAppearanceNothing;  // COUNTED is final: the tiles launch is over
}

}  // namespace

size_t appearance_scratch_bytes(unsigned rows, bool own_hist) { return 256 + (own_hist ? 0 : (size_t)rows * kAppearanceBins * 4); }

hipError_t launch_appearance(const uint8_t* frame, const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, void* scratch,
                             unsigned long long* table, unsigned rows, unsigned* hist, unsigned* counts, hipStream_t s) {
    if (!H || !W || H > kAppearanceMaxSide || W > kAppearanceMaxSide || (elem_bytes != 1 && elem_bytes != 4)) return hipErrorInvalidValue;
    AppOut o{table, hist ? hist : (unsigned*)((uint8_t*)scratch + 256), counts ? counts : (unsigned*)scratch};
    const size_t table_words = table ? (size_t)rows * kAppearanceWords * 2 : 0, hist_words = (size_t)rows * kAppearanceBins;
    const size_t most = table_words > hist_words ? table_words : hist_words;
    size_t blocks = (most + kAppBlock - 1) / kAppBlock;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(appearance_clear_kernel, dim3((unsigned)blocks), dim3(kAppBlock), 0, s, (unsigned*)table, table_words, o.hist, hist_words, o.counts);
    const unsigned tilesX = (W + 63) / 64, tilesY = (H + kAppTileRows - 1) / kAppTileRows;  // at most 512 x 1024
    const AppIn in{frame, plane, H, W, tilesX, skip ? 1u : 0u, skip_value, rows};
    if (elem_bytes == 1)
        hipLaunchKernelGGL(appearance_tiles_kernel<uint8_t>, dim3(tilesX * tilesY), dim3(kAppBlock), 0, s, in, o);
    else
        hipLaunchKernelGGL(appearance_tiles_kernel<uint32_t>, dim3(tilesX * tilesY), dim3(kAppBlock), 0, s, in, o);
    size_t fin = ((size_t)rows + kAppWaves - 1) / kAppWaves;
    fin = fin < 1 ? 1 : (fin > kAppFinishGrid ? kAppFinishGrid : fin);
    hipLaunchKernelGGL(appearance_finish_kernel, dim3((unsigned)fin), dim3(kAppBlock), 0, s, o, rows);
    return hipGetLastError();
}

}  // namespace infur
