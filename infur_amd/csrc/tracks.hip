// tracks.hip -- Tracks: region identities carried from frame to frame (include/infur_hip.h).  The fourth decode
// stage behind Regions: from the current frame's label plane, region table and count, and the frame the tracker remembers, a
// track id per region.  Separate launches -- the kernel boundaries are the only ordering, no workgroup ever waits for another:
//   1 begin    the step's scalars (tracked regions T, fresh frame or not), best[] and claim[] cleared as far as they are read
//   2 runs     R = the number of runs of equal (current, remembered) label pairs along wave-rows (wave_run_starts), one
//              atomic per workgroup.  R bounds the distinct pairs; 2 R > pair_slots is the overflow rule
//   3 insert   the head lane of each run: 64-bit CAS of (c << 32) | p into an open-addressing table, then one non-returning
//              add of the run length.  Inside this kernel the table is touched by atomics only
//   4 choose   one lane per slot: candidates (same class, overlap >= min_overlap) -> atomicMax into best[c]
//   5 keep     one lane per current region: atomicMax into claim[best p]
//   6 assign   new-track flags, their exclusive prefix sum in region order (flag_block_sum, scan_block_sums, flag_rank), ids,
//              table rows, summary
//   7 plane    label plane -> track plane (dword stores)
//   8 save     the per-region words the next step needs (the label plane itself is a device-to-device copy)
// The wave-row and the flag scan are wave_scan.h's.  The slot a pair lands in depends on timing; everything read from the table
// goes through sums and maxima, which commute, so the bytes written do not depend on the order in which atomics arrive.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_scan.h"

namespace infur {

namespace {

constexpr unsigned kNone = 0xFFFFFFFFu;
constexpr unsigned long long kEmpty = ~0ull;
constexpr unsigned long long kHi = 0xFFFFFFFF00000000ull;

__device__ __forceinline__ unsigned trk_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}

__global__ void __launch_bounds__(256) tracks_begin_kernel(TrkMem m, unsigned H, unsigned W, unsigned rows, const unsigned* __restrict__ d_n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    TrkState* st = m.st;
    const size_t N = (size_t)H * W;
    const unsigned n = d_n[0] < N ? d_n[0] : (unsigned)N;  // there are at most H * W regions, whatever the word says
    const unsigned nrows = n < rows ? n : rows, T = nrows < m.M ? nrows : m.M;
    // best[] is read below T, claim[] below the remembered frame's count (pT is written by the save launch only)
    if (i < T || i < st->pT) m.best[i] = m.claim[i] = 0ull;
    if (i == 0) {
        st->nrows = nrows;
        st->T = T;
        st->trunc = T < d_n[0];
        st->fresh = !(st->valid && st->ph == H && st->pw == W);
        st->R = 0;
    }
}

// -> the pair key of this lane's pixel of the wave-row, kEmpty when either label is untracked (or the lane is outside the image,
// or nothing is remembered); *head: the lane starts a run of a tracked pair.
__device__ __forceinline__ unsigned long long trk_pair(const TrkMem& m, const unsigned* __restrict__ labels, unsigned H, unsigned W, unsigned tilesX,
                                                       bool* head, uint64_t* starts) {
    const WaveRow r = wave_row(H, W, tilesX);
    const TrkState* st = m.st;
    unsigned long long key = kEmpty;
    if (r.live && !st->fresh) {
        const unsigned c = labels[r.at], p = m.prev[r.at];
        if (c < st->T && p < st->pT) key = ((unsigned long long)c << 32) | p;
    }
    bool cont;
    *starts = wave_run_starts(key, key != kEmpty, &cont);
    *head = key != kEmpty && !cont;
    return key;
}

__global__ void __launch_bounds__(256) tracks_runs_kernel(TrkMem m, const unsigned* __restrict__ labels, unsigned H, unsigned W, unsigned tilesX) {
    __shared__ unsigned wsum[4];
    bool head;
    uint64_t starts;
    (void)trk_pair(m, labels, H, W, tilesX, &head, &starts);
    const unsigned s = flag_block_sum<256>(head, wsum);
    if (threadIdx.x == 0 && s) atomicAdd(&m.st->R, s);
}

__device__ __forceinline__ bool trk_overflow(const TrkMem& m) { return 2ull * m.st->R > (unsigned long long)m.slots; }

__global__ void __launch_bounds__(256) tracks_insert_kernel(TrkMem m, const unsigned* __restrict__ labels, unsigned H, unsigned W, unsigned tilesX) {
    if (trk_overflow(m)) return;
    bool head;
    uint64_t starts;
    const unsigned long long key = trk_pair(m, labels, H, W, tilesX, &head, &starts);
    if (!head) return;
    const unsigned n = run_length(starts, threadIdx.x & 63);
    const unsigned mask = m.slots - 1;
    unsigned s = trk_hash(key, mask);
    for (unsigned it = 0; it < m.slots; it++) {  // at most half the slots are ever taken: the loop ends long before its bound
        unsigned long long old = kEmpty;
        __hip_atomic_compare_exchange_strong(m.keys + s, &old, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kEmpty || old == key) {
            (void)__hip_atomic_fetch_add(m.cnts + s, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        s = (s + 1) & mask;
    }
}

__global__ void __launch_bounds__(256) tracks_choose_kernel(TrkMem m, const unsigned long long* __restrict__ table, unsigned min_overlap) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= m.slots) return;
    const unsigned long long key = m.keys[s];
    if (key == kEmpty) return;
    const unsigned c = (unsigned)(key >> 32), p = (unsigned)key, ov = m.cnts[s];
    if (ov < (min_overlap ? min_overlap : 1u)) return;
    if ((unsigned)table[(size_t)c * kRegWords + 8] != m.pclass[p]) return;
    atomicMax(m.best + c, ((unsigned long long)ov << 32) | (kNone - p));
}

__global__ void __launch_bounds__(256) tracks_keep_kernel(TrkMem m) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= m.st->T) return;
    const unsigned long long b = m.best[c];
    if (!b) return;
    atomicMax(m.claim + (kNone - (unsigned)b), (b & kHi) | (kNone - (unsigned)c));
}

// region i < T starts a new track unless the remembered region it chose kept it
__device__ __forceinline__ bool trk_new(const TrkMem& m, const size_t i) {
    const unsigned long long b = m.best[i];
    return !b || m.claim[kNone - (unsigned)b] != ((b & kHi) | (kNone - (unsigned)i));
}

__global__ void __launch_bounds__(kScanBlock) tracks_scan_sums_kernel(TrkMem m) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(i < m.st->T && trk_new(m, i), wsum);
    if (threadIdx.x == 0) m.partial[blockIdx.x] = s;
}

// one workgroup: partial[] -> its exclusive prefix sums in place; then the step's decisions: ids exhausted or not, next_id, summary
__global__ void __launch_bounds__(kScanBlock) tracks_scan_partials_kernel(TrkMem m, size_t NB, unsigned* __restrict__ summary) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned fresh_n = scan_block_sums(m.partial, NB, wsum);
    if (threadIdx.x == 0) {
        TrkState* st = m.st;
        const unsigned remembered = st->fresh ? 0u : st->pT, cont = st->T - fresh_n;
        const bool exhausted = (unsigned long long)st->next_id + fresh_n > 0xFFFFFFFEull;
        st->exhausted = exhausted;
        st->base = st->next_id;
        if (!exhausted) st->next_id += fresh_n;
        if (summary) {
            summary[0] = (st->trunc ? kTrkTruncated : 0u) | (trk_overflow(m) ? kTrkOverflow : 0u) | (exhausted ? kTrkExhausted : 0u);
            summary[1] = exhausted ? 0u : cont;
            summary[2] = exhausted ? 0u : fresh_n;
            summary[3] = exhausted ? remembered : remembered - cont;
        }
    }
}

// rows [0, min(n, rows)) of the caller's outputs; the tracker's own copy of id / age / birth for rows below T
__global__ void __launch_bounds__(kScanBlock) tracks_apply_kernel(TrkMem m, unsigned* __restrict__ track_of_region, unsigned long long* __restrict__ ttab) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const TrkState* st = m.st;
    const unsigned T = st->T;
    const bool fresh = i < T && trk_new(m, i);
    // (the rank within the workgroup; partial[] is read below, by new tracks only: it has no word for a workgroup beyond T)
    const unsigned rank = flag_rank(fresh, 0u, wsum);
    if (i >= st->nrows) return;
    unsigned long long row[kTrkWords] = {kNone, 0ull, 0ull, kNone, 0ull, 0ull, 0ull, 0ull};
    if (i < T) {
        if (st->exhausted) {
            m.ctrack[i] = kNone;
            m.cage[i] = m.cborn[i] = 0u;
        } else if (fresh) {
            row[0] = m.ctrack[i] = st->base + m.partial[blockIdx.x] + rank;
            row[1] = m.cage[i] = 1u;
            row[2] = m.cborn[i] = st->frame;
        } else {
            const unsigned long long bc = m.best[i];
            const unsigned p = kNone - (unsigned)bc;
            row[0] = m.ctrack[i] = m.ptrack[p];
            row[1] = m.cage[i] = m.page[p] + 1u;
            row[2] = m.cborn[i] = m.pborn[p];
            row[3] = p;
            row[4] = bc >> 32;
            row[5] = m.ppix[p];
            row[6] = m.psx[p];
            row[7] = m.psy[p];
        }
    }
    if (track_of_region) track_of_region[i] = (unsigned)row[0];
    if (ttab)
#pragma unroll
        for (int k = 0; k < kTrkWords; k++) ttab[i * kTrkWords + k] = row[k];
}

__global__ void __launch_bounds__(256) tracks_plane_kernel(TrkMem m, const unsigned* __restrict__ labels, size_t N, unsigned* __restrict__ plane) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned l = labels[i];
    plane[i] = l < m.st->T ? m.ctrack[l] : kNone;
}

// what the next step needs of this frame (after every reader of the remembered arrays); an exhausted step remembers nothing
__global__ void __launch_bounds__(256) tracks_save_kernel(TrkMem m, const unsigned long long* __restrict__ table, unsigned H, unsigned W) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    TrkState* st = m.st;
    const unsigned T = st->T;
    if (i < T) {
        const unsigned long long* row = table + i * kRegWords;
        m.ppix[i] = row[0];
        m.psx[i] = row[1];
        m.psy[i] = row[2];
        m.pclass[i] = (unsigned)row[8];
        m.ptrack[i] = m.ctrack[i];
        m.page[i] = m.cage[i];
        m.pborn[i] = m.cborn[i];
    }
    if (i == 0) {
        st->valid = !st->exhausted;
        st->ph = H;
        st->pw = W;
        st->pT = T;
        st->frame += 1u;
    }
}

__global__ void tracks_forget_kernel(TrkState* st, int step, int set_id, unsigned first_id, unsigned* __restrict__ summary) {
    st->valid = 0u;
    if (step) st->frame += 1u;
    if (set_id) st->next_id = first_id;
    if (summary) summary[0] = summary[1] = summary[2] = summary[3] = 0u;
}

}  // namespace

hipError_t launch_tracks_forget(TrkState* st, int step, int set_id, unsigned first_id, unsigned* summary, hipStream_t s) {
    hipLaunchKernelGGL(tracks_forget_kernel, dim3(1), dim3(1), 0, s, st, step, set_id, first_id, summary);
    return hipGetLastError();
}

hipError_t launch_tracks(const TrkMem& m, const unsigned* labels, const unsigned long long* table, unsigned rows, const unsigned* d_n, unsigned H,
                         unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane, unsigned long long* track_table,
                         unsigned* summary, hipStream_t s) {
    const size_t N = (size_t)H * W;
    const unsigned tilesX = (W + 63) / 64;
    const size_t rowBlocks = ((size_t)tilesX * H + 3) / 4;
    if (rowBlocks > 0x7FFFFFFFull || (N + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const size_t capRows = rows < N ? rows : N;               // >= min(n, rows): there are at most N regions
    const size_t cap = capRows < m.M ? capRows : (size_t)m.M;  // >= T
    const size_t NB = scan_blocks(cap);
    hipError_t e = hipMemsetAsync(m.keys, 0xFF, (size_t)m.slots * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(m.cnts, 0, (size_t)m.slots * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tracks_begin_kernel, dim3((unsigned)((m.M + 255) / 256)), dim3(256), 0, s, m, H, W, rows, d_n);
    hipLaunchKernelGGL(tracks_runs_kernel, dim3((unsigned)rowBlocks), dim3(256), 0, s, m, labels, H, W, tilesX);
    hipLaunchKernelGGL(tracks_insert_kernel, dim3((unsigned)rowBlocks), dim3(256), 0, s, m, labels, H, W, tilesX);
    hipLaunchKernelGGL(tracks_choose_kernel, dim3((m.slots + 255) / 256), dim3(256), 0, s, m, table, min_overlap);
    if (cap) hipLaunchKernelGGL(tracks_keep_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, m);
    if (NB) hipLaunchKernelGGL(tracks_scan_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, m);
    hipLaunchKernelGGL(tracks_scan_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, m, NB, summary);
    if (capRows)
        hipLaunchKernelGGL(tracks_apply_kernel, dim3((unsigned)scan_blocks(capRows)), dim3(kScanBlock), 0, s, m, track_of_region,
                           track_table);
    if (track_plane) hipLaunchKernelGGL(tracks_plane_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, m, labels, N, track_plane);
    e = hipMemcpyAsync(m.prev, labels, N * 4, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tracks_save_kernel, dim3((unsigned)(cap ? (cap + 255) / 256 : 1)), dim3(256), 0, s, m, table, H, W);
    return hipGetLastError();
}

}  // namespace infur
