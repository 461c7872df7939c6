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
// A tracker with memory (infur_tracker_set_memory) adds launches between 5 and 6 and before 8: "Memory", further down.
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

// ---------------------------------------------------------------------------------------------------------------------------
// Memory (DESIGN 4c'): a gallery of lost tracks.  A tracker with memory runs the launches above up to keep, then
//   clear          rclaim[] = 0, one lane per gallery row
//   revive-choose  one wave per tracked region; an orphan's 64 lanes stride over the gallery, a running maximum of
//                  (score << 32) | (0xFFFFFFFF - g) per lane, a cross-lane maximum, one store by lane 0: no atomic
//   revive-keep    one lane per region: atomicMax of (score << 32) | (0xFFFFFFFF - c) into rclaim[g]
//   assign         as above with the flag "orphan and not revived"; a second flag sum counts the revived
//   gallery        one flag scan over [gallery entries | remembered regions], flags "survives" and "ended", into the other
//                  gallery buffer; the total gives the entries to drop from the front
//   save           also the remembered boxes; its lane 0 flips the gallery buffers
// A step that starts afresh reads the gallery as empty.  Kernel boundaries are the only ordering.
struct LostBox {
    unsigned x0, y0, x1, y1;
};

__device__ __forceinline__ unsigned gal_held(const TrkMem& m, const TrkGal& g) { return m.st->fresh ? 0u : g.gs->held; }
// (an entry's SEEN is below the frame counter of every later step: the gap is at least 1)
__device__ __forceinline__ unsigned gal_gap(const TrkMem& m, const TrkLost& b, const unsigned e) { return m.st->frame - b.seen[e] - 1u; }

// c < T is revived: it chose an entry and that entry kept it
__device__ __forceinline__ bool trk_revived(const TrkGal& g, const size_t c) {
    const unsigned long long b = g.rbest[c];
    return b && g.rclaim[kNone - (unsigned)b] == ((b & kHi) | (kNone - (unsigned)c));
}

__global__ void __launch_bounds__(256) tracks_mem_clear_kernel(TrkGal g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < g.G) g.rclaim[i] = 0ull;
}

__global__ void __launch_bounds__(256) tracks_revive_choose_kernel(TrkMem m, TrkGal g, const unsigned long long* __restrict__ table, unsigned H, unsigned W) {
    const size_t c = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    if (c >= m.st->T) return;
    if (!trk_new(m, c)) {
        if (lane == 0) g.rbest[c] = 0ull;
        return;
    }
    const unsigned long long* row = table + c * kRegWords;
    const unsigned cx0 = (unsigned)row[4], cy0 = (unsigned)row[5], cx1 = (unsigned)row[6], cy1 = (unsigned)row[7], klass = (unsigned)row[8];
    const unsigned held = gal_held(m, g);
    const TrkLost& b = g.buf[g.gs->cur];
    unsigned long long best = 0ull;
    for (unsigned e = lane; e < held; e += 64) {
        const unsigned gap = gal_gap(m, b, e);
        if (gap > g.max_lost || b.klass[e] != klass) continue;
        const unsigned long long far = (unsigned long long)g.reach * gap;
        const unsigned grow = far > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)far;
        const unsigned ex0 = b.x0[e] > grow ? b.x0[e] - grow : 0u, ey0 = b.y0[e] > grow ? b.y0[e] - grow : 0u;
        const unsigned long long fx1 = (unsigned long long)b.x1[e] + grow, fy1 = (unsigned long long)b.y1[e] + grow;
        const unsigned ex1 = fx1 < W - 1 ? (unsigned)fx1 : W - 1, ey1 = fy1 < H - 1 ? (unsigned)fy1 : H - 1;
        const unsigned ix0 = cx0 > ex0 ? cx0 : ex0, iy0 = cy0 > ey0 ? cy0 : ey0, ix1 = cx1 < ex1 ? cx1 : ex1, iy1 = cy1 < ey1 ? cy1 : ey1;
        if (ix0 > ix1 || iy0 > iy1) continue;
        const unsigned long long v = ((unsigned long long)((ix1 - ix0 + 1u) * (iy1 - iy0 + 1u)) << 32) | (kNone - e);  // at most H * W: 32 bits
        best = v > best ? v : best;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) g.rbest[c] = best;
}

__global__ void __launch_bounds__(256) tracks_revive_keep_kernel(TrkMem m, TrkGal g) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= m.st->T) return;
    const unsigned long long b = g.rbest[c];
    if (!b) return;
    atomicMax(g.rclaim + (kNone - (unsigned)b), (b & kHi) | (kNone - (unsigned)c));
}

__global__ void __launch_bounds__(kScanBlock) tracks_mem_scan_sums_kernel(TrkMem m, TrkGal g) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const bool orphan = i < m.st->T && trk_new(m, i), revived = orphan && trk_revived(g, i);
    const unsigned s = flag_block_sum(orphan && !revived, wsum);
    __syncthreads();
    const unsigned r = flag_block_sum(revived, wsum);
    if (threadIdx.x == 0) {
        m.partial[blockIdx.x] = s;
        g.rpart[blockIdx.x] = r;
    }
}

// the decisions of a step with memory: NEW counts the new ids only, CONTINUED + NEW + REVIVED = T
__global__ void __launch_bounds__(kScanBlock) tracks_mem_scan_partials_kernel(TrkMem m, TrkGal g, size_t NB, unsigned* __restrict__ summary) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned fresh_n = scan_block_sums(m.partial, NB, wsum);
    const unsigned rev = scan_block_sums(g.rpart, NB, wsum);
    if (threadIdx.x == 0) {
        TrkState* st = m.st;
        const unsigned remembered = st->fresh ? 0u : st->pT, cont = st->T - fresh_n - rev;
        const bool exhausted = (unsigned long long)st->next_id + fresh_n > 0xFFFFFFFEull;
        st->exhausted = exhausted;
        st->base = st->next_id;
        if (!exhausted) st->next_id += fresh_n;
        g.gs->revived = exhausted ? 0u : rev;
        g.gs->ended = exhausted ? 0u : remembered - cont;
        if (summary) {
            summary[0] = (st->trunc ? kTrkTruncated : 0u) | (trk_overflow(m) ? kTrkOverflow : 0u) | (exhausted ? kTrkExhausted : 0u);
            summary[1] = exhausted ? 0u : cont;
            summary[2] = exhausted ? 0u : fresh_n;
            summary[3] = exhausted ? remembered : remembered - cont;
        }
    }
}

__global__ void __launch_bounds__(kScanBlock) tracks_mem_apply_kernel(TrkMem m, TrkGal g, unsigned* __restrict__ track_of_region,
                                                                      unsigned long long* __restrict__ ttab) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const TrkState* st = m.st;
    const unsigned T = st->T;
    const bool orphan = i < T && trk_new(m, i), revived = orphan && trk_revived(g, i), fresh = orphan && !revived;
    const unsigned rank = flag_rank(fresh, 0u, wsum);
    if (i >= st->nrows) return;
    unsigned long long row[kTrkWords] = {kNone, 0ull, 0ull, kNone, 0ull, 0ull, 0ull, 0ull};
    if (i < T) {
        unsigned gap = 0u;
        if (st->exhausted) {
            m.ctrack[i] = kNone;
            m.cage[i] = m.cborn[i] = 0u;
        } else if (fresh) {
            row[0] = m.ctrack[i] = st->base + m.partial[blockIdx.x] + rank;
            row[1] = m.cage[i] = 1u;
            row[2] = m.cborn[i] = st->frame;
        } else if (revived) {
            const TrkLost& b = g.buf[g.gs->cur];
            const unsigned e = kNone - (unsigned)g.rbest[i];
            row[0] = m.ctrack[i] = b.id[e];
            row[1] = m.cage[i] = b.age[e] + 1u;
            row[2] = m.cborn[i] = b.born[e];
            row[5] = b.pix[e];
            row[6] = b.sx[e];
            row[7] = b.sy[e];
            gap = gal_gap(m, b, e);
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
        g.cgap[i] = gap;
    }
    if (track_of_region) track_of_region[i] = (unsigned)row[0];
    if (ttab)
#pragma unroll
        for (int k = 0; k < kTrkWords; k++) ttab[i * kTrkWords + k] = row[k];
}

// element i of the gallery scan: i < G is entry i ("survives": held, not expired, not revived), i >= G is the remembered region
// i - G ("ended": no current region inherited it; none on a step that started afresh).  An exhausted step keeps nothing.
__device__ __forceinline__ bool gal_flag(const TrkMem& m, const TrkGal& g, const size_t i) {
    const TrkState* st = m.st;
    if (st->exhausted || st->fresh) return false;
    if (i < g.G) return i < g.gs->held && gal_gap(m, g.buf[g.gs->cur], (unsigned)i) <= g.max_lost && !g.rclaim[i];
    const size_t p = i - g.G;
    return p < st->pT && !m.claim[p];
}

__global__ void __launch_bounds__(kScanBlock) tracks_gallery_sums_kernel(TrkMem m, TrkGal g) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const unsigned s = flag_block_sum(gal_flag(m, g, i), wsum);
    if (threadIdx.x == 0) g.gpart[blockIdx.x] = s;
}

// one workgroup: the gallery's block sums -> their prefix sums; the entries to drop from the front, the memory summary
__global__ void __launch_bounds__(kScanBlock) tracks_gallery_partials_kernel(TrkMem m, TrkGal g, size_t NB, unsigned* __restrict__ summary) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const unsigned total = scan_block_sums(g.gpart, NB, wsum);
    if (threadIdx.x == 0) {
        TrkGalState* gs = g.gs;
        const bool none = m.st->exhausted;
        const unsigned lost = gs->ended, survive = total - lost, drop = total > g.G ? total - g.G : 0u;
        gs->drop = drop;
        gs->new_held = total - drop;
        gs->sum[0] = gs->revived;
        gs->sum[1] = lost;
        gs->sum[2] = none ? 0u : gal_held(m, g) - gs->revived - survive;
        gs->sum[3] = total - drop;
        if (drop && summary) summary[0] |= kTrkGalleryFull;
    }
}

__global__ void __launch_bounds__(kScanBlock) tracks_gallery_apply_kernel(TrkMem m, TrkGal g) {
    __shared__ unsigned wsum[kScanBlock / 64];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const bool flag = gal_flag(m, g, i);
    const unsigned rank = flag_rank(flag, g.gpart[blockIdx.x], wsum);
    const TrkGalState* gs = g.gs;
    if (!flag || rank < gs->drop) return;
    const unsigned d = rank - gs->drop;  // < G
    const TrkLost &from = g.buf[gs->cur], &to = g.buf[gs->cur ^ 1u];
    if (i < g.G) {
        to.id[d] = from.id[i], to.age[d] = from.age[i], to.born[d] = from.born[i], to.klass[d] = from.klass[i];
        to.pix[d] = from.pix[i], to.sx[d] = from.sx[i], to.sy[d] = from.sy[i];
        to.x0[d] = from.x0[i], to.y0[d] = from.y0[i], to.x1[d] = from.x1[i], to.y1[d] = from.y1[i];
        to.seen[d] = from.seen[i];
    } else {
        const size_t p = i - g.G;
        to.id[d] = m.ptrack[p], to.age[d] = m.page[p], to.born[d] = m.pborn[p], to.klass[d] = m.pclass[p];
        to.pix[d] = m.ppix[p], to.sx[d] = m.psx[p], to.sy[d] = m.psy[p];
        to.x0[d] = g.px0[p], to.y0[d] = g.py0[p], to.x1[d] = g.px1[p], to.y1[d] = g.py1[p];
        to.seen[d] = m.st->frame - 1u;
    }
}

__global__ void __launch_bounds__(256) tracks_mem_save_kernel(TrkMem m, TrkGal g, const unsigned long long* __restrict__ table, unsigned H, unsigned W) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    TrkState* st = m.st;
    const unsigned T = st->T;
    if (i < T) {
        const unsigned long long* row = table + i * kRegWords;
        m.ppix[i] = row[0];
        m.psx[i] = row[1];
        m.psy[i] = row[2];
        g.px0[i] = (unsigned)row[4];
        g.py0[i] = (unsigned)row[5];
        g.px1[i] = (unsigned)row[6];
        g.py1[i] = (unsigned)row[7];
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
        TrkGalState* gs = g.gs;
        gs->cur ^= 1u;
        gs->held = gs->new_held;
        gs->T = T;
    }
}

__global__ void tracks_mem_forget_kernel(TrkGalState* gs) {
    gs->held = gs->T = 0u;
    gs->sum[0] = gs->sum[1] = gs->sum[2] = gs->sum[3] = 0u;
}

__global__ void __launch_bounds__(256) tracks_mem_read_kernel(TrkGal g, unsigned* __restrict__ gap_of_region, unsigned rows, unsigned* __restrict__ memory_summary,
                                                              unsigned long long* __restrict__ lost, unsigned lost_rows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const TrkGalState* gs = g.gs;
    if (gap_of_region && i < rows) gap_of_region[i] = i < gs->T ? g.cgap[i] : 0u;
    if (memory_summary && i < 4) memory_summary[i] = gs->sum[i];
    if (lost && i < lost_rows && i < gs->held) {
        const TrkLost& b = g.buf[gs->cur];
        unsigned long long* o = lost + i * kLostWords;
        o[0] = b.id[i], o[1] = b.age[i], o[2] = b.born[i], o[3] = b.klass[i], o[4] = b.pix[i], o[5] = b.sx[i], o[6] = b.sy[i];
        o[7] = b.x0[i], o[8] = b.y0[i], o[9] = b.x1[i], o[10] = b.y1[i], o[11] = b.seen[i];
    }
}

}  // namespace

hipError_t launch_tracks_memory_forget(const TrkGal& g, hipStream_t s) {
    hipLaunchKernelGGL(tracks_mem_forget_kernel, dim3(1), dim3(1), 0, s, g.gs);
    return hipGetLastError();
}

hipError_t launch_tracks_memory_read(const TrkGal& g, unsigned* gap_of_region, unsigned rows, unsigned* memory_summary, unsigned long long* lost_table,
                                     unsigned lost_rows, hipStream_t s) {
    const size_t lr = lost_table ? (lost_rows < g.G ? lost_rows : g.G) : 0, gr = gap_of_region ? rows : 0;
    const size_t n = lr > gr ? lr : gr;
    hipLaunchKernelGGL(tracks_mem_read_kernel, dim3((unsigned)(n < 256 ? 1 : (n + 255) / 256)), dim3(256), 0, s, g, gap_of_region, rows, memory_summary,
                       lost_table, lost_rows);
    return hipGetLastError();
}

hipError_t launch_tracks_forget(TrkState* st, int step, int set_id, unsigned first_id, unsigned* summary, hipStream_t s) {
    hipLaunchKernelGGL(tracks_forget_kernel, dim3(1), dim3(1), 0, s, st, step, set_id, first_id, summary);
    return hipGetLastError();
}

namespace {

// g: the tracker's memory, or null: then exactly the launches of a tracker without memory
hipError_t tracks_step(const TrkMem& m, const TrkGal* g, const unsigned* labels, const unsigned long long* table, unsigned rows, const unsigned* d_n,
                       unsigned H, unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane, unsigned long long* track_table,
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
    if (!g) {
        if (NB) hipLaunchKernelGGL(tracks_scan_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, m);
        hipLaunchKernelGGL(tracks_scan_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, m, NB, summary);
        if (capRows)
            hipLaunchKernelGGL(tracks_apply_kernel, dim3((unsigned)scan_blocks(capRows)), dim3(kScanBlock), 0, s, m, track_of_region,
                               track_table);
    } else {
        hipLaunchKernelGGL(tracks_mem_clear_kernel, dim3((g->G + 255) / 256), dim3(256), 0, s, *g);
        if (cap) {
            hipLaunchKernelGGL(tracks_revive_choose_kernel, dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, s, m, *g, table, H, W);
            hipLaunchKernelGGL(tracks_revive_keep_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, m, *g);
        }
        if (NB) hipLaunchKernelGGL(tracks_mem_scan_sums_kernel, dim3((unsigned)NB), dim3(kScanBlock), 0, s, m, *g);
        hipLaunchKernelGGL(tracks_mem_scan_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, m, *g, NB, summary);
        if (capRows)
            hipLaunchKernelGGL(tracks_mem_apply_kernel, dim3((unsigned)scan_blocks(capRows)), dim3(kScanBlock), 0, s, m, *g, track_of_region,
                               track_table);
    }
    if (track_plane) hipLaunchKernelGGL(tracks_plane_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, m, labels, N, track_plane);
    if (g) {  // before save overwrites the remembered regions: the ended ones go to the gallery
        const size_t GB = scan_blocks((size_t)g->G + m.M);
        hipLaunchKernelGGL(tracks_gallery_sums_kernel, dim3((unsigned)GB), dim3(kScanBlock), 0, s, m, *g);
        hipLaunchKernelGGL(tracks_gallery_partials_kernel, dim3(1), dim3(kScanBlock), 0, s, m, *g, GB, summary);
        hipLaunchKernelGGL(tracks_gallery_apply_kernel, dim3((unsigned)GB), dim3(kScanBlock), 0, s, m, *g);
    }
    e = hipMemcpyAsync(m.prev, labels, N * 4, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    if (g)
        hipLaunchKernelGGL(tracks_mem_save_kernel, dim3((unsigned)(cap ? (cap + 255) / 256 : 1)), dim3(256), 0, s, m, *g, table, H, W);
    else
        hipLaunchKernelGGL(tracks_save_kernel, dim3((unsigned)(cap ? (cap + 255) / 256 : 1)), dim3(256), 0, s, m, table, H, W);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tracks(const TrkMem& m, const unsigned* labels, const unsigned long long* table, unsigned rows, const unsigned* d_n, unsigned H,
                         unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane, unsigned long long* track_table,
                         unsigned* summary, hipStream_t s) {
    return tracks_step(m, nullptr, labels, table, rows, d_n, H, W, min_overlap, track_of_region, track_plane, track_table, summary, s);
}

hipError_t launch_tracks_memory(const TrkMem& m, const TrkGal& g, const unsigned* labels, const unsigned long long* table, unsigned rows,
                                const unsigned* d_n, unsigned H, unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane,
                                unsigned long long* track_table, unsigned* summary, hipStream_t s) {
    return tracks_step(m, &g, labels, table, rows, d_n, H, W, min_overlap, track_of_region, track_plane, track_table, summary, s);
}

}  // namespace infur
