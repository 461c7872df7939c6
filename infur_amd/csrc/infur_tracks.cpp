// infur_tracks.cpp -- Tracks, the fourth decode stage (include/infur_hip.h): the tracker object, which remembers one frame of
// Regions output on the device, and its C entry points.  Kernels: tracks.hip.  Everything is enqueued on the context's stream;
// the region count is read on the device, so a step never synchronises.  Like infur_regions.cpp the frame path here always
// enqueues eagerly, and every buffer of this file belongs to the tracker -- no captured graph can point into it: allocating
// or growing it leaves mem_gen, and with it the graphs infur_frame_advance_dev has cached, alone.
#include <cstring>
#include <new>

#include "infur_ctx.h"
#include "infur_rt.h"
#include "kernels.h"
#include "wave_scan.h"

using namespace infur;

struct infur_tracker {
    infur_ctx* ctx = nullptr;  // null: orphaned by infur_ctx_destroy
    uint32_t max_regions = 0, pair_slots = 0;
    void* mem = nullptr;  // state words, per-region arrays, pair table: one allocation made at creation
    TrkMem m{};
    Buf prev;   // the remembered label plane
    Buf io;     // staging of the host-pointer calls
    Buf frame;  // the label plane, table and count the frame calls keep when the caller does not want them
    void* gmem = nullptr;  // memory (infur_tracker_set_memory): the gallery and everything it needs, an allocation of its own
    TrkGal g{};
    Buf mio;  // staging of infur_tracker_memory
};

namespace {

static_assert(kTrkWords == INFUR_TRACK_WORDS, "tracks.hip and the header disagree about the row");
static_assert(kLostWords == INFUR_LOST_WORDS && kTrkGalleryFull == INFUR_TRACKS_GALLERY_FULL, "tracks.hip and the header disagree about memory");
static_assert(kTrkTruncated == INFUR_TRACKS_TRUNCATED && kTrkOverflow == INFUR_TRACKS_OVERFLOW && kTrkExhausted == INFUR_TRACKS_IDS_EXHAUSTED,
              "tracks.hip and the header disagree about the status bits");

constexpr uint32_t kTrkMaxRegions = 1u << 24, kTrkMaxSlots = 1u << 28, kTrkGalleryRows = 4096, kTrkMaxGalleryRows = 65536;

void tracker_release(infur_tracker* t) {
    if (t->mem) (void)hipFree(t->mem);
    if (t->gmem) (void)hipFree(t->gmem);
    for (Buf* b : {&t->prev, &t->io, &t->frame, &t->mio})
        if (b->p) (void)hipFree(b->p);
    t->mem = t->gmem = t->prev.p = t->io.p = t->frame.p = t->mio.p = nullptr;
    t->prev.bytes = t->io.bytes = t->frame.bytes = t->mio.bytes = 0;
}

// forget the remembered frame and, on a tracker with memory, the gallery
hipError_t tracker_forget(infur_tracker* t, int step, int set_id, uint32_t first_id, unsigned* summary, hipStream_t s) {
    const hipError_t e = launch_tracks_forget(t->m.st, step, set_id, first_id, summary, s);
    return e != hipSuccess || !t->gmem ? e : launch_tracks_memory_forget(t->g, s);
}

void tracker_detach(infur_tracker* t) {
    if (infur_ctx* c = t->ctx)
        for (size_t i = 0; i < c->trackers.size(); i++)
            if (c->trackers[i] == t) {
                c->trackers.erase(c->trackers.begin() + (long)i);
                break;
            }
    t->ctx = nullptr;
}

inline infur_ctx* trk_ctx(void* tracker) { return tracker ? ((infur_tracker*)tracker)->ctx : nullptr; }

// staging of the host-pointer calls, on 256-byte boundaries: [count][summary] [table][labels][class][confidence] and the outputs
struct TrkStage {
    size_t rows, summary, table, labels, klass, conf, tor, plane, ttab, bytes;
    TrkStage(size_t npix, uint32_t table_rows, bool planes) {
        rows = table_rows < npix ? table_rows : npix;  // there are at most npix regions
        summary = 128;
        table = 256;
        labels = table + align_up(rows * INFUR_REGION_WORDS * 8, 256);
        klass = labels + align_up(npix * 4, 256);
        conf = klass + (planes ? align_up(npix, 256) : 0);
        tor = conf + (planes ? align_up(npix, 256) : 0);
        plane = tor + align_up(rows * 4, 256);
        ttab = plane + align_up(npix * 4, 256);
        bytes = ttab + align_up(rows * INFUR_TRACK_WORDS * 8, 256);
    }
};

// the wanted outputs of a step to the host; n: the frame's region count
int32_t trk_read_back(infur_ctx* c, const uint8_t* base, const TrkStage& st, size_t npix, uint32_t n, uint32_t* tor, uint32_t* plane, uint64_t* ttab,
                      uint32_t* summary) {
    const size_t rows = n < st.rows ? n : st.rows;
    if (tor && rows) HIPCHK(c, hipMemcpyAsync(tor, base + st.tor, rows * 4, hipMemcpyDeviceToHost, c->stream));
    if (plane && npix) HIPCHK(c, hipMemcpyAsync(plane, base + st.plane, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (ttab && rows) HIPCHK(c, hipMemcpyAsync(ttab, base + st.ttab, rows * INFUR_TRACK_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    if (summary) HIPCHK(c, hipMemcpyAsync(summary, base + st.summary, INFUR_TRACKS_SUMMARY_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return INFUR_OK;
}

}  // namespace

namespace infur {
void tracker_orphan(infur_tracker* t) {
    if (!t || !t->ctx) return;
    (void)hipSetDevice(t->ctx->device);
    tracker_release(t);
    tracker_detach(t);
}
}  // namespace infur

extern "C" {

int32_t infur_tracker_create(infur_ctx* c, uint32_t max_regions, uint32_t pair_slots, void** out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !out) return INFUR_E_INVALID_ARG;
        const uint32_t M = max_regions ? max_regions : 65536u, S = pair_slots ? pair_slots : (1u << 20);
        if (M > kTrkMaxRegions) return fail(c, INFUR_E_INVALID_ARG, "max_regions %u: at most %u", M, kTrkMaxRegions);
        if (S < 64 || S > kTrkMaxSlots || (S & (S - 1))) return fail(c, INFUR_E_INVALID_ARG, "pair_slots %u: a power of two in [64, 2^28]", S);
        infur_tracker* t = new infur_tracker;
        t->max_regions = M;
        t->pair_slots = S;
        const size_t a8 = align_up((size_t)M * 8, 256), a4 = align_up((size_t)M * 4, 256);
        // (one word more than scan_blocks(M) where kScanBlock divides M: kept, so that the allocation is byte for byte what it was)
        const size_t part = align_up(((size_t)M / kScanBlock + 1) * 4, 256), keys = align_up((size_t)S * 8, 256), cnts = align_up((size_t)S * 4, 256);
        const size_t bytes = 256 + 5 * a8 + 7 * a4 + part + keys + cnts;
        if (hipMalloc(&t->mem, bytes) != hipSuccess) {
            (void)hipGetLastError();
            delete t;
            return fail(c, INFUR_E_HIP, "hipMalloc of %zu bytes for a tracker failed", bytes);
        }
        uint8_t* p = (uint8_t*)t->mem;
        auto take = [&](size_t n) {
            uint8_t* q = p;
            p += n;
            return q;
        };
        TrkMem& m = t->m;
        m.st = (TrkState*)take(256);
        m.best = (unsigned long long*)take(a8);
        m.claim = (unsigned long long*)take(a8);
        m.ppix = (unsigned long long*)take(a8);
        m.psx = (unsigned long long*)take(a8);
        m.psy = (unsigned long long*)take(a8);
        m.pclass = (unsigned*)take(a4);
        m.ptrack = (unsigned*)take(a4);
        m.page = (unsigned*)take(a4);
        m.pborn = (unsigned*)take(a4);
        m.ctrack = (unsigned*)take(a4);
        m.cage = (unsigned*)take(a4);
        m.cborn = (unsigned*)take(a4);
        m.partial = (unsigned*)take(part);
        m.keys = (unsigned long long*)take(keys);
        m.cnts = (unsigned*)take(cnts);
        m.prev = nullptr;
        m.slots = S;
        m.M = M;
        // (the arrays need no initialisation: every word is written before a step reads it.  The state words start at zero.)
        if (hipMemsetAsync(m.st, 0, 256, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            tracker_release(t);
            delete t;
            return fail(c, INFUR_E_HIP, "hipMemsetAsync of the tracker's state failed");
        }
        t->ctx = c;
        c->trackers.push_back(t);
        *out = t;
        return INFUR_OK;
    });
}

void infur_tracker_destroy(void* tracker) {
    infur_tracker* t = (infur_tracker*)tracker;
    if (!t) return;
    if (infur_ctx* c = t->ctx) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        tracker_release(t);
        tracker_detach(t);
    }
    delete t;
}

int32_t infur_tracker_reset(void* tracker, uint32_t first_id) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        HIPCHK(c, tracker_forget((infur_tracker*)tracker, 0, 1, first_id, nullptr, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_tracker_set_memory(void* tracker, uint32_t max_lost, uint32_t reach, uint32_t gallery_rows) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        const uint32_t G = gallery_rows ? gallery_rows : kTrkGalleryRows;
        if (max_lost && G > kTrkMaxGalleryRows) return fail(c, INFUR_E_INVALID_ARG, "gallery_rows %u: at most %u", G, kTrkMaxGalleryRows);
        HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch still reads what is freed or replaced below
        void* mem = nullptr;
        TrkGal g{};
        if (max_lost) {
            const size_t M = t->max_regions;
            const size_t m8 = align_up(M * 8, 256), m4 = align_up(M * 4, 256), g8 = align_up((size_t)G * 8, 256), g4 = align_up((size_t)G * 4, 256);
            const size_t rpart = align_up((M / kScanBlock + 1) * 4, 256), gpart = align_up(scan_blocks((size_t)G + M) * 4, 256);
            const size_t bytes = 256 + 2 * (3 * g8 + 9 * g4) + 5 * m4 + m8 + g8 + rpart + gpart;
            if (hipMalloc(&mem, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, INFUR_E_HIP, "hipMalloc of %zu bytes for a tracker's memory failed", bytes);
            }
            uint8_t* p = (uint8_t*)mem;
            auto take = [&](size_t n) {
                uint8_t* q = p;
                p += n;
                return q;
            };
            g.gs = (TrkGalState*)take(256);
            for (TrkLost& b : g.buf) {
                b.pix = (unsigned long long*)take(g8);
                b.sx = (unsigned long long*)take(g8);
                b.sy = (unsigned long long*)take(g8);
                for (unsigned** a : {&b.id, &b.age, &b.born, &b.klass, &b.x0, &b.y0, &b.x1, &b.y1, &b.seen}) *a = (unsigned*)take(g4);
            }
            for (unsigned** a : {&g.px0, &g.py0, &g.px1, &g.py1, &g.cgap}) *a = (unsigned*)take(m4);
            g.rbest = (unsigned long long*)take(m8);
            g.rclaim = (unsigned long long*)take(g8);
            g.rpart = (unsigned*)take(rpart);
            g.gpart = (unsigned*)take(gpart);
            g.max_lost = max_lost;
            g.reach = reach;
            g.G = G;
            // (as at creation: every array word is written before a step reads it, the state words start at zero)
            if (hipMemsetAsync(g.gs, 0, 256, c->stream) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(mem);
                return fail(c, INFUR_E_HIP, "hipMemsetAsync of the tracker's memory state failed");
            }
        }
        // the last step that can fail comes before the swap (it touches the tracker's state words only): an error leaves the tracker as it was
        const hipError_t e = launch_tracks_forget(t->m.st, 0, 0, 0, nullptr, c->stream);
        if (e != hipSuccess) {
            if (mem) (void)hipFree(mem);
            return fail(c, INFUR_E_HIP, "forgetting the remembered frame failed: %s", hipGetErrorString(e));
        }
        if (t->gmem) (void)hipFree(t->gmem);
        t->gmem = mem;
        t->g = g;
        return INFUR_OK;
    });
}

int32_t infur_tracker_memory_dev(void* tracker, void* d_gap, uint32_t rows, void* d_msum, void* d_lost, uint32_t lost_rows) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c || !((infur_tracker*)tracker)->gmem) return INFUR_E_INVALID_ARG;
        if (!d_gap && !d_msum && !d_lost) return INFUR_E_INVALID_ARG;
        HIPCHK(c, launch_tracks_memory_read(((infur_tracker*)tracker)->g, (unsigned*)d_gap, rows, (unsigned*)d_msum, (unsigned long long*)d_lost, lost_rows,
                                            c->stream));
        return INFUR_OK;
    });
}

int32_t infur_tracker_memory(void* tracker, uint32_t* gap, uint32_t rows, uint32_t* msum, uint64_t* lost, uint32_t lost_rows) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c || !((infur_tracker*)tracker)->gmem) return INFUR_E_INVALID_ARG;
        if (!gap && !msum && !lost) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        const size_t lr = lost_rows < t->g.G ? lost_rows : t->g.G;  // the gallery holds no more
        const size_t o_gap = 256, o_lost = o_gap + align_up((size_t)rows * 4, 256), bytes = o_lost + align_up(lr * INFUR_LOST_WORDS * 8, 256);
        RETIF(ensure_private(c, t->mio, bytes));
        uint8_t* base = (uint8_t*)t->mio.p;
        RETIF(infur_tracker_memory_dev(t, gap ? base + o_gap : nullptr, rows, base, lost ? base + o_lost : nullptr, (uint32_t)lr));
        uint32_t sum[INFUR_TRACK_MEMORY_WORDS];
        HIPCHK(c, hipMemcpyAsync(sum, base, sizeof sum, hipMemcpyDeviceToHost, c->stream));
        if (gap && rows) HIPCHK(c, hipMemcpyAsync(gap, base + o_gap, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const size_t held = sum[INFUR_TRACK_MEMORY_HELD] < lr ? sum[INFUR_TRACK_MEMORY_HELD] : lr;  // the count decides how many rows there are to copy
        if (lost && held) HIPCHK(c, hipMemcpy(lost, base + o_lost, held * INFUR_LOST_WORDS * 8, hipMemcpyDeviceToHost));
        if (msum) memcpy(msum, sum, sizeof sum);
        return INFUR_OK;
    });
}

int32_t infur_tracks_dev(void* tracker, const void* d_labels, const void* d_table, uint32_t table_rows, const void* d_n, uint32_t h, uint32_t w,
                         uint32_t min_overlap, void* d_tor, void* d_plane, void* d_ttab, void* d_summary) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        RETIF(plane_check(c, h, w, "a label plane"));
        const size_t hw = (size_t)h * w;
        if (!d_tor && !d_plane && !d_ttab && !d_summary) return INFUR_E_INVALID_ARG;
        if (hw == 0) {  // empty frame: nothing to track, nothing remembered
            HIPCHK(c, tracker_forget(t, 1, 0, 0, (unsigned*)d_summary, c->stream));
            return INFUR_OK;
        }
        if (!d_labels || !d_table || !d_n) return INFUR_E_INVALID_ARG;
        // (a plane that had to grow cannot be the remembered frame's size: the step finds other dimensions and starts afresh)
        RETIF(ensure_private(c, t->prev, hw * 4));
        t->m.prev = (unsigned*)t->prev.p;
        ProfScope ps(c, "tracks", "tracks", 0, (double)hw * (12 + (d_plane ? 4 : 0)) + (double)t->pair_slots * 12);
        if (t->gmem)
            HIPCHK(c, launch_tracks_memory(t->m, t->g, (const unsigned*)d_labels, (const unsigned long long*)d_table, table_rows, (const unsigned*)d_n, h,
                                           w, min_overlap, (unsigned*)d_tor, (unsigned*)d_plane, (unsigned long long*)d_ttab, (unsigned*)d_summary,
                                           c->stream));
        else
            HIPCHK(c, launch_tracks(t->m, (const unsigned*)d_labels, (const unsigned long long*)d_table, table_rows, (const unsigned*)d_n, h, w,
                                    min_overlap, (unsigned*)d_tor, (unsigned*)d_plane, (unsigned long long*)d_ttab, (unsigned*)d_summary, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_tracks(void* tracker, const uint32_t* labels, const uint64_t* table, uint32_t table_rows, uint32_t n_regions, uint32_t h, uint32_t w,
                     uint32_t min_overlap, uint32_t* tor, uint32_t* plane, uint64_t* ttab, uint32_t* summary) {
    infur_ctx* c = trk_ctx(tracker);
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        RETIF(plane_check(c, h, w, "a label plane"));
        const size_t hw = (size_t)h * w;
        if (!tor && !plane && !ttab && !summary) return INFUR_E_INVALID_ARG;
        if (hw && (!labels || (!table && table_rows && n_regions))) return INFUR_E_INVALID_ARG;
        const TrkStage st(hw, table_rows, false);
        RETIF(ensure_private(c, t->io, st.bytes));
        uint8_t* base = (uint8_t*)t->io.p;
        if (hw) {
            const size_t rows_in = n_regions < st.rows ? n_regions : st.rows;
            HIPCHK(c, hipMemcpyAsync(base, &n_regions, 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(base + st.labels, labels, hw * 4, hipMemcpyHostToDevice, c->stream));
            if (rows_in) HIPCHK(c, hipMemcpyAsync(base + st.table, table, rows_in * INFUR_REGION_WORDS * 8, hipMemcpyHostToDevice, c->stream));
        }
        RETIF(infur_tracks_dev(t, base + st.labels, base + st.table, (uint32_t)st.rows, base, h, w, min_overlap, tor ? base + st.tor : nullptr,
                               plane ? base + st.plane : nullptr, ttab ? base + st.ttab : nullptr, base + st.summary));
        return trk_read_back(c, base, st, hw, hw ? n_regions : 0, tor, plane, ttab, summary);
    });
}

int32_t infur_frame_tracks_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                               uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap,
                               void* d_labels, size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow,
                               uint32_t* oh, void* tracker, uint32_t min_overlap, void* d_tor, void* d_plane, void* d_ttab, void* d_summary) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh || trk_ctx(tracker) != c) return INFUR_E_INVALID_ARG;
        if (!d_tor && !d_plane && !d_ttab && !d_summary) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        const size_t npix = scale_npix(w, h, factor);
        void* lab = d_labels;
        void* tab = d_table;
        void* dn = d_n;
        size_t lcap = labels_cap;
        if (c->loaded && npix && (!lab || !tab || !dn)) {  // what the caller does not want of Regions' outputs lives with the tracker
            const TrkStage st(npix, table_rows, false);
            RETIF(ensure_private(c, t->frame, st.tor));
            uint8_t* base = (uint8_t*)t->frame.p;
            if (!dn) dn = base;
            if (!tab) tab = base + st.table;
            if (!lab) {
                lab = base + st.labels;
                lcap = npix * 4;
            }
        }  // (otherwise the call below fails before it labels: bad scale, empty frame or no model)
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lab, lcap,
                                      tab, table_rows, dn, d_scaled, ow, oh));
        return infur_tracks_dev(t, lab, tab, table_rows, dn, *oh, *ow, min_overlap, d_tor, d_plane, d_ttab, d_summary);
    });
}

int32_t infur_frame_tracks(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                           uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap,
                           uint32_t* labels, size_t labels_cap, uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled,
                           uint32_t* ow, uint32_t* oh, void* tracker, uint32_t min_overlap, uint32_t* tor, uint32_t* plane, uint64_t* ttab,
                           uint32_t* summary) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh || trk_ctx(tracker) != c) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        if (!tor && !plane && !ttab && !summary) return INFUR_E_INVALID_ARG;
        infur_tracker* t = (infur_tracker*)tracker;
        TrkStage st(0, 0, true);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
                st = TrkStage(npix, table_rows, true);
                RETIF(ensure_private(c, t->io, st.bytes));
                base = (uint8_t*)t->io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_tracks_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, base + st.klass, base + st.conf, npix,
                                              base + st.labels, npix * 4, base + st.table, (uint32_t)st.rows, base, d_scaled, ow, oh, t, min_overlap,
                                              tor ? base + st.tor : nullptr, plane ? base + st.plane : nullptr, ttab ? base + st.ttab : nullptr,
                                              base + st.summary);
            },
            [&](size_t npix) -> int32_t {
                uint32_t n = 0;  // the count decides how many rows there are to copy
                HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + st.klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + st.conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (labels) HIPCHK(c, hipMemcpyAsync(labels, base + st.labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const size_t rows = n < st.rows ? n : st.rows;
                if (table && rows) HIPCHK(c, hipMemcpy(table, base + st.table, rows * INFUR_REGION_WORDS * 8, hipMemcpyDeviceToHost));
                if (n_regions) *n_regions = n;
                return trk_read_back(c, base, st, npix, n, tor, plane, ttab, summary);
            });
    });
}

}  // extern "C"
