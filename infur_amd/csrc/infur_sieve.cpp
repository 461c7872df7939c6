// infur_sieve.cpp -- Adjacency and Sieve (include/infur_hip.h): the region adjacency graph of a class, label or track plane, and the
// stage that merges every region below a size threshold into the neighbour it shares the longest border with, so that the stages
// behind it see a class plane without speckle.  Kernels: sieve.hip.  Everything is enqueued on the context's stream; the frame
// wrapper is the egress stages' (infur_rt.h), and so is the rule that the buffers of this file are private scratch: growing them
// leaves mem_gen -- and with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kAdjPairWords == INFUR_ADJ_PAIR_WORDS && kAdjRowWords == INFUR_ADJ_ROW_WORDS && kAdjCountWords == INFUR_ADJ_COUNT_WORDS &&
                  kAdjOverflow == INFUR_ADJ_OVERFLOW && kAdjTruncated == INFUR_ADJ_TRUNCATED && kSieveRowWords == INFUR_SIEVE_ROW_WORDS &&
                  kSieveCountWords == INFUR_SIEVE_COUNT_WORDS && kSieveOverflow == INFUR_SIEVE_OVERFLOW &&
                  kSieveRoundsExhausted == INFUR_SIEVE_ROUNDS_EXHAUSTED && kSieveTableShort == INFUR_SIEVE_TABLE_SHORT,
              "sieve.hip and the header disagree");

constexpr uint32_t kAdjMaxSide = 65535;
constexpr uint64_t kAdjMaxPixels = 1ull << 31;  // an edge id is a u32
constexpr uint32_t kAdjDefaultSlots = 1u << 20;
constexpr uint32_t kSieveDefaultRounds = 8, kSieveMaxRounds = 64;
constexpr uint32_t kSieveFrameRows = 1u << 20;  // the frame calls' own region table

int32_t size_check(infur_ctx* c, uint32_t h, uint32_t w) {
    if (h > kAdjMaxSide || w > kAdjMaxSide || (uint64_t)h * w >= kAdjMaxPixels)
        return fail(c, INFUR_E_INVALID_ARG, "%ux%u: planes of width and height up to %u and fewer than 2^31 pixels", w, h, kAdjMaxSide);
    return INFUR_OK;
}
int32_t slots_check(infur_ctx* c, uint32_t pair_slots, uint32_t* slots) {
    *slots = pair_slots ? pair_slots : kAdjDefaultSlots;
    if (*slots < 64 || (*slots & (*slots - 1))) return fail(c, INFUR_E_INVALID_ARG, "pair_slots %u: a power of two of at least 64, or 0", pair_slots);
    return INFUR_OK;
}
int32_t rounds_check(infur_ctx* c, uint32_t max_rounds, uint32_t* rounds) {
    *rounds = max_rounds ? max_rounds : kSieveDefaultRounds;
    if (max_rounds > kSieveMaxRounds) return fail(c, INFUR_E_INVALID_ARG, "max_rounds %u: at most %u, or 0", max_rounds, kSieveMaxRounds);
    return INFUR_OK;
}

struct AdjWant {
    bool pairs, rows, counts;
};
int32_t adjacency_check(infur_ctx* c, uint32_t elem, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t rows, const void* pairs,
                        uint32_t pair_rows, const void* rows_out, const void* counts, uint32_t pair_slots, uint32_t* slots, AdjWant* want) {
    RETIF(elem_check(c, elem, flags, INFUR_ADJ_SKIP, "adjacency", skip_value));
    RETIF(size_check(c, h, w));
    RETIF(slots_check(c, pair_slots, slots));
    *want = AdjWant{pairs != nullptr, rows_out && rows, counts != nullptr};
    if (!want->pairs && !want->rows && !want->counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: pairs, rows_out (with rows) or counts");
    return INFUR_OK;
}

int32_t sieve_check(infur_ctx* c, uint32_t h, uint32_t w, uint32_t max_rounds, uint32_t pair_slots, const void* klass_out, const void* rows_out,
                    const void* counts, uint32_t* rounds, uint32_t* slots) {
    RETIF(size_check(c, h, w));
    RETIF(rounds_check(c, max_rounds, rounds));
    RETIF(slots_check(c, pair_slots, slots));
    if (!klass_out && !rows_out && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: klass_out, rows_out or counts");
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_adjacency_dev(infur_ctx* c, const void* d_plane, uint32_t elem, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t rows,
                            void* d_pairs, uint32_t pair_rows, void* d_rows_out, void* d_counts, uint32_t pair_slots) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        AdjWant want{};
        RETIF(adjacency_check(c, elem, h, w, flags, skip_value, rows, d_pairs, pair_rows, d_rows_out, d_counts, pair_slots, &slots, &want));
        const size_t hw = (size_t)h * w;
        if (hw && !d_plane) return no_plane(c, h, w);
        if (hw) RETIF(ensure_private(c, c->st_sieve, adjacency_scratch_bytes(hw, rows, slots, want.rows, want.pairs && pair_rows)));
        ProfScope ps(c, "adjacency", "adjacency", 0, (double)hw * elem);
        HIPCHK(c, launch_adjacency(d_plane, (int)elem, h, w, (flags & INFUR_ADJ_SKIP) != 0, skip_value, rows, c->st_sieve.p, slots, (unsigned*)d_pairs,
                                   pair_rows, want.rows ? (unsigned*)d_rows_out : nullptr, (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_adjacency(infur_ctx* c, const void* plane, uint32_t elem, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t rows,
                        uint32_t* pairs, uint32_t pair_rows, uint32_t* rows_out, uint32_t* counts, uint32_t pair_slots) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        AdjWant want{};
        RETIF(adjacency_check(c, elem, h, w, flags, skip_value, rows, pairs, pair_rows, rows_out, counts, pair_slots, &slots, &want));
        const size_t hw = (size_t)h * w;
        if (hw && !plane) return no_plane(c, h, w);
        // st_sieve_io: [counts][pairs][rows][plane], on 256-byte boundaries
        const bool recs = want.pairs && pair_rows;
        const size_t o_pairs = 256, o_rows = o_pairs + align_up(recs ? (size_t)pair_rows * INFUR_ADJ_PAIR_WORDS * 4 : 0, 256),
                     o_plane = o_rows + align_up(want.rows ? (size_t)rows * INFUR_ADJ_ROW_WORDS * 4 : 0, 256);
        RETIF(ensure_private(c, c->st_sieve_io, o_plane + align_up(hw * elem, 256) + 256));
        uint8_t* base = (uint8_t*)c->st_sieve_io.p;
        if (hw) HIPCHK(c, hipMemcpyAsync(base + o_plane, plane, hw * elem, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_adjacency_dev(c, hw ? base + o_plane : nullptr, elem, h, w, flags, skip_value, rows, want.pairs ? base + o_pairs : nullptr, pair_rows,
                                  want.rows ? base + o_rows : nullptr, base, pair_slots));
        // the counts first: they say how many records there are to copy
        uint32_t n[INFUR_ADJ_COUNT_WORDS] = {};
        HIPCHK(c, hipMemcpyAsync(n, base, sizeof n, hipMemcpyDeviceToHost, c->stream));
        if (want.rows) HIPCHK(c, hipMemcpyAsync(rows_out, base + o_rows, (size_t)rows * INFUR_ADJ_ROW_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (recs && n[INFUR_ADJ_WRITTEN])
            HIPCHK(c, hipMemcpy(pairs, base + o_pairs, (size_t)n[INFUR_ADJ_WRITTEN] * INFUR_ADJ_PAIR_WORDS * 4, hipMemcpyDeviceToHost));
        if (counts) std::memcpy(counts, n, sizeof n);
        return INFUR_OK;
    });
}

int32_t infur_sieve_dev(infur_ctx* c, const void* d_klass, const void* d_labels, const void* d_table, uint32_t table_rows, const void* d_n_regions,
                        uint32_t h, uint32_t w, uint32_t min_pixels, uint32_t max_rounds, uint32_t pair_slots, void* d_klass_out, void* d_rows_out,
                        void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t rounds = 0, slots = 0;
        RETIF(sieve_check(c, h, w, max_rounds, pair_slots, d_klass_out, d_rows_out, d_counts, &rounds, &slots));
        const size_t hw = (size_t)h * w;
        if (hw == 0) {  // no pixel, no region
            if (d_counts) HIPCHK(c, hipMemsetAsync(d_counts, 0, INFUR_SIEVE_COUNT_WORDS * 4, c->stream));
            return INFUR_OK;
        }
        if (!d_klass || !d_labels || !d_n_regions || (!d_table && table_rows))
            return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no class plane, label plane, region table or n_regions", w, h);
        RETIF(ensure_private(c, c->st_sieve, sieve_scratch_bytes(hw, table_rows, slots)));
        ProfScope ps(c, "sieve", "sieve", 0, (double)hw * (5 + (d_klass_out ? 6 : 0)));
        HIPCHK(c, launch_sieve((const uint8_t*)d_klass, (const unsigned*)d_labels, (const unsigned long long*)d_table, table_rows,
                               (const unsigned*)d_n_regions, h, w, min_pixels, rounds, c->st_sieve.p, slots, (uint8_t*)d_klass_out, (unsigned*)d_rows_out,
                               (unsigned*)d_counts, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_sieve(infur_ctx* c, const uint8_t* klass, const uint32_t* labels, const uint64_t* table, uint32_t table_rows, uint32_t n_regions, uint32_t h,
                    uint32_t w, uint32_t min_pixels, uint32_t max_rounds, uint32_t pair_slots, uint8_t* klass_out, uint32_t* rows_out, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t rounds = 0, slots = 0;
        RETIF(sieve_check(c, h, w, max_rounds, pair_slots, klass_out, rows_out, counts, &rounds, &slots));
        const size_t hw = (size_t)h * w;
        if (hw == 0) {
            if (counts) std::memset(counts, 0, INFUR_SIEVE_COUNT_WORDS * 4);
            return INFUR_OK;
        }
        if (!klass || !labels || (!table && table_rows))
            return fail(c, INFUR_E_INVALID_ARG, "a %ux%u plane and no class plane, label plane or region table", w, h);
        const size_t n = n_regions < table_rows ? n_regions : table_rows;
        // st_sieve_io: [counts, n_regions][rows][table][labels][klass][klass_out]
        const size_t o_rows = 256, o_table = o_rows + align_up(n * INFUR_SIEVE_ROW_WORDS * 4, 256),
                     o_labels = o_table + align_up(n * INFUR_REGION_WORDS * 8, 256), o_klass = o_labels + align_up(hw * 4, 256),
                     o_out = o_klass + align_up(hw, 256);
        RETIF(ensure_private(c, c->st_sieve_io, o_out + align_up(hw, 256)));
        uint8_t* base = (uint8_t*)c->st_sieve_io.p;
        HIPCHK(c, hipMemcpyAsync(base + 128, &n_regions, 4, hipMemcpyHostToDevice, c->stream));
        if (n) HIPCHK(c, hipMemcpyAsync(base + o_table, table, n * INFUR_REGION_WORDS * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + o_labels, labels, hw * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(base + o_klass, klass, hw, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_sieve_dev(c, base + o_klass, base + o_labels, base + o_table, table_rows, base + 128, h, w, min_pixels, max_rounds, pair_slots,
                              klass_out ? base + o_out : nullptr, (rows_out && n) ? base + o_rows : nullptr, counts ? base : nullptr));
        if (klass_out) HIPCHK(c, hipMemcpyAsync(klass_out, base + o_out, hw, hipMemcpyDeviceToHost, c->stream));
        if (rows_out && n) HIPCHK(c, hipMemcpyAsync(rows_out, base + o_rows, n * INFUR_SIEVE_ROW_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_SIEVE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_sieve_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                              uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels, size_t labels_cap,
                              void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh, uint32_t max_rounds,
                              uint32_t pair_slots, void* d_klass_out, void* d_counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        uint32_t rounds = 0, slots = 0;
        RETIF(rounds_check(c, max_rounds, &rounds));
        RETIF(slots_check(c, pair_slots, &slots));
        const size_t npix = scale_npix(w, h, factor);
        const bool again = d_labels || d_table || d_n;  // Regions of the cleaned plane
        // st_sieve_frame: [n_regions][class plane][confidence plane][cleaned plane][label plane][region table]
        const size_t rows1 = npix < kSieveFrameRows ? npix : kSieveFrameRows;
        const size_t o_klass = 256, o_conf = o_klass + align_up(npix, 256), o_out = o_conf + align_up(npix, 256), o_labels = o_out + align_up(npix, 256),
                     o_table = o_labels + align_up(npix * 4, 256);
        void *kl = d_klass, *cf = d_conf, *out = d_klass_out;
        uint8_t* base = nullptr;
        if (c->loaded && npix) {
            if (!again && !d_klass_out && !d_counts) return INFUR_E_INVALID_ARG;
            if (d_labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
            if (d_klass_out && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
            RETIF(ensure_private(c, c->st_sieve_frame, o_table + align_up(rows1 * INFUR_REGION_WORDS * 8, 256)));
            base = (uint8_t*)c->st_sieve_frame.p;
            if (!kl) kl = base + o_klass;
            if (!cf) cf = base + o_conf;
            if (!out && again) out = base + o_out;
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions of the plane as decoded: everything, the background included
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, 0, 0, kl, cf, (d_klass || d_conf) ? plane_cap : npix,
                                      base ? base + o_labels : nullptr, npix * 4, base ? base + o_table : nullptr, (uint32_t)rows1, base, d_scaled, ow,
                                      oh));
        if (!base) return INFUR_E_INVALID_ARG;  // (not reached: without a model or a frame the call above has failed)
        RETIF(infur_sieve_dev(c, kl, base + o_labels, base + o_table, (uint32_t)rows1, base, *oh, *ow, min_pixels, max_rounds, pair_slots, out, nullptr,
                              d_counts));
        if (!again) return INFUR_OK;
        return infur_regions_dev(c, out, cf, *oh, *ow, connectivity, 0, flags, d_labels, d_table, table_rows, d_n);
    });
}

int32_t infur_frame_sieve(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t connectivity,
                          uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels, size_t labels_cap,
                          uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh, uint32_t max_rounds,
                          uint32_t pair_slots, uint8_t* klass_out, uint32_t* counts) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        // st_sieve_io: [n_regions, counts][table][label plane][class plane][confidence plane][cleaned plane]
        size_t rows = 0, o_table = 256, o_labels = 0, o_klass = 0, o_conf = 0, o_out = 0;
        uint8_t* base = nullptr;
        const bool again = labels || table || n_regions;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf || klass_out) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
                rows = table ? (table_rows < npix ? table_rows : npix) : 0;
                o_labels = o_table + align_up(rows * INFUR_REGION_WORDS * 8, 256);
                o_klass = o_labels + align_up(npix * 4, 256);
                o_conf = o_klass + align_up(npix, 256);
                o_out = o_conf + align_up(npix, 256);
                RETIF(ensure_private(c, c->st_sieve_io, o_out + align_up(npix, 256)));
                base = (uint8_t*)c->st_sieve_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                return infur_frame_sieve_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, klass ? base + o_klass : nullptr,
                                             conf ? base + o_conf : nullptr, npix, labels ? base + o_labels : nullptr, npix * 4,
                                             (table && rows) ? base + o_table : nullptr, (uint32_t)rows, again ? base : nullptr, d_scaled, ow, oh,
                                             max_rounds, pair_slots, klass_out ? base + o_out : nullptr, counts ? base + 128 : nullptr);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + o_klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + o_conf, npix, hipMemcpyDeviceToHost, c->stream));
                if (klass_out) HIPCHK(c, hipMemcpyAsync(klass_out, base + o_out, npix, hipMemcpyDeviceToHost, c->stream));
                if (counts) HIPCHK(c, hipMemcpyAsync(counts, base + 128, INFUR_SIEVE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
                if (!again) return INFUR_OK;
                uint32_t n = 0;
                HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
                if (labels) HIPCHK(c, hipMemcpyAsync(labels, base + o_labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const size_t got = n < rows ? n : rows;
                if (table && got) HIPCHK(c, hipMemcpy(table, base + o_table, got * INFUR_REGION_WORDS * 8, hipMemcpyDeviceToHost));
                if (n_regions) *n_regions = n;
                return INFUR_OK;
            });
    });
}

}  // extern "C"
