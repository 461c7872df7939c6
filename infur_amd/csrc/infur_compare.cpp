// infur_compare.cpp -- Compare, the stage that grades a result (include/infur_hip.h): the confusion matrix of two byte or u32 planes
// and per value its best partner with intersection and union, so that a host gets pixel accuracy, IoU and panoptic quality from
// a few hundred integers and not from planes pulled across the bus.  Kernels: compare.hip.  Everything is enqueued on the
// context's stream; the frame wrapper and the decode of the class plane are the egress stages' (infur_egress.h, infur_rt.h), and
// so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs
// infur_frame_advance_dev has cached -- alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kCompareWords == INFUR_COMPARE_WORDS && kCompareCountWords == INFUR_COMPARE_COUNT_WORDS && kCmpOverflow == INFUR_COMPARE_OVERFLOW &&
                  kCmpTable == INFUR_COMPARE_TABLE,
              "compare.hip and the header disagree");

constexpr uint32_t kCmpMaxSide = 65535;
constexpr uint32_t kCmpDefaultSlots = 1u << 20;
constexpr uint64_t kCmpMaxMatrix = 1ull << 20;

struct CmpWant {
    bool matrix, rows_a, rows_b, counts;
};

// the header's checks up to "nothing wanted" and the matrix bound; *slots: the table's slots
int32_t compare_check(infur_ctx* c, uint32_t elem_a, uint32_t elem_b, uint32_t h, uint32_t w, uint32_t flags, uint32_t ignore_a, uint32_t ignore_b,
                      const void* matrix, uint32_t rows_a, uint32_t rows_b, const void* rows_a_out, const void* rows_b_out, const void* counts,
                      uint32_t pair_slots, uint32_t* slots, CmpWant* want) {
    if (elem_a != 1 && elem_a != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_a %u: 1 or 4", elem_a);
    if (elem_b != 1 && elem_b != 4) return fail(c, INFUR_E_INVALID_ARG, "elem_b %u: 1 or 4", elem_b);
    if (flags & ~(uint32_t)(INFUR_COMPARE_IGNORE_A | INFUR_COMPARE_IGNORE_B)) return fail(c, INFUR_E_INVALID_ARG, "unknown compare flags 0x%x", flags);
    if (elem_a == 1 && ignore_a > 255) return fail(c, INFUR_E_INVALID_ARG, "ignore_a %u: a byte plane holds at most 255", ignore_a);
    if (elem_b == 1 && ignore_b > 255) return fail(c, INFUR_E_INVALID_ARG, "ignore_b %u: a byte plane holds at most 255", ignore_b);
    if (h > kCmpMaxSide || w > kCmpMaxSide) return fail(c, INFUR_E_INVALID_ARG, "%ux%u: planes of width and height up to %u", w, h, kCmpMaxSide);
    *slots = pair_slots ? pair_slots : kCmpDefaultSlots;
    if (*slots < 64 || (*slots & (*slots - 1))) return fail(c, INFUR_E_INVALID_ARG, "pair_slots %u: a power of two of at least 64, or 0", pair_slots);
    const uint64_t entries = (uint64_t)rows_a * rows_b;
    *want = CmpWant{matrix && entries, rows_a_out && rows_a, rows_b_out && rows_b, counts != nullptr};
    if (!want->matrix && !want->rows_a && !want->rows_b && !want->counts)
        return fail(c, INFUR_E_INVALID_ARG, "no output wanted: matrix, rows_a_out, rows_b_out (each with rows) or counts");
    if (want->matrix && entries > kCmpMaxMatrix)
        return fail(c, INFUR_E_INVALID_ARG, "a matrix of %u x %u: at most 2^20 entries (the row tables have no such bound)", rows_a, rows_b);
    return INFUR_OK;
}

// st_cmp_io: [counts][matrix][rows of a][rows of b][plane a][plane b], on 256-byte boundaries
struct CmpStage {
    size_t matrix, rows_a, rows_b, a, b, bytes;
    CmpStage(const CmpWant& w, size_t ra, size_t rb, size_t a_bytes, size_t b_bytes) {
        matrix = 256;
        rows_a = matrix + align_up(w.matrix ? ra * rb * 4 : 0, 256);
        rows_b = rows_a + align_up(w.rows_a ? ra * INFUR_COMPARE_WORDS * 4 : 0, 256);
        a = rows_b + align_up(w.rows_b ? rb * INFUR_COMPARE_WORDS * 4 : 0, 256);
        b = a + align_up(a_bytes, 256);
        bytes = b + align_up(b_bytes, 256) + 256;
    }
};

int32_t compare_read_back(infur_ctx* c, const uint8_t* base, const CmpStage& st, const CmpWant& w, size_t ra, size_t rb, uint32_t* matrix,
                          uint32_t* rows_a_out, uint32_t* rows_b_out, uint32_t* counts) {
    if (w.counts) HIPCHK(c, hipMemcpyAsync(counts, base, INFUR_COMPARE_COUNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if (w.matrix) HIPCHK(c, hipMemcpyAsync(matrix, base + st.matrix, ra * rb * 4, hipMemcpyDeviceToHost, c->stream));
    if (w.rows_a) HIPCHK(c, hipMemcpyAsync(rows_a_out, base + st.rows_a, ra * INFUR_COMPARE_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if (w.rows_b) HIPCHK(c, hipMemcpyAsync(rows_b_out, base + st.rows_b, rb * INFUR_COMPARE_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_compare_dev(infur_ctx* c, const void* d_a, uint32_t elem_a, const void* d_b, uint32_t elem_b, uint32_t h, uint32_t w, uint32_t flags,
                          uint32_t ignore_a, uint32_t ignore_b, void* d_matrix, uint32_t rows_a, uint32_t rows_b, void* d_rows_a_out, void* d_rows_b_out,
                          void* d_counts, uint32_t pair_slots) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        CmpWant want{};
        RETIF(compare_check(c, elem_a, elem_b, h, w, flags, ignore_a, ignore_b, d_matrix, rows_a, rows_b, d_rows_a_out, d_rows_b_out, d_counts, pair_slots,
                            &slots, &want));
        const size_t hw = (size_t)h * w;
        if (hw && (!d_a || !d_b)) return no_plane(c, h, w);
        if (hw) RETIF(ensure_private(c, c->st_cmp, compare_scratch_bytes(rows_a, rows_b, slots)));
        ProfScope ps(c, "compare", compare_dense(rows_a, rows_b) ? "compare_dense" : "compare_table", 0, (double)hw * (elem_a + elem_b));
        // (an empty plane: zeros and NONE rows, and nothing else)
        HIPCHK(c, launch_compare(d_a, (int)elem_a, d_b, (int)elem_b, h, w, (flags & INFUR_COMPARE_IGNORE_A) != 0, ignore_a,
                                 (flags & INFUR_COMPARE_IGNORE_B) != 0, ignore_b, rows_a, rows_b, c->st_cmp.p, slots, want.matrix ? (unsigned*)d_matrix : nullptr,
                                 want.rows_a ? (unsigned*)d_rows_a_out : nullptr, want.rows_b ? (unsigned*)d_rows_b_out : nullptr, (unsigned*)d_counts,
                                 c->stream));
        return INFUR_OK;
    });
}

int32_t infur_compare(infur_ctx* c, const void* a, uint32_t elem_a, const void* b, uint32_t elem_b, uint32_t h, uint32_t w, uint32_t flags,
                      uint32_t ignore_a, uint32_t ignore_b, uint32_t* matrix, uint32_t rows_a, uint32_t rows_b, uint32_t* rows_a_out, uint32_t* rows_b_out,
                      uint32_t* counts, uint32_t pair_slots) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        uint32_t slots = 0;
        CmpWant want{};
        RETIF(compare_check(c, elem_a, elem_b, h, w, flags, ignore_a, ignore_b, matrix, rows_a, rows_b, rows_a_out, rows_b_out, counts, pair_slots, &slots,
                            &want));
        const size_t hw = (size_t)h * w;
        if (hw && (!a || !b)) return no_plane(c, h, w);
        const CmpStage st(want, rows_a, rows_b, hw * elem_a, hw * elem_b);
        RETIF(ensure_private(c, c->st_cmp_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_cmp_io.p;
        if (hw) {
            HIPCHK(c, hipMemcpyAsync(base + st.a, a, hw * elem_a, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(base + st.b, b, hw * elem_b, hipMemcpyHostToDevice, c->stream));
        }
        RETIF(infur_compare_dev(c, hw ? base + st.a : nullptr, elem_a, hw ? base + st.b : nullptr, elem_b, h, w, flags, ignore_a, ignore_b,
                                want.matrix ? base + st.matrix : nullptr, rows_a, rows_b, want.rows_a ? base + st.rows_a : nullptr,
                                want.rows_b ? base + st.rows_b : nullptr, want.counts ? base : nullptr, pair_slots));
        RETIF(compare_read_back(c, base, st, want, rows_a, rows_b, matrix, rows_a_out, rows_b_out, counts));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return INFUR_OK;
    });
}

int32_t infur_frame_compare_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                                uint32_t ignore_b, const void* d_truth, size_t truth_cap, void* d_klass, void* d_conf, size_t plane_cap, void* d_matrix,
                                uint32_t rows_a, uint32_t rows_b, void* d_rows_a_out, void* d_rows_b_out, void* d_counts, uint32_t pair_slots, void* d_scaled,
                                uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        if (flags & ~(uint32_t)INFUR_COMPARE_IGNORE_B) return fail(c, INFUR_E_INVALID_ARG, "compare flags 0x%x: only INFUR_COMPARE_IGNORE_B applies to a frame", flags);
        uint32_t slots = 0;
        CmpWant want{};
        // the stage's own checks, made only where a model is loaded and the frame scales, so that without one Scale still runs
        auto check = [&](uint32_t rows) -> int32_t {
            const size_t npix = scale_npix(w, h, factor);
            RETIF(compare_check(c, 1, 1, rows, (uint32_t)(npix / rows), flags, 0, ignore_b, d_matrix, rows_a, rows_b, d_rows_a_out, d_rows_b_out, d_counts,
                                pair_slots, &slots, &want));
            if ((d_klass || d_conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
            if (!d_truth) return fail(c, INFUR_E_INVALID_ARG, "no truth plane");
            if (truth_cap < npix) return fail(c, INFUR_E_CAPACITY, "the truth plane needs %zu bytes, buffer has %zu", npix, truth_cap);
            return INFUR_OK;
        };
        void* kl = d_klass;
        if (!d_klass && !d_conf) {  // the class plane alone, into scratch of the library's own
            RETIF(frame_class_plane(c, c->st_cmp_plane, d_bgr, w, h, factor, mode, decode, nullptr, 0, d_scaled, ow, oh, &kl, check));
        } else {  // the caller's planes are Segments' own outputs, with its capacity check
            uint32_t rows = 0;
            const size_t npix = scale_npix(w, h, factor, &rows);
            if (c->loaded && npix) {
                RETIF(check(rows));
                if (!kl) {
                    RETIF(ensure_private(c, c->st_cmp_plane, npix));
                    kl = c->st_cmp_plane.p;
                }
            }
            RETIF(infur_frame_segments_dev(c, d_bgr, w, h, factor, mode, decode, kl, d_conf, npix, nullptr, 0, nullptr, 0, d_scaled,
                                           ow, oh));
        }
        return infur_compare_dev(c, kl, 1, d_truth, 1, *oh, *ow, flags, 0, ignore_b, d_matrix, rows_a, rows_b, d_rows_a_out, d_rows_b_out, d_counts, pair_slots);
    });
}

int32_t infur_frame_compare(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                            uint32_t ignore_b, const uint8_t* truth, size_t truth_cap, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* matrix,
                            uint32_t rows_a, uint32_t rows_b, uint32_t* rows_a_out, uint32_t* rows_b_out, uint32_t* counts, uint32_t pair_slots,
                            uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        if (flags & ~(uint32_t)INFUR_COMPARE_IGNORE_B) return fail(c, INFUR_E_INVALID_ARG, "compare flags 0x%x: only INFUR_COMPARE_IGNORE_B applies to a frame", flags);
        const uint64_t entries = (uint64_t)rows_a * rows_b;
        const CmpWant want{matrix && entries && entries <= kCmpMaxMatrix, rows_a_out && rows_a, rows_b_out && rows_b, counts != nullptr};
        CmpStage st(CmpWant{}, 0, 0, 0, 0);
        size_t d_klass = 0, d_conf = 0;  // offsets behind the stage
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (c->loaded && npix && truth && truth_cap < npix)
                    return fail(c, INFUR_E_CAPACITY, "the truth plane needs %zu bytes, buffer has %zu", npix, truth_cap);
                st = CmpStage(want, rows_a, rows_b, 0, npix);
                d_klass = st.bytes;
                d_conf = d_klass + align_up(npix, 256);
                RETIF(ensure_private(c, c->st_cmp_io, d_conf + align_up(npix, 256)));
                base = (uint8_t*)c->st_cmp_io.p;
                if (c->loaded && npix && truth) HIPCHK(c, hipMemcpyAsync(base + st.b, truth, npix, hipMemcpyHostToDevice, c->stream));
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                // (a matrix too large to stage reaches the device call as wanted, and is refused there)
                return infur_frame_compare_dev(c, d_bgr, w, h, factor, mode, decode, flags, ignore_b, truth ? base + st.b : nullptr, npix,
                                               klass ? base + d_klass : nullptr, conf ? base + d_conf : nullptr, npix,
                                               (matrix && entries) ? base + st.matrix : nullptr, rows_a, rows_b, want.rows_a ? base + st.rows_a : nullptr,
                                               want.rows_b ? base + st.rows_b : nullptr, counts ? base : nullptr, pair_slots, d_scaled, ow, oh);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + d_klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + d_conf, npix, hipMemcpyDeviceToHost, c->stream));
                return compare_read_back(c, base, st, want, rows_a, rows_b, matrix, rows_a_out, rows_b_out, counts);
            });
    });
}

}  // extern "C"
