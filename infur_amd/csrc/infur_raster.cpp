// infur_raster.cpp -- Raster, the stage that goes the other way (include/infur_hip.h): the loops of a polygon stage, or Runs'
// records, filled back into a dense plane on the device, with the pixels no loop or several loops claim counted.  Kernels:
// raster.hip.  Everything is enqueued on the context's stream; the checks and row rules are the egress stages' (infur_egress.h),
// and so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and with it the graphs
// infur_frame_advance_dev has cached -- alone.  There is no frame call: the input is not a product of the frame.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kRasterCountWords == INFUR_RASTER_COUNT_WORDS && kRasterTruncated == INFUR_RASTER_TRUNCATED && kRasterMalformed == INFUR_RASTER_MALFORMED &&
                  kRasterOutside == INFUR_RASTER_OUTSIDE && kRunWords == INFUR_RUN_WORDS,
              "raster.hip and the header disagree");

constexpr size_t kRunBytes = INFUR_RUN_WORDS * 4;

// what both front ends check before their input, in this order
int32_t raster_check(infur_ctx* c, uint32_t h, uint32_t w, uint32_t elem_bytes, uint32_t fill_value, const void* plane, const void* counts) {
    RETIF(elem_check(c, elem_bytes, 0, 0, "raster", 0));
    if (elem_bytes == 1 && fill_value > 255) return fail(c, INFUR_E_INVALID_ARG, "fill_value %u: a byte plane holds at most 255", fill_value);
    RETIF(side_check(c, h, w, false));
    if (!plane && !counts) return fail(c, INFUR_E_INVALID_ARG, "no output wanted: plane_out or counts_out");
    return INFUR_OK;
}

int32_t runs_input_check(infur_ctx* c, const void* runs, uint32_t runs_rows_in, bool have_n) {
    if (!have_n) return fail(c, INFUR_E_INVALID_ARG, "no n_runs: Runs' count says how much of the input there is");
    if (!runs && runs_rows_in) return fail(c, INFUR_E_INVALID_ARG, "%u records declared and no pointer to them", runs_rows_in);
    return INFUR_OK;
}

int32_t raster_dev(infur_ctx* c, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in, const void* d_counts,
                   uint32_t h, uint32_t w, uint32_t elem_bytes, uint32_t fill_value, void* d_plane, void* d_counts_out) {
    RETIF(raster_check(c, h, w, elem_bytes, fill_value, d_plane, d_counts_out));
    RETIF(input_check(c, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts));
    const size_t npix = (size_t)h * w;
    RETIF(ensure_private(c, c->st_raster, raster_scratch_bytes(npix)));
    ProfScope ps(c, "raster", "raster", 0, (double)npix * (16 + (d_plane ? elem_bytes : 0)) + (double)vertex_rows_in * 4 + (double)loops_rows_in * 16);
    HIPCHK(c, launch_raster((const unsigned*)d_loops, loops_rows_in, (const unsigned*)d_vertices, vertex_rows_in, (const unsigned*)d_counts, h, w,
                            (int)elem_bytes, fill_value, c->st_raster.p, d_plane, (unsigned*)d_counts_out, c->stream));
    return INFUR_OK;
}

int32_t raster_runs_dev(infur_ctx* c, const void* d_runs, uint32_t runs_rows_in, const void* d_n, uint32_t h, uint32_t w, uint32_t elem_bytes,
                        uint32_t fill_value, void* d_plane, void* d_counts_out) {
    RETIF(raster_check(c, h, w, elem_bytes, fill_value, d_plane, d_counts_out));
    RETIF(runs_input_check(c, d_runs, runs_rows_in, d_n != nullptr));
    const size_t npix = (size_t)h * w;
    RETIF(ensure_private(c, c->st_raster, raster_scratch_bytes(npix)));
    ProfScope ps(c, "raster_runs", "raster", 0, (double)npix * (16 + (d_plane ? elem_bytes : 0)) + (double)runs_rows_in * kRunBytes);
    HIPCHK(c, launch_raster_runs((const unsigned*)d_runs, runs_rows_in, (const unsigned*)d_n, h, w, (int)elem_bytes, fill_value, c->st_raster.p, d_plane,
                                 (unsigned*)d_counts_out, c->stream));
    return INFUR_OK;
}

// the staging of the host-pointer calls, in st_raster_io: [counts out][counts in][records][vertices][plane], on 256-byte boundaries
struct RasterStage {
    size_t counts_out, counts_in, records, vertices, plane, bytes;
    RasterStage(size_t record_bytes, size_t vertex_bytes, size_t plane_bytes) {
        counts_out = 0;
        counts_in = kSlotAlign;
        records = counts_in + kSlotAlign;
        vertices = records + align_up(record_bytes, kSlotAlign);
        plane = vertices + align_up(vertex_bytes, kSlotAlign);
        bytes = plane + align_up(plane_bytes, kSlotAlign);
    }
};

// The counts first: they say whether there is a plane to copy.
int32_t raster_read_back(infur_ctx* c, const uint8_t* base, const RasterStage& st, size_t plane_bytes, void* plane, uint32_t* counts_out) {
    uint32_t n[INFUR_RASTER_COUNT_WORDS] = {};
    HIPCHK(c, hipMemcpyAsync(n, base + st.counts_out, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (plane && !(n[INFUR_RASTER_STATUS] & INFUR_RASTER_TRUNCATED)) HIPCHK(c, hipMemcpy(plane, base + st.plane, plane_bytes, hipMemcpyDeviceToHost));
    if (counts_out) std::memcpy(counts_out, n, sizeof n);
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_raster_dev(infur_ctx* c, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in,
                         const void* d_counts, uint32_t h, uint32_t w, uint32_t elem_bytes, uint32_t fill_value, void* d_plane_out,
                         void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        return raster_dev(c, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts, h, w, elem_bytes, fill_value, d_plane_out, d_counts_out);
    });
}

int32_t infur_raster(infur_ctx* c, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices, uint32_t vertex_rows_in,
                     const uint32_t* counts, uint32_t h, uint32_t w, uint32_t elem_bytes, uint32_t fill_value, void* plane_out, uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(raster_check(c, h, w, elem_bytes, fill_value, plane_out, counts_out));
        RETIF(input_check(c, loops, loops_rows_in, vertices, vertex_rows_in, counts));
        // only what the counts say there is travels
        const size_t nl = copy_rows(counts[0], loops_rows_in), nv = copy_rows(counts[1], vertex_rows_in);
        const size_t plane_bytes = (size_t)h * w * elem_bytes;
        const RasterStage st(nl * kLoopBytes, nv * kVertexBytes, plane_out ? plane_bytes : 0);
        RETIF(ensure_private(c, c->st_raster_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_raster_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.counts_in, counts, 8, hipMemcpyHostToDevice, c->stream));
        if (nl) HIPCHK(c, hipMemcpyAsync(base + st.records, loops, nl * kLoopBytes, hipMemcpyHostToDevice, c->stream));
        if (nv) HIPCHK(c, hipMemcpyAsync(base + st.vertices, vertices, nv * kVertexBytes, hipMemcpyHostToDevice, c->stream));
        // (the rows declared to the device are what was copied: truncated input stays truncated, counts[k] > rows)
        RETIF(raster_dev(c, base + st.records, (uint32_t)nl, base + st.vertices, (uint32_t)nv, base + st.counts_in, h, w, elem_bytes, fill_value,
                         plane_out ? base + st.plane : nullptr, base + st.counts_out));
        return raster_read_back(c, base, st, plane_bytes, plane_out, counts_out);
    });
}

int32_t infur_raster_runs_dev(infur_ctx* c, const void* d_runs, uint32_t runs_rows_in, const void* d_n_runs, uint32_t h, uint32_t w,
                              uint32_t elem_bytes, uint32_t fill_value, void* d_plane_out, void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        return raster_runs_dev(c, d_runs, runs_rows_in, d_n_runs, h, w, elem_bytes, fill_value, d_plane_out, d_counts_out);
    });
}

int32_t infur_raster_runs(infur_ctx* c, const uint32_t* runs, uint32_t runs_rows_in, uint32_t n_runs, uint32_t h, uint32_t w, uint32_t elem_bytes,
                          uint32_t fill_value, void* plane_out, uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(raster_check(c, h, w, elem_bytes, fill_value, plane_out, counts_out));
        RETIF(runs_input_check(c, runs, runs_rows_in, true));
        const size_t n = copy_rows(n_runs, runs_rows_in);
        const size_t plane_bytes = (size_t)h * w * elem_bytes;
        const RasterStage st(n * kRunBytes, 0, plane_out ? plane_bytes : 0);
        RETIF(ensure_private(c, c->st_raster_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_raster_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.counts_in, &n_runs, 4, hipMemcpyHostToDevice, c->stream));
        if (n) HIPCHK(c, hipMemcpyAsync(base + st.records, runs, n * kRunBytes, hipMemcpyHostToDevice, c->stream));
        RETIF(raster_runs_dev(c, base + st.records, (uint32_t)n, base + st.counts_in, h, w, elem_bytes, fill_value, plane_out ? base + st.plane : nullptr,
                              base + st.counts_out));
        return raster_read_back(c, base, st, plane_bytes, plane_out, counts_out);
    });
}

}  // extern "C"
