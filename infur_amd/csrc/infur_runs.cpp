// infur_runs.cpp -- Runs, the egress stage behind the four decodes (include/infur_hip.h): a byte or u32 plane as raster-ordered
// run-length records, a per-row index and the count, so that a host copies out only as many records as there are.  Kernels:
// runs.hip.  Everything is enqueued on the context's stream; the checks, the statistics staging and the decode of the class
// plane it shares with the other egress stages are infur_egress.h's, and so is the rule that its buffers are private scratch.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kRunWords == INFUR_RUN_WORDS, "runs.hip and the header disagree about the record");

constexpr size_t kRunsScratchFloor = 64 << 10;  // block sums of 16 Mi pixels: a captured infur_runs_dev keeps its pointer

int32_t runs_check(infur_ctx* c, uint32_t elem_bytes, uint32_t flags, uint32_t skip_value) {
    return elem_check(c, elem_bytes, flags, INFUR_RUNS_SKIP, "runs", skip_value);
}
int32_t runs_wanted(infur_ctx* c, const void* runs, uint32_t runs_rows, const void* row_start, const void* n_runs) {
    if ((runs && runs_rows) || row_start || n_runs) return INFUR_OK;
    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: runs (with rows), row_start or n_runs");
}
// the frame calls' row index: checked only where a model is loaded, so that without one Scale still runs
int32_t row_index_check(infur_ctx* c, const void* row_start, uint32_t row_start_rows, uint32_t h) {
    if (c->loaded && row_start && row_start_rows < (size_t)h + 1)
        return fail(c, INFUR_E_CAPACITY, "the row index needs %zu words, buffer has %u", (size_t)h + 1, row_start_rows);
    return INFUR_OK;
}

// st_runs_io: [count][row_start, h + 1 words][statistics table k x 8 u64][records, at most one per pixel][plane], on 256-byte boundaries
struct RunStage {
    size_t rows, row_start, stats, runs, plane, bytes;
    RunStage(size_t npix, size_t h, uint32_t runs_rows, uint32_t k, size_t plane_bytes) {
        rows = runs_rows < npix ? runs_rows : npix;
        row_start = 256;
        stats = row_start + align_up((h + 1) * 4, 256);
        runs = stats + align_up((size_t)k * INFUR_STAT_WORDS * 8, 256);
        plane = runs + align_up(rows * INFUR_RUN_WORDS * 4, 256);
        bytes = plane + align_up(plane_bytes, 256);
    }
};

// count, per-row index and the written records to the host: the count decides how many records there are to copy
int32_t runs_read_back(infur_ctx* c, const uint8_t* base, const RunStage& st, size_t h, uint32_t* runs, uint32_t* row_start, uint32_t* n_runs) {
    uint32_t n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
    if (row_start) HIPCHK(c, hipMemcpyAsync(row_start, base + st.row_start, (h + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t rows = n < st.rows ? n : st.rows;
    if (runs && rows) HIPCHK(c, hipMemcpy(runs, base + st.runs, rows * INFUR_RUN_WORDS * 4, hipMemcpyDeviceToHost));
    if (n_runs) *n_runs = n;
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_runs_dev(infur_ctx* c, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value,
                       void* d_runs, uint32_t runs_rows, void* d_row_start, void* d_n) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(runs_check(c, elem_bytes, flags, skip_value));
        RETIF(plane_check(c, h, w, "a run"));
        const size_t hw = (size_t)h * w;
        RETIF(runs_wanted(c, d_runs, runs_rows, d_row_start, d_n));
        if (hw == 0) {  // empty plane: no run, every row starts at 0
            if (d_n) HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
            if (d_row_start) HIPCHK(c, hipMemsetAsync(d_row_start, 0, ((size_t)h + 1) * 4, c->stream));
            return INFUR_OK;
        }
        if (!d_plane) return no_plane(c, h, w);
        const size_t scratch = runs_scratch_bytes(hw);
        RETIF(ensure_private(c, c->st_runs, scratch > kRunsScratchFloor ? scratch : kRunsScratchFloor));
        ProfScope ps(c, "runs", "runs", 0, (double)hw * elem_bytes * ((d_runs && runs_rows) || d_row_start ? 2 : 1));
        HIPCHK(c, launch_runs(d_plane, (int)elem_bytes, h, w, (flags & INFUR_RUNS_SKIP) != 0, skip_value, c->st_runs.p, (unsigned*)d_runs, runs_rows,
                              (unsigned*)d_row_start, (unsigned*)d_n, c->stream));
        return INFUR_OK;
    });
}

int32_t infur_runs(infur_ctx* c, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags, uint32_t skip_value, uint32_t* runs,
                   uint32_t runs_rows, uint32_t* row_start, uint32_t* n_runs) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        RETIF(runs_check(c, elem_bytes, flags, skip_value));
        RETIF(plane_check(c, h, w, "a run"));
        const size_t hw = (size_t)h * w;
        RETIF(runs_wanted(c, runs, runs_rows, row_start, n_runs));
        if (hw == 0) {
            if (n_runs) *n_runs = 0;
            if (row_start) std::memset(row_start, 0, ((size_t)h + 1) * 4);
            return INFUR_OK;
        }
        if (!plane) return no_plane(c, h, w);
        const RunStage st(hw, h, runs ? runs_rows : 0, 0, hw * elem_bytes);
        RETIF(ensure_private(c, c->st_runs_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_runs_io.p;
        HIPCHK(c, hipMemcpyAsync(base + st.plane, plane, hw * elem_bytes, hipMemcpyHostToDevice, c->stream));
        RETIF(infur_runs_dev(c, base + st.plane, elem_bytes, h, w, flags, skip_value, st.rows ? base + st.runs : nullptr, (uint32_t)st.rows,
                             row_start ? base + st.row_start : nullptr, base));
        return runs_read_back(c, base, st, h, runs, row_start, n_runs);
    });
}

int32_t infur_frame_runs_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                             uint32_t skip_value, void* d_runs, uint32_t runs_rows, void* d_row_start, uint32_t row_start_rows, void* d_n,
                             void* d_stats, uint32_t stats_capacity, void* d_scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(runs_check(c, 1, flags, skip_value));
        void* kl = nullptr;
        RETIF(frame_class_plane(c, c->st_runs_plane, d_bgr, w, h, factor, mode, decode, d_stats, stats_capacity, d_scaled, ow, oh, &kl, [&](uint32_t rows) {
            RETIF(runs_wanted(c, d_runs, runs_rows, d_row_start, d_n));
            return row_index_check(c, d_row_start, row_start_rows, rows);
        }));
        return infur_runs_dev(c, kl, 1, *oh, *ow, flags, skip_value, d_runs, runs_rows, d_row_start, d_n);
    });
}

int32_t infur_frame_runs(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode, uint32_t flags,
                         uint32_t skip_value, uint32_t* runs, uint32_t runs_rows, uint32_t* row_start, uint32_t row_start_rows, uint32_t* n_runs,
                         uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled, uint32_t* ow, uint32_t* oh) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(runs_check(c, 1, flags, skip_value));
        RunStage st(0, 0, 0, 0, 0);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                RETIF(row_index_check(c, row_start, row_start_rows, *oh));
                st = RunStage(npix, *oh, runs ? runs_rows : 0, staged_classes(stats, stats_capacity), 0);
                RETIF(ensure_private(c, c->st_runs_io, st.bytes));
                base = (uint8_t*)c->st_runs_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                return infur_frame_runs_dev(c, d_bgr, w, h, factor, mode, decode, flags, skip_value, st.rows ? base + st.runs : nullptr, (uint32_t)st.rows,
                                            row_start ? base + st.row_start : nullptr, row_start_rows, ((runs && runs_rows) || row_start || n_runs) ? base : nullptr,
                                            stats ? base + st.stats : nullptr, stats_capacity, d_scaled, ow, oh);
            },
            [&](size_t) -> int32_t {
                RETIF(stats_read_back(c, stats, base + st.stats));
                return runs_read_back(c, base, st, *oh, runs, row_start, n_runs);
            });
    });
}

}  // extern "C"
