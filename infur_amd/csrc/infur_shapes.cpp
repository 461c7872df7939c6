// infur_shapes.cpp -- Shapes, the descriptor stage behind Outlines (include/infur_hip.h): per loop its area, perimeter, moments,
// convex hull and minimum rectangle, per value the sums, so that a host learns what shape an object has without pulling its
// polygon across PCIe.  Kernels: shapes.hip.  Everything is enqueued on the context's stream; the checks and row rules are the
// egress stages' (infur_egress.h), and so is the rule that its buffers are private scratch: growing them leaves mem_gen -- and
// with it the graphs infur_frame_advance_dev has cached -- alone.
#include "infur_egress.h"

using namespace infur;

namespace {

static_assert(kShapeWords == INFUR_SHAPE_WORDS && kShapesCountWords == INFUR_SHAPES_COUNT_WORDS && kShapesTruncated == INFUR_SHAPES_TRUNCATED &&
                  kShapesMalformed == INFUR_SHAPES_MALFORMED && kShapeMeasures == INFUR_SHAPE_HULL_AREA2,
              "shapes.hip and the header disagree");

constexpr size_t kShapeBytes = INFUR_SHAPE_WORDS * 8;

// the caller's five outputs, host or device pointers
struct ShapesOut {
    void* loops;
    uint32_t loops_rows;
    void* vertices;
    uint32_t vertex_rows;
    void* shapes;
    uint32_t shape_rows;
    void* values;
    uint32_t value_rows;
    void* counts;
    bool any() const { return (loops && loops_rows) || (vertices && vertex_rows) || (shapes && shape_rows) || (values && value_rows) || counts; }
};

int32_t shapes_wanted(infur_ctx* c, const ShapesOut& o) {
    if (o.any()) return INFUR_OK;
    return fail(c, INFUR_E_INVALID_ARG, "no output wanted: loops_out, vertices_out, shapes, values (each with rows) or counts_out");
}

// Simplify's checks, in Simplify's order
int32_t shapes_check(infur_ctx* c, uint32_t h, uint32_t w, const ShapesOut& o, const void* loops, uint32_t loops_rows_in, const void* vertices,
                     uint32_t vertex_rows_in, const void* counts) {
    RETIF(side_check(c, h, w, true));
    RETIF(shapes_wanted(c, o));
    return input_check(c, loops, loops_rows_in, vertices, vertex_rows_in, counts);
}

// the staging of the outputs, in st_shapes_io behind `from`: [counts][records][vertices][shapes][values], on 256-byte boundaries
struct OutStage {
    size_t loops_rows, vertex_rows, shape_rows, value_rows;
    size_t counts, loops, vertices, shapes, values, bytes;
    OutStage(size_t from, const ShapesOut& o, size_t most_loops, size_t most_vertices) {
        loops_rows = stage_rows(o.loops, o.loops_rows, most_loops);
        vertex_rows = stage_rows(o.vertices, o.vertex_rows, most_vertices);
        shape_rows = stage_rows(o.shapes, o.shape_rows, most_loops);
        value_rows = o.values ? o.value_rows : 0;  // every row is written
        counts = from;
        loops = counts + kSlotAlign;
        vertices = loops + align_up(loops_rows * kLoopBytes, kSlotAlign);
        shapes = vertices + align_up(vertex_rows * kVertexBytes, kSlotAlign);
        values = shapes + align_up(shape_rows * kShapeBytes, kSlotAlign);
        bytes = values + align_up(value_rows * kShapeBytes, kSlotAlign);
    }
    ShapesOut dev(uint8_t* base, bool counts_wanted) const {
        return {loops_rows ? base + loops : nullptr,  (uint32_t)loops_rows, vertex_rows ? base + vertices : nullptr, (uint32_t)vertex_rows,
                shape_rows ? base + shapes : nullptr, (uint32_t)shape_rows, value_rows ? base + values : nullptr,    (uint32_t)value_rows,
                counts_wanted ? base + counts : nullptr};
    }
};

// The counts first: they decide how many records and vertices there are to copy.  Truncated input wrote the counts and the
// per-value table only.
int32_t shapes_read_back(infur_ctx* c, const uint8_t* base, const OutStage& st, const ShapesOut& o) {
    uint32_t n[INFUR_SHAPES_COUNT_WORDS] = {};
    HIPCHK(c, hipMemcpyAsync(n, base + st.counts, sizeof n, hipMemcpyDeviceToHost, c->stream));
    if (st.value_rows) HIPCHK(c, hipMemcpyAsync(o.values, base + st.values, st.value_rows * kShapeBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool nothing = (n[INFUR_SHAPES_STATUS] & INFUR_SHAPES_TRUNCATED) != 0;
    const size_t nl = copy_rows(n[INFUR_SHAPES_LOOPS], st.loops_rows, nothing), nv = copy_rows(n[INFUR_SHAPES_VERTICES], st.vertex_rows),
                 ns = copy_rows(n[INFUR_SHAPES_LOOPS], st.shape_rows, nothing);
    if (nl) HIPCHK(c, hipMemcpy(o.loops, base + st.loops, nl * kLoopBytes, hipMemcpyDeviceToHost));
    if (nv) HIPCHK(c, hipMemcpy(o.vertices, base + st.vertices, nv * kVertexBytes, hipMemcpyDeviceToHost));
    if (ns) HIPCHK(c, hipMemcpy(o.shapes, base + st.shapes, ns * kShapeBytes, hipMemcpyDeviceToHost));
    if (o.counts) std::memcpy(o.counts, n, sizeof n);
    return INFUR_OK;
}

int32_t shapes_dev(infur_ctx* c, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in, const void* d_counts,
                   uint32_t h, uint32_t w, const ShapesOut& o) {
    RETIF(shapes_check(c, h, w, o, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts));
    if (vertex_rows_in == 0xFFFFFFFFu) return fail(c, INFUR_E_INVALID_ARG, "vertex_rows_in: at most 2^32 - 2");
    RETIF(ensure_private(c, c->st_shapes, shapes_scratch_bytes(loops_rows_in, vertex_rows_in)));
    ProfScope ps(c, "shapes", "shapes", 0, (double)vertex_rows_in * 4 + (double)loops_rows_in * 16);
    HIPCHK(c, launch_shapes((const unsigned*)d_loops, loops_rows_in, (const unsigned*)d_vertices, vertex_rows_in, (const unsigned*)d_counts, w,
                            c->st_shapes.p, o.loops_rows ? (unsigned*)o.loops : nullptr, o.loops ? o.loops_rows : 0,
                            o.vertex_rows ? (unsigned*)o.vertices : nullptr, o.vertices ? o.vertex_rows : 0,
                            o.shape_rows ? (long long*)o.shapes : nullptr, o.shapes ? o.shape_rows : 0, o.value_rows ? (long long*)o.values : nullptr,
                            o.values ? o.value_rows : 0, (unsigned*)o.counts, c->stream));
    return INFUR_OK;
}

}  // namespace

extern "C" {

int32_t infur_shapes_dev(infur_ctx* c, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices, uint32_t vertex_rows_in,
                         const void* d_counts, uint32_t h, uint32_t w, void* d_loops_out, uint32_t loops_rows_out, void* d_vertices_out,
                         uint32_t vertex_rows_out, void* d_shapes, uint32_t shape_rows, void* d_values, uint32_t value_rows, void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        return shapes_dev(c, d_loops, loops_rows_in, d_vertices, vertex_rows_in, d_counts, h, w,
                          {d_loops_out, loops_rows_out, d_vertices_out, vertex_rows_out, d_shapes, shape_rows, d_values, value_rows, d_counts_out});
    });
}

int32_t infur_shapes(infur_ctx* c, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices, uint32_t vertex_rows_in,
                     const uint32_t* counts, uint32_t h, uint32_t w, uint32_t* loops_out, uint32_t loops_rows_out, uint32_t* vertices_out,
                     uint32_t vertex_rows_out, uint64_t* shapes, uint32_t shape_rows, uint64_t* values, uint32_t value_rows, uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c) return INFUR_E_INVALID_ARG;
        const ShapesOut o = {loops_out, loops_rows_out, vertices_out, vertex_rows_out, shapes, shape_rows, values, value_rows, counts_out};
        RETIF(shapes_check(c, h, w, o, loops, loops_rows_in, vertices, vertex_rows_in, counts));
        // only what the counts say there is travels; an output is never longer than its input
        const size_t nl = copy_rows(counts[0], loops_rows_in), nv = copy_rows(counts[1], vertex_rows_in);
        const PolyStage in(0, 0, 0, nl, nv, 0);
        const OutStage st(in.bytes, o, nl, nv);
        RETIF(ensure_private(c, c->st_shapes_io, st.bytes));
        uint8_t* base = (uint8_t*)c->st_shapes_io.p;
        HIPCHK(c, hipMemcpyAsync(base + in.counts_in, counts, 8, hipMemcpyHostToDevice, c->stream));
        if (nl) HIPCHK(c, hipMemcpyAsync(base + in.loops_in, loops, nl * kLoopBytes, hipMemcpyHostToDevice, c->stream));
        if (nv) HIPCHK(c, hipMemcpyAsync(base + in.vertices_in, vertices, nv * kVertexBytes, hipMemcpyHostToDevice, c->stream));
        // (the rows declared to the device are what was copied: truncated input stays truncated, counts[k] > rows)
        ShapesOut d = st.dev(base, true);
        RETIF(shapes_dev(c, base + in.loops_in, (uint32_t)nl, base + in.vertices_in, (uint32_t)nv, base + in.counts_in, h, w, d));
        return shapes_read_back(c, base, st, o);
    });
}

int32_t infur_frame_shapes_dev(infur_ctx* c, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                               uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass, void* d_conf, size_t plane_cap, void* d_labels,
                               size_t labels_cap, void* d_table, uint32_t table_rows, void* d_n, void* d_scaled, uint32_t* ow, uint32_t* oh,
                               uint32_t max_edges, void* d_loops_out, uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out,
                               void* d_shapes, uint32_t shape_rows, void* d_values, void* d_counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const ShapesOut o = {d_loops_out, loops_rows_out, d_vertices_out, vertex_rows_out, d_shapes, shape_rows, d_values, table_rows, d_counts_out};
        const bool shp = o.any();  // whether there is anything to do behind Regions
        const size_t npix = scale_npix(w, h, factor);
        uint32_t sw = 0, sh = 0;
        if (shp && npix && infur_scale_out_dims(w, h, factor, &sw, &sh) == INFUR_OK) RETIF(side_check(c, sh, sw, false));
        void* lb = d_labels;
        size_t lb_cap = labels_cap;
        PolyScratch at(1);
        if (c->loaded && npix) {
            if (!d_labels && !d_table && !d_n && !shp) return INFUR_E_INVALID_ARG;
            if (d_labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
            if (!lb && shp) {  // the label plane Outlines reads, when the caller does not want it
                RETIF(ensure_private(c, c->st_shapes_plane, npix * 4));
                lb = c->st_shapes_plane.p;
                lb_cap = npix * 4;
            }
            if (shp) {
                at = PolyScratch(edge_capacity(npix, max_edges));
                RETIF(ensure_private(c, c->st_shapes_poly, at.bytes));
            }
        }  // (otherwise the call below fails before it decodes: bad scale, empty frame or no model)
        // scale -> model -> Segments decode -> Regions, with that call's own checks, errors and MODEL_NOT_LOADED rule
        RETIF(infur_frame_regions_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, d_klass, d_conf, plane_cap, lb, lb_cap,
                                      d_table, table_rows, d_n, d_scaled, ow, oh));
        if (!shp) return INFUR_OK;
        uint8_t* base = (uint8_t*)c->st_shapes_poly.p;
        const uint32_t oflags = INFUR_OUTLINES_SKIP | (connectivity == INFUR_CONNECT_8 ? INFUR_OUTLINES_CONN8 : 0);
        RETIF(infur_outlines_dev(c, lb, 4, *oh, *ow, oflags, INFUR_REGION_NONE, max_edges, base + at.loops, (uint32_t)at.loops_rows, base + at.vertices,
                                 (uint32_t)at.vertex_rows, base));
        return shapes_dev(c, base + at.loops, (uint32_t)at.loops_rows, base + at.vertices, (uint32_t)at.vertex_rows, base, *oh, *ow, o);
    });
}

int32_t infur_frame_shapes(infur_ctx* c, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t mode, uint32_t decode,
                           uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_cap, uint32_t* labels,
                           size_t labels_cap, uint64_t* table, uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled, uint32_t* ow, uint32_t* oh,
                           uint32_t max_edges, uint32_t* loops_out, uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out,
                           uint64_t* shapes, uint32_t shape_rows, uint64_t* values, uint32_t* counts_out) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !ow || !oh) return INFUR_E_INVALID_ARG;
        RETIF(reg_check(c, connectivity, flags));
        const ShapesOut o = {loops_out, loops_rows_out, vertices_out, vertex_rows_out, shapes, shape_rows, values, table_rows, counts_out};
        const bool shp = o.any();  // whether there is anything to do behind Regions
        // st_shapes_io: [n][table, at most one row per pixel][label plane][class plane][confidence plane], then the outputs
        size_t rows = 0, at_table = 256, at_labels = 0, at_klass = 0, at_conf = 0;
        OutStage st(0, ShapesOut{}, 0, 0);
        uint8_t* base = nullptr;
        return frame_host(
            c, bgr, w, h, factor, scaled, ow, oh,
            [&](size_t npix) -> int32_t {
                if ((klass || conf) && plane_cap < npix) return fail(c, INFUR_E_CAPACITY, "a plane needs %zu bytes, buffer has %zu", npix, plane_cap);
                if (labels && labels_cap < npix * 4) return fail(c, INFUR_E_CAPACITY, "the label plane needs %zu bytes, buffer has %zu", npix * 4, labels_cap);
                rows = table ? min_rows(table_rows, npix) : 0;
                at_labels = at_table + align_up(rows * INFUR_REGION_WORDS * 8, 256);
                at_klass = at_labels + align_up(npix * 4, 256);
                at_conf = at_klass + align_up(npix, 256);
                st = OutStage(at_conf + align_up(npix, 256), o, frame_max_loops(npix), frame_max_vertices(npix));
                RETIF(ensure_private(c, c->st_shapes_io, st.bytes));
                base = (uint8_t*)c->st_shapes_io.p;
                return INFUR_OK;
            },
            [&](void* d_bgr, void* d_scaled) {
                const size_t npix = (size_t)*ow * *oh;
                const ShapesOut d = st.dev(base, shp);
                // (table_rows reaches the device call as given when the per-value table is wanted: its rows are all written)
                return infur_frame_shapes_dev(c, d_bgr, w, h, factor, mode, decode, connectivity, min_pixels, flags, base + at_klass,
                                              (conf || table) ? base + at_conf : nullptr, npix, (labels || shp) ? base + at_labels : nullptr, npix * 4,
                                              (table && rows) ? base + at_table : nullptr, values ? table_rows : (uint32_t)rows,
                                              (labels || table || n_regions) ? base : nullptr, d_scaled, ow, oh, max_edges, d.loops, d.loops_rows,
                                              d.vertices, d.vertex_rows, d.shapes, d.shape_rows, d.values, d.counts);
            },
            [&](size_t npix) -> int32_t {
                if (klass) HIPCHK(c, hipMemcpyAsync(klass, base + at_klass, npix, hipMemcpyDeviceToHost, c->stream));
                if (conf) HIPCHK(c, hipMemcpyAsync(conf, base + at_conf, npix, hipMemcpyDeviceToHost, c->stream));
                uint32_t n = 0;
                HIPCHK(c, hipMemcpyAsync(&n, base, 4, hipMemcpyDeviceToHost, c->stream));
                if (labels) HIPCHK(c, hipMemcpyAsync(labels, base + at_labels, npix * 4, hipMemcpyDeviceToHost, c->stream));
                if (shp) RETIF(shapes_read_back(c, base, st, o));  // (synchronises)
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const size_t nr = n < rows ? n : rows;
                if (table && nr) HIPCHK(c, hipMemcpy(table, base + at_table, nr * INFUR_REGION_WORDS * 8, hipMemcpyDeviceToHost));
                if (n_regions) *n_regions = n;
                return INFUR_OK;
            });
    });
}

}  // extern "C"
