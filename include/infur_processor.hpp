// infur_processor.hpp -- header-only C++ mirror of the reference's `Processor` plugin surface
// over the C ABI of infur_hip.h.  (The reference is Rust; no Rust toolchain exists in the build
// image, so the compiled-language host layer is C++.  The Rust adapter is in INTEGRATION.md.)
//
//   trait Processor          infur/src/processing.rs:23-60
//   Scale                    infur/src/processing.rs:179-282
//   Model<f32>               infur/src/predict_onnx.rs:146-345
//   ColorCode                infur/src/decode_predict.rs:38-84
//   Segments                 ColorCode's sibling for a headless host (infur_hip.h: class / confidence planes, statistics)
//   Regions                  the third decode stage (infur_hip.h: connected components, label plane, per-region table)
//
// Rust `Result<_, E>` becomes a status code (`infur::Status`, 0 = Ok) carried by small error
// structs; `&mut Option<T>` outputs become `std::optional<T>&`; buffers are reused across calls
// exactly where the reference reuses them.
#pragma once
#include <cstdint>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "infur_hip.h"

namespace infur {

using Status = int32_t;

/// processing.rs:9-18 -- `Frame { id, img: BgrImage }`; packed B,G,R u8, row-major, no padding
struct BgrImage {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;  // height * width * 3
    BgrImage() = default;
    BgrImage(uint32_t w, uint32_t h) : width(w), height(h), data((size_t)w * h * 3, 0) {}
};
struct Frame {
    uint64_t id = 0;
    BgrImage img;
    bool operator==(const Frame& o) const { return id == o.id; }  // processing.rs:14-18
};

/// epaint ColorImage: premultiplied r,g,b,a bytes
struct ColorImage {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> rgba;  // height * width * 4
};

/// [K, H, W] f32 planar tensor (ndarray Array3 / ArrayD of the reference)
struct Tensor3 {
    uint32_t k = 0, h = 0, w = 0;
    std::vector<float> data;
};

/// RAII owner of an infur_ctx (one GPU, one stream; not thread-safe)
class Context {
public:
    /// compute_dtype: INFUR_DTYPE_F32 (exact f32 MFMA), INFUR_DTYPE_F32_SPLIT_FP8 (see infur_hip.h), INFUR_DTYPE_F32_SPLIT (f32 tensors, f16 matrix cores with
    /// hi+lo operand pairs: f32-grade logits at ~1.9x the rate) or INFUR_DTYPE_F16
    explicit Context(int device = 0, bool compute_aux = true, uint32_t compute_dtype = INFUR_DTYPE_F32) {
        infur_options o;
        infur_options_default(&o);
        o.device = device;
        o.compute_aux = compute_aux ? 1 : 0;
        o.compute_dtype = compute_dtype;
        status_ = infur_ctx_create(&o, &ctx_);
    }
    ~Context() { infur_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    bool ok() const { return status_ == INFUR_OK; }
    Status status() const { return status_; }
    infur_ctx* get() const { return ctx_; }
    std::string last_error() const { return ctx_ ? infur_last_error(ctx_) : infur_status_string(status_); }

private:
    infur_ctx* ctx_ = nullptr;
    Status status_ = INFUR_OK;
};

/// processing.rs:179-282.  Command = f32, Input = Output = Option<Frame>.
class Scale {
public:
    explicit Scale(Context& c, uint32_t mode = INFUR_SCALE_NEAREST) : c_(c), mode_(mode) {}

    /// ValidScale::try_from + dirty tracking (processing.rs:220-226).  On error state is untouched.
    Status control(float factor) {
        Status s = infur_scale_validate(factor);
        if (s != INFUR_OK) return s;  // ValidScaleError
        dirty_ = factor != factor_;
        factor_ = factor;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }

    /// processing.rs:232-281
    Status advance(const std::optional<Frame>& input, std::optional<Frame>& out) {
        dirty_ = false;
        if (!input) return INFUR_OK;
        if (factor_ == 1.0f) {  // clone
            out = *input;
            return INFUR_OK;
        }
        uint32_t ow = 0, oh = 0;
        Status s = infur_scale_out_dims(input->img.width, input->img.height, factor_, &ow, &oh);
        if (s != INFUR_OK) return s;  // ZeroSizeIn / ZeroSizeOut
        if (!out) out = Frame{input->id, BgrImage(ow, oh)};
        if (out->img.width != ow || out->img.height != oh) out->img = BgrImage(ow, oh);  // only on size change
        out->id = input->id;
        return infur_scale(c_.get(), input->img.data.data(), input->img.width, input->img.height, factor_, mode_,
                           out->img.data.data(), out->img.data.size(), &ow, &oh);
    }

private:
    Context& c_;
    uint32_t mode_;
    float factor_ = 1.0f;  // Default: ValidScale(1.0), dirty = true (processing.rs:185-193)
    bool dirty_ = true;
};

/// predict_onnx.rs:56-62
struct ModelInfo {
    std::vector<std::string> input_names;
    std::string input0_dtype;
    std::vector<std::string> output_names;
    bool quantised = false;        ///< a QOperator / QDQ int8 model: runs on the i8 MFMA whatever the context's dtype (ABI 4)
    bool resize_u8_heads = false;  ///< ... whose file resizes the u8 logits before DequantizeLinear
};

/// predict_onnx.rs:146-345.  Command = ModelCmd::Load(path), Input = BgrImage, Output = Vec<ArrayD<f32>>.
class Model {
public:
    explicit Model(Context& c) : c_(c) {}

    /// ModelCmd::Load(path); empty path unloads (predict_onnx.rs:288-312)
    Status control_load(const std::string& path) { return infur_model_load(c_.get(), path.c_str()); }
    Status control_load_blob(const void* blob, size_t len) { return infur_model_load_blob(c_.get(), blob, len); }
    bool is_dirty() const { return false; }  // predict_onnx.rs:336-338

    std::optional<ModelInfo> get_info() const {
        infur_model_info mi;
        if (infur_model_info_get(c_.get(), &mi) != INFUR_OK) return std::nullopt;
        ModelInfo r;
        r.input_names = {mi.input_name};
        r.input0_dtype = mi.input0_dtype;
        for (uint32_t i = 0; i < mi.n_outputs; i++) r.output_names.push_back(mi.output_names[i]);
        r.quantised = mi.quantised != 0;
        r.resize_u8_heads = mi.resize_u8_heads != 0;
        return r;
    }

    /// predict_onnx.rs:317-334: with no model `out` is left untouched and Ok is returned.  `out` receives as many
    /// tensors as the model has outputs (2, or 1 without the aux head / with compute_aux = false).
    Status advance(const BgrImage& img, std::vector<Tensor3>& out) {
        infur_model_info mi;
        if (infur_model_info_get(c_.get(), &mi) != INFUR_OK) return INFUR_OK;
        std::vector<Tensor3> t(mi.n_outputs);
        for (auto& x : t) {
            x.k = mi.num_classes;
            x.h = img.height;
            x.w = img.width;
            x.data.resize((size_t)x.k * x.h * x.w);
        }
        uint32_t n = 0;
        Status s = infur_model_advance(c_.get(), img.data.data(), img.width, img.height, t[0].data.data(),
                                       t.size() > 1 ? t[1].data.data() : nullptr, &n);
        if (s != INFUR_OK) return s;
        out.clear();
        for (auto& x : t) out.push_back(std::move(x));
        return INFUR_OK;
    }

private:
    Context& c_;
};

/// decode_predict.rs:38-84.  Input = Array3<f32> [K,H,W], Output = Option<ColorImage>.
class ColorCode {
public:
    explicit ColorCode(Context& c) : c_(c) {}
    Status control() { return INFUR_OK; }
    bool is_dirty() const { return false; }
    Status advance(const Tensor3& inp, std::optional<ColorImage>& out) {
        if (!out || out->width != inp.w || out->height != inp.h) {  // decode_predict.rs:58-65
            ColorImage img;
            img.width = inp.w;
            img.height = inp.h;
            img.rgba.assign((size_t)inp.w * inp.h * 4, 0);
            out = std::move(img);
        }
        return infur_colorcode(c_.get(), inp.data.data(), inp.k, inp.h, inp.w, out->rgba.data());
    }

private:
    Context& c_;
};

/// What `Segments` produces: ask with the `want_*` flags; planes are h * w bytes, `stats` is k rows of INFUR_STAT_WORDS words
/// (index with INFUR_STAT_*), `rgba` h * w * 4 bytes.  Unwanted outputs are left empty.
struct SegmentsOut {
    bool want_klass = true, want_conf = true, want_stats = true, want_rgba = false;
    uint32_t width = 0, height = 0, classes = 0;
    std::vector<uint8_t> klass, conf, rgba;
    std::vector<uint64_t> stats;
    uint64_t stat(uint32_t k, uint32_t word) const { return stats[(size_t)k * INFUR_STAT_WORDS + word]; }
};

/// ColorCode's sibling: per-pixel argmax class, confidence byte, per-class statistics, optionally the shaded overlay.
/// Command = decode mode (INFUR_DECODE_RAW: decode_predict.rs:67-78; INFUR_DECODE_SOFTMAX: the reference's README.md:76 todo).
/// Input = Array3<f32> [K,H,W], Output = SegmentsOut.
class Segments {
public:
    explicit Segments(Context& c, uint32_t decode = INFUR_DECODE_RAW) : c_(c), decode_(decode) {}
    Status control(uint32_t decode) {
        if (decode > INFUR_DECODE_SOFTMAX) return INFUR_E_INVALID_ARG;  // state untouched
        dirty_ = decode != decode_;
        decode_ = decode;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const Tensor3& inp, SegmentsOut& out) {
        dirty_ = false;
        const size_t hw = (size_t)inp.w * inp.h;
        out.width = inp.w;
        out.height = inp.h;
        out.classes = inp.k;
        out.klass.assign(out.want_klass ? hw : 0, 0);
        out.conf.assign(out.want_conf ? hw : 0, 0);
        out.rgba.assign(out.want_rgba ? hw * 4 : 0, 0);
        out.stats.assign(out.want_stats ? (size_t)inp.k * INFUR_STAT_WORDS : 0, 0);
        return infur_segments(c_.get(), inp.data.data(), inp.k, inp.h, inp.w, decode_, out.want_klass ? out.klass.data() : nullptr,
                              out.want_conf ? out.conf.data() : nullptr, out.want_stats ? out.stats.data() : nullptr,
                              out.want_rgba ? out.rgba.data() : nullptr);
    }

private:
    Context& c_;
    uint32_t decode_;
    bool dirty_ = true;
};

/// What `Regions` consumes: the planes `Segments` wrote (`conf` may be empty: the rows' SUM_CONF is then 0).
struct Planes {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> klass, conf;
};

/// What `Regions` produces: `labels` is h * w region ids (INFUR_REGION_NONE: no kept region), `table` holds min(n, table_rows)
/// rows of INFUR_REGION_WORDS words in ascending order of the regions' first pixel, `n` counts every kept region.
struct RegionsOut {
    bool want_labels = true;
    uint32_t table_rows = 1024;
    uint32_t width = 0, height = 0, n = 0;
    std::vector<uint32_t> labels;
    std::vector<uint64_t> table;
    uint32_t rows() const { return n < table_rows ? n : table_rows; }
    uint64_t word(uint32_t id, uint32_t w) const { return table[(size_t)id * INFUR_REGION_WORDS + w]; }
};

/// The third decode stage: connected components of the class plane under 4- or 8-connectivity, regions below `min_pixels`
/// dropped, optionally without the background class.  Integer results, identical from run to run.
/// Command = one of connectivity / min_pixels / flags; Input = Planes, Output = RegionsOut.
class Regions {
public:
    struct Cmd {
        enum Kind { Connectivity, MinPixels, Flags } kind;
        uint32_t value;
    };
    explicit Regions(Context& c, uint32_t connectivity = INFUR_CONNECT_8) : c_(c), connectivity_(connectivity) {}
    Status control(Cmd cmd) {
        uint32_t conn = connectivity_, minpx = min_pixels_, flags = flags_;
        switch (cmd.kind) {
            case Cmd::Connectivity:
                if (cmd.value != INFUR_CONNECT_4 && cmd.value != INFUR_CONNECT_8) return INFUR_E_INVALID_ARG;  // state untouched
                conn = cmd.value;
                break;
            case Cmd::MinPixels: minpx = cmd.value; break;
            case Cmd::Flags:
                if (cmd.value & ~(uint32_t)INFUR_REGIONS_SKIP_BACKGROUND) return INFUR_E_INVALID_ARG;
                flags = cmd.value;
                break;
            default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || conn != connectivity_ || minpx != min_pixels_ || flags != flags_;
        connectivity_ = conn;
        min_pixels_ = minpx;
        flags_ = flags;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const Planes& inp, RegionsOut& out) {
        dirty_ = false;
        const size_t hw = (size_t)inp.width * inp.height;
        if (inp.klass.size() != hw || (!inp.conf.empty() && inp.conf.size() != hw)) return INFUR_E_SHAPE;
        out.width = inp.width;
        out.height = inp.height;
        out.labels.assign(out.want_labels ? hw : 0, INFUR_REGION_NONE);
        out.table.assign((size_t)out.table_rows * INFUR_REGION_WORDS, 0);
        return infur_regions(c_.get(), inp.klass.data(), inp.conf.empty() ? nullptr : inp.conf.data(), inp.height, inp.width, connectivity_,
                             min_pixels_, flags_, out.want_labels ? out.labels.data() : nullptr,
                             out.table_rows ? out.table.data() : nullptr, out.table_rows, &out.n);
    }

private:
    Context& c_;
    uint32_t connectivity_, min_pixels_ = 0, flags_ = 0;
    bool dirty_ = true;
};

/// What `Tracks` produces: `track_of_region` and `table` hold min(n, table rows of the input) entries / rows of
/// INFUR_TRACK_WORDS words in region order (INFUR_TRACK_NONE: not tracked), `plane` is h * w track ids, `summary` the four
/// INFUR_TRACKS_SUMMARY_* words.
struct TracksOut {
    bool want_plane = false;
    uint32_t rows = 0;
    std::vector<uint32_t> track_of_region, plane;
    std::vector<uint64_t> table;
    uint32_t summary[INFUR_TRACKS_SUMMARY_WORDS] = {0, 0, 0, 0};
    uint32_t status() const { return summary[INFUR_TRACKS_SUMMARY_STATUS]; }
    uint64_t word(uint32_t id, uint32_t w) const { return table[(size_t)id * INFUR_TRACK_WORDS + w]; }
};

/// What `Tracks::memory` reads of a tracker with memory: `gap_of_region` (as many words as asked for; 0 for a region that was
/// not revived), the four INFUR_TRACK_MEMORY_* words and the gallery's first rows of INFUR_LOST_WORDS words, in gallery order.
struct TracksMemory {
    std::vector<uint32_t> gap_of_region;
    uint32_t summary[INFUR_TRACK_MEMORY_WORDS] = {0, 0, 0, 0};
    std::vector<uint64_t> lost;
    uint32_t held() const { return summary[INFUR_TRACK_MEMORY_HELD]; }
    uint64_t word(uint32_t entry, uint32_t w) const { return lost[(size_t)entry * INFUR_LOST_WORDS + w]; }
};

/// The fourth decode stage: region identities carried from frame to frame.  Owns its tracker -- one remembered frame on the
/// device -- and must not outlive its context.  A region inherits the track of the remembered region of its class it overlaps
/// most (when that region prefers it too), otherwise it starts a new one.  Integer results, identical from run to run.
/// Command = min_overlap or reset (value: the first id of the tracks that follow); Input = RegionsOut, Output = TracksOut.
class Tracks {
public:
    struct Cmd {
        enum Kind { MinOverlap, Reset } kind;
        uint32_t value;
    };
    explicit Tracks(Context& c, uint32_t max_regions = 0, uint32_t pair_slots = 0) {
        status_ = infur_tracker_create(c.get(), max_regions, pair_slots, &t_);
    }
    ~Tracks() { infur_tracker_destroy(t_); }
    Tracks(const Tracks&) = delete;
    Tracks& operator=(const Tracks&) = delete;
    bool ok() const { return status_ == INFUR_OK; }
    void* get() const { return t_; }
    Status control(Cmd cmd) {
        switch (cmd.kind) {
            case Cmd::MinOverlap:
                dirty_ = dirty_ || cmd.value != min_overlap_;
                min_overlap_ = cmd.value;
                return INFUR_OK;
            case Cmd::Reset: dirty_ = true; return infur_tracker_reset(t_, cmd.value);
            default: return INFUR_E_INVALID_ARG;
        }
    }
    bool is_dirty() const { return dirty_; }
    /// Keep lost tracks for up to `max_lost` steps (0: memory off); forgets the remembered frame and the gallery.
    Status set_memory(uint32_t max_lost, uint32_t reach = 0, uint32_t gallery_rows = 0) {
        dirty_ = true;
        return infur_tracker_set_memory(t_, max_lost, reach, gallery_rows);
    }
    /// What the last step left: `rows` words of gap_of_region, the memory summary, at most `lost_rows` gallery rows.
    /// INFUR_E_INVALID_ARG on a tracker without memory.
    Status memory(TracksMemory& out, uint32_t rows, uint32_t lost_rows = 0) const {
        out.gap_of_region.assign(rows, 0);
        out.lost.assign((size_t)lost_rows * INFUR_LOST_WORDS, 0);
        const Status s = infur_tracker_memory(t_, rows ? out.gap_of_region.data() : nullptr, rows, out.summary,
                                              lost_rows ? out.lost.data() : nullptr, lost_rows);
        const uint32_t got = out.held() < lost_rows ? out.held() : lost_rows;  // the rows the call wrote
        out.lost.resize(s == INFUR_OK ? (size_t)got * INFUR_LOST_WORDS : 0);
        return s;
    }
    Status advance(const RegionsOut& inp, TracksOut& out) {
        dirty_ = false;
        const size_t hw = (size_t)inp.width * inp.height;
        if (inp.labels.size() != hw) return INFUR_E_SHAPE;  // (a RegionsOut made with want_labels)
        const uint32_t rows = (uint32_t)(inp.table.size() / INFUR_REGION_WORDS);
        out.rows = hw ? (inp.n < rows ? inp.n : rows) : 0;
        out.track_of_region.assign(rows, INFUR_TRACK_NONE);
        out.table.assign((size_t)rows * INFUR_TRACK_WORDS, 0);
        out.plane.assign(out.want_plane ? hw : 0, INFUR_TRACK_NONE);
        const Status s = infur_tracks(t_, inp.labels.data(), inp.table.data(), rows, inp.n, inp.height, inp.width, min_overlap_,
                                      rows ? out.track_of_region.data() : nullptr, out.want_plane && hw ? out.plane.data() : nullptr,
                                      rows ? out.table.data() : nullptr, out.summary);
        out.track_of_region.resize(out.rows);
        out.table.resize((size_t)out.rows * INFUR_TRACK_WORDS);
        return s;
    }

private:
    void* t_ = nullptr;
    Status status_ = INFUR_OK;
    uint32_t min_overlap_ = 1;
    bool dirty_ = true;
};

/// What `Runs` produces: `runs` holds min(n, runs_rows) records of INFUR_RUN_WORDS words in raster order, `row_start` the
/// height + 1 words of the per-row index, `n` counts every run (above runs_rows: truncated).
struct RunsOut {
    uint32_t runs_rows = 1u << 16;
    bool want_row_start = true;
    uint32_t width = 0, height = 0, n = 0;
    std::vector<uint32_t> runs, row_start;
    uint32_t rows() const { return n < runs_rows ? n : runs_rows; }
    uint32_t word(uint32_t run, uint32_t w) const { return runs[(size_t)run * INFUR_RUN_WORDS + w]; }
};

/// The egress stage: a byte plane (class, confidence) or a u32 plane (labels, tracks) as raster-ordered runs of equal values
/// within a row.  Integer results, identical from run to run.
/// Command = skip (the runs of `value` are dropped) or emit everything; Input = a plane of uint8_t or uint32_t, Output = RunsOut.
class Runs {
public:
    struct Cmd {
        enum Kind { Skip, NoSkip } kind;
        uint32_t value;
    };
    explicit Runs(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        const uint32_t flags = cmd.kind == Cmd::Skip ? (uint32_t)INFUR_RUNS_SKIP : 0u, value = cmd.kind == Cmd::Skip ? cmd.value : 0u;
        if (cmd.kind != Cmd::Skip && cmd.kind != Cmd::NoSkip) return INFUR_E_INVALID_ARG;
        dirty_ = dirty_ || flags != flags_ || value != skip_value_;
        flags_ = flags;
        skip_value_ = value;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const std::vector<uint8_t>& plane, uint32_t height, uint32_t width, RunsOut& out) {
        return run(plane.data(), plane.size(), 1, height, width, out);
    }
    Status advance(const std::vector<uint32_t>& plane, uint32_t height, uint32_t width, RunsOut& out) {
        return run(plane.data(), plane.size(), 4, height, width, out);
    }

private:
    Status run(const void* plane, size_t elems, uint32_t elem_bytes, uint32_t height, uint32_t width, RunsOut& out) {
        dirty_ = false;
        if (elems != (size_t)width * height) return INFUR_E_SHAPE;
        out.width = width;
        out.height = height;
        out.n = 0;
        out.runs.assign((size_t)out.runs_rows * INFUR_RUN_WORDS, 0);
        out.row_start.assign(out.want_row_start ? (size_t)height + 1 : 0, 0);
        const Status s = infur_runs(c_.get(), plane, elem_bytes, height, width, flags_, skip_value_, out.runs_rows ? out.runs.data() : nullptr,
                                    out.runs_rows, out.want_row_start ? out.row_start.data() : nullptr, &out.n);
        out.runs.resize((size_t)out.rows() * INFUR_RUN_WORDS);
        return s;
    }
    Context& c_;
    uint32_t flags_ = 0, skip_value_ = 0;
    bool dirty_ = true;
};

/// What `Anchors` produces: `dist2` holds the width * height squared distances to the nearest pixel of another value or to the
/// frame (0: a skipped pixel), `anchors` `rows` rows of INFUR_ANCHOR_WORDS words, one per value below `rows`;
/// (INFUR_ANCHOR_NONE, 0): no pixel holds the value.
struct AnchorsOut {
    uint32_t rows = 256;
    bool want_dist2 = true;
    uint32_t width = 0, height = 0;
    std::vector<uint32_t> dist2, anchors;
    uint32_t word(uint32_t row, uint32_t w) const { return anchors[(size_t)row * INFUR_ANCHOR_WORDS + w]; }
    bool has(uint32_t row) const { return word(row, INFUR_ANCHOR_PIXEL) != INFUR_ANCHOR_NONE; }
    uint32_t x(uint32_t row) const { return word(row, INFUR_ANCHOR_PIXEL) % width; }
    uint32_t y(uint32_t row) const { return word(row, INFUR_ANCHOR_PIXEL) / width; }
};

/// The stage that measures how thick a region is: the exact squared distance transform of a byte plane (class) or a u32 plane
/// (labels, tracks) by value, the frame counting as a border, and per value its most interior pixel (ties to the smallest index).
/// Integer results, identical from run to run.
/// Command = skip (the pixels of `value` belong to no region) or not; Input = a plane of uint8_t or uint32_t, Output = AnchorsOut.
class Anchors {
public:
    struct Cmd {
        enum Kind { Skip, NoSkip } kind;
        uint32_t value;
    };
    explicit Anchors(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        const uint32_t flags = cmd.kind == Cmd::Skip ? (uint32_t)INFUR_ANCHORS_SKIP : 0u, value = cmd.kind == Cmd::Skip ? cmd.value : 0u;
        if (cmd.kind != Cmd::Skip && cmd.kind != Cmd::NoSkip) return INFUR_E_INVALID_ARG;
        dirty_ = dirty_ || flags != flags_ || value != skip_value_;
        flags_ = flags;
        skip_value_ = value;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const std::vector<uint8_t>& plane, uint32_t height, uint32_t width, AnchorsOut& out) {
        return run(plane.data(), plane.size(), 1, height, width, out);
    }
    Status advance(const std::vector<uint32_t>& plane, uint32_t height, uint32_t width, AnchorsOut& out) {
        return run(plane.data(), plane.size(), 4, height, width, out);
    }

private:
    Status run(const void* plane, size_t elems, uint32_t elem_bytes, uint32_t height, uint32_t width, AnchorsOut& out) {
        dirty_ = false;
        if (elems != (size_t)width * height) return INFUR_E_SHAPE;
        out.width = width;
        out.height = height;
        out.dist2.assign(out.want_dist2 ? elems : 0, 0);
        out.anchors.assign((size_t)out.rows * INFUR_ANCHOR_WORDS, 0);
        return infur_anchors(c_.get(), plane, elem_bytes, height, width, flags_, skip_value_, out.want_dist2 ? out.dist2.data() : nullptr,
                             out.rows ? out.anchors.data() : nullptr, out.rows);
    }
    Context& c_;
    uint32_t flags_ = 0, skip_value_ = 0;
    bool dirty_ = true;
};

/// What `Compare` produces for `rows_a` x `rows_b` values: `matrix` row-major (pixels with a == i and b == j), `a` and `b` rows of
/// INFUR_COMPARE_WORDS words per value of either plane ((0, INFUR_COMPARE_NONE, 0, 0): no compared pixel holds the value) and the
/// INFUR_COMPARE_COUNT_WORDS counts.
struct CompareOut {
    uint32_t rows_a = 21, rows_b = 21;
    bool want_matrix = true;
    std::vector<uint32_t> matrix, a, b, counts;
    uint32_t at(uint32_t i, uint32_t j) const { return matrix[(size_t)i * rows_b + j]; }
    uint32_t count(uint32_t word) const { return counts[word]; }
    /// row i of a's table is matched: 2 INTER > UNION, the rule of panoptic quality
    bool matched_a(uint32_t i) const {
        return 2ull * a[(size_t)i * INFUR_COMPARE_WORDS + INFUR_COMPARE_INTER] > a[(size_t)i * INFUR_COMPARE_WORDS + INFUR_COMPARE_UNION];
    }
    /// the share of the pixels that take part on which the planes agree; -1 when there is none
    double pixel_accuracy() const {
        const uint32_t n = count(INFUR_COMPARE_COMPARED) - count(INFUR_COMPARE_OUTSIDE);
        return n ? (double)count(INFUR_COMPARE_EQUAL) / n : -1.0;
    }
};

/// The stage that grades a result: the confusion matrix of two planes -- byte planes (class) or u32 planes (labels, tracks), in
/// any combination -- and per value of either its best partner in the other with intersection and union.  Integer results,
/// identical from run to run.
/// Command = which value of either plane is not compared, and the pair table's slots; Input = two planes of one size,
/// Output = CompareOut.
class Compare {
public:
    struct Cmd {
        enum Kind { IgnoreA, IgnoreB, IgnoreNone, PairSlots } kind;
        uint32_t value;
    };
    explicit Compare(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        uint32_t flags = flags_, ia = ignore_a_, ib = ignore_b_, slots = pair_slots_;
        switch (cmd.kind) {
        case Cmd::IgnoreA: flags |= INFUR_COMPARE_IGNORE_A, ia = cmd.value; break;
        case Cmd::IgnoreB: flags |= INFUR_COMPARE_IGNORE_B, ib = cmd.value; break;
        case Cmd::IgnoreNone: flags = ia = ib = 0; break;
        case Cmd::PairSlots: slots = cmd.value; break;
        default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || flags != flags_ || ia != ignore_a_ || ib != ignore_b_ || slots != pair_slots_;
        flags_ = flags, ignore_a_ = ia, ignore_b_ = ib, pair_slots_ = slots;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    template <class A, class B>
    Status advance(const std::vector<A>& a, const std::vector<B>& b, uint32_t height, uint32_t width, CompareOut& out) {
        static_assert((sizeof(A) == 1 || sizeof(A) == 4) && (sizeof(B) == 1 || sizeof(B) == 4), "planes of uint8_t or uint32_t");
        dirty_ = false;
        if (a.size() != (size_t)width * height || b.size() != a.size()) return INFUR_E_SHAPE;
        out.matrix.assign(out.want_matrix ? (size_t)out.rows_a * out.rows_b : 0, 0);
        out.a.assign((size_t)out.rows_a * INFUR_COMPARE_WORDS, 0);
        out.b.assign((size_t)out.rows_b * INFUR_COMPARE_WORDS, 0);
        out.counts.assign(INFUR_COMPARE_COUNT_WORDS, 0);
        return infur_compare(c_.get(), a.data(), sizeof(A), b.data(), sizeof(B), height, width, flags_, ignore_a_, ignore_b_,
                             out.matrix.empty() ? nullptr : out.matrix.data(), out.rows_a, out.rows_b, out.a.empty() ? nullptr : out.a.data(),
                             out.b.empty() ? nullptr : out.b.data(), out.counts.data(), pair_slots_);
    }

private:
    Context& c_;
    uint32_t flags_ = 0, ignore_a_ = 0, ignore_b_ = 0, pair_slots_ = 0;
    bool dirty_ = true;
};

/// What `Adjacency` produces for `rows` values: `pairs` holds the WRITTEN = min(PAIRS, pair_rows) records of INFUR_ADJ_PAIR_WORDS
/// words (A < B, BORDER, FIRST) in ascending FIRST, `table` INFUR_ADJ_ROW_WORDS words per value (DEGREE, LONGEST, BORDER,
/// PERIMETER; LONGEST == INFUR_ADJ_NONE: no neighbour) and the INFUR_ADJ_COUNT_WORDS counts.
struct AdjacencyOut {
    uint32_t rows = 21, pair_rows = 4096;
    std::vector<uint32_t> pairs, table, counts;
    uint32_t count(uint32_t word) const { return counts[word]; }
    uint32_t n_pairs() const { return (uint32_t)(pairs.size() / INFUR_ADJ_PAIR_WORDS); }
    /// the border edges between the values a and b: 0 when they do not touch (or the record was not written)
    uint32_t border(uint32_t a, uint32_t b) const {
        if (a > b) { const uint32_t t = a; a = b, b = t; }
        for (size_t i = 0; i + INFUR_ADJ_PAIR_WORDS <= pairs.size(); i += INFUR_ADJ_PAIR_WORDS)
            if (pairs[i + INFUR_ADJ_A] == a && pairs[i + INFUR_ADJ_B] == b) return pairs[i + INFUR_ADJ_BORDER];
        return 0;
    }
};

/// The region adjacency graph of a plane -- a byte plane (class) or a u32 plane (labels, tracks): which values touch along how
/// many pixel edges.  Integer results, identical from run to run.
/// Command = the value that belongs to no region, and the pair table's slots; Input = a plane, Output = AdjacencyOut.
class Adjacency {
public:
    struct Cmd {
        enum Kind { Skip, SkipNone, PairSlots } kind;
        uint32_t value;
    };
    explicit Adjacency(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        uint32_t flags = flags_, skip = skip_, slots = pair_slots_;
        switch (cmd.kind) {
        case Cmd::Skip: flags = INFUR_ADJ_SKIP, skip = cmd.value; break;
        case Cmd::SkipNone: flags = skip = 0; break;
        case Cmd::PairSlots: slots = cmd.value; break;
        default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || flags != flags_ || skip != skip_ || slots != pair_slots_;
        flags_ = flags, skip_ = skip, pair_slots_ = slots;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    template <class T>
    Status advance(const std::vector<T>& plane, uint32_t height, uint32_t width, AdjacencyOut& out) {
        static_assert(sizeof(T) == 1 || sizeof(T) == 4, "a plane of uint8_t or uint32_t");
        dirty_ = false;
        if (plane.size() != (size_t)width * height) return INFUR_E_SHAPE;
        out.pairs.assign((size_t)out.pair_rows * INFUR_ADJ_PAIR_WORDS, 0);
        out.table.assign((size_t)out.rows * INFUR_ADJ_ROW_WORDS, 0);
        out.counts.assign(INFUR_ADJ_COUNT_WORDS, 0);
        uint32_t none = 0;  // (a pointer for zero records: they are wanted, and none fits)
        const Status rc = infur_adjacency(c_.get(), plane.data(), sizeof(T), height, width, flags_, skip_, out.rows,
                                          out.pairs.empty() ? &none : out.pairs.data(), out.pair_rows, out.table.empty() ? nullptr : out.table.data(),
                                          out.counts.data(), pair_slots_);
        out.pairs.resize(rc == INFUR_OK ? (size_t)out.counts[INFUR_ADJ_WRITTEN] * INFUR_ADJ_PAIR_WORDS : 0);
        return rc;
    }

private:
    Context& c_;
    uint32_t flags_ = 0, skip_ = 0, pair_slots_ = 0;
    bool dirty_ = true;
};

/// What `Sieve` produces: `klass` the cleaned h * w class plane, `rows` INFUR_SIEVE_ROW_WORDS words per region (CLASS, INTO, ROUND,
/// BORDER; ROUND == INFUR_SIEVE_NONE: stranded) and the INFUR_SIEVE_COUNT_WORDS counts.
struct SieveOut {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> klass;
    std::vector<uint32_t> rows, counts;
    uint32_t count(uint32_t word) const { return counts[word]; }
    uint32_t word(uint32_t region, uint32_t w) const { return rows[(size_t)region * INFUR_SIEVE_ROW_WORDS + w]; }
};

/// The stage that removes speckle: every region of fewer than `min_pixels` pixels takes the class of the neighbour it shares the
/// longest border with, round by round.  Integer results, identical from run to run.
/// Command = one of min_pixels / max_rounds / pair_slots; Input = the class plane and what Regions made of it (min_pixels 0, no
/// background skip, want_labels), Output = SieveOut.
class Sieve {
public:
    struct Cmd {
        enum Kind { MinPixels, MaxRounds, PairSlots } kind;
        uint32_t value;
    };
    explicit Sieve(Context& c, uint32_t min_pixels = 0) : c_(c), min_pixels_(min_pixels) {}
    Status control(Cmd cmd) {
        uint32_t minpx = min_pixels_, rounds = max_rounds_, slots = pair_slots_;
        switch (cmd.kind) {
        case Cmd::MinPixels: minpx = cmd.value; break;
        case Cmd::MaxRounds:
            if (cmd.value > 64) return INFUR_E_INVALID_ARG;  // state untouched
            rounds = cmd.value;
            break;
        case Cmd::PairSlots: slots = cmd.value; break;
        default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || minpx != min_pixels_ || rounds != max_rounds_ || slots != pair_slots_;
        min_pixels_ = minpx, max_rounds_ = rounds, pair_slots_ = slots;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const std::vector<uint8_t>& klass, const RegionsOut& regions, SieveOut& out) {
        dirty_ = false;
        const size_t hw = (size_t)regions.width * regions.height;
        if (klass.size() != hw || regions.labels.size() != hw) return INFUR_E_SHAPE;  // (a RegionsOut made with want_labels)
        out.width = regions.width;
        out.height = regions.height;
        out.klass.assign(hw, 0);
        out.rows.assign((size_t)regions.rows() * INFUR_SIEVE_ROW_WORDS, 0);
        out.counts.assign(INFUR_SIEVE_COUNT_WORDS, 0);
        return infur_sieve(c_.get(), klass.data(), regions.labels.data(), regions.table.data(), regions.table_rows, regions.n, regions.height,
                           regions.width, min_pixels_, max_rounds_, pair_slots_, hw ? out.klass.data() : nullptr,
                           out.rows.empty() ? nullptr : out.rows.data(), out.counts.data());
    }

private:
    Context& c_;
    uint32_t min_pixels_, max_rounds_ = 0, pair_slots_ = 0;
    bool dirty_ = true;
};

/// What `Outlines` produces: `loops` holds min(n_loops, loops_rows) records of INFUR_LOOP_WORDS words, `vertices` the first
/// min(n_vertices, vertex_rows) vertex ids Y*(width+1) + X, loops back to back; the three counts are complete whatever the rows
/// are (n_loops == 0 with n_edges > 0: the edges exceeded the capacity).
struct OutlinesOut {
    uint32_t loops_rows = 1u << 16, vertex_rows = 1u << 20;
    uint32_t width = 0, height = 0, n_loops = 0, n_vertices = 0, n_edges = 0;
    std::vector<uint32_t> loops, vertices;
    uint32_t rows() const { return n_loops < loops_rows ? n_loops : loops_rows; }
    uint32_t word(uint32_t loop, uint32_t w) const { return loops[(size_t)loop * INFUR_LOOP_WORDS + w]; }
    bool is_hole(uint32_t loop) const { return (word(loop, INFUR_LOOP_START) & 3u) == 2u; }
    uint32_t x(uint32_t vertex) const { return vertices[vertex] % (width + 1); }
    uint32_t y(uint32_t vertex) const { return vertices[vertex] / (width + 1); }
};

/// The polygon stage: the boundaries of the value-regions of a byte plane (class) or a u32 plane (labels, tracks) as closed loops
/// of lattice vertices, outer loops clockwise on a y-down screen, holes counter-clockwise.  Integer results, identical from run to run.
/// Command = skip (pixels of `value` belong to no region) / no skip, the connectivity Regions was given (the saddle rule), the
/// edge capacity (0: four per pixel); Input = a plane of uint8_t or uint32_t, Output = OutlinesOut.
class Outlines {
public:
    struct Cmd {
        enum Kind { Skip, NoSkip, Connectivity, MaxEdges } kind;
        uint32_t value;
    };
    explicit Outlines(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        uint32_t flags = flags_, skip_value = skip_value_, max_edges = max_edges_;
        switch (cmd.kind) {
            case Cmd::Skip: flags |= (uint32_t)INFUR_OUTLINES_SKIP, skip_value = cmd.value; break;
            case Cmd::NoSkip: flags &= ~(uint32_t)INFUR_OUTLINES_SKIP, skip_value = 0; break;
            case Cmd::Connectivity:
                if (cmd.value != 4 && cmd.value != 8) return INFUR_E_INVALID_ARG;
                flags = cmd.value == 8 ? flags | (uint32_t)INFUR_OUTLINES_CONN8 : flags & ~(uint32_t)INFUR_OUTLINES_CONN8;
                break;
            case Cmd::MaxEdges: max_edges = cmd.value; break;
            default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || flags != flags_ || skip_value != skip_value_ || max_edges != max_edges_;
        flags_ = flags;
        skip_value_ = skip_value;
        max_edges_ = max_edges;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const std::vector<uint8_t>& plane, uint32_t height, uint32_t width, OutlinesOut& out) {
        return run(plane.data(), plane.size(), 1, height, width, out);
    }
    Status advance(const std::vector<uint32_t>& plane, uint32_t height, uint32_t width, OutlinesOut& out) {
        return run(plane.data(), plane.size(), 4, height, width, out);
    }

private:
    Status run(const void* plane, size_t elems, uint32_t elem_bytes, uint32_t height, uint32_t width, OutlinesOut& out) {
        dirty_ = false;
        if (elems != (size_t)width * height) return INFUR_E_SHAPE;
        out.width = width;
        out.height = height;
        out.loops.assign((size_t)out.loops_rows * INFUR_LOOP_WORDS, 0);
        out.vertices.assign(out.vertex_rows, 0);
        uint32_t counts[3] = {0, 0, 0};
        const Status s = infur_outlines(c_.get(), plane, elem_bytes, height, width, flags_, skip_value_, max_edges_,
                                        out.loops_rows ? out.loops.data() : nullptr, out.loops_rows, out.vertex_rows ? out.vertices.data() : nullptr,
                                        out.vertex_rows, counts);
        out.n_loops = counts[0];
        out.n_vertices = counts[1];
        out.n_edges = counts[2];
        out.loops.resize((size_t)out.rows() * INFUR_LOOP_WORDS);
        out.vertices.resize(out.n_vertices < out.vertex_rows ? out.n_vertices : out.vertex_rows);
        return s;
    }
    Context& c_;
    uint32_t flags_ = 0, skip_value_ = 0, max_edges_ = 0;
    bool dirty_ = true;
};

/// What `Simplify` produces, in Outlines' layout: `loops` holds min(n_loops, loops_rows) records (OFFSET', COUNT', VALUE, START),
/// `vertices` the first min(n_vertices, vertex_rows) kept vertex ids; n_degenerate counts the loops with COUNT' < 3 (skip them);
/// status: INFUR_SIMPLIFY_TRUNCATED (the input was cut off: nothing was produced), INFUR_SIMPLIFY_MALFORMED.
struct SimplifyOut {
    uint32_t loops_rows = 1u << 16, vertex_rows = 1u << 20;
    uint32_t width = 0, height = 0, n_loops = 0, n_vertices = 0, n_degenerate = 0, status = 0;
    std::vector<uint32_t> loops, vertices;
    uint32_t rows() const { return (status & INFUR_SIMPLIFY_TRUNCATED) ? 0 : (n_loops < loops_rows ? n_loops : loops_rows); }
    uint32_t word(uint32_t loop, uint32_t w) const { return loops[(size_t)loop * INFUR_LOOP_WORDS + w]; }
    bool is_hole(uint32_t loop) const { return (word(loop, INFUR_LOOP_START) & 3u) == 2u; }
    bool is_degenerate(uint32_t loop) const { return word(loop, INFUR_LOOP_COUNT) < 3u; }
    uint32_t x(uint32_t vertex) const { return vertices[vertex] % (width + 1); }
    uint32_t y(uint32_t vertex) const { return vertices[vertex] / (width + 1); }
};

/// The stage behind Outlines: Douglas-Peucker on every loop within tol16 sixteenths of a pixel.  Integer results, identical from
/// run to run; topology is not preserved.  Command = the tolerance; Input = an OutlinesOut, Output = SimplifyOut.
class Simplify {
public:
    struct Cmd {
        enum Kind { Tol16 } kind;
        uint32_t value;
    };
    explicit Simplify(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        if (cmd.kind != Cmd::Tol16 || cmd.value > 65535) return INFUR_E_INVALID_ARG;
        dirty_ = dirty_ || cmd.value != tol16_;
        tol16_ = cmd.value;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const OutlinesOut& in, SimplifyOut& out) {
        dirty_ = false;
        out.width = in.width;
        out.height = in.height;
        const uint32_t rows_in = (uint32_t)(in.loops.size() / INFUR_LOOP_WORDS), verts_in = (uint32_t)in.vertices.size();
        const uint32_t lrows = out.loops_rows < rows_in ? out.loops_rows : rows_in, vrows = out.vertex_rows < verts_in ? out.vertex_rows : verts_in;
        out.loops.assign((size_t)lrows * INFUR_LOOP_WORDS, 0);
        out.vertices.assign(vrows, 0);
        const uint32_t counts_in[2] = {in.n_loops, in.n_vertices};
        uint32_t counts[INFUR_SIMPLIFY_COUNT_WORDS] = {0, 0, 0, 0};
        const Status s = infur_simplify(c_.get(), rows_in ? in.loops.data() : nullptr, rows_in, verts_in ? in.vertices.data() : nullptr, verts_in, counts_in,
                                        in.height, in.width, tol16_, lrows ? out.loops.data() : nullptr, lrows, vrows ? out.vertices.data() : nullptr, vrows,
                                        counts);
        out.n_loops = counts[INFUR_SIMPLIFY_LOOPS];
        out.n_vertices = counts[INFUR_SIMPLIFY_VERTICES];
        out.n_degenerate = counts[INFUR_SIMPLIFY_DEGENERATE];
        out.status = counts[INFUR_SIMPLIFY_STATUS];
        const uint32_t nl = (out.status & INFUR_SIMPLIFY_TRUNCATED) ? 0 : (out.n_loops < lrows ? out.n_loops : lrows);
        out.loops.resize((size_t)nl * INFUR_LOOP_WORDS);
        out.vertices.resize(out.n_vertices < vrows ? out.n_vertices : vrows);
        return s;
    }

private:
    Context& c_;
    uint32_t tol16_ = 16;
    bool dirty_ = true;
};

/// What `Shapes` produces: the hulls in Outlines' layout (`loops`, `vertices`), `shapes` with INFUR_SHAPE_WORDS signed words per
/// loop (INFUR_SHAPE_AREA2 .. INFUR_SHAPE_RECT_L) and `values` with as many per value (words 8 .. 10: INFUR_SHAPE_OUTER,
/// INFUR_SHAPE_HOLES, INFUR_SHAPE_LOOP), every one of value_rows written; status: INFUR_SHAPES_TRUNCATED (the input was cut off),
/// INFUR_SHAPES_MALFORMED; largest: the largest COUNT'.
struct ShapesOut {
    uint32_t loops_rows = 1u << 16, vertex_rows = 1u << 20, shape_rows = 1u << 16, value_rows = 0;
    uint32_t width = 0, height = 0, n_loops = 0, n_vertices = 0, status = 0, largest = 0;
    std::vector<uint32_t> loops, vertices;
    std::vector<int64_t> shapes, values;
    uint32_t word(uint32_t loop, uint32_t w) const { return loops[(size_t)loop * INFUR_LOOP_WORDS + w]; }
    int64_t shape(uint32_t loop, uint32_t w) const { return shapes[(size_t)loop * INFUR_SHAPE_WORDS + w]; }
    int64_t value(uint32_t v, uint32_t w) const { return values[(size_t)v * INFUR_SHAPE_WORDS + w]; }
    uint32_t x(uint32_t vertex) const { return vertices[vertex] % (width + 1); }
    uint32_t y(uint32_t vertex) const { return vertices[vertex] / (width + 1); }
};

/// The descriptor stage behind Outlines: per loop the area, perimeter and moments, the convex hull and the minimum rectangle, per
/// value the sums.  Integer results, identical from run to run.  No command; Input = an OutlinesOut, Output = ShapesOut.
class Shapes {
public:
    explicit Shapes(Context& c) : c_(c) {}
    bool is_dirty() const { return dirty_; }
    Status advance(const OutlinesOut& in, ShapesOut& out) {
        dirty_ = false;
        out.width = in.width;
        out.height = in.height;
        const uint32_t rows_in = (uint32_t)(in.loops.size() / INFUR_LOOP_WORDS), verts_in = (uint32_t)in.vertices.size();
        const uint32_t lrows = out.loops_rows < rows_in ? out.loops_rows : rows_in, vrows = out.vertex_rows < verts_in ? out.vertex_rows : verts_in;
        const uint32_t srows = out.shape_rows < rows_in ? out.shape_rows : rows_in;
        out.loops.assign((size_t)lrows * INFUR_LOOP_WORDS, 0);
        out.vertices.assign(vrows, 0);
        out.shapes.assign((size_t)srows * INFUR_SHAPE_WORDS, 0);
        out.values.assign((size_t)out.value_rows * INFUR_SHAPE_WORDS, 0);
        const uint32_t counts_in[2] = {in.n_loops, in.n_vertices};
        uint32_t counts[INFUR_SHAPES_COUNT_WORDS] = {0, 0, 0, 0};
        const Status s = infur_shapes(c_.get(), rows_in ? in.loops.data() : nullptr, rows_in, verts_in ? in.vertices.data() : nullptr, verts_in, counts_in,
                                      in.height, in.width, lrows ? out.loops.data() : nullptr, lrows, vrows ? out.vertices.data() : nullptr, vrows,
                                      srows ? (uint64_t*)out.shapes.data() : nullptr, srows, out.value_rows ? (uint64_t*)out.values.data() : nullptr,
                                      out.value_rows, counts);
        out.n_loops = counts[INFUR_SHAPES_LOOPS];
        out.n_vertices = counts[INFUR_SHAPES_VERTICES];
        out.status = counts[INFUR_SHAPES_STATUS];
        out.largest = counts[INFUR_SHAPES_LARGEST];
        const bool cut = (out.status & INFUR_SHAPES_TRUNCATED) != 0;
        out.loops.resize((size_t)(cut ? 0 : (out.n_loops < lrows ? out.n_loops : lrows)) * INFUR_LOOP_WORDS);
        out.vertices.resize(out.n_vertices < vrows ? out.n_vertices : vrows);
        out.shapes.resize((size_t)(cut ? 0 : (out.n_loops < srows ? out.n_loops : srows)) * INFUR_SHAPE_WORDS);
        return s;
    }

private:
    Context& c_;
    bool dirty_ = true;
};

/// What `Raster` produces: `plane` holds height * width elements of elem_bytes bytes each (empty when the input was truncated);
/// painted and conflict count the pixels exactly one loop claims and the pixels that were refused (overlapping loops, a hole
/// alone, crossed arcs, a value a byte plane cannot hold: they read the fill value); status: INFUR_RASTER_TRUNCATED, _MALFORMED,
/// _OUTSIDE; n: the loops or records read.
struct RasterOut {
    uint32_t width = 0, height = 0, elem_bytes = 1, n = 0, painted = 0, conflict = 0, status = 0;
    std::vector<uint8_t> plane;
    uint32_t at(uint32_t x, uint32_t y) const {
        const size_t i = (size_t)y * width + x;
        if (elem_bytes == 1) return plane[i];
        uint32_t v;
        std::memcpy(&v, plane.data() + i * 4, 4);
        return v;
    }
};

/// The stage that goes the other way: the loops of Outlines, Simplify, Coverage or Shapes (its hulls), or the records of Runs,
/// filled back into a plane.  Winding 1 paints the loop's value; everything else reads the fill value.  Integer results,
/// identical from run to run.  Command = the plane's element size and fill value; Input = an OutlinesOut or a RunsOut,
/// Output = RasterOut.
class Raster {
public:
    struct Cmd {
        enum Kind { Fill } kind;
        uint32_t elem_bytes, fill_value;
    };
    explicit Raster(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        if (cmd.kind != Cmd::Fill || (cmd.elem_bytes != 1 && cmd.elem_bytes != 4) || (cmd.elem_bytes == 1 && cmd.fill_value > 255))
            return INFUR_E_INVALID_ARG;
        dirty_ = dirty_ || cmd.elem_bytes != elem_bytes_ || cmd.fill_value != fill_value_;
        elem_bytes_ = cmd.elem_bytes;
        fill_value_ = cmd.fill_value;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const OutlinesOut& in, RasterOut& out) {
        begin(in.width, in.height, out);
        const uint32_t rows_in = (uint32_t)(in.loops.size() / INFUR_LOOP_WORDS), verts_in = (uint32_t)in.vertices.size();
        const uint32_t counts_in[2] = {in.n_loops, in.n_vertices};
        uint32_t counts[INFUR_RASTER_COUNT_WORDS] = {0, 0, 0, 0};
        const Status s = infur_raster(c_.get(), rows_in ? in.loops.data() : nullptr, rows_in, verts_in ? in.vertices.data() : nullptr, verts_in, counts_in,
                                      in.height, in.width, elem_bytes_, fill_value_, out.plane.empty() ? nullptr : out.plane.data(), counts);
        return end(s, counts, out);
    }
    Status advance(const RunsOut& in, RasterOut& out) {
        begin(in.width, in.height, out);
        const uint32_t rows_in = (uint32_t)(in.runs.size() / INFUR_RUN_WORDS);
        uint32_t counts[INFUR_RASTER_COUNT_WORDS] = {0, 0, 0, 0};
        const Status s = infur_raster_runs(c_.get(), rows_in ? in.runs.data() : nullptr, rows_in, in.n, in.height, in.width, elem_bytes_, fill_value_,
                                           out.plane.empty() ? nullptr : out.plane.data(), counts);
        return end(s, counts, out);
    }

private:
    void begin(uint32_t w, uint32_t h, RasterOut& out) {
        dirty_ = false;
        out.width = w;
        out.height = h;
        out.elem_bytes = elem_bytes_;
        out.plane.assign((size_t)w * h * elem_bytes_, 0);
    }
    static Status end(Status s, const uint32_t* counts, RasterOut& out) {
        out.n = counts[INFUR_RASTER_LOOPS];
        out.painted = counts[INFUR_RASTER_PAINTED];
        out.conflict = counts[INFUR_RASTER_CONFLICT];
        out.status = counts[INFUR_RASTER_STATUS];
        if (out.status & INFUR_RASTER_TRUNCATED) out.plane.clear();
        return s;
    }
    Context& c_;
    uint32_t elem_bytes_ = 1, fill_value_ = 0;
    bool dirty_ = true;
};

/// What `Coverage` produces, in Outlines' layout: `loops` holds min(n_loops, loops_rows) records (OFFSET', COUNT', VALUE, START),
/// `vertices` the first min(n_vertices, vertex_rows) kept vertex ids; n_degenerate counts the loops with COUNT' < 3 (skip them);
/// status: INFUR_COVERAGE_TRUNCATED and INFUR_COVERAGE_OVERFLOW (nothing was produced), INFUR_COVERAGE_MALFORMED; n_aug: the
/// vertices once the junctions were inserted; n_arcs: the stretches between junctions, a ring counting as one.
struct CoverageOut {
    uint32_t loops_rows = 1u << 16, vertex_rows = 1u << 20;
    uint32_t width = 0, height = 0, n_loops = 0, n_vertices = 0, n_degenerate = 0, status = 0, n_aug = 0, n_arcs = 0;
    std::vector<uint32_t> loops, vertices;
    uint32_t rows() const {
        return (status & (INFUR_COVERAGE_TRUNCATED | INFUR_COVERAGE_OVERFLOW)) ? 0 : (n_loops < loops_rows ? n_loops : loops_rows);
    }
    uint32_t word(uint32_t loop, uint32_t w) const { return loops[(size_t)loop * INFUR_LOOP_WORDS + w]; }
    bool is_hole(uint32_t loop) const { return (word(loop, INFUR_LOOP_START) & 3u) == 2u; }
    bool is_degenerate(uint32_t loop) const { return word(loop, INFUR_LOOP_COUNT) < 3u; }
    uint32_t x(uint32_t vertex) const { return vertices[vertex] % (width + 1); }
    uint32_t y(uint32_t vertex) const { return vertices[vertex] / (width + 1); }
};

/// Simplify's sibling behind Outlines: the loops are cut at the plane's junctions and every arc is simplified once within tol16
/// sixteenths of a pixel, so that neighbouring polygons still share their borders.  Integer results, identical from run to run.
/// Command = the tolerance, skip / no skip (what Outlines was given), the capacity in augmented vertices (0: the worst case);
/// Input = the plane Outlines was given and its OutlinesOut, Output = CoverageOut.
class Coverage {
public:
    struct Cmd {
        enum Kind { Tol16, Skip, NoSkip, AugRows } kind;
        uint32_t value;
    };
    explicit Coverage(Context& c) : c_(c) {}
    Status control(Cmd cmd) {
        uint32_t tol16 = tol16_, flags = flags_, skip_value = skip_value_, aug_rows = aug_rows_;
        switch (cmd.kind) {
            case Cmd::Tol16:
                if (cmd.value > 65535) return INFUR_E_INVALID_ARG;
                tol16 = cmd.value;
                break;
            case Cmd::Skip: flags = INFUR_COVERAGE_SKIP, skip_value = cmd.value; break;
            case Cmd::NoSkip: flags = 0, skip_value = 0; break;
            case Cmd::AugRows: aug_rows = cmd.value; break;
            default: return INFUR_E_INVALID_ARG;
        }
        dirty_ = dirty_ || tol16 != tol16_ || flags != flags_ || skip_value != skip_value_ || aug_rows != aug_rows_;
        tol16_ = tol16, flags_ = flags, skip_value_ = skip_value, aug_rows_ = aug_rows;
        return INFUR_OK;
    }
    bool is_dirty() const { return dirty_; }
    Status advance(const std::vector<uint8_t>& plane, const OutlinesOut& in, CoverageOut& out) { return run(plane.data(), plane.size(), 1, in, out); }
    Status advance(const std::vector<uint32_t>& plane, const OutlinesOut& in, CoverageOut& out) { return run(plane.data(), plane.size(), 4, in, out); }

private:
    Status run(const void* plane, size_t elems, uint32_t elem_bytes, const OutlinesOut& in, CoverageOut& out) {
        dirty_ = false;
        if (elems != (size_t)in.width * in.height) return INFUR_E_SHAPE;
        out.width = in.width;
        out.height = in.height;
        const uint32_t rows_in = (uint32_t)(in.loops.size() / INFUR_LOOP_WORDS), verts_in = (uint32_t)in.vertices.size();
        const uint64_t most = (uint64_t)verts_in + (uint64_t)(in.width + 1) * (in.height + 1);  // junctions are inserted
        const uint32_t lrows = out.loops_rows < rows_in ? out.loops_rows : rows_in, vrows = out.vertex_rows < most ? out.vertex_rows : (uint32_t)most;
        out.loops.assign((size_t)lrows * INFUR_LOOP_WORDS, 0);
        out.vertices.assign(vrows, 0);
        const uint32_t counts_in[2] = {in.n_loops, in.n_vertices};
        uint32_t counts[INFUR_COVERAGE_COUNT_WORDS] = {0, 0, 0, 0, 0, 0};
        const Status s = infur_coverage(c_.get(), plane, elem_bytes, in.height, in.width, flags_, skip_value_, rows_in ? in.loops.data() : nullptr, rows_in,
                                        verts_in ? in.vertices.data() : nullptr, verts_in, counts_in, tol16_, aug_rows_, lrows ? out.loops.data() : nullptr,
                                        lrows, vrows ? out.vertices.data() : nullptr, vrows, counts);
        out.n_loops = counts[INFUR_COVERAGE_LOOPS];
        out.n_vertices = counts[INFUR_COVERAGE_VERTICES];
        out.n_degenerate = counts[INFUR_COVERAGE_DEGENERATE];
        out.status = counts[INFUR_COVERAGE_STATUS];
        out.n_aug = counts[INFUR_COVERAGE_AUG];
        out.n_arcs = counts[INFUR_COVERAGE_ARCS];
        const bool nothing = (out.status & (INFUR_COVERAGE_TRUNCATED | INFUR_COVERAGE_OVERFLOW)) != 0;
        const uint32_t nl = nothing ? 0 : (out.n_loops < lrows ? out.n_loops : lrows);
        out.loops.resize((size_t)nl * INFUR_LOOP_WORDS);
        out.vertices.resize(out.n_vertices < vrows ? out.n_vertices : vrows);
        return s;
    }
    Context& c_;
    uint32_t tol16_ = 16, flags_ = 0, skip_value_ = 0, aug_rows_ = 0;
    bool dirty_ = true;
};

/// infur_group: n contexts (one per GPU) of one process -- RCCL weight broadcast + frame-batch sharding
/// (BASELINE configs[3]).  The contexts must outlive the group.
class Group {
public:
    explicit Group(const std::vector<Context*>& ctxs) {
        std::vector<infur_ctx*> raw;
        for (Context* c : ctxs) raw.push_back(c->get());
        status_ = infur_group_create(raw.data(), (uint32_t)raw.size(), &g_);
    }
    ~Group() { infur_group_destroy(g_); }
    Group(const Group&) = delete;
    Group& operator=(const Group&) = delete;
    bool ok() const { return status_ == INFUR_OK; }
    infur_group* get() const { return g_; }
    std::string last_error() const { return infur_group_last_error(g_); }
    Status weights_broadcast(uint32_t root = 0) { return infur_group_weights_broadcast(g_, root); }
    /// masks[i] is resized to the mask of frames[i] (scale `factor` applied first, as app.rs:107-153 does per frame)
    Status batch_advance(const std::vector<BgrImage>& frames, float factor, std::vector<ColorImage>& masks,
                         uint32_t scale_mode = INFUR_SCALE_NEAREST) {
        const size_t n = frames.size();
        masks.resize(n);
        std::vector<const uint8_t*> in(n);
        std::vector<uint8_t*> out(n);
        std::vector<uint32_t> ws(n), hs(n);
        std::vector<size_t> caps(n);
        for (size_t i = 0; i < n; i++) {
            uint32_t ow = 0, oh = 0;
            Status s = infur_scale_out_dims(frames[i].width, frames[i].height, factor, &ow, &oh);
            if (s != INFUR_OK) return s;
            masks[i].width = ow;
            masks[i].height = oh;
            masks[i].rgba.resize((size_t)ow * oh * 4);
            in[i] = frames[i].data.data();
            out[i] = masks[i].rgba.data();
            ws[i] = frames[i].width;
            hs[i] = frames[i].height;
            caps[i] = masks[i].rgba.size();
        }
        return infur_group_batch_advance(g_, in.data(), ws.data(), hs.data(), (uint32_t)n, factor, scale_mode, out.data(),
                                         caps.data(), nullptr, nullptr);
    }

private:
    infur_group* g_ = nullptr;
    Status status_ = INFUR_OK;
};

}  // namespace infur
