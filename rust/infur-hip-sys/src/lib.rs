//! Raw bindings of `include/infur_hip.h`.  UNTESTED: never compiled (no Rust toolchain here).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

#[repr(C)]
pub struct infur_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct infur_stream {
    _private: [u8; 0],
}
#[repr(C)]
pub struct infur_group {
    _private: [u8; 0],
}

#[repr(C)]
pub struct infur_options {
    pub struct_size: u32,
    pub device: i32,
    pub compute_dtype: u32,
    pub compute_aux: u32,
    pub profile: u32,
    pub keep_activations: u32,
    pub winograd_min_cin: u32,
    pub winograd_tile: u32,
    pub no_autotune: u32,
    pub no_fuse_downsample: u32,
    pub no_fuse_stem_pool: u32,
    pub no_fuse_b2b: u32,
    pub stream: *mut c_void,
}

#[repr(C)]
pub struct infur_model_info {
    pub input_name: [c_char; 32],
    pub input0_dtype: [c_char; 16],
    pub output_names: [[c_char; 32]; 2],
    pub n_outputs: u32,
    pub num_classes: u32,
    pub depth: u32,
    pub n_convs: u32,
    pub weight_bytes: u64,
    pub quantised: u32,
    pub resize_u8_heads: u32,
}

/// one profiled kernel launch of the last advance (`infur_profile_get`)
#[repr(C)]
pub struct infur_kernel_record {
    pub name: [c_char; 48],
    pub kernel: [c_char; 32],
    pub ms: f32,
    pub flops: f64,
    pub bytes: f64,
    pub algo_flops: f64,
}

pub const INFUR_OK: i32 = 0;
pub const INFUR_E_INVALID_SCALE: i32 = 1;
pub const INFUR_E_ZERO_SIZE_IN: i32 = 2;
pub const INFUR_E_ZERO_SIZE_OUT: i32 = 3;
pub const INFUR_E_SHAPE: i32 = 4;
pub const INFUR_E_MODEL_NOT_LOADED: i32 = 5;
pub const INFUR_E_MODEL_FORMAT: i32 = 6;
pub const INFUR_E_HIP: i32 = 7;
pub const INFUR_E_RCCL: i32 = 8;
pub const INFUR_E_INVALID_ARG: i32 = 9;
pub const INFUR_E_IO: i32 = 10;
pub const INFUR_E_CAPACITY: i32 = 11;
pub const INFUR_ABI_VERSION: u32 = 7;
pub const INFUR_SCALE_NEAREST: u32 = 0;
pub const INFUR_SCALE_BILINEAR: u32 = 1;
pub const INFUR_DTYPE_F32: u32 = 0;
pub const INFUR_DTYPE_F16: u32 = 1;
/// f32 tensors, conv GEMMs on the f16 matrix cores with hi+lo operand pairs (f32-grade logits, ~1.9x the f32 MFMA rate)
pub const INFUR_DTYPE_F32_SPLIT: u32 = 2;
/// split mode with the two cross terms on the fp8 (e4m3) MX MFMA: logits ~1.5e-4 from f32, ~8 % faster than F32_SPLIT
pub const INFUR_DTYPE_F32_SPLIT_FP8: u32 = 3;
/// three-byte tensors (f16 hi + e5m2 lo planes written by the producer, staged by LDS-DMA), two MFMA units per product:
/// logits ~1.5e-4 from f32 on heavy-tailed weights, ~2.5x the f32 MFMA rate (round 5; 4 is not an option value)
pub const INFUR_DTYPE_F16_HL: u32 = 5;
/// Segments: decode modes (the reference's loop / the same from -inf with a softmax confidence)
pub const INFUR_DECODE_RAW: u32 = 0;
pub const INFUR_DECODE_SOFTMAX: u32 = 1;
/// Segments: the columns of one class's row of the statistics table (`INFUR_STAT_WORDS` u64 each)
pub const INFUR_STAT_PIXELS: u32 = 0;
pub const INFUR_STAT_SUM_X: u32 = 1;
pub const INFUR_STAT_SUM_Y: u32 = 2;
pub const INFUR_STAT_SUM_CONF: u32 = 3;
pub const INFUR_STAT_MIN_X: u32 = 4;
pub const INFUR_STAT_MIN_Y: u32 = 5;
pub const INFUR_STAT_MAX_X: u32 = 6;
pub const INFUR_STAT_MAX_Y: u32 = 7;
pub const INFUR_STAT_WORDS: u32 = 8;
/// bit of `infur_features()`: the Segments calls below exist
pub const INFUR_FEATURE_SEGMENTS: u32 = 1;
/// Regions: connectivity, flags, the two extra columns of a region's row (`INFUR_REGION_WORDS` u64 each; words 0-7 are `INFUR_STAT_*`)
pub const INFUR_CONNECT_4: u32 = 4;
pub const INFUR_CONNECT_8: u32 = 8;
pub const INFUR_REGIONS_SKIP_BACKGROUND: u32 = 1;
pub const INFUR_REGION_CLASS: u32 = 8;
pub const INFUR_REGION_FIRST: u32 = 9;
pub const INFUR_REGION_WORDS: u32 = 10;
/// label of a pixel that belongs to no kept region
pub const INFUR_REGION_NONE: u32 = 0xFFFF_FFFF;
/// bit of `infur_features()`: the Regions calls below exist
pub const INFUR_FEATURE_REGIONS: u32 = 2;
/// Tracks: the columns of a track row (`INFUR_TRACK_WORDS` u64 each), the status bits, the words of the summary
pub const INFUR_TRACK_ID: u32 = 0;
pub const INFUR_TRACK_AGE: u32 = 1;
pub const INFUR_TRACK_BORN: u32 = 2;
pub const INFUR_TRACK_PREV_REGION: u32 = 3;
pub const INFUR_TRACK_OVERLAP: u32 = 4;
pub const INFUR_TRACK_PREV_PIXELS: u32 = 5;
pub const INFUR_TRACK_PREV_SUM_X: u32 = 6;
pub const INFUR_TRACK_PREV_SUM_Y: u32 = 7;
pub const INFUR_TRACK_WORDS: u32 = 8;
pub const INFUR_TRACKS_TRUNCATED: u32 = 1;
pub const INFUR_TRACKS_OVERFLOW: u32 = 2;
pub const INFUR_TRACKS_IDS_EXHAUSTED: u32 = 4;
pub const INFUR_TRACKS_SUMMARY_STATUS: u32 = 0;
pub const INFUR_TRACKS_SUMMARY_CONTINUED: u32 = 1;
pub const INFUR_TRACKS_SUMMARY_NEW: u32 = 2;
pub const INFUR_TRACKS_SUMMARY_ENDED: u32 = 3;
pub const INFUR_TRACKS_SUMMARY_WORDS: u32 = 4;
/// track of a region that is not tracked
pub const INFUR_TRACK_NONE: u32 = 0xFFFF_FFFF;
/// bit of `infur_features()`: the Tracks calls below exist
pub const INFUR_FEATURE_TRACKS: u32 = 4;
/// Tracks' memory: the status bit, the words of a gallery entry (`INFUR_LOST_WORDS` u64 each) and of the memory summary
pub const INFUR_TRACKS_GALLERY_FULL: u32 = 8;
pub const INFUR_LOST_ID: u32 = 0;
pub const INFUR_LOST_AGE: u32 = 1;
pub const INFUR_LOST_BORN: u32 = 2;
pub const INFUR_LOST_CLASS: u32 = 3;
pub const INFUR_LOST_PIXELS: u32 = 4;
pub const INFUR_LOST_SUM_X: u32 = 5;
pub const INFUR_LOST_SUM_Y: u32 = 6;
pub const INFUR_LOST_MIN_X: u32 = 7;
pub const INFUR_LOST_MIN_Y: u32 = 8;
pub const INFUR_LOST_MAX_X: u32 = 9;
pub const INFUR_LOST_MAX_Y: u32 = 10;
pub const INFUR_LOST_SEEN: u32 = 11;
pub const INFUR_LOST_WORDS: u32 = 12;
pub const INFUR_TRACK_MEMORY_REVIVED: u32 = 0;
pub const INFUR_TRACK_MEMORY_LOST: u32 = 1;
pub const INFUR_TRACK_MEMORY_EXPIRED: u32 = 2;
pub const INFUR_TRACK_MEMORY_HELD: u32 = 3;
pub const INFUR_TRACK_MEMORY_WORDS: u32 = 4;
/// bit of `infur_features()`: the memory calls of a tracker exist
pub const INFUR_FEATURE_TRACK_MEMORY: u32 = 128;
/// Runs: the flag, the words of a record (`INFUR_RUN_WORDS` u32 each)
pub const INFUR_RUNS_SKIP: u32 = 1;
pub const INFUR_RUN_START: u32 = 0;
pub const INFUR_RUN_END: u32 = 1;
pub const INFUR_RUN_VALUE: u32 = 2;
pub const INFUR_RUN_WORDS: u32 = 3;
/// bit of `infur_features()`: the Runs calls below exist
pub const INFUR_FEATURE_RUNS: u32 = 8;
/// Outlines: the flags, the words of a loop record (`INFUR_LOOP_WORDS` u32 each)
pub const INFUR_OUTLINES_SKIP: u32 = 1;
pub const INFUR_OUTLINES_CONN8: u32 = 2;
pub const INFUR_LOOP_OFFSET: u32 = 0;
pub const INFUR_LOOP_COUNT: u32 = 1;
pub const INFUR_LOOP_VALUE: u32 = 2;
pub const INFUR_LOOP_START: u32 = 3;
pub const INFUR_LOOP_WORDS: u32 = 4;
/// bit of `infur_features()`: the Outlines calls below exist
pub const INFUR_FEATURE_OUTLINES: u32 = 16;
/// Simplify: the words of its counts (`INFUR_SIMPLIFY_COUNT_WORDS` u32), the status bits
pub const INFUR_SIMPLIFY_LOOPS: u32 = 0;
pub const INFUR_SIMPLIFY_VERTICES: u32 = 1;
pub const INFUR_SIMPLIFY_DEGENERATE: u32 = 2;
pub const INFUR_SIMPLIFY_STATUS: u32 = 3;
pub const INFUR_SIMPLIFY_COUNT_WORDS: u32 = 4;
pub const INFUR_SIMPLIFY_TRUNCATED: u32 = 1;
pub const INFUR_SIMPLIFY_MALFORMED: u32 = 2;
/// bit of `infur_features()`: the Simplify calls below exist
pub const INFUR_FEATURE_SIMPLIFY: u32 = 32;
/// Coverage: its flag, the words of its counts (`INFUR_COVERAGE_COUNT_WORDS` u32), the status bits
pub const INFUR_COVERAGE_SKIP: u32 = 1;
pub const INFUR_COVERAGE_LOOPS: u32 = 0;
pub const INFUR_COVERAGE_VERTICES: u32 = 1;
pub const INFUR_COVERAGE_DEGENERATE: u32 = 2;
pub const INFUR_COVERAGE_STATUS: u32 = 3;
pub const INFUR_COVERAGE_AUG: u32 = 4;
pub const INFUR_COVERAGE_ARCS: u32 = 5;
pub const INFUR_COVERAGE_COUNT_WORDS: u32 = 6;
pub const INFUR_COVERAGE_TRUNCATED: u32 = 1;
pub const INFUR_COVERAGE_MALFORMED: u32 = 2;
pub const INFUR_COVERAGE_OVERFLOW: u32 = 4;
/// bit of `infur_features()`: the Coverage calls below exist
pub const INFUR_FEATURE_COVERAGE: u32 = 64;
/// Anchors: the flag, the words of a row (`INFUR_ANCHOR_WORDS` u32 each), the index of a row no pixel reached
pub const INFUR_ANCHORS_SKIP: u32 = 1;
pub const INFUR_ANCHOR_PIXEL: u32 = 0;
pub const INFUR_ANCHOR_DIST2: u32 = 1;
pub const INFUR_ANCHOR_WORDS: u32 = 2;
pub const INFUR_ANCHOR_NONE: u32 = 0xFFFF_FFFF;
/// bit of `infur_features()`: the Anchors calls below exist
pub const INFUR_FEATURE_ANCHORS: u32 = 256;
/// Compare: the flags, the words of a row (`INFUR_COMPARE_WORDS` u32 each) and of the counts, the status bits, "no partner"
pub const INFUR_COMPARE_IGNORE_A: u32 = 1;
pub const INFUR_COMPARE_IGNORE_B: u32 = 2;
pub const INFUR_COMPARE_PIXELS: u32 = 0;
pub const INFUR_COMPARE_PARTNER: u32 = 1;
pub const INFUR_COMPARE_INTER: u32 = 2;
pub const INFUR_COMPARE_UNION: u32 = 3;
pub const INFUR_COMPARE_WORDS: u32 = 4;
pub const INFUR_COMPARE_COMPARED: u32 = 0;
pub const INFUR_COMPARE_EQUAL: u32 = 1;
pub const INFUR_COMPARE_IGNORED: u32 = 2;
pub const INFUR_COMPARE_OUTSIDE: u32 = 3;
pub const INFUR_COMPARE_PAIRS: u32 = 4;
pub const INFUR_COMPARE_MATCHED: u32 = 5;
pub const INFUR_COMPARE_RUNS: u32 = 6;
pub const INFUR_COMPARE_STATUS: u32 = 7;
pub const INFUR_COMPARE_COUNT_WORDS: u32 = 8;
pub const INFUR_COMPARE_OVERFLOW: u32 = 1;
pub const INFUR_COMPARE_TABLE: u32 = 2;
pub const INFUR_COMPARE_NONE: u32 = 0xFFFF_FFFF;
/// bit of `infur_features()`: the Compare calls below exist
pub const INFUR_FEATURE_COMPARE: u32 = 512;
/// Adjacency: the flag, the words of a pair record, of a row and of the counts, the status bits, "no neighbour"
pub const INFUR_ADJ_SKIP: u32 = 1;
pub const INFUR_ADJ_A: u32 = 0;
pub const INFUR_ADJ_B: u32 = 1;
pub const INFUR_ADJ_BORDER: u32 = 2;
pub const INFUR_ADJ_FIRST: u32 = 3;
pub const INFUR_ADJ_PAIR_WORDS: u32 = 4;
pub const INFUR_ADJ_DEGREE: u32 = 0;
pub const INFUR_ADJ_LONGEST: u32 = 1;
pub const INFUR_ADJ_ROW_BORDER: u32 = 2;
pub const INFUR_ADJ_PERIMETER: u32 = 3;
pub const INFUR_ADJ_ROW_WORDS: u32 = 4;
pub const INFUR_ADJ_PAIRS: u32 = 0;
pub const INFUR_ADJ_EDGES: u32 = 1;
pub const INFUR_ADJ_SKIPPED: u32 = 2;
pub const INFUR_ADJ_OUTSIDE: u32 = 3;
pub const INFUR_ADJ_RUNS: u32 = 4;
pub const INFUR_ADJ_WRITTEN: u32 = 5;
pub const INFUR_ADJ_STATUS: u32 = 7;
pub const INFUR_ADJ_COUNT_WORDS: u32 = 8;
pub const INFUR_ADJ_OVERFLOW: u32 = 1;
pub const INFUR_ADJ_TRUNCATED: u32 = 2;
pub const INFUR_ADJ_NONE: u32 = 0xFFFF_FFFF;
/// Sieve: the words of a row and of the counts, the status bits, "stranded"
pub const INFUR_SIEVE_CLASS: u32 = 0;
pub const INFUR_SIEVE_INTO: u32 = 1;
pub const INFUR_SIEVE_ROUND: u32 = 2;
pub const INFUR_SIEVE_BORDER: u32 = 3;
pub const INFUR_SIEVE_ROW_WORDS: u32 = 4;
pub const INFUR_SIEVE_REGIONS: u32 = 0;
pub const INFUR_SIEVE_SMALL: u32 = 1;
pub const INFUR_SIEVE_ABSORBED: u32 = 2;
pub const INFUR_SIEVE_STRANDED: u32 = 3;
pub const INFUR_SIEVE_ROUNDS: u32 = 4;
pub const INFUR_SIEVE_PIXELS_CHANGED: u32 = 5;
pub const INFUR_SIEVE_PAIRS: u32 = 6;
pub const INFUR_SIEVE_STATUS: u32 = 7;
pub const INFUR_SIEVE_COUNT_WORDS: u32 = 8;
pub const INFUR_SIEVE_OVERFLOW: u32 = 1;
pub const INFUR_SIEVE_ROUNDS_EXHAUSTED: u32 = 2;
pub const INFUR_SIEVE_TABLE_SHORT: u32 = 4;
pub const INFUR_SIEVE_NONE: u32 = 0xFFFF_FFFF;
/// bit of `infur_features()`: the Adjacency and Sieve calls below exist
pub const INFUR_FEATURE_SIEVE: u32 = 1024;
/// Shapes: the words of a per-loop record and of a per-value row (words 8 .. 10 differ), of the counts, the status bits
pub const INFUR_SHAPE_AREA2: u32 = 0;
pub const INFUR_SHAPE_PERIMETER: u32 = 1;
pub const INFUR_SHAPE_M10_6: u32 = 2;
pub const INFUR_SHAPE_M01_6: u32 = 3;
pub const INFUR_SHAPE_M20_12: u32 = 4;
pub const INFUR_SHAPE_M02_12: u32 = 5;
pub const INFUR_SHAPE_M11_24: u32 = 6;
pub const INFUR_SHAPE_HULL_AREA2: u32 = 7;
pub const INFUR_SHAPE_RECT_EDGE: u32 = 8;
pub const INFUR_SHAPE_RECT_W: u32 = 9;
pub const INFUR_SHAPE_RECT_H: u32 = 10;
pub const INFUR_SHAPE_RECT_L: u32 = 11;
pub const INFUR_SHAPE_WORDS: u32 = 12;
pub const INFUR_SHAPE_OUTER: u32 = 8;
pub const INFUR_SHAPE_HOLES: u32 = 9;
pub const INFUR_SHAPE_LOOP: u32 = 10;
pub const INFUR_SHAPES_LOOPS: u32 = 0;
pub const INFUR_SHAPES_VERTICES: u32 = 1;
pub const INFUR_SHAPES_STATUS: u32 = 2;
pub const INFUR_SHAPES_LARGEST: u32 = 3;
pub const INFUR_SHAPES_COUNT_WORDS: u32 = 4;
pub const INFUR_SHAPES_TRUNCATED: u32 = 1;
pub const INFUR_SHAPES_MALFORMED: u32 = 2;
/// bit of `infur_features()`: the Shapes calls below exist
pub const INFUR_FEATURE_SHAPES: u32 = 2048;
/// Raster: the words of the counts, the status bits
pub const INFUR_RASTER_LOOPS: u32 = 0;
pub const INFUR_RASTER_PAINTED: u32 = 1;
pub const INFUR_RASTER_CONFLICT: u32 = 2;
pub const INFUR_RASTER_STATUS: u32 = 3;
pub const INFUR_RASTER_COUNT_WORDS: u32 = 4;
pub const INFUR_RASTER_TRUNCATED: u32 = 1;
pub const INFUR_RASTER_MALFORMED: u32 = 2;
pub const INFUR_RASTER_OUTSIDE: u32 = 4;
/// bit of `infur_features()`: the Raster calls below exist
pub const INFUR_FEATURE_RASTER: u32 = 4096;

extern "C" {
    pub fn infur_abi_version() -> u32;
    pub fn infur_status_string(status: i32) -> *const c_char;
    pub fn infur_device_count() -> i32;
    pub fn infur_options_default(o: *mut infur_options);
    pub fn infur_ctx_create(o: *const infur_options, out: *mut *mut infur_ctx) -> i32;
    pub fn infur_ctx_destroy(c: *mut infur_ctx);
    pub fn infur_last_error(c: *const infur_ctx) -> *const c_char;
    pub fn infur_ctx_synchronize(c: *mut infur_ctx) -> i32;

    pub fn infur_scale_validate(factor: f32) -> i32;
    pub fn infur_scale_out_dims(w: u32, h: u32, factor: f32, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_scale(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, mode: u32,
                       out: *mut u8, out_capacity: usize, ow: *mut u32, oh: *mut u32) -> i32;

    pub fn infur_model_load(c: *mut infur_ctx, path: *const c_char) -> i32;
    pub fn infur_model_load_blob(c: *mut infur_ctx, blob: *const c_void, len: usize) -> i32;
    pub fn infur_model_unload(c: *mut infur_ctx) -> i32;
    pub fn infur_model_info_get(c: *const infur_ctx, info: *mut infur_model_info) -> i32;
    pub fn infur_model_info_get_sized(c: *const infur_ctx, info: *mut c_void, info_size: usize) -> i32;
    pub fn infur_model_advance(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, out: *mut f32,
                               aux: *mut f32, n_outputs: *mut u32) -> i32;

    pub fn infur_colorcode(c: *mut infur_ctx, khw: *const f32, k: u32, h: u32, w: u32, rgba: *mut u8) -> i32;
    pub fn infur_bgr_to_rgba(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, rgba: *mut u8) -> i32;
    pub fn infur_frame_advance(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, mode: u32,
                               rgba: *mut u8, rgba_capacity: usize, scaled_bgr: *mut u8,
                               ow: *mut u32, oh: *mut u32) -> i32;

    pub fn infur_stream_create(c: *mut infur_ctx, depth: u32, out: *mut *mut infur_stream) -> i32;
    pub fn infur_stream_destroy(s: *mut infur_stream);
    pub fn infur_stream_add_lane(s: *mut infur_stream, other: *mut infur_ctx) -> i32;
    pub fn infur_stream_submit(s: *mut infur_stream, bgr: *const u8, w: u32, h: u32, factor: f32,
                               mode: u32, frame_id: u64) -> i32;
    pub fn infur_stream_pending(s: *const infur_stream) -> u32;
    pub fn infur_stream_next_dims(s: *const infur_stream, frame_id: *mut u64, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_stream_collect(s: *mut infur_stream, rgba: *mut u8, cap: usize, scaled_bgr: *mut u8,
                                frame_id: *mut u64, ow: *mut u32, oh: *mut u32) -> i32;
    // zero-copy ingest / egress (ABI 5): the ring's pinned slots lent to the caller
    pub fn infur_stream_acquire(s: *mut infur_stream, w: u32, h: u32, factor: f32, bgr_slot: *mut *mut u8) -> i32;
    pub fn infur_stream_commit(s: *mut infur_stream, w: u32, h: u32, factor: f32, mode: u32, frame_id: u64) -> i32;
    pub fn infur_stream_collect_view(s: *mut infur_stream, rgba: *mut *const u8, scaled_bgr: *mut *const u8,
                                     frame_id: *mut u64, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_stream_release(s: *mut infur_stream) -> i32;
    pub fn infur_stream_abandon(s: *mut infur_stream) -> i32;
    // pinned host memory for caller-owned frame / mask buffers (moved by DMA by the batch calls)
    pub fn infur_host_alloc(bytes: usize, p: *mut *mut c_void) -> i32;
    pub fn infur_host_free(p: *mut c_void) -> i32;
    pub fn infur_host_is_pinned(p: *const c_void) -> u32;
    /// n frames through one context's depth-3 ring, masks in frame order (BASELINE configs[3] on one GPU)
    pub fn infur_batch_advance(c: *mut infur_ctx, frames: *const *const u8, ws: *const u32, hs: *const u32, n: u32,
                               factor: f32, mode: u32, rgba: *const *mut u8, caps: *const usize,
                               ows: *mut u32, ohs: *mut u32) -> i32;
    pub fn infur_model_warmup(c: *mut infur_ctx, w: u32, h: u32) -> i32;
    pub fn infur_ctx_set_graph_replay(c: *mut infur_ctx, enable: u32) -> i32;
    pub fn infur_ctx_graph_stats(c: *const infur_ctx, captures: *mut u64, replays: *mut u64, cached: *mut u32) -> i32;

    // several GPUs from one process: RCCL weight broadcast + frame-batch sharding
    pub fn infur_group_create(ctxs: *const *mut infur_ctx, n_ctx: u32, out: *mut *mut infur_group) -> i32;
    pub fn infur_group_destroy(g: *mut infur_group);
    pub fn infur_group_last_error(g: *const infur_group) -> *const c_char;
    pub fn infur_group_size(g: *const infur_group) -> u32;
    pub fn infur_group_uses_rccl(g: *const infur_group) -> u32;
    pub fn infur_group_worker_numa_node(g: *const infur_group, i: u32) -> i32;
    pub fn infur_group_weights_broadcast(g: *mut infur_group, root: u32) -> i32;
    pub fn infur_group_batch_advance(g: *mut infur_group, frames: *const *const u8, ws: *const u32, hs: *const u32,
                                     n: u32, factor: f32, mode: u32, rgba: *const *mut u8, caps: *const usize,
                                     ows: *mut u32, ohs: *mut u32) -> i32;
    pub fn infur_weights_broadcast(ctxs: *const *mut infur_ctx, n_ctx: u32) -> i32;
    pub fn infur_batch_advance_multi(ctxs: *const *mut infur_ctx, n_ctx: u32, frames: *const *const u8, ws: *const u32,
                                     hs: *const u32, n: u32, factor: f32, mode: u32, rgba: *const *mut u8,
                                     caps: *const usize, ows: *mut u32, ohs: *mut u32) -> i32;

    /// INFUR_DTYPE_F32_SPLIT: largest |activation| fed to a GEMM and largest |Winograd-domain input| of the last
    /// forward, and whether either left the exact range of the f16 pairs
    pub fn infur_split_range(c: *mut infur_ctx, act_amax: *mut f32, wino_amax: *mut f32, saturated: *mut u32) -> i32;
    /// INFUR_DTYPE_F16_HL (ABI 7): the opt-in range monitor of the three-byte mode -- switch it on / off; read (and clear) what the
    /// splits saw since it was enabled or last read: largest |activation|, largest |Winograd-domain input|, saturated, NaN seen
    pub fn infur_hl_monitor_enable(c: *mut infur_ctx, on: u32) -> i32;
    pub fn infur_hl_range(c: *mut infur_ctx, act_amax: *mut f32, wino_amax: *mut f32, saturated: *mut u32, nan_seen: *mut u32) -> i32;
    // ---- the rest of the header (round 5): device-resident entry points, stage kernels on device buffers, the ONNX converter,
    //      tuning database, per-kernel profile, device memory helpers -- for hosts that keep frames in HBM (a decoder writing into
    //      device memory, a display reading from it) or want the library's measurements; none is needed by `impl Processor` ----
    pub fn infur_ctx_stream(c: *mut infur_ctx) -> *mut c_void;
    pub fn infur_scale_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, mode: u32, d_out: *mut c_void,
                           out_capacity: usize, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_onnx_to_blob(onnx: *const c_void, len: usize, blob: *mut *mut c_void, blob_len: *mut usize, err: *mut c_char,
                              errcap: usize) -> i32;
    pub fn infur_buffer_free(p: *mut c_void);
    pub fn infur_model_load_blob_dev(c: *mut infur_ctx, d_blob: *const c_void, len: usize) -> i32;
    pub fn infur_model_advance_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, d_out: *mut c_void, d_aux: *mut c_void,
                                   n_outputs: *mut u32) -> i32;
    pub fn infur_model_lowres_dims(h: u32, w: u32, lh: *mut u32, lw: *mut u32) -> i32;
    pub fn infur_model_read_lowres(c: *mut infur_ctx, out_low: *mut f32, aux_low: *mut f32, lh: *mut u32, lw: *mut u32) -> i32;
    pub fn infur_debug_read_activation(c: *mut infur_ctx, index: u32, host_chw: *mut f32, cap_floats: usize, ch: *mut u32,
                                       h: *mut u32, w: *mut u32) -> i32;
    pub fn infur_pack_normalize(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, chw: *mut f32) -> i32;
    pub fn infur_pack_normalize_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, d_chw: *mut c_void) -> i32;
    pub fn infur_colorcode_dev(c: *mut infur_ctx, d_khw: *const c_void, k: u32, h: u32, w: u32, d_rgba: *mut c_void) -> i32;
    pub fn infur_bgr_to_rgba_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, d_rgba: *mut c_void) -> i32;
    pub fn infur_frame_advance_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32,
                                   d_rgba: *mut c_void, rgba_capacity: usize, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                   oh: *mut u32) -> i32;
    pub fn infur_tune_export(c: *mut infur_ctx, buf: *mut c_char, cap: usize, len: *mut usize) -> i32;
    pub fn infur_tune_import(c: *mut infur_ctx, text: *const c_char, len: usize) -> i32;
    pub fn infur_profile_enable(c: *mut infur_ctx, on: u32) -> i32;
    pub fn infur_profile_count(c: *mut infur_ctx, n: *mut u32) -> i32;
    pub fn infur_profile_get(c: *mut infur_ctx, i: u32, rec: *mut infur_kernel_record) -> i32;
    pub fn infur_debug_profile_variant(c: *mut infur_ctx, i: u32, buf: *mut c_char, cap: usize) -> i32;
    pub fn infur_dev_alloc(c: *mut infur_ctx, bytes: usize, d_ptr: *mut *mut c_void) -> i32;
    pub fn infur_dev_free(c: *mut infur_ctx, d_ptr: *mut c_void) -> i32;
    pub fn infur_memcpy_h2d(c: *mut infur_ctx, d_dst: *mut c_void, src: *const c_void, bytes: usize) -> i32;
    pub fn infur_memcpy_d2h(c: *mut infur_ctx, dst: *mut c_void, d_src: *const c_void, bytes: usize) -> i32;
    // ---- Segments: class plane, confidence plane, per-class statistics, RGBA shaded by that confidence (any may be null) ----
    pub fn infur_features() -> u32;
    pub fn infur_voc_class_name(k: u32) -> *const c_char;
    pub fn infur_segments(c: *mut infur_ctx, khw: *const f32, k: u32, h: u32, w: u32, decode: u32, klass: *mut u8, conf: *mut u8,
                          stats: *mut u64, rgba: *mut u8) -> i32;
    pub fn infur_segments_dev(c: *mut infur_ctx, d_khw: *const c_void, k: u32, h: u32, w: u32, decode: u32, d_klass: *mut c_void,
                              d_conf: *mut c_void, d_stats: *mut c_void, d_rgba: *mut c_void) -> i32;
    pub fn infur_frame_segments(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                klass: *mut u8, conf: *mut u8, plane_capacity: usize, stats: *mut u64, stats_classes: u32,
                                rgba: *mut u8, rgba_capacity: usize, scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_frame_segments_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32,
                                    decode: u32, d_klass: *mut c_void, d_conf: *mut c_void, plane_capacity: usize,
                                    d_stats: *mut c_void, stats_classes: u32, d_rgba: *mut c_void, rgba_capacity: usize,
                                    d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32) -> i32;
    // ---- Regions: connected components of the class plane: label plane, per-region table, count (any may be null) ----
    pub fn infur_regions(c: *mut infur_ctx, klass: *const u8, conf: *const u8, h: u32, w: u32, connectivity: u32, min_pixels: u32,
                         flags: u32, labels: *mut u32, table: *mut u64, table_rows: u32, n_regions: *mut u32) -> i32;
    pub fn infur_regions_dev(c: *mut infur_ctx, d_klass: *const c_void, d_conf: *const c_void, h: u32, w: u32, connectivity: u32,
                             min_pixels: u32, flags: u32, d_labels: *mut c_void, d_table: *mut c_void, table_rows: u32,
                             d_n_regions: *mut c_void) -> i32;
    pub fn infur_frame_regions(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                               connectivity: u32, min_pixels: u32, flags: u32, klass: *mut u8, conf: *mut u8, plane_capacity: usize,
                               labels: *mut u32, labels_capacity: usize, table: *mut u64, table_rows: u32, n_regions: *mut u32,
                               scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_frame_regions_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                   connectivity: u32, min_pixels: u32, flags: u32, d_klass: *mut c_void, d_conf: *mut c_void,
                                   plane_capacity: usize, d_labels: *mut c_void, labels_capacity: usize, d_table: *mut c_void,
                                   table_rows: u32, d_n_regions: *mut c_void, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                   oh: *mut u32) -> i32;
    // Tracks: the tracker handle is an untyped pointer in the C header
    pub fn infur_tracker_create(c: *mut infur_ctx, max_regions: u32, pair_slots: u32, tracker: *mut *mut c_void) -> i32;
    pub fn infur_tracker_destroy(tracker: *mut c_void);
    pub fn infur_tracker_reset(tracker: *mut c_void, first_id: u32) -> i32;
    pub fn infur_tracker_set_memory(tracker: *mut c_void, max_lost: u32, reach: u32, gallery_rows: u32) -> i32;
    pub fn infur_tracker_memory(tracker: *mut c_void, gap_of_region: *mut u32, rows: u32, memory_summary: *mut u32,
                                lost_table: *mut u64, lost_rows: u32) -> i32;
    pub fn infur_tracker_memory_dev(tracker: *mut c_void, d_gap_of_region: *mut c_void, rows: u32, d_memory_summary: *mut c_void,
                                    d_lost_table: *mut c_void, lost_rows: u32) -> i32;
    pub fn infur_tracks(tracker: *mut c_void, labels: *const u32, table: *const u64, table_rows: u32, n_regions: u32, h: u32, w: u32,
                        min_overlap: u32, track_of_region: *mut u32, track_plane: *mut u32, track_table: *mut u64,
                        summary: *mut u32) -> i32;
    pub fn infur_tracks_dev(tracker: *mut c_void, d_labels: *const c_void, d_table: *const c_void, table_rows: u32,
                            d_n_regions: *const c_void, h: u32, w: u32, min_overlap: u32, d_track_of_region: *mut c_void,
                            d_track_plane: *mut c_void, d_track_table: *mut c_void, d_summary: *mut c_void) -> i32;
    pub fn infur_frame_tracks(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                              connectivity: u32, min_pixels: u32, flags: u32, klass: *mut u8, conf: *mut u8, plane_capacity: usize,
                              labels: *mut u32, labels_capacity: usize, table: *mut u64, table_rows: u32, n_regions: *mut u32,
                              scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32, tracker: *mut c_void, min_overlap: u32,
                              track_of_region: *mut u32, track_plane: *mut u32, track_table: *mut u64, summary: *mut u32) -> i32;
    pub fn infur_frame_tracks_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                  connectivity: u32, min_pixels: u32, flags: u32, d_klass: *mut c_void, d_conf: *mut c_void,
                                  plane_capacity: usize, d_labels: *mut c_void, labels_capacity: usize, d_table: *mut c_void,
                                  table_rows: u32, d_n_regions: *mut c_void, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                  oh: *mut u32, tracker: *mut c_void, min_overlap: u32, d_track_of_region: *mut c_void,
                                  d_track_plane: *mut c_void, d_track_table: *mut c_void, d_summary: *mut c_void) -> i32;
    // Runs: a byte or u32 plane as run-length records
    pub fn infur_runs(c: *mut infur_ctx, plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                      runs: *mut u32, runs_rows: u32, row_start: *mut u32, n_runs: *mut u32) -> i32;
    pub fn infur_runs_dev(c: *mut infur_ctx, d_plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                          d_runs: *mut c_void, runs_rows: u32, d_row_start: *mut c_void, d_n_runs: *mut c_void) -> i32;
    pub fn infur_frame_runs(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32, flags: u32,
                            skip_value: u32, runs: *mut u32, runs_rows: u32, row_start: *mut u32, row_start_rows: u32,
                            n_runs: *mut u32, stats: *mut u64, stats_capacity: u32, scaled_bgr: *mut u8, ow: *mut u32,
                            oh: *mut u32) -> i32;
    pub fn infur_frame_runs_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                flags: u32, skip_value: u32, d_runs: *mut c_void, runs_rows: u32, d_row_start: *mut c_void,
                                row_start_rows: u32, d_n_runs: *mut c_void, d_stats: *mut c_void, stats_capacity: u32,
                                d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32) -> i32;
    // Outlines: the region boundaries of a byte or u32 plane as polygon loops
    pub fn infur_outlines(c: *mut infur_ctx, plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                          max_edges: u32, loops: *mut u32, loops_rows: u32, vertices: *mut u32, vertex_rows: u32,
                          counts: *mut u32) -> i32;
    pub fn infur_outlines_dev(c: *mut infur_ctx, d_plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32,
                              skip_value: u32, max_edges: u32, d_loops: *mut c_void, loops_rows: u32, d_vertices: *mut c_void,
                              vertex_rows: u32, d_counts: *mut c_void) -> i32;
    pub fn infur_frame_outlines(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                flags: u32, skip_value: u32, max_edges: u32, loops: *mut u32, loops_rows: u32, vertices: *mut u32,
                                vertex_rows: u32, counts: *mut u32, stats: *mut u64, stats_capacity: u32, scaled_bgr: *mut u8,
                                ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_frame_outlines_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32,
                                    decode: u32, flags: u32, skip_value: u32, max_edges: u32, d_loops: *mut c_void,
                                    loops_rows: u32, d_vertices: *mut c_void, vertex_rows: u32, d_counts: *mut c_void,
                                    d_stats: *mut c_void, stats_capacity: u32, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                    oh: *mut u32) -> i32;
    // Simplify: Douglas-Peucker on Outlines' loops, and the frame path that ends in it
    pub fn infur_simplify(c: *mut infur_ctx, loops: *const u32, loops_rows_in: u32, vertices: *const u32, vertex_rows_in: u32,
                          counts: *const u32, h: u32, w: u32, tol16: u32, loops_out: *mut u32, loops_rows_out: u32,
                          vertices_out: *mut u32, vertex_rows_out: u32, counts_out: *mut u32) -> i32;
    pub fn infur_simplify_dev(c: *mut infur_ctx, d_loops: *const c_void, loops_rows_in: u32, d_vertices: *const c_void,
                              vertex_rows_in: u32, d_counts: *const c_void, h: u32, w: u32, tol16: u32, d_loops_out: *mut c_void,
                              loops_rows_out: u32, d_vertices_out: *mut c_void, vertex_rows_out: u32,
                              d_counts_out: *mut c_void) -> i32;
    pub fn infur_frame_polygons(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                flags: u32, skip_value: u32, max_edges: u32, tol16: u32, loops: *mut u32, loops_rows: u32,
                                vertices: *mut u32, vertex_rows: u32, counts: *mut u32, stats: *mut u64, stats_capacity: u32,
                                scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_frame_polygons_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32,
                                    decode: u32, flags: u32, skip_value: u32, max_edges: u32, tol16: u32, d_loops: *mut c_void,
                                    loops_rows: u32, d_vertices: *mut c_void, vertex_rows: u32, d_counts: *mut c_void,
                                    d_stats: *mut c_void, stats_capacity: u32, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                    oh: *mut u32) -> i32;
    // Coverage: Outlines' loops simplified arc by arc, shared borders once, and the frame path that ends in it
    pub fn infur_coverage(c: *mut infur_ctx, plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                          loops: *const u32, loops_rows_in: u32, vertices: *const u32, vertex_rows_in: u32, counts: *const u32,
                          tol16: u32, aug_rows: u32, loops_out: *mut u32, loops_rows_out: u32, vertices_out: *mut u32,
                          vertex_rows_out: u32, counts_out: *mut u32) -> i32;
    pub fn infur_coverage_dev(c: *mut infur_ctx, d_plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32,
                              skip_value: u32, d_loops: *const c_void, loops_rows_in: u32, d_vertices: *const c_void,
                              vertex_rows_in: u32, d_counts: *const c_void, tol16: u32, aug_rows: u32, d_loops_out: *mut c_void,
                              loops_rows_out: u32, d_vertices_out: *mut c_void, vertex_rows_out: u32,
                              d_counts_out: *mut c_void) -> i32;
    pub fn infur_frame_coverage(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                flags: u32, skip_value: u32, max_edges: u32, tol16: u32, loops: *mut u32, loops_rows: u32,
                                vertices: *mut u32, vertex_rows: u32, counts: *mut u32, stats: *mut u64, stats_capacity: u32,
                                scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32) -> i32;
    pub fn infur_frame_coverage_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32,
                                    decode: u32, flags: u32, skip_value: u32, max_edges: u32, tol16: u32, d_loops: *mut c_void,
                                    loops_rows: u32, d_vertices: *mut c_void, vertex_rows: u32, d_counts: *mut c_void,
                                    d_stats: *mut c_void, stats_capacity: u32, d_scaled_bgr: *mut c_void, ow: *mut u32,
                                    oh: *mut u32) -> i32;
    // Anchors: the squared distance transform of a byte or u32 plane by value, one interior point per value
    pub fn infur_anchors(c: *mut infur_ctx, plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                         dist2: *mut u32, anchors: *mut u32, rows: u32) -> i32;
    pub fn infur_anchors_dev(c: *mut infur_ctx, d_plane: *const c_void, elem_bytes: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                             d_dist2: *mut c_void, d_anchors: *mut c_void, rows: u32) -> i32;
    pub fn infur_frame_anchors(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                               connectivity: u32, min_pixels: u32, flags: u32, klass: *mut u8, conf: *mut u8, plane_capacity: usize,
                               labels: *mut u32, labels_capacity: usize, table: *mut u64, table_rows: u32, n_regions: *mut u32,
                               scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32, dist2: *mut u32, dist2_capacity: usize,
                               anchors: *mut u32) -> i32;
    pub fn infur_frame_anchors_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                   connectivity: u32, min_pixels: u32, flags: u32, d_klass: *mut c_void, d_conf: *mut c_void,
                                   plane_capacity: usize, d_labels: *mut c_void, labels_capacity: usize, d_table: *mut c_void,
                                   table_rows: u32, d_n_regions: *mut c_void, d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32,
                                   d_dist2: *mut c_void, dist2_capacity: usize, d_anchors: *mut c_void) -> i32;
    // Compare: the confusion matrix of two byte or u32 planes and the best partner per value of either
    pub fn infur_compare(c: *mut infur_ctx, a: *const c_void, elem_a: u32, b: *const c_void, elem_b: u32, h: u32, w: u32, flags: u32,
                         ignore_a: u32, ignore_b: u32, matrix: *mut u32, rows_a: u32, rows_b: u32, rows_a_out: *mut u32,
                         rows_b_out: *mut u32, counts: *mut u32, pair_slots: u32) -> i32;
    pub fn infur_compare_dev(c: *mut infur_ctx, d_a: *const c_void, elem_a: u32, d_b: *const c_void, elem_b: u32, h: u32, w: u32,
                             flags: u32, ignore_a: u32, ignore_b: u32, d_matrix: *mut c_void, rows_a: u32, rows_b: u32,
                             d_rows_a_out: *mut c_void, d_rows_b_out: *mut c_void, d_counts: *mut c_void, pair_slots: u32) -> i32;
    pub fn infur_frame_compare(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32, flags: u32,
                               ignore_b: u32, truth: *const u8, truth_capacity: usize, klass: *mut u8, conf: *mut u8,
                               plane_capacity: usize, matrix: *mut u32, rows_a: u32, rows_b: u32, rows_a_out: *mut u32,
                               rows_b_out: *mut u32, counts: *mut u32, pair_slots: u32, scaled_bgr: *mut u8, ow: *mut u32,
                               oh: *mut u32) -> i32;
    pub fn infur_frame_compare_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                   flags: u32, ignore_b: u32, d_truth: *const c_void, truth_capacity: usize, d_klass: *mut c_void,
                                   d_conf: *mut c_void, plane_capacity: usize, d_matrix: *mut c_void, rows_a: u32, rows_b: u32,
                                   d_rows_a_out: *mut c_void, d_rows_b_out: *mut c_void, d_counts: *mut c_void, pair_slots: u32,
                                   d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32) -> i32;
    // Adjacency: which values of a plane touch, along how many pixel edges; Sieve: speckle regions merged into their neighbours
    pub fn infur_adjacency(c: *mut infur_ctx, plane: *const c_void, elem: u32, h: u32, w: u32, flags: u32, skip_value: u32, rows: u32,
                           pairs: *mut u32, pair_rows: u32, rows_out: *mut u32, counts: *mut u32, pair_slots: u32) -> i32;
    pub fn infur_adjacency_dev(c: *mut infur_ctx, d_plane: *const c_void, elem: u32, h: u32, w: u32, flags: u32, skip_value: u32,
                               rows: u32, d_pairs: *mut c_void, pair_rows: u32, d_rows_out: *mut c_void, d_counts: *mut c_void,
                               pair_slots: u32) -> i32;
    pub fn infur_sieve(c: *mut infur_ctx, klass: *const u8, labels: *const u32, table: *const u64, table_rows: u32, n_regions: u32,
                       h: u32, w: u32, min_pixels: u32, max_rounds: u32, pair_slots: u32, klass_out: *mut u8, rows_out: *mut u32,
                       counts: *mut u32) -> i32;
    pub fn infur_sieve_dev(c: *mut infur_ctx, d_klass: *const c_void, d_labels: *const c_void, d_table: *const c_void, table_rows: u32,
                           d_n_regions: *const c_void, h: u32, w: u32, min_pixels: u32, max_rounds: u32, pair_slots: u32,
                           d_klass_out: *mut c_void, d_rows_out: *mut c_void, d_counts: *mut c_void) -> i32;
    pub fn infur_frame_sieve(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                             connectivity: u32, min_pixels: u32, flags: u32, klass: *mut u8, conf: *mut u8, plane_capacity: usize,
                             labels: *mut u32, labels_capacity: usize, table: *mut u64, table_rows: u32, n_regions: *mut u32,
                             scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32, max_rounds: u32, pair_slots: u32, klass_out: *mut u8,
                             counts: *mut u32) -> i32;
    pub fn infur_frame_sieve_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                 connectivity: u32, min_pixels: u32, flags: u32, d_klass: *mut c_void, d_conf: *mut c_void,
                                 plane_capacity: usize, d_labels: *mut c_void, labels_capacity: usize, d_table: *mut c_void,
                                 table_rows: u32, d_n_regions: *mut c_void, d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32,
                                 max_rounds: u32, pair_slots: u32, d_klass_out: *mut c_void, d_counts: *mut c_void) -> i32;
    // Shapes: area, moments, convex hull and minimum rectangle per outline loop, and the frame path that ends in it.  The 64-bit
    // words are signed (two's complement)
    pub fn infur_shapes(c: *mut infur_ctx, loops: *const u32, loops_rows_in: u32, vertices: *const u32, vertex_rows_in: u32,
                        counts: *const u32, h: u32, w: u32, loops_out: *mut u32, loops_rows_out: u32, vertices_out: *mut u32,
                        vertex_rows_out: u32, shapes: *mut u64, shape_rows: u32, values: *mut u64, value_rows: u32,
                        counts_out: *mut u32) -> i32;
    pub fn infur_shapes_dev(c: *mut infur_ctx, d_loops: *const c_void, loops_rows_in: u32, d_vertices: *const c_void,
                            vertex_rows_in: u32, d_counts: *const c_void, h: u32, w: u32, d_loops_out: *mut c_void,
                            loops_rows_out: u32, d_vertices_out: *mut c_void, vertex_rows_out: u32, d_shapes: *mut c_void,
                            shape_rows: u32, d_values: *mut c_void, value_rows: u32, d_counts_out: *mut c_void) -> i32;
    pub fn infur_frame_shapes(c: *mut infur_ctx, bgr: *const u8, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                              connectivity: u32, min_pixels: u32, flags: u32, klass: *mut u8, conf: *mut u8, plane_capacity: usize,
                              labels: *mut u32, labels_capacity: usize, table: *mut u64, table_rows: u32, n_regions: *mut u32,
                              scaled_bgr: *mut u8, ow: *mut u32, oh: *mut u32, max_edges: u32, loops_out: *mut u32,
                              loops_rows_out: u32, vertices_out: *mut u32, vertex_rows_out: u32, shapes: *mut u64, shape_rows: u32,
                              values: *mut u64, counts_out: *mut u32) -> i32;
    pub fn infur_frame_shapes_dev(c: *mut infur_ctx, d_bgr: *const c_void, w: u32, h: u32, factor: f32, scale_mode: u32, decode: u32,
                                  connectivity: u32, min_pixels: u32, flags: u32, d_klass: *mut c_void, d_conf: *mut c_void,
                                  plane_capacity: usize, d_labels: *mut c_void, labels_capacity: usize, d_table: *mut c_void,
                                  table_rows: u32, d_n_regions: *mut c_void, d_scaled_bgr: *mut c_void, ow: *mut u32, oh: *mut u32,
                                  max_edges: u32, d_loops_out: *mut c_void, loops_rows_out: u32, d_vertices_out: *mut c_void,
                                  vertex_rows_out: u32, d_shapes: *mut c_void, shape_rows: u32, d_values: *mut c_void,
                                  d_counts_out: *mut c_void) -> i32;
    // Raster: polygon loops, or run-length records, filled back into a plane of 1- or 4-byte elements
    pub fn infur_raster(c: *mut infur_ctx, loops: *const u32, loops_rows_in: u32, vertices: *const u32, vertex_rows_in: u32,
                        counts: *const u32, h: u32, w: u32, elem_bytes: u32, fill_value: u32, plane_out: *mut c_void,
                        counts_out: *mut u32) -> i32;
    pub fn infur_raster_dev(c: *mut infur_ctx, d_loops: *const c_void, loops_rows_in: u32, d_vertices: *const c_void,
                            vertex_rows_in: u32, d_counts: *const c_void, h: u32, w: u32, elem_bytes: u32, fill_value: u32,
                            d_plane_out: *mut c_void, d_counts_out: *mut c_void) -> i32;
    pub fn infur_raster_runs(c: *mut infur_ctx, runs: *const u32, runs_rows_in: u32, n_runs: u32, h: u32, w: u32, elem_bytes: u32,
                             fill_value: u32, plane_out: *mut c_void, counts_out: *mut u32) -> i32;
    pub fn infur_raster_runs_dev(c: *mut infur_ctx, d_runs: *const c_void, runs_rows_in: u32, d_n_runs: *const c_void, h: u32,
                                 w: u32, elem_bytes: u32, fill_value: u32, d_plane_out: *mut c_void, d_counts_out: *mut c_void) -> i32;
}
