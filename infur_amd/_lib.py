"""ctypes binding of ``libinfur_hip.so`` (the C ABI declared in include/infur_hip.h).

There is no fallback: if the shared library is missing or does not load, importing
the product path fails loudly with instructions to build it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# INFUR_LIB_PATH: an instrumentation build of the same ABI (scripts/ktrace.py: `make ktrace` -> libinfur_hip_ktrace.so)
LIB_PATH = os.environ.get("INFUR_LIB_PATH") or os.path.join(_HERE, "libinfur_hip.so")

ABI_VERSION = 7  # INFUR_ABI_VERSION of include/infur_hip.h

# status codes (include/infur_hip.h)
OK = 0
E_INVALID_SCALE = 1
E_ZERO_SIZE_IN = 2
E_ZERO_SIZE_OUT = 3
E_SHAPE = 4
E_MODEL_NOT_LOADED = 5
E_MODEL_FORMAT = 6
E_HIP = 7
E_RCCL = 8
E_INVALID_ARG = 9
E_IO = 10
E_CAPACITY = 11

SCALE_NEAREST, SCALE_BILINEAR = 0, 1
DTYPE_F32 = 0
DTYPE_F16 = 1
DTYPE_F32_SPLIT = 2
DTYPE_F32_SPLIT_FP8 = 3  # split mode with the cross terms on the fp8 MX MFMA ("f32x")
DTYPE_F16_HL = 5  # three-byte tensors (f16 hi + e5m2 lo planes), two MFMA units per product ("f16hl")

# Segments (infur_segments / infur_frame_segments): decode modes, the columns of the statistics table, the feature bit
DECODE_RAW, DECODE_SOFTMAX = 0, 1
STAT_PIXELS, STAT_SUM_X, STAT_SUM_Y, STAT_SUM_CONF, STAT_MIN_X, STAT_MIN_Y, STAT_MAX_X, STAT_MAX_Y = range(8)
STAT_WORDS = 8
FEATURE_SEGMENTS = 1
# Regions (infur_regions / infur_frame_regions): connectivity, flags, the two extra columns of a region's row, the feature bit
CONNECT_4, CONNECT_8 = 4, 8
REGIONS_SKIP_BACKGROUND = 1
REGION_CLASS, REGION_FIRST, REGION_WORDS = 8, 9, 10
REGION_NONE = 0xFFFFFFFF
FEATURE_REGIONS = 2
# Tracks (infur_tracks / infur_frame_tracks): the columns of a track row, the status bits, the words of the summary, the feature bit
TRACK_ID, TRACK_AGE, TRACK_BORN, TRACK_PREV_REGION, TRACK_OVERLAP, TRACK_PREV_PIXELS, TRACK_PREV_SUM_X, TRACK_PREV_SUM_Y = range(8)
TRACK_WORDS = 8
TRACK_NONE = 0xFFFFFFFF
TRACKS_TRUNCATED, TRACKS_OVERFLOW, TRACKS_IDS_EXHAUSTED = 1, 2, 4
TRACKS_SUMMARY_STATUS, TRACKS_SUMMARY_CONTINUED, TRACKS_SUMMARY_NEW, TRACKS_SUMMARY_ENDED = range(4)
TRACKS_SUMMARY_WORDS = 4
FEATURE_TRACKS = 4
# Tracks' memory (infur_tracker_set_memory / infur_tracker_memory): the status bit, the words of a gallery entry and of the memory summary
TRACKS_GALLERY_FULL = 8
(LOST_ID, LOST_AGE, LOST_BORN, LOST_CLASS, LOST_PIXELS, LOST_SUM_X, LOST_SUM_Y, LOST_MIN_X, LOST_MIN_Y, LOST_MAX_X, LOST_MAX_Y,
 LOST_SEEN) = range(12)
LOST_WORDS = 12
TRACK_MEMORY_REVIVED, TRACK_MEMORY_LOST, TRACK_MEMORY_EXPIRED, TRACK_MEMORY_HELD = range(4)
TRACK_MEMORY_WORDS = 4
FEATURE_TRACK_MEMORY = 128
# Runs (infur_runs / infur_frame_runs): the flag, the words of a record, the feature bit
RUNS_SKIP = 1
RUN_START, RUN_END, RUN_VALUE, RUN_WORDS = 0, 1, 2, 3
FEATURE_RUNS = 8
# Outlines (infur_outlines / infur_frame_outlines): the flags, the words of a loop record, the feature bit
OUTLINES_SKIP, OUTLINES_CONN8 = 1, 2
LOOP_OFFSET, LOOP_COUNT, LOOP_VALUE, LOOP_START, LOOP_WORDS = 0, 1, 2, 3, 4
FEATURE_OUTLINES = 16
# Simplify (infur_simplify / infur_frame_polygons): the words of its counts, the status bits, the feature bit
SIMPLIFY_LOOPS, SIMPLIFY_VERTICES, SIMPLIFY_DEGENERATE, SIMPLIFY_STATUS, SIMPLIFY_COUNT_WORDS = 0, 1, 2, 3, 4
SIMPLIFY_TRUNCATED, SIMPLIFY_MALFORMED = 1, 2
FEATURE_SIMPLIFY = 32
# Coverage (infur_coverage / infur_frame_coverage): the flag, the words of its counts, the status bits, the feature bit
COVERAGE_SKIP = 1
COVERAGE_LOOPS, COVERAGE_VERTICES, COVERAGE_DEGENERATE, COVERAGE_STATUS, COVERAGE_AUG, COVERAGE_ARCS, COVERAGE_COUNT_WORDS = 0, 1, 2, 3, 4, 5, 6
COVERAGE_TRUNCATED, COVERAGE_MALFORMED, COVERAGE_OVERFLOW = 1, 2, 4
FEATURE_COVERAGE = 64
# Anchors (infur_anchors / infur_frame_anchors): the flag, the words of a row, the "no pixel" index, the feature bit
ANCHORS_SKIP = 1
ANCHOR_PIXEL, ANCHOR_DIST2, ANCHOR_WORDS = 0, 1, 2
ANCHOR_NONE = 0xFFFFFFFF
FEATURE_ANCHORS = 256
# Compare (infur_compare / infur_frame_compare): the flags, the words of a row and of the counts, the status bits, the feature bit
COMPARE_IGNORE_A, COMPARE_IGNORE_B = 1, 2
COMPARE_PIXELS, COMPARE_PARTNER, COMPARE_INTER, COMPARE_UNION, COMPARE_WORDS = 0, 1, 2, 3, 4
(COMPARE_COMPARED, COMPARE_EQUAL, COMPARE_IGNORED, COMPARE_OUTSIDE, COMPARE_PAIRS, COMPARE_MATCHED, COMPARE_RUNS, COMPARE_STATUS,
 COMPARE_COUNT_WORDS) = 0, 1, 2, 3, 4, 5, 6, 7, 8
COMPARE_OVERFLOW, COMPARE_TABLE = 1, 2
COMPARE_NONE = 0xFFFFFFFF
FEATURE_COMPARE = 512
# Adjacency and Sieve (infur_adjacency / infur_sieve / infur_frame_sieve): the flag, the words of a pair record, of a row and of the
# counts, the status bits, the feature bit both groups share
ADJ_SKIP = 1
ADJ_A, ADJ_B, ADJ_BORDER, ADJ_FIRST, ADJ_PAIR_WORDS = 0, 1, 2, 3, 4
ADJ_DEGREE, ADJ_LONGEST, ADJ_ROW_BORDER, ADJ_PERIMETER, ADJ_ROW_WORDS = 0, 1, 2, 3, 4
ADJ_PAIRS, ADJ_EDGES, ADJ_SKIPPED, ADJ_OUTSIDE, ADJ_RUNS, ADJ_WRITTEN, ADJ_STATUS, ADJ_COUNT_WORDS = 0, 1, 2, 3, 4, 5, 7, 8
ADJ_OVERFLOW, ADJ_TRUNCATED = 1, 2
ADJ_NONE = 0xFFFFFFFF
SIEVE_CLASS, SIEVE_INTO, SIEVE_ROUND, SIEVE_BORDER, SIEVE_ROW_WORDS = 0, 1, 2, 3, 4
(SIEVE_REGIONS, SIEVE_SMALL, SIEVE_ABSORBED, SIEVE_STRANDED, SIEVE_ROUNDS, SIEVE_PIXELS_CHANGED, SIEVE_PAIRS, SIEVE_STATUS,
 SIEVE_COUNT_WORDS) = 0, 1, 2, 3, 4, 5, 6, 7, 8
SIEVE_OVERFLOW, SIEVE_ROUNDS_EXHAUSTED, SIEVE_TABLE_SHORT = 1, 2, 4
SIEVE_NONE = 0xFFFFFFFF
FEATURE_SIEVE = 1024
# Shapes (infur_shapes / infur_frame_shapes): the words of a per-loop record, of a per-value row (8 .. 10 differ) and of the counts,
# the status bits, the feature bit
(SHAPE_AREA2, SHAPE_PERIMETER, SHAPE_M10_6, SHAPE_M01_6, SHAPE_M20_12, SHAPE_M02_12, SHAPE_M11_24, SHAPE_HULL_AREA2, SHAPE_RECT_EDGE,
 SHAPE_RECT_W, SHAPE_RECT_H, SHAPE_RECT_L, SHAPE_WORDS) = range(13)
SHAPE_OUTER, SHAPE_HOLES, SHAPE_LOOP = 8, 9, 10
SHAPES_LOOPS, SHAPES_VERTICES, SHAPES_STATUS, SHAPES_LARGEST, SHAPES_COUNT_WORDS = 0, 1, 2, 3, 4
SHAPES_TRUNCATED, SHAPES_MALFORMED = 1, 2
FEATURE_SHAPES = 2048
# Raster (infur_raster / infur_raster_runs): the words of the counts, the status bits, the feature bit
RASTER_LOOPS, RASTER_PAINTED, RASTER_CONFLICT, RASTER_STATUS, RASTER_COUNT_WORDS = 0, 1, 2, 3, 4
RASTER_TRUNCATED, RASTER_MALFORMED, RASTER_OUTSIDE = 1, 2, 4
FEATURE_RASTER = 4096


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("compute_dtype", C.c_uint32),
        ("compute_aux", C.c_uint32),
        ("profile", C.c_uint32),
        ("keep_activations", C.c_uint32),
        ("winograd_min_cin", C.c_uint32),
        ("winograd_tile", C.c_uint32),
        ("no_autotune", C.c_uint32),
        ("no_fuse_downsample", C.c_uint32),
        ("no_fuse_stem_pool", C.c_uint32),
        ("no_fuse_b2b", C.c_uint32),
        ("stream", C.c_void_p),
    ]


class ModelInfoC(C.Structure):
    _fields_ = [
        ("input_name", C.c_char * 32),
        ("input0_dtype", C.c_char * 16),
        ("output_names", (C.c_char * 32) * 2),
        ("n_outputs", C.c_uint32),
        ("num_classes", C.c_uint32),
        ("depth", C.c_uint32),
        ("n_convs", C.c_uint32),
        ("weight_bytes", C.c_uint64),
        ("quantised", C.c_uint32),        # ABI 4
        ("resize_u8_heads", C.c_uint32),  # ABI 4
    ]


class KernelRecord(C.Structure):
    _fields_ = [
        ("name", C.c_char * 48),
        ("kernel", C.c_char * 32),
        ("ms", C.c_float),
        ("flops", C.c_double),
        ("bytes", C.c_double),
        ("algo_flops", C.c_double),
    ]


_u32p = C.POINTER(C.c_uint32)
_vp = C.c_void_p
_sz = C.c_size_t
_u32 = C.c_uint32
_f = C.c_float

# every symbol include/infur_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "infur_abi_version": (C.c_uint32, []),
    "infur_status_string": (C.c_char_p, [C.c_int32]),
    "infur_device_count": (C.c_int32, []),
    "infur_options_default": (None, [C.POINTER(Options)]),
    "infur_ctx_create": (C.c_int32, [C.POINTER(Options), C.POINTER(_vp)]),
    "infur_ctx_destroy": (None, [_vp]),
    "infur_last_error": (C.c_char_p, [_vp]),
    "infur_ctx_synchronize": (C.c_int32, [_vp]),
    "infur_ctx_stream": (_vp, [_vp]),
    "infur_scale_validate": (C.c_int32, [_f]),
    "infur_scale_out_dims": (C.c_int32, [_u32, _u32, _f, _u32p, _u32p]),
    "infur_scale": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _vp, _sz, _u32p, _u32p]),
    "infur_scale_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _vp, _sz, _u32p, _u32p]),
    "infur_model_load": (C.c_int32, [_vp, C.c_char_p]),
    "infur_onnx_to_blob": (C.c_int32, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz), C.c_char_p, _sz]),
    "infur_buffer_free": (None, [_vp]),
    "infur_model_load_blob": (C.c_int32, [_vp, _vp, _sz]),
    "infur_model_load_blob_dev": (C.c_int32, [_vp, _vp, _sz]),
    "infur_model_unload": (C.c_int32, [_vp]),
    "infur_model_info_get": (C.c_int32, [_vp, C.POINTER(ModelInfoC)]),
    "infur_model_info_get_sized": (C.c_int32, [_vp, _vp, C.c_size_t]),
    "infur_model_advance": (C.c_int32, [_vp, _vp, _u32, _u32, _vp, _vp, _u32p]),
    "infur_model_advance_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _vp, _vp, _u32p]),
    "infur_model_warmup": (C.c_int32, [_vp, _u32, _u32]),
    "infur_ctx_set_graph_replay": (C.c_int32, [_vp, _u32]),
    "infur_ctx_graph_stats": (C.c_int32, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_u32)]),
    "infur_model_lowres_dims": (C.c_int32, [_u32, _u32, _u32p, _u32p]),
    "infur_model_read_lowres": (C.c_int32, [_vp, _vp, _vp, _u32p, _u32p]),
    "infur_debug_read_activation": (C.c_int32, [_vp, _u32, _vp, _sz, _u32p, _u32p, _u32p]),
    "infur_pack_normalize": (C.c_int32, [_vp, _vp, _u32, _u32, _vp]),
    "infur_pack_normalize_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _vp]),
    "infur_colorcode": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "infur_colorcode_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "infur_bgr_to_rgba": (C.c_int32, [_vp, _vp, _u32, _u32, _vp]),
    "infur_bgr_to_rgba_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _vp]),
    "infur_frame_advance": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _vp, _sz, _vp, _u32p, _u32p]),
    "infur_frame_advance_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _vp, _sz, _vp, _u32p, _u32p]),
    "infur_features": (C.c_uint32, []),
    "infur_voc_class_name": (C.c_char_p, [_u32]),
    "infur_segments": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "infur_segments_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "infur_frame_segments": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _vp, _vp, _sz, _vp, _u32, _vp, _sz, _vp, _u32p, _u32p]),
    "infur_frame_segments_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _vp, _vp, _sz, _vp, _u32, _vp, _sz, _vp, _u32p,
                                             _u32p]),
    "infur_regions": (C.c_int32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32, _vp]),
    "infur_regions_dev": (C.c_int32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32, _vp]),
    "infur_frame_regions": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                        _u32p, _u32p]),
    "infur_frame_regions_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp,
                                            _vp, _u32p, _u32p]),
    "infur_tracker_create": (C.c_int32, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "infur_tracker_destroy": (None, [_vp]),
    "infur_tracker_reset": (C.c_int32, [_vp, _u32]),
    "infur_tracker_set_memory": (C.c_int32, [_vp, _u32, _u32, _u32]),
    "infur_tracker_memory": (C.c_int32, [_vp, _vp, _u32, _vp, _vp, _u32]),
    "infur_tracker_memory_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _vp, _u32]),
    "infur_tracks": (C.c_int32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "infur_tracks_dev": (C.c_int32, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "infur_frame_tracks": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                       _u32p, _u32p, _vp, _u32, _vp, _vp, _vp, _vp]),
    "infur_frame_tracks_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp,
                                           _vp, _u32p, _u32p, _vp, _u32, _vp, _vp, _vp, _vp]),
    "infur_runs": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "infur_runs_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "infur_frame_runs": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _u32p,
                                     _u32p]),
    "infur_frame_runs_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp,
                                         _u32p, _u32p]),
    "infur_outlines": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_outlines_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_frame_outlines": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp,
                                         _u32p, _u32p]),
    "infur_frame_outlines_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32,
                                             _vp, _u32p, _u32p]),
    "infur_simplify": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_simplify_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_frame_polygons": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32,
                                         _vp, _u32p, _u32p]),
    "infur_frame_polygons_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp,
                                             _u32, _vp, _u32p, _u32p]),
    "infur_coverage": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_coverage_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_frame_coverage": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32,
                                         _vp, _u32p, _u32p]),
    "infur_frame_coverage_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp,
                                             _u32, _vp, _u32p, _u32p]),
    "infur_anchors": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32]),
    "infur_anchors_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32]),
    "infur_frame_anchors": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                        _u32p, _u32p, _vp, _sz, _vp]),
    "infur_frame_anchors_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp,
                                            _vp, _u32p, _u32p, _vp, _sz, _vp]),
    "infur_compare": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _u32]),
    "infur_compare_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _u32]),
    "infur_frame_compare": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp, _u32, _u32, _vp, _vp, _vp,
                                        _u32, _vp, _u32p, _u32p]),
    "infur_frame_compare_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp, _u32, _u32, _vp, _vp,
                                            _vp, _u32, _vp, _u32p, _u32p]),
    "infur_adjacency": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _u32]),
    "infur_adjacency_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _u32]),
    "infur_sieve": (C.c_int32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "infur_sieve_dev": (C.c_int32, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "infur_frame_sieve": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                      _u32p, _u32p, _u32, _u32, _vp, _vp]),
    "infur_frame_sieve_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                          _u32p, _u32p, _u32, _u32, _vp, _vp]),
    "infur_shapes": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_shapes_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "infur_frame_shapes": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                       _u32p, _u32p, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "infur_frame_shapes_dev": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp,
                                           _u32p, _u32p, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "infur_raster": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "infur_raster_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "infur_raster_runs": (C.c_int32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "infur_raster_runs_dev": (C.c_int32, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "infur_stream_create": (C.c_int32, [_vp, _u32, C.POINTER(_vp)]),
    "infur_stream_destroy": (None, [_vp]),
    "infur_stream_add_lane": (C.c_int32, [_vp, _vp]),
    "infur_stream_submit": (C.c_int32, [_vp, _vp, _u32, _u32, _f, _u32, C.c_uint64]),
    "infur_stream_pending": (C.c_uint32, [_vp]),
    "infur_stream_next_dims": (C.c_int32, [_vp, C.POINTER(C.c_uint64), _u32p, _u32p]),
    "infur_stream_collect": (C.c_int32, [_vp, _vp, _sz, _vp, C.POINTER(C.c_uint64), _u32p, _u32p]),
    "infur_stream_acquire": (C.c_int32, [_vp, _u32, _u32, _f, C.POINTER(_vp)]),
    "infur_stream_commit": (C.c_int32, [_vp, _u32, _u32, _f, _u32, C.c_uint64]),
    "infur_stream_collect_view": (C.c_int32, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_uint64), _u32p, _u32p]),
    "infur_stream_release": (C.c_int32, [_vp]),
    "infur_stream_abandon": (C.c_int32, [_vp]),
    "infur_host_alloc": (C.c_int32, [_sz, C.POINTER(_vp)]),
    "infur_host_free": (C.c_int32, [_vp]),
    "infur_host_is_pinned": (C.c_uint32, [_vp]),
    "infur_batch_advance": (C.c_int32, [_vp, C.POINTER(_vp), _u32p, _u32p, _u32, _f, _u32, C.POINTER(_vp),
                                        C.POINTER(_sz), _u32p, _u32p]),
    "infur_group_create": (C.c_int32, [C.POINTER(_vp), _u32, C.POINTER(_vp)]),
    "infur_group_destroy": (None, [_vp]),
    "infur_group_last_error": (C.c_char_p, [_vp]),
    "infur_group_size": (C.c_uint32, [_vp]),
    "infur_group_uses_rccl": (C.c_uint32, [_vp]),
    "infur_group_worker_numa_node": (C.c_int32, [_vp, _u32]),
    "infur_group_weights_broadcast": (C.c_int32, [_vp, _u32]),
    "infur_group_batch_advance": (C.c_int32, [_vp, C.POINTER(_vp), _u32p, _u32p, _u32, _f, _u32, C.POINTER(_vp),
                                              C.POINTER(_sz), _u32p, _u32p]),
    "infur_weights_broadcast": (C.c_int32, [C.POINTER(_vp), _u32]),
    "infur_batch_advance_multi": (C.c_int32, [C.POINTER(_vp), _u32, C.POINTER(_vp), _u32p, _u32p, _u32, _f, _u32,
                                              C.POINTER(_vp), C.POINTER(_sz), _u32p, _u32p]),
    "infur_split_range": (C.c_int32, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _u32p]),
    "infur_hl_monitor_enable": (C.c_int32, [_vp, _u32]),
    "infur_hl_range": (C.c_int32, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _u32p, _u32p]),
    "infur_tune_export": (C.c_int32, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    "infur_tune_import": (C.c_int32, [_vp, C.c_char_p, _sz]),
    "infur_profile_enable": (C.c_int32, [_vp, _u32]),
    "infur_profile_count": (C.c_int32, [_vp, _u32p]),
    "infur_profile_get": (C.c_int32, [_vp, _u32, C.POINTER(KernelRecord)]),
    "infur_debug_profile_variant": (C.c_int32, [_vp, _u32, C.c_char_p, _sz]),
    "infur_dev_alloc": (C.c_int32, [_vp, _sz, C.POINTER(_vp)]),
    "infur_dev_free": (C.c_int32, [_vp, _vp]),
    "infur_memcpy_h2d": (C.c_int32, [_vp, _vp, _vp, _sz]),
    "infur_memcpy_d2h": (C.c_int32, [_vp, _vp, _vp, _sz]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP extension; raise (never fall back) when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C infur_amd/csrc). "
            "infur_amd has no CPU fallback."
        )
    # PyTorch wheels bundle their own HIP/HSA runtime (soname libamdhip64.so.7, same as
    # /opt/rocm's).  Two runtimes in one process cannot both own the GPU, so when torch is
    # installed it is imported FIRST: the loader then binds libinfur_hip.so's libamdhip64.so.7
    # dependency to the copy torch already mapped and the process has a single runtime
    # (needed for torch.distributed/RCCL next to our kernels).  The same holds for librccl.so.1,
    # which libinfur_hip.so links for infur_group_* (torch bundles its own copy under that soname).
    # Without torch the system libraries from the library's RUNPATH are used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.infur_abi_version() != ABI_VERSION:
        raise ImportError("libinfur_hip.so ABI version mismatch")
    _lib = lib
    return lib


def status_string(code: int) -> str:
    return load().infur_status_string(code).decode()
