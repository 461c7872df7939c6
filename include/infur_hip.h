/*
 * infur_hip.h -- C ABI of the MI355X-native InFur segmentation hot path.
 *
 * This is the drop-in boundary: exactly the calls the reference's three `Processor`
 * implementations on the per-frame path would bind over FFI (the Rust-side stubs are in
 * INTEGRATION.md).  Citations are path:line in the reference tree (ahirner/infur v0.2.0).
 *
 *   Scale      infur/src/processing.rs:179-282   -> infur_scale_validate / _out_dims / infur_scale
 *   Model<f32> infur/src/predict_onnx.rs:283-345 -> infur_model_load / _info / infur_model_advance
 *   ColorCode  infur/src/decode_predict.rs:41-84 -> infur_colorcode
 *   app graph  infur/src/app.rs:107-153          -> infur_frame_advance (scale->model->decode fused)
 *
 * Conventions
 *   - Plain pointers and sizes only; no C++ or torch types.  All functions return an
 *     int32_t status (0 = ok) and never throw or abort; infur_last_error(ctx) gives the
 *     detail string for the last failing call on that context.
 *   - One `infur_ctx` = one GPU + one HIP stream + its device arena.  A context is NOT
 *     thread-safe: use it from one thread at a time, as the reference's `&mut self`
 *     processors are (infur/src/main.rs:38-40).
 *   - The caller owns every buffer it passes; the context owns all device memory it
 *     allocates.  Functions ending in `_dev` take device pointers (resident data, no PCIe
 *     copy) and are asynchronous on the context's stream; the host-pointer forms copy in,
 *     run, copy out and return after the results are in the caller's buffers.
 *   - There is no CPU fallback: without a usable HIP device infur_ctx_create fails with
 *     INFUR_E_HIP.
 */
#ifndef INFUR_HIP_H
#define INFUR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INFUR_ABI_VERSION 7

/* status codes */
enum {
    INFUR_OK = 0,
    INFUR_E_INVALID_SCALE = 1,    /* ValidScaleError, processing.rs:161-163 (factor <= 0) */
    INFUR_E_ZERO_SIZE_IN = 2,     /* ScaleProcError::ZeroSizeIn, processing.rs:203-204 */
    INFUR_E_ZERO_SIZE_OUT = 3,    /* ScaleProcError::ZeroSizeOut, processing.rs:205-206 */
    INFUR_E_SHAPE = 4,            /* ModelProcError::ShapeError, predict_onnx.rs:35-36 */
    INFUR_E_MODEL_NOT_LOADED = 5, /* advance without a model where one is required */
    INFUR_E_MODEL_FORMAT = 6,     /* ModelCmdError / ModelInputFormatError, predict_onnx.rs:41-54 */
    INFUR_E_HIP = 7,              /* HIP runtime error (ModelProcError::RuntimeError analogue) */
    INFUR_E_RCCL = 8,             /* RCCL error in infur_group_* / infur_weights_broadcast */
    INFUR_E_INVALID_ARG = 9,
    INFUR_E_IO = 10,              /* model file could not be read */
    INFUR_E_CAPACITY = 11         /* caller's output buffer is too small */
};

/* Scale resampling mode */
enum {
    INFUR_SCALE_NEAREST = 0, /* the reference's fr::ResizeAlg::Nearest, processing.rs:189 */
    INFUR_SCALE_BILINEAR = 1 /* north-star extension (todo at processing.rs:224) */
};

/* arithmetic type of the conv stack */
enum {
    INFUR_DTYPE_F32 = 0, /* exact f32 MFMA (v_mfma_f32_32x32x2_f32): the parity mode */
    INFUR_DTYPE_F16 = 1, /* f16 activations/weights on v_mfma_f32_32x32x16_f16, f32 accumulation,
                            bias/residual/ReLU in f32, logits f32 (BASELINE configs[4]) */
    INFUR_DTYPE_F32_SPLIT = 2, /* f32 tensors everywhere; inside the conv GEMMs every operand value is
                            split into an f16 pair hi + lo (22 significand bits) and the product is
                            accumulated in f32 from three f16 MFMAs (lo*hi + hi*lo + hi*hi).  f32-grade
                            logits (tests: <= 2e-5 of the f32 oracle) at a multiple of the f32 MFMA rate */
    INFUR_DTYPE_F32_SPLIT_FP8 = 3, /* as INFUR_DTYPE_F32_SPLIT, but only hi*hi runs on the f16 MFMA; the two cross terms
                            hi*lo + lo*hi run on the bf8 (OCP e5m2) MX MFMA at twice the f16 rate: 2 MFMA units per
                            product instead of 3.  e5m2 has f16's exponent range, so no tensor-level scale is involved and
                            the error does not depend on the tensors' dynamic range: products exact to ~2^-13, logits
                            2-3e-4 (max-abs / max-abs) from the f32 oracle on the synthetic weights and 1.4e-4 max-abs /
                            1.0e-2 worst per-element on heavy-tailed weights with per-channel scales over three decades
                            (winograd_tile = 4: 1.1e-4 / 7e-3; tests/test_gpu_hostile.py) -- inside north_star's 1e-3 with
                            7x room, ~15x closer than INFUR_DTYPE_F16; a side mode, never the bench headline: at 1080p
                            it is only ~6 % faster than INFUR_DTYPE_F32_SPLIT, whose logits are 9x closer still.
                            (Round 3 used e4m3 under static scales: 7.1e-4 / 5.1e-2 on the same hostile set.) */
    /* (4 is not an option value: the integer arithmetic of a quantised model is selected by the model file) */
    INFUR_DTYPE_F16_HL = 5 /* round 5: THREE-BYTE tensors -- every activation and weight tensor is an f16 hi plane plus an e5m2
                            (OCP bf8) lo plane of (x - hi) * 2^11, written by the producing kernel's epilogue and staged by
                            LDS-DMA by its consumers (no register staging, no conversion): 3 bytes per element through HBM, L2 and
                            the CU's ingest path instead of the split modes' 4.  Products as INFUR_DTYPE_F32_SPLIT_FP8 (hi*hi
                            on the f16 MFMA, both cross terms on the bf8 MX MFMA: 2 units) with the hi bytes of the cross terms
                            taken by TRUNCATION from the f16 fragments (one v_perm per four values; the mean of the truncation
                            is folded into the lo planes).  ~14 significant bits per operand and per stored tensor: the mode
                            built to satisfy both halves of north_star's sentence (logits within 1e-3, f16-matrix-core rate).
                            Stride-1 3x3 convs with Cin >= 128 run in the Winograd domain as in the f32 modes. */
};

typedef struct infur_ctx infur_ctx;

typedef struct infur_options {
    uint32_t struct_size;  /* = sizeof(infur_options) */
    int32_t device;        /* HIP device ordinal */
    uint32_t compute_dtype; /* INFUR_DTYPE_* */
    uint32_t compute_aux;  /* 1: evaluate the aux head as the ONNX graph does (default 1) */
    uint32_t profile;      /* 1: bracket every kernel with HIP events (infur_profile_*) */
    uint32_t keep_activations; /* 1: debug -- every conv output keeps its own buffer */
    uint32_t winograd_min_cin; /* f32 stride-1 3x3 convs with Cin >= this run in the Winograd domain;
                                  0 = default (128), 0xFFFFFFFF = never */
    uint32_t winograd_tile;    /* output tile: 2 = F(2x2,3x3), 4 = F(4x4,3x3), 6 = F(6x6,3x3); 0 = default (6) */
    uint32_t no_autotune;      /* 0 (default): the first advance at a new frame size times the tile
                                  configurations of the conv kernel per layer shape and keeps the fastest
                                  (results are bit-identical across configurations); 1: fixed heuristic */
    uint32_t no_fuse_downsample; /* 0 (default): the first block of a stage runs conv3 and its downsample branch as one
                                  two-source GEMM (the branch tensor is never written); 1: two launches + residual */
    uint32_t no_fuse_stem_pool; /* 0 (default): the 7x7 stem convolution and the 3x3/2 max-pool run as one kernel (the stem
                                  tensor is never written); 1: two kernels.  Results are bit-identical. */
    uint32_t no_fuse_b2b;  /* 0 (default): in the f16 mode a bottleneck's conv3 + residual and the next bottleneck's conv1 run
                              as one launch where that measures faster (the widest tensor of the stage is written once and
                              not read back); 1: always two launches.  Results are bit-identical. */
    void* stream;          /* optional caller-owned hipStream_t; NULL = context creates one */
} infur_options;

/* ModelInfo, predict_onnx.rs:56-62 */
typedef struct infur_model_info {
    char input_name[32];    /* "input" */
    char input0_dtype[16];  /* "Float" | "Uint8": the model's declared image input (predict_onnx.rs:90,255) */
    char output_names[2][32]; /* "out", "aux" */
    uint32_t n_outputs;     /* 2, or 1 when the file has no aux head or options.compute_aux == 0 */
    uint32_t num_classes;
    uint32_t depth;         /* 50 | 101 */
    uint32_t n_convs;
    uint64_t weight_bytes;
    /* ABI 4 (appended; infur_model_info_get_sized copies only as many bytes as the caller's struct has): */
    uint32_t quantised;       /* 1: a QOperator / QDQ int8 model (INFURQ01): u8 activations x s8 weights on the i8 MFMA whatever
                                 options.compute_dtype says; 0: a float model run in options.compute_dtype */
    uint32_t resize_u8_heads; /* 1: the quantised file resizes the u8 logits BEFORE DequantizeLinear (onnxruntime's QOperator
                                 quantiser keeps Resize on the u8 tensor): infur_model_read_lowres returns the dequantised codes,
                                 the full-resolution outputs are interpolate -> truncate -> dequantise */
} infur_model_info;

/* one profiled kernel launch of the last advance */
typedef struct infur_kernel_record {
    char name[48];      /* layer name, e.g. "backbone.layer4.1.conv2" */
    char kernel[32];    /* kernel family, e.g. "conv_igemm_f32" */
    float ms;           /* HIP-event duration */
    double flops;       /* FLOPs this launch executes (2 x MAC); 0 for byte kernels */
    double bytes;       /* compulsory HBM bytes of this launch */
    double algo_flops;  /* direct-convolution FLOPs of the layer this launch completes (== flops except
                           for Winograd-domain GEMMs, where it is up to 5x larger; 0 for transforms) */
} infur_kernel_record;

/* ---- library ---- */
uint32_t infur_abi_version(void);
const char* infur_status_string(int32_t status);
/* number of visible HIP devices (0 when there is none); never fails */
int32_t infur_device_count(void);

/* ---- context ---- */
void infur_options_default(infur_options* opts);
int32_t infur_ctx_create(const infur_options* opts, infur_ctx** out);
void infur_ctx_destroy(infur_ctx* ctx);
const char* infur_last_error(const infur_ctx* ctx);
int32_t infur_ctx_synchronize(infur_ctx* ctx);
void* infur_ctx_stream(infur_ctx* ctx); /* the hipStream_t all work is enqueued on */

/* ---- Scale (processing.rs:142-282); host-only helpers need no context ---- */
/* ValidScale::try_from (processing.rs:158-168): INFUR_E_INVALID_SCALE iff factor <= 0 */
int32_t infur_scale_validate(float factor);
/* output dims and the ZeroSizeIn / ZeroSizeOut checks (processing.rs:238-256) */
int32_t infur_scale_out_dims(uint32_t w, uint32_t h, float factor, uint32_t* ow, uint32_t* oh);
/* replaces self.resizer.resize (processing.rs:278) and the unit-scale clone (:238-242).
 * bgr: packed B,G,R u8, h*w*3 bytes (image-ext/src/image_bgr.rs:7-11).  out: capacity bytes. */
int32_t infur_scale(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor,
                    uint32_t mode, uint8_t* out, size_t out_capacity, uint32_t* ow, uint32_t* oh);
int32_t infur_scale_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor,
                        uint32_t mode, void* d_out, size_t out_capacity, uint32_t* ow,
                        uint32_t* oh);

/* ---- Model (predict_onnx.rs:283-345) ---- */
/* ModelCmd::Load(path) (predict_onnx.rs:288-312): empty path unloads.  The file is an
 * INFURW01 weight blob (float FCN-ResNet50/101) or an INFURQ01 blob (the quantised form: u8 activations, s8 weights,
 * QLinearConv / QLinearAdd arithmetic; both layouts in infur_amd/weights.py), or an ONNX model: float (Conv), QOperator
 * (QLinearConv -- the shape of fcn-resnet50-12-int8.onnx, the file the reference's tests load, predict_onnx.rs:357-381) or
 * QDQ (DequantizeLinear -> Conv -> QuantizeLinear groups, fused as ONNX Runtime fuses them).  A quantised model runs on the
 * i8 MFMA whatever options.compute_dtype says; infur_model_info.quantised tells.  What the model is fed follows the
 * reference (predict_onnx.rs:103-139,296-301): a Float image input gets RGB planes normalised with
 * the torchvision constants; a Uint8 image input gets the frame's bytes themselves, BGR kept;
 * NCHW / NHWC is the file's own business (a Transpose in front of its stem). */
int32_t infur_model_load(infur_ctx* ctx, const char* path);
/* Host-only converter behind infur_model_load's .onnx support (no context, no GPU): parses an
 * ONNX ModelProto (FCN-ResNet50/101 as exported by torchvision, BN folded or not; float, or quantised in QOperator / QDQ
 * form) with the reference's input checks (predict_onnx.rs:223-265) and returns a malloc'ed INFURW01 (float) or INFURQ01
 * (quantised) blob;
 * release it with infur_buffer_free.  err (optional, errcap bytes) receives the message. */
int32_t infur_onnx_to_blob(const void* onnx, size_t len, void** blob, size_t* blob_len, char* err,
                           size_t errcap);
void infur_buffer_free(void* p);
int32_t infur_model_load_blob(infur_ctx* ctx, const void* blob, size_t len);
/* blob already resident on this context's device (e.g. after an RCCL broadcast) */
int32_t infur_model_load_blob_dev(infur_ctx* ctx, const void* d_blob, size_t len);
int32_t infur_model_unload(infur_ctx* ctx);
/* Model::get_info (predict_onnx.rs:341-345): INFUR_E_MODEL_NOT_LOADED when none */
int32_t infur_model_info_get(const infur_ctx* ctx, infur_model_info* info);
/* the same for a host compiled against an older (shorter) infur_model_info: at most info_size bytes are written, so the
 * struct can grow at its end without an overrun; info_size == 0 is INFUR_E_INVALID_ARG */
int32_t infur_model_info_get_sized(const infur_ctx* ctx, void* info, size_t info_size);
/* Model::advance (predict_onnx.rs:317-334): pre-proc (:97-140) + forward (:138) + batch
 * strip (:326-330).  out / aux: [num_classes, h, w] f32 planar, either may be NULL.
 * With no model loaded this is a no-op returning INFUR_OK (predict_onnx.rs:318,333) and
 * *n_outputs (optional) is set to 0; otherwise to infur_model_info.n_outputs (the length of the
 * reference's output Vec).  Passing `aux` for a one-output model is INFUR_E_INVALID_ARG, reported
 * before any work is done.
 * Limits: a single activation tensor must stay below 2 GiB (32-bit buffer offsets in the conv
 * kernel; INFUR_E_HIP otherwise) -- far above every BASELINE config (4K f32: 0.53 GiB). */
int32_t infur_model_advance(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h,
                            float* out, float* aux, uint32_t* n_outputs);
int32_t infur_model_advance_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h,
                                void* d_out, void* d_aux, uint32_t* n_outputs);
/* Optional: run one throw-away frame of w x h so that the first real advance at that size finds its activation
 * arena allocated and every conv shape's tile configuration measured (options.no_autotune == 0 times the
 * candidates on first use: a few hundred ms).  A GUI calls this when the scale slider settles
 * (processing.rs:220-226 marks the processor dirty at that moment).  INFUR_E_MODEL_NOT_LOADED without a model. */
int32_t infur_model_warmup(infur_ctx* ctx, uint32_t w, uint32_t h);
/* Optional (ABI 3, additive): replay the fused frame path (infur_frame_advance[_dev], the stream ring, the batch calls) as a
 * hipGraph.  A frame is 55-110 kernel launches; for SMALL frames in the fast modes (640x480 through the quantised model: 0.7 ms)
 * the host's enqueue time bounds the rate.  With replay enabled, a frame shape that has run unchanged for 6 frames (arena settled,
 * tile configurations measured) is captured from the same enqueue code -- one graph per (input pointer, output pointer, w, h,
 * factor, mode), at most 12 cached -- and launched as one graph from then on; any allocation, release, model or tuning change
 * drops the cached graphs.  Results are the eager path's bits.  Ignored (eager) while options.profile or
 * options.keep_activations is set.  infur_ctx_graph_stats: captures / replays so far, graphs cached now (any pointer may be NULL).
 * The context's stream (infur_ctx_stream) does NOT change when replay is enabled (ABI 5; ABI 3-4 replaced a library-owned stream by a
 * private one, which left hosts holding a stale handle): a library-owned stream is reserved for this context while it is the only
 * one using it; a stream that is already shared with another context of the device simply never captures (the frames run eagerly). */
int32_t infur_ctx_set_graph_replay(infur_ctx* ctx, uint32_t enable);
int32_t infur_ctx_graph_stats(const infur_ctx* ctx, uint64_t* captures, uint64_t* replays, uint32_t* cached);
/* output-stride-8 logits of the last advance, [num_classes, lh, lw] f32 planar (host) */
int32_t infur_model_lowres_dims(uint32_t h, uint32_t w, uint32_t* lh, uint32_t* lw);
int32_t infur_model_read_lowres(infur_ctx* ctx, float* out_low, float* aux_low, uint32_t* lh,
                                uint32_t* lw);
/* debug (needs keep_activations): output of conv #index of the last advance as
 * [C, H, W] f32 planar; cap_floats = capacity of host_chw */
int32_t infur_debug_read_activation(infur_ctx* ctx, uint32_t index, float* host_chw,
                                    size_t cap_floats, uint32_t* c, uint32_t* h, uint32_t* w);

/* pre-proc on its own (predict_onnx.rs:103-137): packed BGR u8 -> [3,h,w] f32, RGB planar,
 * ((v*1)/255 - mean) * (1/std): the ColorRange::Float32 arm.  The fused path folds this into the
 * stem convolution (for Uint8-input models: the identity table); it is exported so this stage can
 * be parity-checked (and used) in isolation. */
int32_t infur_pack_normalize(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h,
                             float* chw);
int32_t infur_pack_normalize_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h,
                                 void* d_chw);

/* ---- ColorCode (decode_predict.rs:32-79) ---- */
/* khw: [k, h, w] f32 planar confidences; rgba: h*w*4 bytes premultiplied [r,g,b,a] */
int32_t infur_colorcode(infur_ctx* ctx, const float* khw, uint32_t k, uint32_t h, uint32_t w,
                        uint8_t* rgba);
int32_t infur_colorcode_dev(infur_ctx* ctx, const void* d_khw, uint32_t k, uint32_t h,
                            uint32_t w, void* d_rgba);

/* ---- display conversion of the scaled frame (app.rs:132-144): packed BGR -> [r,g,b,255] ---- */
int32_t infur_bgr_to_rgba(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, uint8_t* rgba);
int32_t infur_bgr_to_rgba_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, void* d_rgba);

/* ---- fused per-frame path (app.rs:107-153): scale -> model -> decode(out[0]) ---- */
/* rgba: oh*ow*4 bytes.  scaled_bgr (optional): the scaled frame, oh*ow*3 bytes (the GUI
 * shows it, app.rs:132-144).  With no model loaded returns INFUR_E_MODEL_NOT_LOADED after
 * producing scaled_bgr (the reference clears the mask, app.rs:127-129). */
int32_t infur_frame_advance(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h,
                            float factor, uint32_t scale_mode, uint8_t* rgba,
                            size_t rgba_capacity, uint8_t* scaled_bgr, uint32_t* ow,
                            uint32_t* oh);
int32_t infur_frame_advance_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h,
                                float factor, uint32_t scale_mode, void* d_rgba,
                                size_t rgba_capacity, void* d_scaled_bgr, uint32_t* ow,
                                uint32_t* oh);

/* ---- Segments: the segmentation result itself, for a host without a display ----
 * ColorCode turns a pixel's K class values into one shaded colour for the GUI.  A headless host wants the argmax class
 * index, a usable confidence and per-class data to caption -- the two open items of the reference's own todo list,
 * README.md:76-77: "softmax if model predictions are logits (and/or clamp confidence shading)" and "class label captions".
 * Presence of this group is announced by infur_features() & INFUR_FEATURE_SEGMENTS (INFUR_ABI_VERSION does not move:
 * nothing existing changed).
 *
 * Per pixel, over the class values c_k in class order:
 *   INFUR_DECODE_RAW      the reference's loop, decode_predict.rs:67-78: k_max = 0, c_max = 0.0, strict '>';
 *                         conf = (c_max * 255.0) as u8 (saturating, truncating)
 *   INFUR_DECODE_SOFTMAX  the same loop from c_max = -inf (NaN never wins, the first maximum wins);
 *                         conf = (p * 255.0) as u8, p = 1 / sum_k exp(c_k - c_max) in f32 (NaN terms count 0);
 *                         nothing won: class 0, conf 0;  c_max = +inf: conf 255
 * Outputs, each optional (NULL = not wanted; all NULL is INFUR_E_INVALID_ARG):
 *   klass  h*w bytes, k_max (not wrapped: more than 256 classes is INFUR_E_INVALID_ARG)
 *   conf   h*w bytes
 *   stats  k * INFUR_STAT_WORDS uint64_t, class-major: pixel count, sum of x (column), sum of y (row), sum of the
 *          confidence bytes, bounding box.  A class without a pixel reads 0 everywhere except MIN_X = MIN_Y = UINT64_MAX.
 *          Integer sums: exact and repeatable.  The table needs no initialisation.
 *   rgba   h*w*4 bytes, the context's colour table at [k_max % 20][conf]: in RAW mode exactly infur_colorcode's bytes
 * h*w == 0 writes nothing; k == 0 writes zero planes, infur_colorcode's rgba, and leaves stats alone. */
enum { INFUR_DECODE_RAW = 0, INFUR_DECODE_SOFTMAX = 1 };
enum {
    INFUR_STAT_PIXELS = 0,
    INFUR_STAT_SUM_X = 1,
    INFUR_STAT_SUM_Y = 2,
    INFUR_STAT_SUM_CONF = 3,
    INFUR_STAT_MIN_X = 4,
    INFUR_STAT_MIN_Y = 5,
    INFUR_STAT_MAX_X = 6,
    INFUR_STAT_MAX_Y = 7,
    INFUR_STAT_WORDS = 8
};
enum { INFUR_FEATURE_SEGMENTS = 1 };
uint32_t infur_features(void); /* bit mask of additive capabilities of this build */
/* the 21 Pascal-VOC names torchvision's FCN heads are trained on (0 = "__background__", 15 = "person"); NULL for k >= 21 */
const char* infur_voc_class_name(uint32_t k);

/* ColorCode's sibling on given confidences.  khw: [k, h, w] f32 planar */
int32_t infur_segments(infur_ctx* ctx, const float* khw, uint32_t k, uint32_t h, uint32_t w, uint32_t decode,
                       uint8_t* klass, uint8_t* conf, uint64_t* stats, uint8_t* rgba);
int32_t infur_segments_dev(infur_ctx* ctx, const void* d_khw, uint32_t k, uint32_t h, uint32_t w, uint32_t decode,
                           void* d_klass, void* d_conf, void* d_stats, void* d_rgba);
/* The fused frame path (scale -> model -> decode(out[0])) with this decode instead of ColorCode, fused into the up-sampling
 * kernel like the first: the full-resolution logits are never materialised.  plane_capacity is that of klass and of conf,
 * stats_classes the number of classes the table has room for (model_info.num_classes are written); too small is
 * INFUR_E_CAPACITY.  With no model loaded the Scale stage still runs and the call returns INFUR_E_MODEL_NOT_LOADED.
 * infur_model_read_lowres works afterwards.  These calls always enqueue eagerly: they neither use nor disturb the graphs
 * infur_ctx_set_graph_replay has cached for infur_frame_advance_dev.  (The stream ring, batch and group calls produce RGBA
 * only.) */
int32_t infur_frame_segments(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor,
                             uint32_t scale_mode, uint32_t decode, uint8_t* klass, uint8_t* conf,
                             size_t plane_capacity, uint64_t* stats, uint32_t stats_classes, uint8_t* rgba,
                             size_t rgba_capacity, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_segments_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor,
                                 uint32_t scale_mode, uint32_t decode, void* d_klass, void* d_conf,
                                 size_t plane_capacity, void* d_stats, uint32_t stats_classes, void* d_rgba,
                                 size_t rgba_capacity, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Regions: the connected components of the class plane, one table row per object ----
 * Segments' statistics are per class: two people are one "person" row whose centroid lies between them.  Regions is the
 * third decode stage: per-object captions, counts, boxes and speckle removal.  Presence of this group is announced by
 * infur_features() & INFUR_FEATURE_REGIONS (INFUR_ABI_VERSION does not move).
 *
 * A region is a maximal set of pixels of equal class, connected under INFUR_CONNECT_4 or INFUR_CONNECT_8 (any other
 * connectivity, or an unknown flag bit, is INFUR_E_INVALID_ARG).
 *   flags & INFUR_REGIONS_SKIP_BACKGROUND   class-0 pixels form no region and are labelled INFUR_REGION_NONE
 *   min_pixels                              regions with fewer pixels are dropped, their pixels labelled INFUR_REGION_NONE
 *                                           (0 and 1 keep everything)
 * Kept regions are numbered densely from 0 in ascending order of their FIRST pixel (the smallest linear index y*w + x in
 * the region); the table is in that order.  Everything is an integer and nothing depends on the order in which the
 * device happened to work: two runs give identical bytes.
 * Outputs, each optional (NULL = not wanted; all NULL is INFUR_E_INVALID_ARG), none needs initialisation:
 *   labels     h*w uint32_t: the id of the pixel's region, or INFUR_REGION_NONE
 *   table      table_rows rows of INFUR_REGION_WORDS uint64_t: words 0-7 are the INFUR_STAT_* words restricted to the
 *              region (conf == NULL: SUM_CONF = 0), word INFUR_REGION_CLASS its class, word INFUR_REGION_FIRST its first
 *              pixel.  Only the first min(n, table_rows) rows are written; rows at or beyond n are left alone.
 *   n_regions  the number of kept regions, even when it exceeds table_rows (truncation is not an error; ids at or above
 *              table_rows are still written to the label plane)
 * h*w == 0 writes n_regions = 0 and nothing else; h*w >= 2^32 - 1 is INFUR_E_INVALID_ARG. */
#define INFUR_REGION_NONE 0xFFFFFFFFu
enum { INFUR_CONNECT_4 = 4, INFUR_CONNECT_8 = 8 };
enum { INFUR_REGIONS_SKIP_BACKGROUND = 1 };
enum { INFUR_REGION_CLASS = 8, INFUR_REGION_FIRST = 9, INFUR_REGION_WORDS = 10 };
enum { INFUR_FEATURE_REGIONS = 2 };

/* on given planes (klass: h*w class bytes; conf: h*w confidence bytes or NULL) */
int32_t infur_regions(infur_ctx* ctx, const uint8_t* klass, const uint8_t* conf, uint32_t h, uint32_t w,
                      uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint32_t* labels, uint64_t* table,
                      uint32_t table_rows, uint32_t* n_regions);
/* device pointers throughout, d_n_regions included (one device uint32_t); enqueued on the context's stream */
int32_t infur_regions_dev(infur_ctx* ctx, const void* d_klass, const void* d_conf, uint32_t h, uint32_t w,
                          uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_labels, void* d_table,
                          uint32_t table_rows, void* d_n_regions);
/* The fused frame path with both decode stages: scale -> model -> Segments decode(out[0]) -> Regions, in one call.  klass and
 * conf are optional outputs here (plane_capacity bytes each; the library decodes into scratch of its own otherwise);
 * labels_capacity is in bytes (ow*oh*4 needed).  Too little capacity is INFUR_E_CAPACITY.  With no model loaded the Scale
 * stage still runs and the call returns INFUR_E_MODEL_NOT_LOADED.  Like infur_frame_segments these calls always enqueue
 * eagerly and leave the graphs cached for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce
 * RGBA only.) */
int32_t infur_frame_regions(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor,
                            uint32_t scale_mode, uint32_t decode, uint32_t connectivity, uint32_t min_pixels,
                            uint32_t flags, uint8_t* klass, uint8_t* conf, size_t plane_capacity, uint32_t* labels,
                            size_t labels_capacity, uint64_t* table, uint32_t table_rows, uint32_t* n_regions,
                            uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_regions_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor,
                                uint32_t scale_mode, uint32_t decode, uint32_t connectivity, uint32_t min_pixels,
                                uint32_t flags, void* d_klass, void* d_conf, size_t plane_capacity, void* d_labels,
                                size_t labels_capacity, void* d_table, uint32_t table_rows, void* d_n_regions,
                                void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Tracks: region identities carried from frame to frame ----
 * Regions is stateless: ids are the raster order of each region's first pixel, so the same object is row 3 in one frame and
 * row 5 in the next.  Tracks is the fourth decode stage: a TRACKER remembers the last frame it saw (its label plane and, per
 * region, class, track id, age, birth frame and the PIXELS / SUM_X / SUM_Y words) and gives every region of the next frame
 * either the id of the remembered region it overlaps most, or a new one.  Presence of this group is announced by
 * infur_features() & INFUR_FEATURE_TRACKS (INFUR_ABI_VERSION does not move).  Integers throughout: identical bytes from run
 * to run and from device to device.
 *
 * A tracker is bound to one context and is used, like it, from one thread at a time.  Its handle is an untyped pointer
 * (void*) in this header.  Destroying the context first leaves the tracker an empty handle (every call on it returns
 * INFUR_E_INVALID_ARG) that must still be passed to infur_tracker_destroy.
 *
 * One step takes the Regions outputs of the current h x w frame: labels, table (table_rows rows) and n_regions.
 *   tracked     current regions with id < T = min(n_regions, table_rows, max_regions); every other region gets
 *               INFUR_TRACK_NONE and the status bit INFUR_TRACKS_TRUNCATED is set
 *   overlap     overlap(c, p) = the number of pixels whose current label c and remembered label p are both tracked (p in
 *               the remembered frame's sense); (c, p) is a candidate iff the two regions have the same class and
 *               overlap >= max(min_overlap, 1)
 *   match       1. each c chooses the candidate p of largest overlap (ties: the smaller p);  2. each p is kept by the chooser
 *               c of largest overlap (ties: the smaller c);  3. a kept c inherits p's track id and birth frame, AGE =
 *               age(p) + 1;  4. every other tracked c starts a new track, AGE = 1.  A loser of step 2 does not fall back to a
 *               second choice: a split keeps the id on the larger part, a merge the id of the larger contributor
 *   new ids     next_id + rank, rank counting the new tracks in ascending region id; next_id then advances by their number.
 *               If next_id + new > 0xFFFFFFFE the step sets INFUR_TRACKS_IDS_EXHAUSTED, gives INFUR_TRACK_NONE to every
 *               region (rows as for untracked regions; CONTINUED = NEW = 0), leaves next_id alone and forgets the frame
 *   resets      on the first frame, after infur_tracker_reset, after an exhausted step, or when h or w differs from the
 *               remembered frame, every tracked region is new (and ENDED = 0).  Ids keep counting; the frame counter counts
 *               every step since the tracker was created.  Memory beyond one frame is opt-in: "Tracks: memory" below
 *   overflow    the pair table has pair_slots slots.  R = the number of runs of equal tracked (c, p) along rows, rows cut
 *               every 64 columns: a function of the two planes alone that bounds the number of distinct pairs.  If
 *               2 R > pair_slots the step sets INFUR_TRACKS_OVERFLOW and every tracked region is new; it still remembers
 *               its frame, so the next step tracks normally
 * Outputs, each optional (NULL = not wanted; all NULL is INFUR_E_INVALID_ARG), none needs initialisation:
 *   track_of_region  table_rows uint32_t; rows at or beyond min(n_regions, table_rows) are left alone
 *   track_plane      h*w uint32_t: each pixel's label mapped through track_of_region (untracked and INFUR_REGION_NONE:
 *                    INFUR_TRACK_NONE)
 *   track_table      table_rows rows of INFUR_TRACK_WORDS uint64_t, the same rows left alone: ID, AGE (frames this track has
 *                    been seen), BORN (the frame counter when it began), PREV_REGION (its region id in the remembered frame,
 *                    or INFUR_REGION_NONE), OVERLAP with that region, and that region's PIXELS, SUM_X, SUM_Y (0 for a new
 *                    track): a centroid step is one subtraction on the host.  An untracked region reads ID =
 *                    INFUR_TRACK_NONE, PREV_REGION = INFUR_REGION_NONE and 0 elsewhere
 *   summary          four uint32_t: STATUS (INFUR_TRACKS_* bits), CONTINUED, NEW, ENDED (remembered tracked regions that
 *                    no current region inherits)
 * h*w == 0 writes the summary (all zero) and forgets the frame.  A null or orphaned tracker, a null labels / table /
 * n_regions input on a non-empty frame and h*w >= 2^32 - 1 are INFUR_E_INVALID_ARG with no output touched. */
#define INFUR_TRACK_NONE 0xFFFFFFFFu
enum {
    INFUR_TRACK_ID = 0,
    INFUR_TRACK_AGE = 1,
    INFUR_TRACK_BORN = 2,
    INFUR_TRACK_PREV_REGION = 3,
    INFUR_TRACK_OVERLAP = 4,
    INFUR_TRACK_PREV_PIXELS = 5,
    INFUR_TRACK_PREV_SUM_X = 6,
    INFUR_TRACK_PREV_SUM_Y = 7,
    INFUR_TRACK_WORDS = 8
};
enum { INFUR_TRACKS_TRUNCATED = 1, INFUR_TRACKS_OVERFLOW = 2, INFUR_TRACKS_IDS_EXHAUSTED = 4 };
enum {
    INFUR_TRACKS_SUMMARY_STATUS = 0,
    INFUR_TRACKS_SUMMARY_CONTINUED = 1,
    INFUR_TRACKS_SUMMARY_NEW = 2,
    INFUR_TRACKS_SUMMARY_ENDED = 3,
    INFUR_TRACKS_SUMMARY_WORDS = 4
};
enum { INFUR_FEATURE_TRACKS = 4 };

/* max_regions: 0 = 65536 (at most 2^24); pair_slots: 0 = 1 << 20, else a power of two >= 64 (at most 2^28).  The tracker owns
 * its device memory: 12 bytes per slot, 68 per region and the remembered plane (h*w*4 bytes, grown on demand).  None of it
 * is visible to the graphs infur_ctx_set_graph_replay caches. */
int32_t infur_tracker_create(infur_ctx* ctx, uint32_t max_regions, uint32_t pair_slots, void** tracker);
void infur_tracker_destroy(void* tracker);
/* stream-ordered: forget the remembered frame, next_id = first_id (a new tracker starts at 0) */
int32_t infur_tracker_reset(void* tracker, uint32_t first_id);
/* one step, host pointers (labels: h*w; table: table_rows rows of INFUR_REGION_WORDS, of which min(n_regions, table_rows)
 * are read) */
int32_t infur_tracks(void* tracker, const uint32_t* labels, const uint64_t* table, uint32_t table_rows, uint32_t n_regions,
                     uint32_t h, uint32_t w, uint32_t min_overlap, uint32_t* track_of_region, uint32_t* track_plane,
                     uint64_t* track_table, uint32_t* summary);
/* device pointers throughout, d_n_regions included (one device uint32_t, read on the device: no host synchronisation);
 * enqueued on the context's stream */
int32_t infur_tracks_dev(void* tracker, const void* d_labels, const void* d_table, uint32_t table_rows,
                         const void* d_n_regions, uint32_t h, uint32_t w, uint32_t min_overlap, void* d_track_of_region,
                         void* d_track_plane, void* d_track_table, void* d_summary);
/* The fused frame path with all three decode stages: scale -> model -> Segments decode -> Regions -> Tracks in one call:
 * infur_frame_regions' arguments, then the tracker (of this context), min_overlap and the four outputs.  labels, table and
 * n_regions are optional outputs here (the tracker keeps buffers of its own otherwise); table_rows is the row count of the
 * region table and of the track outputs either way.  Like infur_frame_regions these calls always enqueue eagerly and leave
 * the graphs cached for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_tracks(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                           uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass,
                           uint8_t* conf, size_t plane_capacity, uint32_t* labels, size_t labels_capacity, uint64_t* table,
                           uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh,
                           void* tracker, uint32_t min_overlap, uint32_t* track_of_region, uint32_t* track_plane,
                           uint64_t* track_table, uint32_t* summary);
int32_t infur_frame_tracks_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                               uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass,
                               void* d_conf, size_t plane_capacity, void* d_labels, size_t labels_capacity, void* d_table,
                               uint32_t table_rows, void* d_n_regions, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh,
                               void* tracker, uint32_t min_overlap, void* d_track_of_region, void* d_track_plane,
                               void* d_track_table, void* d_summary);

/* ---- Tracks: memory -- lost tracks are kept for a few frames, so a flicker keeps its id ----
 * A per-frame argmax flickers: a region drops below min_pixels, changes class or merges with a neighbour for one frame, and the
 * same object returns with a new id, AGE = 1 and a new BORN.  Memory is an opt-in GALLERY of lost tracks on the device: a track
 * whose region vanished stays in it for up to max_lost steps, and a region that would start a new track takes a lost track of
 * its class back when it appears where that track was last seen.  Presence of this group is announced by infur_features() &
 * INFUR_FEATURE_TRACK_MEMORY (INFUR_ABI_VERSION does not move).  A tracker without memory does exactly what is described above.
 * Integers throughout, a function of the sequence of planes alone.
 *
 * infur_tracker_set_memory(tracker, max_lost, reach, gallery_rows): max_lost == 0 turns memory off and frees its device memory
 * (the other two arguments are ignored); gallery_rows: 0 = 4096, at most 65536 (more is INFUR_E_INVALID_ARG).  The call
 * synchronises the context's stream before it frees or replaces memory, and forgets the remembered frame and the gallery as a
 * reset does; next_id and the frame counter keep counting.  A failed allocation is INFUR_E_HIP and leaves the tracker as it was.
 * (So does every other error of this call.)
 *
 * The gallery is an ordered list of at most gallery_rows entries of INFUR_LOST_WORDS words: ID, AGE, BORN, CLASS, PIXELS, SUM_X,
 * SUM_Y, MIN_X, MIN_Y, MAX_X, MAX_Y of the track's last region, and SEEN, the value of the frame counter at the last step in
 * which the track had a region.  A step at frame counter f (the value BORN uses) on a tracker with memory:
 *   1 forget      a step that starts afresh (first frame, after infur_tracker_reset, after set_memory, after an exhausted
 *                 step, another h x w) empties the gallery first.  An empty frame (h*w == 0) empties it too; its memory
 *                 summary is all zero
 *   2 expire      gap(e) = f - SEEN(e) - 1 is the number of steps in which the track had no region; entries with
 *                 gap > max_lost are removed, EXPIRED counts them
 *   3 match       exactly the match above: overlap table, choose, keep.  ORPHANS are the tracked regions c < T that no
 *                 remembered region kept (those that start new tracks without memory)
 *   4 candidates  (c, e) is a candidate iff c is an orphan, CLASS(c) == CLASS(e) and box(c) intersects
 *                 grow(box(e), reach * gap(e)); grow moves each side outwards by that many pixels and clamps to
 *                 [0, w-1] x [0, h-1]; the product is taken in 64 bits and clamped, so no reach can wrap.
 *                 score = (x1 - x0 + 1)(y1 - y0 + 1) of the intersection (at most h*w)
 *   5 revive      two-sided and greedy, with Tracks' own rule: every orphan chooses its candidate of largest score (ties:
 *                 the smaller gallery index); every entry is kept by its chooser of largest score (ties: the smaller c); a
 *                 loser does not fall back.  A kept orphan c is REVIVED: ID and BORN from e, AGE = AGE(e) + 1; its
 *                 track-table row has PREV_REGION = INFUR_REGION_NONE, OVERLAP = 0 and PREV_PIXELS / PREV_SUM_X /
 *                 PREV_SUM_Y from e, so a centroid step is still one subtraction.  gap_of_region[c] = gap(e) for a revived c
 *                 and 0 for every other region
 *   6 new ids     next_id + rank over the orphans that were not revived, in ascending region id.  next_id + new >
 *                 0xFFFFFFFE is INFUR_TRACKS_IDS_EXHAUSTED as above; in addition the gallery is emptied and the memory
 *                 summary is all zero.  (A step that would exhaust the ids without memory may therefore pass with it.)
 *   7 summary     CONTINUED and ENDED mean what they mean above; NEW counts only the tracks that got a new id, so
 *                 CONTINUED + NEW + REVIVED = T on a step that is not exhausted
 *   8 gallery     the revived entries leave the gallery.  The remembered regions that no current region inherited (the ones
 *                 ENDED counts) are appended in ascending region id with SEEN = f - 1 -- none on a step that started afresh;
 *                 LOST counts them.  If the list is now longer than gallery_rows, entries are dropped from the front (the
 *                 longest lost) and the status bit INFUR_TRACKS_GALLERY_FULL is set.  HELD is the length afterwards.  An
 *                 OVERFLOW step is not special: all its tracked regions are orphans, all remembered regions end.
 *                 The bit is reported in the step's summary only: a caller that passes no summary does not see it (in the
 *                 memory summary HELD == gallery_rows says that the gallery is full, not whether entries were dropped)
 * The gallery's order is a function of the history: survivors in their old order, then the newly ended regions in ascending
 * region id.  infur_tracker_reset empties the gallery.  Memory costs 2 * 60 + 8 bytes per gallery row and 28 per region. */
enum { INFUR_FEATURE_TRACK_MEMORY = 128 };
enum { INFUR_TRACKS_GALLERY_FULL = 8 };
enum {
    INFUR_LOST_ID = 0,
    INFUR_LOST_AGE = 1,
    INFUR_LOST_BORN = 2,
    INFUR_LOST_CLASS = 3,
    INFUR_LOST_PIXELS = 4,
    INFUR_LOST_SUM_X = 5,
    INFUR_LOST_SUM_Y = 6,
    INFUR_LOST_MIN_X = 7,
    INFUR_LOST_MIN_Y = 8,
    INFUR_LOST_MAX_X = 9,
    INFUR_LOST_MAX_Y = 10,
    INFUR_LOST_SEEN = 11,
    INFUR_LOST_WORDS = 12
};
enum {
    INFUR_TRACK_MEMORY_REVIVED = 0,
    INFUR_TRACK_MEMORY_LOST = 1,
    INFUR_TRACK_MEMORY_EXPIRED = 2,
    INFUR_TRACK_MEMORY_HELD = 3,
    INFUR_TRACK_MEMORY_WORDS = 4
};
int32_t infur_tracker_set_memory(void* tracker, uint32_t max_lost, uint32_t reach, uint32_t gallery_rows);
/* What the last step left.  Each output is optional (all NULL is INFUR_E_INVALID_ARG), none needs initialisation:
 *   gap_of_region   exactly `rows` uint32_t are written; a word at or beyond the last step's T is 0
 *   memory_summary  INFUR_TRACK_MEMORY_WORDS uint32_t: REVIVED, LOST, EXPIRED, HELD
 *   lost_table      the first min(HELD, lost_rows) gallery entries in gallery order, INFUR_LOST_WORDS uint64_t each; rows
 *                   beyond that are left alone
 * On a tracker without memory, or a null or orphaned tracker, both calls are INFUR_E_INVALID_ARG with no output touched. */
int32_t infur_tracker_memory(void* tracker, uint32_t* gap_of_region, uint32_t rows, uint32_t* memory_summary,
                             uint64_t* lost_table, uint32_t lost_rows);
/* device pointers; stream-ordered, no synchronisation */
int32_t infur_tracker_memory_dev(void* tracker, void* d_gap_of_region, uint32_t rows, void* d_memory_summary,
                                 void* d_lost_table, uint32_t lost_rows);

/* ---- Runs: a class, label or track plane as run-length records ----
 * The four decode stages end in dense planes: at 1080p a 2 MB class plane, an 8 MB label plane, an 8 MB track plane.  A
 * segmentation plane is spatially coherent, so run-length encoded (12 bytes per run) it is a fraction of that -- and RLE is
 * the form in which masks are exchanged, stored and drawn.  Runs encodes any byte or u32 plane on the device, and a host copies out only
 * as many records as there are.  Presence of this group is announced by infur_features() & INFUR_FEATURE_RUNS
 * (INFUR_ABI_VERSION does not move).
 *
 * The input is a plane of h x w elements of elem_bytes = 1 (a class or confidence plane) or 4 (a label or track plane); any
 * other elem_bytes is INFUR_E_INVALID_ARG.  A RUN is a maximal sequence of equal values within one row: a run never continues
 * into the next row, so that a per-row index can exist.  Runs are numbered from 0 in raster order of their first pixel.
 *   flags & INFUR_RUNS_SKIP   runs whose value equals skip_value are neither emitted nor counted (typically class 0,
 *                             INFUR_REGION_NONE, INFUR_TRACK_NONE).  An unknown flag bit, or skip_value > 255 with 1-byte
 *                             elements, is INFUR_E_INVALID_ARG
 * Outputs, each optional (NULL = not wanted, and so is runs with runs_rows == 0; nothing wanted is INFUR_E_INVALID_ARG), none
 * needs initialisation:
 *   runs       runs_rows records of INFUR_RUN_WORDS uint32_t: INFUR_RUN_START the linear index y*w + x of the run's first
 *              pixel, INFUR_RUN_END one past its last pixel (the length is END - START, the row START / w), INFUR_RUN_VALUE
 *              the value, zero-extended.  Only the first min(n, runs_rows) records are written; records at or beyond that are
 *              left alone
 *   row_start  h + 1 uint32_t: row_start[y] is the number of emitted runs that start before row y, whatever runs_rows is;
 *              row_start[h] = n
 *   n_runs     the number of emitted runs n, even when it exceeds runs_rows (truncation is not an error)
 * h*w == 0 writes n_runs = 0 and row_start[0..h] = 0, and nothing else; h*w >= 2^32 - 1 and a NULL plane with h*w > 0 are
 * INFUR_E_INVALID_ARG.  No output is touched when a call is rejected.  Everything is an integer and a function of the plane
 * alone: identical bytes from run to run. */
enum { INFUR_RUNS_SKIP = 1 };
enum { INFUR_RUN_START = 0, INFUR_RUN_END = 1, INFUR_RUN_VALUE = 2, INFUR_RUN_WORDS = 3 };
enum { INFUR_FEATURE_RUNS = 8 };

/* on a given plane, host pointers: the count is read first and only min(n, runs_rows) records are copied back */
int32_t infur_runs(infur_ctx* ctx, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                   uint32_t skip_value, uint32_t* runs, uint32_t runs_rows, uint32_t* row_start, uint32_t* n_runs);
/* device pointers throughout, d_n_runs included (one device uint32_t); enqueued on the context's stream, never synchronises,
 * capturable after one call outside the capture (which allocates the scratch: one word per 1024 pixels, owned by the context;
 * it grows only with a plane of more than 16 Mi pixels that is larger than any before, and a graph captured around the call
 * is re-captured after that).  This is the call that
 * composes on the device: infur_frame_regions_dev or infur_frame_tracks_dev, then infur_runs_dev on the label or track plane
 * they left in device memory, gives per-object runs with no dense plane crossing PCIe. */
int32_t infur_runs_dev(infur_ctx* ctx, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                       uint32_t skip_value, void* d_runs, uint32_t runs_rows, void* d_row_start, void* d_n_runs);
/* The fused frame path with the class plane run-length encoded: scale -> model -> Segments decode(out[0]) -> Runs of the class
 * plane, in one call.  The class plane is decoded into scratch of the library's own.  row_start_rows counts the words of
 * row_start: fewer than oh + 1 is INFUR_E_CAPACITY (checked, like the other capacities, once a model is loaded).  stats is Segments' per-class table, optional, so that captions come with
 * the mask; stats_capacity is the number of classes it has room for, as infur_frame_segments' stats_classes.  At least one of
 * runs, row_start and n_runs must be given.  The calls inherit infur_frame_segments' checks and errors: with no model loaded
 * the Scale stage still runs and the call returns INFUR_E_MODEL_NOT_LOADED.  They always enqueue eagerly and leave the graphs
 * cached for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_runs(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                         uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t* runs, uint32_t runs_rows,
                         uint32_t* row_start, uint32_t row_start_rows, uint32_t* n_runs, uint64_t* stats,
                         uint32_t stats_capacity, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_runs_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                             uint32_t decode, uint32_t flags, uint32_t skip_value, void* d_runs, uint32_t runs_rows,
                             void* d_row_start, uint32_t row_start_rows, void* d_n_runs, void* d_stats,
                             uint32_t stats_capacity, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Outlines: the boundaries of a class, label or track plane as closed polygon loops ----
 * Runs gives a mask as records to fill; a polygon is what GeoJSON and COCO `segmentation` hold, what a GUI strokes as a vector
 * outline, what a simplifier, a hit test or a tracker gate takes.  Outlines turns the boundary of every value-region of a byte
 * or u32 plane into closed loops of lattice vertices on the device, in a deterministic order.  Presence of this group is
 * announced by infur_features() & INFUR_FEATURE_OUTLINES (INFUR_ABI_VERSION does not move).
 *
 * INPUT.  A plane of h x w elements of elem_bytes = 1 or 4.  Runs' rules hold for elem_bytes, for a NULL plane, for unknown flag
 * bits and for skip_value > 255 on bytes (each INFUR_E_INVALID_ARG).  In addition 4*h*w must be below 2^32 - 1, otherwise the
 * call returns INFUR_E_INVALID_ARG.
 * FLAGS.
 *   INFUR_OUTLINES_SKIP   pixels whose value equals skip_value belong to no region: they own no edges, and a kept pixel beside
 *                         one has a boundary there
 *   INFUR_OUTLINES_CONN8  the saddle rule below.  Callers pass the connectivity they gave Regions
 * LATTICE.  Vertices are (X, Y) with 0 <= X <= w and 0 <= Y <= h; the vertex id is Y*(w+1) + X.
 * EDGES.  Pixel p = (x, y) has the linear index i = y*w + x and the sides N=0, E=1, S=2, W=3.  Side s of a kept pixel is a
 * boundary EDGE when the neighbour across it is outside the plane, is skipped, or has a different value; the edge id is 4*i + s.
 * Edges are directed with their pixel on the right hand (clockwise on a y-down screen):
 *   N goes (x,y) -> (x+1,y), heading east         E goes (x+1,y) -> (x+1,y+1), heading south
 *   S goes (x+1,y+1) -> (x,y+1), heading west     W goes (x,y+1) -> (x,y), heading north
 * so the side index is also the heading d.
 * SUCCESSOR.  Take an edge of pixel p with value v and heading d that ends at vertex V = (X, Y).  R is the right-ahead pixel and
 * L the left-ahead pixel:
 *   d      R            L
 *   east   (X, Y)       (X, Y-1)
 *   south  (X-1, Y)     (X, Y)
 *   west   (X-1, Y-1)   (X-1, Y)
 *   north  (X, Y-1)     (X-1, Y-1)
 * A pixel "is v" when it is inside the plane, kept, and equal to v.  The successor is:
 *   R and L are both v          turn left: edge (L, side (d+3)%4)
 *   only R is v                 go straight: edge (R, side d)
 *   only L is v (the saddle)    under CONN8 turn left: edge (L, (d+3)%4); otherwise turn right: edge (p, (d+1)%4)
 *   neither is v                turn right: edge (p, (d+1)%4)
 * Every edge has exactly one successor and one predecessor (the predecessor rule is the mirror image and as local: the 2 x 2
 * pixels around the edge's tail), so the edges fall into disjoint cycles.  Each cycle is a LOOP.
 * CORNER EDGES AND LOOP ORDER.  An edge is a CORNER EDGE when its heading differs from its predecessor's; its tail vertex is a
 * polygon vertex.  A loop's START is its corner edge with the smallest edge id.  Loops are numbered from 0 in ascending order of
 * their start edge id.  A loop's vertices are the tail vertices of its corner edges, in succession order beginning at the start.
 * Collinear lattice points are never emitted: a rectangle is 4 vertices whatever its size.
 * OUTPUTS, each optional (NULL = not wanted, and so are loops with loops_rows == 0 and vertices with vertex_rows == 0; nothing
 * wanted is INFUR_E_INVALID_ARG), none needs initialisation; a rejected call touches no output:
 *   loops     loops_rows records of INFUR_LOOP_WORDS uint32_t: INFUR_LOOP_OFFSET the index of the loop's first vertex in
 *             `vertices` (a full exclusive prefix sum: it does not depend on any truncation), INFUR_LOOP_COUNT its number of
 *             vertices, INFUR_LOOP_VALUE the region's value, zero-extended, INFUR_LOOP_START the start edge id.  Only the first
 *             min(n_loops, loops_rows) records are written
 *   vertices  vertex_rows uint32_t vertex ids, loops back to back.  Positions at or beyond min(n_vertices, vertex_rows) are
 *             left alone
 *   counts    3 uint32_t {n_loops, n_vertices, n_edges}: the full counts whatever the rows are
 * EDGE CAPACITY.  The stage needs scratch per boundary edge, and a noise plane has up to 4*h*w of them.  max_edges = 0 means
 * 4*h*w, the worst case, so that no plane is ever refused for its content (a larger value is taken as 4*h*w).  When n_edges >
 * max_edges, counts is written as {0, 0, n_edges} and no other output is touched: overflow is visible and is not an error, the
 * sibling of Runs' truncation rule.  h*w == 0 writes counts = {0, 0, 0} and nothing else.
 * FACTS THAT FOLLOW.  Every loop has an even number of vertices, at least 4.  START & 3 is 0 (N) for an outer boundary and 2 (S)
 * for the boundary of a hole.  The shoelace sum of (x[i]*y[i+1] - x[i+1]*y[i]) is positive exactly for the outer loops, and over
 * all loops it is twice the number of kept pixels.  For an outer loop of a Regions label plane START >> 2 is the region's
 * INFUR_REGION_FIRST (a region that 4-connectivity holds together only around a hole's diagonal has further outer loops, with
 * larger starts).  Everything is an integer and a function of the plane alone: identical bytes from run to run. */
enum { INFUR_OUTLINES_SKIP = 1, INFUR_OUTLINES_CONN8 = 2 };
enum { INFUR_LOOP_OFFSET = 0, INFUR_LOOP_COUNT = 1, INFUR_LOOP_VALUE = 2, INFUR_LOOP_START = 3, INFUR_LOOP_WORDS = 4 };
enum { INFUR_FEATURE_OUTLINES = 16 };

/* on a given plane, host pointers: the counts are read first, then min(n_loops, loops_rows) records and min(n_vertices,
 * vertex_rows) vertices are copied back */
int32_t infur_outlines(infur_ctx* ctx, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                       uint32_t skip_value, uint32_t max_edges, uint32_t* loops, uint32_t loops_rows, uint32_t* vertices,
                       uint32_t vertex_rows, uint32_t* counts);
/* device pointers throughout, d_counts included (three device uint32_t); enqueued on the context's stream in 9 + ceil(log2(edge
 * capacity)) launches, a number fixed by the arguments: the call never synchronises.  Capturable after one call outside the
 * capture, which allocates the scratch: 36 bytes per edge of capacity, 4 bytes per pixel and the scan's sums, owned by the
 * context.  It grows only with a request larger than any before, and a graph captured around the call is re-captured after
 * that.  This is the call that composes on the device: infur_frame_regions_dev (or infur_frame_tracks_dev), then
 * infur_outlines_dev on the label (track) plane they left in device memory with INFUR_OUTLINES_SKIP, skip_value =
 * INFUR_REGION_NONE (INFUR_TRACK_NONE) and the same connectivity gives per-object polygons with no dense plane crossing PCIe. */
int32_t infur_outlines_dev(infur_ctx* ctx, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                           uint32_t skip_value, uint32_t max_edges, void* d_loops, uint32_t loops_rows, void* d_vertices,
                           uint32_t vertex_rows, void* d_counts);
/* The fused frame path with the class plane outlined: scale -> model -> Segments decode(out[0]) -> Outlines of the class plane,
 * in one call.  The class plane is decoded into scratch of the library's own.  stats is Segments' per-class table, optional;
 * stats_capacity is the number of classes it has room for, as infur_frame_segments' stats_classes.  At least one of loops,
 * vertices and counts must be given (checked once a model is loaded).  The calls inherit infur_frame_segments' checks and
 * errors: with no model loaded the Scale stage still runs and the call returns INFUR_E_MODEL_NOT_LOADED.  They always enqueue
 * eagerly and leave the graphs cached for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA
 * only.) */
int32_t infur_frame_outlines(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                             uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, uint32_t* loops,
                             uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows, uint32_t* counts, uint64_t* stats,
                             uint32_t stats_capacity, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_outlines_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                                 uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, void* d_loops,
                                 uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows, void* d_counts, void* d_stats,
                                 uint32_t stats_capacity, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Simplify: Outlines' loops with a tolerance (Douglas-Peucker) ----
 * On a pixel lattice the boundary of a slanted region is a staircase: every step costs two vertices.  COCO `segmentation`, GeoJSON
 * and a GUI that strokes an outline want the polygon within a tolerance, not the staircase.  Simplify takes what Outlines left in
 * device memory and keeps, loop by loop, the vertices the Douglas-Peucker rule keeps, in the same three-array layout.  Presence of
 * this group is announced by infur_features() & INFUR_FEATURE_SIMPLIFY (INFUR_ABI_VERSION does not move).
 *
 * INPUT.  Outlines' three outputs for a plane of width w: `loops` (records OFFSET, COUNT, VALUE, START), `vertices` (ids
 * Y*(w+1) + X) and `counts` ({n_loops, n_vertices, ..}: the first two words are read), with loops_rows_in and vertex_rows_in, the
 * rows the caller declares for the two arrays, and tol16, the tolerance in 1/16 pixel (the outer corners of a 45-degree staircase
 * are 0.707 pixel off their chord: the interesting range lies between 8 and 16).  w must be in 1 .. 8191, h at most 8191 and
 * tol16 at most 65535, otherwise the call returns INFUR_E_INVALID_ARG.  Then every coordinate difference is below 2^13 and every
 * quantity below fits 64 bits: 256 * cross^2 < 2^62 and tol16^2 * L < 2^59.  (A vertex id whose Y exceeds 8191 -- no plane the
 * call accepts has one -- is read as Y = 8191.)  A NULL counts, or a NULL array with rows declared, is INFUR_E_INVALID_ARG.
 * THE RULE FOR ONE LOOP with vertices v_0 .. v_{n-1}; set v_n := v_0.
 *   1 ANCHORS.  Vertex 0 is kept.  B is the index in 1 .. n-1 that maximises |v_i - v_0|^2, on ties the smallest; B is kept.
 *   2 SPLIT(a, c), run for (0, B) and (B, n).  With c - a < 2 nothing happens.  Otherwise, for a < i < c,
 *       cross_i = (x_c - x_a)(y_i - y_a) - (y_c - y_a)(x_i - x_a),   D_i = cross_i^2,   L = |v_c - v_a|^2.
 *     When L = 0 (the segment's ends coincide), D_i = |v_i - v_a|^2 and L = 1.  m is the smallest i with maximal D_i.  If
 *     256 * D_m > tol16^2 * L, then m is kept and SPLIT(a, m) and SPLIT(m, c) run.  (A loop may pass a saddle vertex twice, but
 *     a kept m has D_m > 0 and so differs from both ends of its segment: L = 0 arises only when all of a loop's vertices are one
 *     point, which no plane produces; the clause makes the rule total.)
 *   3 OUTPUT.  The kept vertices come out in their original order, v_0 first; COUNT' >= 2.
 * The kept set is a function of the loop alone and no segment's decision depends on the order in which segments are visited:
 * identical bytes from run to run.  tol16 = 0 drops only vertices that lie on the chord of a segment whose other vertices all do.
 * OUTPUTS, each optional (NULL = not wanted, and so are loops_out with loops_rows_out == 0 and vertices_out with vertex_rows_out
 * == 0; nothing wanted is INFUR_E_INVALID_ARG), none needs initialisation; a rejected call touches no output:
 *   loops_out     record i belongs to input loop i: (OFFSET', COUNT', VALUE, START) with VALUE and START copied.  Only the first
 *                 min(n_loops, loops_rows_out) records are written.  OFFSET' is the number of kept vertices in front of the loop's
 *                 OFFSET: for Outlines' records, which lie back to back, the full exclusive prefix sum of COUNT', whatever is
 *                 truncated
 *   vertices_out  the first min(n_vertices', vertex_rows_out) kept vertex ids, loops back to back
 *   counts_out    INFUR_SIMPLIFY_COUNT_WORDS uint32_t {n_loops, n_vertices', n_degenerate, status}, always complete
 * n_degenerate counts the loops with COUNT' < 3: a thin region collapsed to its two anchors.  Such a loop keeps its record, so that
 * indices stay aligned with Outlines' loops; a consumer skips it.  This is not an error.
 * STATUS.  INFUR_SIMPLIFY_TRUNCATED: the input was truncated, counts[0] > loops_rows_in or counts[1] > vertex_rows_in (Outlines
 * was given fewer rows than it had loops or vertices).  Nothing but counts_out is written, as {counts[0], 0, 0, 1}.
 * INFUR_SIMPLIFY_MALFORMED: some record had COUNT < 2 or OFFSET + COUNT > counts[1].  Such a loop gets COUNT' = 0 (and counts as
 * degenerate) and keeps none of its vertices.  Every read is clamped to the rows the caller declared: no value held in the input
 * buffers can take a load or a store outside them.  Records that overlap or leave gaps -- Outlines writes none -- are read
 * safely: a vertex no record covers is dropped, a vertex two records cover is kept when either keeps it, COUNT' is the number of
 * kept vertices in the record's range.
 * COST.  A wave owns a loop and reads a segment once per level of the recursion below it, 64 vertices a step: O(n * depth / 64)
 * steps for a loop of n vertices, O(n^2 / 64) when every split is lopsided.  The plane's longest loop bounds the call.
 * WHAT IT DOES NOT DO.  It does not preserve topology: two regions that share a border are simplified independently, so their
 * polygons may overlap or leave slivers, and a loop may touch or cross itself -- COCO polygons have the same property.  It does
 * not convert to COCO JSON.  It has no sub-pixel contours.  It offers no Visvalingam simplification and no area-based criterion. */
enum { INFUR_SIMPLIFY_LOOPS = 0, INFUR_SIMPLIFY_VERTICES = 1, INFUR_SIMPLIFY_DEGENERATE = 2, INFUR_SIMPLIFY_STATUS = 3, INFUR_SIMPLIFY_COUNT_WORDS = 4 };
enum { INFUR_SIMPLIFY_TRUNCATED = 1, INFUR_SIMPLIFY_MALFORMED = 2 };
enum { INFUR_FEATURE_SIMPLIFY = 32 };

/* host pointers: counts is read first, min(counts[0], loops_rows_in) records and min(counts[1], vertex_rows_in) vertices travel to
 * the device; then counts_out is read, and min(n_loops, loops_rows_out) records and min(n_vertices', vertex_rows_out) vertices are
 * copied back */
int32_t infur_simplify(infur_ctx* ctx, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices,
                       uint32_t vertex_rows_in, const uint32_t* counts, uint32_t h, uint32_t w, uint32_t tol16, uint32_t* loops_out,
                       uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out, uint32_t* counts_out);
/* device pointers throughout, d_counts and d_counts_out (four device uint32_t) included; enqueued on the context's stream as one
 * memset and at most 6 launches, a number fixed by the arguments: the call never synchronises, so its grids are sized by
 * loops_rows_in and vertex_rows_in -- declare the rows Outlines was given, not more.  Capturable after one call outside the
 * capture, which allocates the scratch: 5 bytes per vertex row (a keep flag and a rank) and the scan's sums, owned by the context.
 * It grows only with a request larger than any before, and a graph captured around the call is re-captured after that.  The
 * outputs must not overlap the inputs.  infur_frame_regions_dev, infur_outlines_dev on the label plane, then infur_simplify_dev
 * gives per-object polygons with a tolerance and no dense plane crossing PCIe. */
int32_t infur_simplify_dev(infur_ctx* ctx, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices,
                           uint32_t vertex_rows_in, const void* d_counts, uint32_t h, uint32_t w, uint32_t tol16, void* d_loops_out,
                           uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out, void* d_counts_out);
/* The fused frame path with simplified polygons: scale -> model -> Segments decode(out[0]) -> Outlines of the class plane into
 * scratch of the library's own -> Simplify into the caller's buffers, in one call.  The arguments are infur_frame_outlines' plus
 * tol16, and counts is Simplify's four words.  The scaled frame must be at most 8191 x 8191 (INFUR_E_INVALID_ARG, before the model
 * runs).  The scratch holds Outlines' worst case for max_edges: 8 bytes per edge of capacity beside Outlines' own 36 and
 * Simplify's 5, so callers that know their scenes pass max_edges; a plane with more edges than that reads counts = {0, 0, 0, 0}
 * (infur_frame_outlines tells the edge count).  The calls inherit infur_frame_outlines' checks and errors: with no model loaded
 * the Scale stage still runs and the call returns INFUR_E_MODEL_NOT_LOADED.  They always enqueue eagerly and leave the graphs cached
 * for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_polygons(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                             uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, uint32_t tol16,
                             uint32_t* loops, uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows, uint32_t* counts,
                             uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_polygons_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                                 uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, uint32_t tol16,
                                 void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows, void* d_counts,
                                 void* d_stats, uint32_t stats_capacity, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Coverage: shared borders simplified once, so that neighbouring polygons fit ----
 * Simplify treats every loop on its own: two regions that share a border get two different chords for it, and the polygons of
 * one frame overlap and leave slivers.  GeoJSON coverages, panoptic exports and stroked overlays want neighbours that fit.  GIS
 * libraries call the operation coverage simplification.  Coverage takes the plane Outlines was given and what Outlines left,
 * cuts every loop at the plane's junctions into arcs, and simplifies each arc by a rule that does not depend on the direction of
 * travel: both neighbours of a border keep the same vertices.  Presence of this group is announced by infur_features() &
 * INFUR_FEATURE_COVERAGE (INFUR_ABI_VERSION does not move).
 *
 * INPUT.  The plane Outlines was given (elem_bytes 1 or 4, h and w both in 1 .. 8191), Outlines' three outputs for it with
 * loops_rows_in and vertex_rows_in (counts[0..1] are read), flags (INFUR_COVERAGE_SKIP with skip_value: what Outlines got;
 * unknown bits, and skip_value > 255 on bytes, are INFUR_E_INVALID_ARG), tol16 <= 65535 in 1/16 pixel, and aug_rows (SCRATCH
 * below).  Connectivity is not an input: junctions are a property of the plane, and the kept set is the same under either
 * connectivity although the loops differ.  A NULL plane or counts, or a NULL array with rows declared, is INFUR_E_INVALID_ARG.
 * CELLS AND RAYS.  A cell outside the plane, or (under SKIP) equal to skip_value, is NONE: one value, distinct from every plane
 * value, 0xFFFFFFFF included.  Lattice vertex (X, Y) has the cells UL = (X-1, Y-1), UR = (X, Y-1), LL = (X-1, Y), LR = (X, Y) and
 * four rays: N is a border when UL != UR, S when LL != LR, W when UL != LL, E when UR != LR.  Its DEGREE is the number of border
 * rays: 0, 2, 3 or 4.  A JUNCTION is a vertex of degree >= 3: T- and four-way junctions, both saddles under either connectivity,
 * and every point where an interior border meets the plane's frame.
 * 1 AUGMENT.  For every loop and every edge v_i -> v_{i+1} (cyclic): v_i, then the junctions strictly inside the edge in travel
 *   order.  (A T-junction is a corner for two of its regions and an interior point of a straight edge for the third.)  Every
 *   junction is inserted into at most one loop: n_aug <= n_vertices + (h+1)(w+1).  An edge that is not axis-parallel, has no
 *   length, or has an id outside the lattice makes its loop MALFORMED, as does COUNT < 2 or OFFSET + COUNT > counts[1].
 * 2 ARCS.  The augmented loop is cut at its junction vertices, which are always kept.  The stretch from one junction to the next,
 *   cyclically, is an ARC (from a junction round to itself when the loop has one).  A loop with no junction is a RING: the whole
 *   border between an island and its surround.
 * 3 THE RULE FOR AN ARC u_0 .. u_k: Simplify's SPLIT(0, k) -- D_i, L, the L = 0 clause and the test 256 * D_m > tol16^2 * L are
 *   exactly Simplify's -- with one change: m is the i with maximal D_i and, on ties, the smallest vertex ID (should a hand-made
 *   loop hold one id twice, the first in travel order).  FOR A RING: anchor A is the vertex with the smallest id, anchor B
 *   maximises |v - A|^2 (ties to the smallest id); A and B are kept, and SPLIT runs on A..B and on B..A.  Both neighbours see an
 *   arc as the same sequence reversed and cross^2 is symmetric in its ends: both keep the same set.
 * 4 OUTPUT, in Simplify's layout, each optional, none needs initialisation, a rejected call touches nothing:
 *   loops_out     record i is (OFFSET', COUNT', VALUE, START) of input loop i, VALUE and START copied, OFFSET' the full exclusive
 *                 prefix sum of COUNT'.  Only the first min(n_loops, loops_rows_out) records are written
 *   vertices_out  the first min(n_vertices', vertex_rows_out) kept ids, loops back to back, each loop in augmented order from its
 *                 first kept vertex at or after v_0.  Unlike Simplify's, v_0 may be dropped, and the output is no subset of
 *                 the input: junctions are inserted.  A kept junction may be collinear with its kept neighbours; it stays,
 *                 because the neighbour across the border has it
 *   counts_out    INFUR_COVERAGE_COUNT_WORDS uint32_t {n_loops, n_vertices', n_degenerate (COUNT' < 3), status, n_aug, n_arcs};
 *                 in n_arcs a ring counts as 1 and an arc once per loop that walks it
 * STATUS.  INFUR_COVERAGE_TRUNCATED: counts[0] > loops_rows_in or counts[1] > vertex_rows_in; only counts_out is written, as
 * {counts[0], 0, 0, 1, 0, 0}.  INFUR_COVERAGE_MALFORMED: some loop was malformed; it gets COUNT' = 0 and counts as degenerate, the
 * other loops are as ever.  INFUR_COVERAGE_OVERFLOW: n_aug > aug_rows; counts_out = {n_loops, 0, 0, 4, n_aug, 0} and nothing else
 * is touched: visible, and not an error.  Every load is clamped to the declared rows and to the plane: no value held in the
 * input arrays can move a load or a store outside them.  (n_aug is reported saturated at 2^32 - 1.)
 * SCRATCH.  aug_rows is the capacity in augmented vertices: 18 bytes each, beside two junction bitmaps of one bit per lattice
 * vertex and 17 bytes per loop row.  aug_rows = 0 means vertex_rows_in + (h+1)(w+1), which cannot overflow; callers that know
 * their scenes pass less.
 * WHAT IT GUARANTEES.  Take the directed segments p -> q of all output loops with multiplicity, N(p, q) = count(p -> q) -
 * count(q -> p).  With nothing skipped, N is 0 for every segment except those of one simple closed cycle, each with N = 1: the
 * plane's frame as simplified.  The shoelace sum over all loops equals that cycle's.  tol16 = 0 keeps every augmented vertex.
 * WHAT IT DOES NOT DO.  Arcs are simplified independently: at a large tolerance two different arcs may still cross (TopoJSON and
 * mapshaper have the same property), and nothing repairs that.  No hole-to-parent nesting, no COCO JSON. */
enum { INFUR_COVERAGE_SKIP = 1 };
enum {
    INFUR_COVERAGE_LOOPS = 0, INFUR_COVERAGE_VERTICES = 1, INFUR_COVERAGE_DEGENERATE = 2, INFUR_COVERAGE_STATUS = 3, INFUR_COVERAGE_AUG = 4,
    INFUR_COVERAGE_ARCS = 5, INFUR_COVERAGE_COUNT_WORDS = 6
};
enum { INFUR_COVERAGE_TRUNCATED = 1, INFUR_COVERAGE_MALFORMED = 2, INFUR_COVERAGE_OVERFLOW = 4 };
enum { INFUR_FEATURE_COVERAGE = 64 };

/* host pointers: the plane, counts, min(counts[0], loops_rows_in) records and min(counts[1], vertex_rows_in) vertices travel to
 * the device; then counts_out is read, and min(n_loops, loops_rows_out) records and min(n_vertices', vertex_rows_out) vertices are
 * copied back */
int32_t infur_coverage(infur_ctx* ctx, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                       uint32_t skip_value, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices,
                       uint32_t vertex_rows_in, const uint32_t* counts, uint32_t tol16, uint32_t aug_rows, uint32_t* loops_out,
                       uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out, uint32_t* counts_out);
/* device pointers throughout, d_counts and d_counts_out (six device uint32_t) included; enqueued on the context's stream as one
 * memset and at most 13 launches, a number fixed by the arguments: the call never synchronises, so its grids are sized by h, w,
 * loops_rows_in and aug_rows.  Capturable after one call outside the capture, which allocates the scratch, owned by the context.
 * It grows only with a request larger than any before, and a graph captured around the call is re-captured after that.  The
 * outputs must not overlap the inputs. */
int32_t infur_coverage_dev(infur_ctx* ctx, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                           uint32_t skip_value, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices,
                           uint32_t vertex_rows_in, const void* d_counts, uint32_t tol16, uint32_t aug_rows, void* d_loops_out,
                           uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out, void* d_counts_out);
/* The fused frame path with polygons that fit: scale -> model -> Segments decode(out[0]) -> Outlines of the class plane into
 * scratch of the library's own -> Coverage of that plane into the caller's buffers, in one call: the twins of
 * infur_frame_polygons(_dev), with their arguments (flags are Outlines': SKIP reaches Coverage, CONN8 only Outlines) and checks;
 * counts is Coverage's six words and aug_rows is 0.  The scaled frame must be at most 8191 x 8191 (INFUR_E_INVALID_ARG, before the
 * model runs).  A plane with more edges than max_edges reads all-zero counts. */
int32_t infur_frame_coverage(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                             uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, uint32_t tol16,
                             uint32_t* loops, uint32_t loops_rows, uint32_t* vertices, uint32_t vertex_rows, uint32_t* counts,
                             uint64_t* stats, uint32_t stats_capacity, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_coverage_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                                 uint32_t decode, uint32_t flags, uint32_t skip_value, uint32_t max_edges, uint32_t tol16,
                                 void* d_loops, uint32_t loops_rows, void* d_vertices, uint32_t vertex_rows, void* d_counts,
                                 void* d_stats, uint32_t stats_capacity, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Anchors: a distance transform and one interior label point per region ----
 * A table row places its object at a centroid or a box corner, and neither has to lie on the object: the centroid of a "C", a
 * ring or a horseshoe is a pixel of something else.  The point a caption, a click target or a "where is it" answer needs is the
 * region's most interior pixel, with the radius of the largest disc that fits there: the argmax of a distance transform.  Anchors
 * computes both on the device.  Presence of this group is announced by infur_features() & INFUR_FEATURE_ANCHORS
 * (INFUR_ABI_VERSION does not move).
 *
 * The input is a plane of h x w elements of elem_bytes = 1 (a class plane) or 4 (a label or track plane), h and w at most 65535.
 * Runs' rules hold for elem_bytes, for a NULL plane, for unknown flag bits and for skip_value.
 *   flags & INFUR_ANCHORS_SKIP   pixels whose value equals skip_value belong to no region (typically class 0, INFUR_REGION_NONE,
 *                                INFUR_TRACK_NONE)
 * Outputs, each optional (NULL = not wanted, and so is anchors with rows == 0; nothing wanted is INFUR_E_INVALID_ARG), none needs
 * initialisation:
 *   dist2     h*w uint32_t: for a pixel p of value v, the squared Euclidean distance between pixel centres from p to the nearest
 *             position whose value differs from v.  Positions outside the frame count as differing -- the frame is a border, so an
 *             anchor and its disc lie inside the picture -- and so do skipped pixels.  Every pixel that is not skipped has
 *             dist2 >= 1, and exactly 1 where it touches a border; a skipped pixel has 0.  The distance is by VALUE, not by
 *             connected component: on a label plane the two coincide, on a class plane two touching objects of one class share
 *             one interior
 *   anchors   rows rows of INFUR_ANCHOR_WORDS uint32_t, one per value v < rows: INFUR_ANCHOR_PIXEL the linear index y*w + x of the
 *             pixel of value v with the largest dist2, ties to the smallest index, INFUR_ANCHOR_DIST2 that dist2.  A value no
 *             pixel holds, and the skipped value, read (INFUR_ANCHOR_NONE, 0).  Every one of the rows is written, whatever the
 *             plane holds; a pixel whose value is at or above rows still gets its dist2 and touches no row
 * h*w == 0 writes the NONE rows and nothing else; h or w above 65535 and a NULL plane with h*w > 0 are INFUR_E_INVALID_ARG.  No
 * output is touched when a call is rejected.  Everything is an integer, exact, and a function of the plane alone: identical bytes
 * from run to run. */
#define INFUR_ANCHOR_NONE 0xFFFFFFFFu
enum { INFUR_ANCHORS_SKIP = 1 };
enum { INFUR_ANCHOR_PIXEL = 0, INFUR_ANCHOR_DIST2 = 1, INFUR_ANCHOR_WORDS = 2 };
enum { INFUR_FEATURE_ANCHORS = 256 };

/* on a given plane, host pointers */
int32_t infur_anchors(infur_ctx* ctx, const void* plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                      uint32_t skip_value, uint32_t* dist2, uint32_t* anchors, uint32_t rows);
/* device pointers throughout; enqueued on the context's stream as one memset and three launches, never synchronises, capturable
 * after one call outside the capture (which allocates the scratch: two bytes per pixel and eight per row, owned by the context;
 * it grows only with a request larger than any before, and a graph captured around the call is re-captured after that).  This is
 * the call that composes on the device: infur_frame_regions_dev or infur_frame_tracks_dev, then infur_anchors_dev on the label or
 * track plane they left in device memory.  The outputs must not overlap the plane. */
int32_t infur_anchors_dev(infur_ctx* ctx, const void* d_plane, uint32_t elem_bytes, uint32_t h, uint32_t w, uint32_t flags,
                          uint32_t skip_value, void* d_dist2, void* d_anchors, uint32_t rows);
/* The fused frame path with an anchor per object: scale -> model -> Segments decode(out[0]) -> Regions -> Anchors of the label
 * plane with INFUR_REGION_NONE skipped, in one call.  The arguments are infur_frame_regions' own, then dist2 (dist2_capacity in
 * bytes, ow*oh*4 needed; less is INFUR_E_CAPACITY, checked, like the other capacities, once a model is loaded) and anchors, which
 * has table_rows rows: row i belongs to region i, table or no table.  Every output is optional, and at least one of labels,
 * table, n_regions, dist2 and anchors (with table_rows) must be given; the label plane goes to scratch of the library's own when
 * the caller does not want it.  The calls inherit infur_frame_regions' checks and errors: with no model loaded the Scale stage
 * still runs and the call returns INFUR_E_MODEL_NOT_LOADED.  They always enqueue eagerly and leave the graphs cached for
 * infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_anchors(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                            uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass,
                            uint8_t* conf, size_t plane_capacity, uint32_t* labels, size_t labels_capacity, uint64_t* table,
                            uint32_t table_rows, uint32_t* n_regions, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh,
                            uint32_t* dist2, size_t dist2_capacity, uint32_t* anchors);
int32_t infur_frame_anchors_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                                uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass,
                                void* d_conf, size_t plane_capacity, void* d_labels, size_t labels_capacity, void* d_table,
                                uint32_t table_rows, void* d_n_regions, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh,
                                void* d_dist2, size_t dist2_capacity, void* d_anchors);

/* ---- Compare: the confusion matrix and the per-object IoU between two planes ----
 * The stages above say what is in a frame; Compare says how good that answer is.  It takes two planes that lie in device memory
 * -- a class plane and ground truth, the class planes of two arithmetic modes, a label plane and ground-truth instances -- and
 * returns the integers every segmentation measure is made of: the confusion matrix (pixel accuracy, IoU per class, mIoU), and
 * per value of either plane its best partner in the other with intersection and union (IoU per object, panoptic quality).
 * Presence of this group is announced by infur_features() & INFUR_FEATURE_COMPARE (INFUR_ABI_VERSION does not move).
 *
 * The inputs are two planes a and b of the same h x w elements, h and w at most 65535, each with its own element size elem_a,
 * elem_b = 1 (a class plane) or 4 (a label or track plane).  Runs' rules hold for the element sizes, for unknown flag bits, for
 * an ignore value no 1-byte element can hold and for a NULL plane.
 *   flags & INFUR_COMPARE_IGNORE_A   pixels with a == ignore_a are not compared
 *   flags & INFUR_COMPARE_IGNORE_B   pixels with b == ignore_b are not compared (typically a "void" label such as 255 in ground
 *                                    truth, INFUR_REGION_NONE, INFUR_TRACK_NONE)
 * rows_a and rows_b are the number of values on each side.  A pixel is IGNORED or COMPARED; a compared pixel with a >= rows_a or
 * b >= rows_b is OUTSIDE: it is counted and takes part in nothing else.  The rest are INSIDE.
 * Outputs, each optional (NULL = not wanted, and so are a matrix with rows_a * rows_b == 0 and a row table of 0 rows; nothing
 * wanted is INFUR_E_INVALID_ARG), none needs initialisation:
 *   matrix      rows_a x rows_b uint32_t, row-major: matrix[i][j] is the number of inside pixels with a == i and b == j.  Every
 *               entry is written.  Wanting it with rows_a * rows_b above 2^20 is INFUR_E_INVALID_ARG
 *   rows_a_out  rows_a rows of INFUR_COMPARE_WORDS uint32_t, one per value i of a: INFUR_COMPARE_PIXELS the inside pixels of
 *               value i, INFUR_COMPARE_PARTNER the value j of b with the largest intersection, ties to the smallest j,
 *               INFUR_COMPARE_INTER that intersection, INFUR_COMPARE_UNION PIXELS + the partner's PIXELS - INTER.  IoU is
 *               INTER / UNION, and the pair is MATCHED iff 2 * INTER > UNION -- the rule of panoptic quality: an IoU above one
 *               half makes the match unique and mutual.  A value no inside pixel holds reads (0, INFUR_COMPARE_NONE, 0, 0)
 *   rows_b_out  the mirror image: rows_b rows, the partner a value of a
 *   counts      INFUR_COMPARE_COUNT_WORDS uint32_t: INFUR_COMPARE_COMPARED, INFUR_COMPARE_EQUAL (inside pixels with a == b),
 *               INFUR_COMPARE_IGNORED, INFUR_COMPARE_OUTSIDE, INFUR_COMPARE_PAIRS (distinct (i, j) with a non-zero
 *               intersection), INFUR_COMPARE_MATCHED (matched rows of a, which is the number of matched rows of b),
 *               INFUR_COMPARE_RUNS (R, below), INFUR_COMPARE_STATUS.  COMPARED + IGNORED == h * w
 * h * w == 0 writes zeros and NONE rows, and nothing else (STATUS 0).
 *
 * Two forms, chosen by the arguments alone.  With rows_a * rows_b <= 4096 the matrix is counted in LDS (the dense form): there is
 * no table and nothing can overflow.  Everything larger goes through an open-addressing table of (i, j) pairs of pair_slots
 * slots (the table form; INFUR_COMPARE_TABLE in STATUS): pair_slots is a power of two >= 64, 0 means 2^20, anything else is
 * INFUR_E_INVALID_ARG in either form.  R is the number of runs of equal inside (i, j) along rows cut every 64 columns, reported in
 * both forms; it bounds the distinct pairs.  In the table form 2 * R > pair_slots sets INFUR_COMPARE_OVERFLOW in STATUS: every
 * PARTNER / INTER / UNION then reads (INFUR_COMPARE_NONE, 0, 0) and PAIRS = MATCHED = 0, while PIXELS, the matrix and the other
 * counts are still exact.  The overflow is visible and is not an error.
 *
 * Example: a = [[0,0,1,1],[0,1,1,2]], b = [[0,0,0,1],[0,1,1,1]], rows 3 x 3, nothing ignored: matrix [[3,0,0],[1,3,0],[0,1,0]],
 * rows_a_out (3,0,3,4) (4,1,3,5) (1,1,1,4), rows_b_out (4,0,3,4) (4,1,3,5) (0,NONE,0,0), counts COMPARED 8, EQUAL 6, IGNORED 0,
 * OUTSIDE 0, PAIRS 4, MATCHED 2, RUNS 6, STATUS 0.  Pixel accuracy is 6/8, the class IoUs from the diagonal 3/4, 3/5 and 0/1.
 *
 * Checks, in this order, each INFUR_E_INVALID_ARG: the context; elem_a, then elem_b (1 or 4); unknown flag bits; ignore_a, then
 * ignore_b, above 255 on a 1-byte plane; h or w above 65535; pair_slots; nothing wanted; a wanted matrix above 2^20 entries; a
 * NULL plane with h * w > 0.  No output is touched when a call is rejected.  Everything is an integer, exact, and a function of the
 * two planes alone: identical bytes from run to run. */
#define INFUR_COMPARE_NONE 0xFFFFFFFFu
enum { INFUR_COMPARE_IGNORE_A = 1, INFUR_COMPARE_IGNORE_B = 2 };
enum { INFUR_COMPARE_PIXELS = 0, INFUR_COMPARE_PARTNER = 1, INFUR_COMPARE_INTER = 2, INFUR_COMPARE_UNION = 3, INFUR_COMPARE_WORDS = 4 };
enum {
    INFUR_COMPARE_COMPARED = 0,
    INFUR_COMPARE_EQUAL = 1,
    INFUR_COMPARE_IGNORED = 2,
    INFUR_COMPARE_OUTSIDE = 3,
    INFUR_COMPARE_PAIRS = 4,
    INFUR_COMPARE_MATCHED = 5,
    INFUR_COMPARE_RUNS = 6,
    INFUR_COMPARE_STATUS = 7,
    INFUR_COMPARE_COUNT_WORDS = 8
};
enum { INFUR_COMPARE_OVERFLOW = 1, INFUR_COMPARE_TABLE = 2 };
enum { INFUR_FEATURE_COMPARE = 512 };

/* on two given planes, host pointers */
int32_t infur_compare(infur_ctx* ctx, const void* a, uint32_t elem_a, const void* b, uint32_t elem_b, uint32_t h, uint32_t w,
                      uint32_t flags, uint32_t ignore_a, uint32_t ignore_b, uint32_t* matrix, uint32_t rows_a, uint32_t rows_b,
                      uint32_t* rows_a_out, uint32_t* rows_b_out, uint32_t* counts, uint32_t pair_slots);
/* device pointers throughout; enqueued on the context's stream, never synchronises.  The number of memsets and launches is fixed
 * by the arguments: the dense form is one memset and four launches, the table form two memsets -- three when the matrix is
 * wanted -- and five launches; without counts each is one launch fewer; an empty plane is at most two memsets and one launch.
 * Capturable after one call outside the capture (which allocates the scratch, owned by the context: 12 bytes per row of either
 * side, and four per matrix entry or twelve per slot; it grows only with a request larger than any before, and a graph captured
 * around the call is re-captured after that).  This is the call that composes on the device: infur_frame_regions_dev or
 * infur_frame_tracks_dev, then infur_compare_dev of the label or track plane they left in device memory against a ground-truth
 * instance plane, with INFUR_REGION_NONE ignored.  The outputs must not overlap the planes or each other. */
int32_t infur_compare_dev(infur_ctx* ctx, const void* d_a, uint32_t elem_a, const void* d_b, uint32_t elem_b, uint32_t h,
                          uint32_t w, uint32_t flags, uint32_t ignore_a, uint32_t ignore_b, void* d_matrix, uint32_t rows_a,
                          uint32_t rows_b, void* d_rows_a_out, void* d_rows_b_out, void* d_counts, uint32_t pair_slots);
/* The fused frame path with a grade: scale -> model -> Segments decode(out[0]) -> Compare of the class plane (a, one byte per
 * pixel) against the caller's uint8_t truth plane of ow x oh (b), in one call.  Of the flags only INFUR_COMPARE_IGNORE_B (with
 * ignore_b) is meaningful, and INFUR_COMPARE_IGNORE_A is INFUR_E_INVALID_ARG.  truth_capacity is in bytes, ow * oh needed; less
 * is INFUR_E_CAPACITY, checked, like plane_capacity for klass and conf, once a model is loaded.  klass, conf and scaled_bgr are
 * optional outputs as in infur_frame_segments; at least one of matrix, rows_a_out, rows_b_out and counts must be wanted.  The
 * calls inherit infur_frame_segments' checks and errors: with no model loaded the Scale stage still runs and the call returns
 * INFUR_E_MODEL_NOT_LOADED.  They always enqueue eagerly and leave the graphs cached for infur_frame_advance_dev alone.  (The
 * stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_compare(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                            uint32_t decode, uint32_t flags, uint32_t ignore_b, const uint8_t* truth, size_t truth_capacity,
                            uint8_t* klass, uint8_t* conf, size_t plane_capacity, uint32_t* matrix, uint32_t rows_a,
                            uint32_t rows_b, uint32_t* rows_a_out, uint32_t* rows_b_out, uint32_t* counts, uint32_t pair_slots,
                            uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh);
int32_t infur_frame_compare_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                                uint32_t decode, uint32_t flags, uint32_t ignore_b, const void* d_truth, size_t truth_capacity,
                                void* d_klass, void* d_conf, size_t plane_capacity, void* d_matrix, uint32_t rows_a,
                                uint32_t rows_b, void* d_rows_a_out, void* d_rows_b_out, void* d_counts, uint32_t pair_slots,
                                void* d_scaled_bgr, uint32_t* ow, uint32_t* oh);

/* ---- Adjacency: which regions touch, and along how many pixel edges ----
 * The region adjacency graph of a class, label or track plane in device memory: "person touches bicycle", the perimeter and the
 * degree of every object, and the graph Sieve (below) merges speckle along.  Presence of this group and of Sieve is announced by
 * infur_features() & INFUR_FEATURE_SIEVE (INFUR_ABI_VERSION does not move).
 *
 * The input is a plane of h x w elements of elem = 1 or 4 bytes, h and w at most 65535 and h * w below 2^31.  Runs' rules hold for
 * the element size, for unknown flag bits, for a skip value no 1-byte element can hold and for a NULL plane.
 *   flags & INFUR_ADJ_SKIP   pixels whose value equals skip_value belong to no region (class 0, INFUR_REGION_NONE, INFUR_TRACK_NONE)
 * rows is the number of values.  A pixel is INSIDE when its value is below rows and is not the skipped value; the others are
 * SKIPPED or OUTSIDE: they are counted and take part in nothing else.  A border edge is a pixel edge between two 4-neighbours
 * that are both inside and have different values.  Diagonal contact has length 0 and is no adjacency, whatever connectivity made
 * the labels.  The edge between (x, y) and (x+1, y) has id 2 * (y*w + x), the edge between (x, y) and (x, y+1) id 2 * (y*w + x) + 1.
 * Outputs, each optional (NULL = not wanted, and so is a row table of 0 rows; nothing wanted is INFUR_E_INVALID_ARG), none needs
 * initialisation:
 *   pairs     pair_rows records of INFUR_ADJ_PAIR_WORDS uint32_t, one per unordered pair of values that share at least one border
 *             edge: INFUR_ADJ_A < INFUR_ADJ_B the two values, INFUR_ADJ_BORDER the number of border edges between them,
 *             INFUR_ADJ_FIRST the smallest of their ids.  The records are in ascending order of FIRST -- Regions' numbering rule
 *             carried over to edges -- and min(PAIRS, pair_rows) of them are written; the rest is left alone
 *   rows_out  rows records of INFUR_ADJ_ROW_WORDS uint32_t, one per value: INFUR_ADJ_DEGREE the number of distinct neighbours,
 *             INFUR_ADJ_LONGEST the neighbour with the longest shared border, ties to the smallest value (INFUR_ADJ_NONE without a
 *             neighbour), INFUR_ADJ_ROW_BORDER that border's length, INFUR_ADJ_PERIMETER every pixel edge of the value against
 *             anything that is not the value: other values, skipped and outside pixels, and the frame
 *   counts    INFUR_ADJ_COUNT_WORDS uint32_t: INFUR_ADJ_PAIRS, INFUR_ADJ_EDGES (the sum of all BORDER words), INFUR_ADJ_SKIPPED
 *             and INFUR_ADJ_OUTSIDE pixels, INFUR_ADJ_RUNS (R, below), INFUR_ADJ_WRITTEN (the records written: 0 when pairs is
 *             NULL), one reserved word written as 0, INFUR_ADJ_STATUS
 * h * w == 0 writes zero counts and rows (0, INFUR_ADJ_NONE, 0, 0), and nothing else.
 *
 * The pairs are collected in an open-addressing table of pair_slots slots: a power of two >= 64, 0 means 2^20, anything else is
 * INFUR_E_INVALID_ARG.  R is the number of border runs: the maximal sequences of border edges between rows y and y+1 that are
 * consecutive in x and have the same ordered (top, bottom) pair, and of border edges between columns x and x+1 that are consecutive
 * in y and have the same ordered (left, right) pair.  R bounds the distinct pairs and is a function of the plane.  2 * R > pair_slots
 * sets INFUR_ADJ_OVERFLOW in STATUS: no pair record is written, every row reads (0, INFUR_ADJ_NONE, 0, PERIMETER) and PAIRS = EDGES
 * = WRITTEN = 0.  With pairs wanted, PAIRS > pair_rows sets INFUR_ADJ_TRUNCATED.  Neither is an error.
 *
 * Example (used by Sieve below): the label plane [[0,0,0,1,1,1],[0,2,0,1,1,1],[0,0,0,1,3,3],[0,0,0,1,3,4]], rows 5, nothing skipped:
 * pairs (0,2,4,3) (0,1,4,4) (1,3,4,21) (3,4,2,35); rows_out (2,1,4,18) (2,0,4,14) (1,0,4,4) (2,1,4,8) (1,3,2,4); counts PAIRS 4,
 * EDGES 14, SKIPPED 0, OUTSIDE 0, RUNS 9, WRITTEN 4, 0, STATUS 0.
 *
 * Checks, in this order, each INFUR_E_INVALID_ARG: the context; elem (1 or 4); unknown flag bits; skip_value above 255 on a 1-byte
 * plane; h or w above 65535 or h * w >= 2^31; pair_slots; nothing wanted; a NULL plane with h * w > 0.  No output is touched when a
 * call is rejected.  Everything is an integer, exact, and a function of the plane alone: identical bytes from run to run. */
#define INFUR_ADJ_NONE 0xFFFFFFFFu
enum { INFUR_ADJ_SKIP = 1 };
enum { INFUR_ADJ_A = 0, INFUR_ADJ_B = 1, INFUR_ADJ_BORDER = 2, INFUR_ADJ_FIRST = 3, INFUR_ADJ_PAIR_WORDS = 4 };
enum { INFUR_ADJ_DEGREE = 0, INFUR_ADJ_LONGEST = 1, INFUR_ADJ_ROW_BORDER = 2, INFUR_ADJ_PERIMETER = 3, INFUR_ADJ_ROW_WORDS = 4 };
enum {
    INFUR_ADJ_PAIRS = 0,
    INFUR_ADJ_EDGES = 1,
    INFUR_ADJ_SKIPPED = 2,
    INFUR_ADJ_OUTSIDE = 3,
    INFUR_ADJ_RUNS = 4,
    INFUR_ADJ_WRITTEN = 5,
    INFUR_ADJ_STATUS = 7,
    INFUR_ADJ_COUNT_WORDS = 8
};
enum { INFUR_ADJ_OVERFLOW = 1, INFUR_ADJ_TRUNCATED = 2 };
enum { INFUR_FEATURE_SIEVE = 1024 };

/* on a given plane, host pointers */
int32_t infur_adjacency(infur_ctx* ctx, const void* plane, uint32_t elem, uint32_t h, uint32_t w, uint32_t flags,
                        uint32_t skip_value, uint32_t rows, uint32_t* pairs, uint32_t pair_rows, uint32_t* rows_out,
                        uint32_t* counts, uint32_t pair_slots);
/* device pointers throughout; enqueued on the context's stream, never synchronises: two memsets and at most nine launches, fixed by
 * the arguments.  The scratch is owned by the context (twelve bytes per slot, sixteen per row, a quarter of a byte per pixel for
 * ordered records) and grows only with a request larger than any before.  The outputs must not overlap the plane or each other. */
int32_t infur_adjacency_dev(infur_ctx* ctx, const void* d_plane, uint32_t elem, uint32_t h, uint32_t w, uint32_t flags,
                            uint32_t skip_value, uint32_t rows, void* d_pairs, uint32_t pair_rows, void* d_rows_out,
                            void* d_counts, uint32_t pair_slots);

/* ---- Sieve: merge speckle regions into their neighbours ----
 * A decoded class plane has speckle: islands of a few pixels of the wrong class, pin-holes inside objects.  Regions' min_pixels
 * drops them from the label plane and leaves the class plane as it is.  Sieve is the standard remedy (GDAL's gdal_sieve): a region
 * below a size threshold takes the class of the neighbour it shares the longest border with.  The result is again a complete
 * class plane, so Regions, Tracks, Runs, Outlines, Coverage, Anchors and Compare run on it unchanged.  Announced by
 * infur_features() & INFUR_FEATURE_SIEVE.
 *
 * infur_sieve_dev takes what infur_regions_dev (infur_frame_regions_dev) leaves in device memory after a run with min_pixels = 0
 * and without INFUR_REGIONS_SKIP_BACKGROUND: the h x w uint8_t class plane, the uint32_t label plane, the region table
 * (table_rows rows of INFUR_REGION_WORDS uint64_t) and the device word n_regions; h and w at most 65535, h * w below 2^31.
 *   n = min(n_regions, table_rows).  A pixel whose label is >= n, or is INFUR_REGION_NONE, is FIXED: it keeps its class and is
 *   neither a source nor a target.
 *   Region r is SMALL when PIXELS(r) < min_pixels; every other region is KEPT.
 *   Round 0: the kept regions are resolved with their own CLASS.
 *   Round t >= 1, over every region still unresolved after round t-1: among its neighbours that were resolved after round t-1
 *   take the one with the largest BORDER, ties to the smallest region id.  The neighbours are the Adjacency pairs of the label
 *   plane as given; borders are never re-evaluated after a merger.  If such a neighbour q exists, r becomes resolved with q's
 *   class, INTO(r) = INTO(q) and ROUND(r) = t.  A kept region's INTO is itself.
 *   The loop ends after the first round that resolves nothing, or after max_rounds rounds (0 means 8; above 64 is
 *   INFUR_E_INVALID_ARG).  What is still unresolved is STRANDED and keeps its class.
 * Outputs, each optional (all NULL is INFUR_E_INVALID_ARG), none needs initialisation; they must not overlap the inputs or each other:
 *   klass_out  h*w uint8_t: the final class of the pixel's region; fixed pixels are copied
 *   rows_out   n records of INFUR_SIEVE_ROW_WORDS uint32_t: INFUR_SIEVE_CLASS the final class, INFUR_SIEVE_INTO the kept region it
 *              was absorbed into (itself for kept and stranded regions), INFUR_SIEVE_ROUND (0 for kept, INFUR_SIEVE_NONE for
 *              stranded), INFUR_SIEVE_BORDER the winning border (0 for kept and stranded)
 *   counts     INFUR_SIEVE_COUNT_WORDS uint32_t: INFUR_SIEVE_REGIONS (n), INFUR_SIEVE_SMALL, INFUR_SIEVE_ABSORBED,
 *              INFUR_SIEVE_STRANDED, INFUR_SIEVE_ROUNDS (the last round that resolved something), INFUR_SIEVE_PIXELS_CHANGED,
 *              INFUR_SIEVE_PAIRS, INFUR_SIEVE_STATUS
 * STATUS bits: INFUR_SIEVE_OVERFLOW -- Adjacency's overflow rule fired for pair_slots (as above): klass_out is the input, every
 * small region is stranded and PAIRS = 0; INFUR_SIEVE_ROUNDS_EXHAUSTED -- round max_rounds still resolved something and unresolved
 * regions remain; INFUR_SIEVE_TABLE_SHORT -- n_regions > table_rows.  None is an error.  h * w == 0 writes zero counts and nothing else.
 *
 * A small region only ever joins a neighbour across a shared pixel edge.  So with STRANDED == 0 and no fixed pixels every region of
 * klass_out holds at least min_pixels pixels, whichever of the two connectivities made the labels (counted under that connectivity),
 * and the pixels of kept regions are unchanged.
 *
 * Example: the class plane [[1,1,1,2,2,2],[1,3,1,2,2,2],[1,1,1,2,4,4],[1,1,1,2,4,5]] has the label plane of the example above and
 * the regions 0 (class 1, 11 pixels), 1 (class 2, 8), 2 (class 3, 1), 3 (class 4, 3), 4 (class 5, 1).  With min_pixels = 4 regions
 * 2, 3 and 4 are small.  Round 1: 2 joins 0 (border 4), 3 joins 1 (border 4); 4 touches only 3, which was unresolved.  Round 2: 4
 * joins 3 (border 2) and with it region 1.  rows_out (1,0,0,0) (2,1,0,0) (1,0,1,4) (2,1,1,4) (2,1,2,2); klass_out has three columns
 * of 1 and three of 2; counts REGIONS 5, SMALL 3, ABSORBED 3, STRANDED 0, ROUNDS 2, PIXELS_CHANGED 5, PAIRS 4, STATUS 0.
 *
 * Checks, in this order, each INFUR_E_INVALID_ARG: the context; h or w above 65535 or h * w >= 2^31; max_rounds; pair_slots;
 * nothing wanted; a NULL input with h * w > 0.  Everything is an integer and a function of the inputs alone: identical bytes from
 * run to run. */
#define INFUR_SIEVE_NONE 0xFFFFFFFFu
enum { INFUR_SIEVE_CLASS = 0, INFUR_SIEVE_INTO = 1, INFUR_SIEVE_ROUND = 2, INFUR_SIEVE_BORDER = 3, INFUR_SIEVE_ROW_WORDS = 4 };
enum {
    INFUR_SIEVE_REGIONS = 0,
    INFUR_SIEVE_SMALL = 1,
    INFUR_SIEVE_ABSORBED = 2,
    INFUR_SIEVE_STRANDED = 3,
    INFUR_SIEVE_ROUNDS = 4,
    INFUR_SIEVE_PIXELS_CHANGED = 5,
    INFUR_SIEVE_PAIRS = 6,
    INFUR_SIEVE_STATUS = 7,
    INFUR_SIEVE_COUNT_WORDS = 8
};
enum { INFUR_SIEVE_OVERFLOW = 1, INFUR_SIEVE_ROUNDS_EXHAUSTED = 2, INFUR_SIEVE_TABLE_SHORT = 4 };

/* host pointers: klass and labels h*w, table min(n_regions, table_rows) rows, n_regions by value */
int32_t infur_sieve(infur_ctx* ctx, const uint8_t* klass, const uint32_t* labels, const uint64_t* table, uint32_t table_rows,
                    uint32_t n_regions, uint32_t h, uint32_t w, uint32_t min_pixels, uint32_t max_rounds, uint32_t pair_slots,
                    uint8_t* klass_out, uint32_t* rows_out, uint32_t* counts);
/* device pointers throughout, d_n_regions included (one device uint32_t); enqueued on the context's stream, never synchronises and
 * reads nothing back: three memsets, 4 + 2 * max_rounds launches (a choose launch over the pair slots and an apply launch over the
 * regions per round; a round behind one that resolved nothing exits at once on a device flag) and one launch per wanted output.
 * The scratch is owned by the context (twelve bytes per slot, twenty-four per table row). */
int32_t infur_sieve_dev(infur_ctx* ctx, const void* d_klass, const void* d_labels, const void* d_table, uint32_t table_rows,
                        const void* d_n_regions, uint32_t h, uint32_t w, uint32_t min_pixels, uint32_t max_rounds,
                        uint32_t pair_slots, void* d_klass_out, void* d_rows_out, void* d_counts);
/* The fused frame path with a cleaned class plane: scale -> model -> Segments decode(out[0]) -> Regions (the caller's connectivity,
 * min_pixels = 0, no skip) -> Sieve (min_pixels), in one call.  The arguments are infur_frame_regions' own, then max_rounds,
 * pair_slots, klass_out (plane_capacity bytes, like klass and conf) and the sieve counts.  klass and conf are the planes as decoded;
 * klass_out is the cleaned plane.  When labels, table or n_regions is wanted Regions runs a second time, on the cleaned plane, with
 * the caller's flags and min_pixels = 0: they describe the cleaned plane.  At least one of labels, table, n_regions, klass_out and
 * counts must be wanted.  The library's own region table holds 2^20 rows: a frame with more regions has INFUR_SIEVE_TABLE_SHORT in
 * its status and the regions beyond stay as they are.  The calls inherit infur_frame_regions' checks, errors and check order
 * (max_rounds and pair_slots are checked behind connectivity and flags); they always enqueue eagerly and leave the graphs cached
 * for infur_frame_advance_dev alone.  (The stream ring, batch and group calls produce RGBA only.) */
int32_t infur_frame_sieve(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                          uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf,
                          size_t plane_capacity, uint32_t* labels, size_t labels_capacity, uint64_t* table, uint32_t table_rows,
                          uint32_t* n_regions, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh, uint32_t max_rounds,
                          uint32_t pair_slots, uint8_t* klass_out, uint32_t* counts);
int32_t infur_frame_sieve_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                              uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass,
                              void* d_conf, size_t plane_capacity, void* d_labels, size_t labels_capacity, void* d_table,
                              uint32_t table_rows, void* d_n_regions, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh,
                              uint32_t max_rounds, uint32_t pair_slots, void* d_klass_out, void* d_counts);

/* ---- Shapes: convex hull, moments and minimum rectangle per outline loop ----
 * The stages above say where an object is and where its edge runs; none says what shape it has: elongated or round, lying or
 * standing, solid or ragged.  Shapes takes what Outlines left in device memory and computes, loop by loop, the area, perimeter and
 * second-order moments, the convex hull, and the smallest rectangle around the hull; per value it sums them.  Every quantity is an
 * exact integer function of a loop: identical bytes from run to run and no tolerance anywhere.  Presence of this group is announced
 * by infur_features() & INFUR_FEATURE_SHAPES (INFUR_ABI_VERSION does not move).
 *
 * INPUT.  Simplify's exactly: Outlines' `loops`, `vertices` and `counts` for a plane of width w, with loops_rows_in and
 * vertex_rows_in; w in 1 .. 8191 and h at most 8191, otherwise INFUR_E_INVALID_ARG; a NULL counts, or a NULL array with rows
 * declared, is INFUR_E_INVALID_ARG.  No plane is read.
 * PER LOOP with vertices v_0 .. v_{n-1}, v_n := v_0, and c_i = x_i * y_{i+1} - x_{i+1} * y_i.  Every word is a signed 64-bit
 * integer (the arrays are declared uint64_t: read them as two's complement); the sums are formed modulo 2^64, intermediates may
 * wrap, the true values fit (24 * integral of xy < 2^57 with coordinates up to 8191).  A record has INFUR_SHAPE_WORDS words:
 *   INFUR_SHAPE_AREA2       sum c_i                                                  twice the area; negative for a hole
 *   INFUR_SHAPE_PERIMETER   sum |x_{i+1} - x_i| + |y_{i+1} - y_i|                    the lattice length
 *   INFUR_SHAPE_M10_6       sum c_i (x_i + x_{i+1})                                  6 * integral of x
 *   INFUR_SHAPE_M01_6       sum c_i (y_i + y_{i+1})                                  6 * integral of y
 *   INFUR_SHAPE_M20_12      sum c_i (x_i^2 + x_i x_{i+1} + x_{i+1}^2)                12 * integral of x^2
 *   INFUR_SHAPE_M02_12      sum c_i (y_i^2 + y_i y_{i+1} + y_{i+1}^2)                12 * integral of y^2
 *   INFUR_SHAPE_M11_24      sum c_i (x_i y_{i+1} + 2 x_i y_i + 2 x_{i+1} y_{i+1} + x_{i+1} y_i)   24 * integral of xy
 *   INFUR_SHAPE_HULL_AREA2  the shoelace sum of the hull's vertices: it has the loop's sign
 *   INFUR_SHAPE_RECT_EDGE, _RECT_W, _RECT_H, _RECT_L   the minimum rectangle, below
 * The integrals run over the union of pixel squares, pixel (x, y) being [x, x+1] x [y, y+1]; summed over the loops of a value
 * (holes are negative) AREA2 = 2 * pixels, M10_6 = 3 * sum(2x + 1), M20_12 = 2 * sum(6x^2 + 6x + 2), M11_24 = 6 * sum(2x + 1)(2y + 1),
 * and likewise in y.
 * HULL.  The kept set is the set of strictly extreme points of the loop's vertices: collinear points on a hull edge are dropped.
 * It is written in the loop's own order in Simplify's output layout: loops_out record i is (OFFSET', COUNT', VALUE, START) for
 * input loop i, vertices_out holds the kept ids back to back, with Simplify's truncation rules.  The set is defined mathematically
 * and does not depend on how it is found.  (This holds for every loop that is a polygon's boundary, which is every loop Outlines
 * writes: the kernel walks index ranges and relies on the hull's vertices appearing in the loop's order.  For other vertex lists
 * the output is some subset of the vertices, a function of the list alone and inside the buffers.  When all vertices are one point,
 * COUNT' = 1.)
 * MINIMUM RECTANGLE over the hull's edges j (kept vertex j -> j+1, vector e, L = |e|^2): W_j = max_p e.p - min_p e.p and
 * H_j = max_p |e x (p - v_j)| over the hull's vertices p; the rectangle on edge j has the sides sqrt(W^2 / L) along e and
 * sqrt(H^2 / L) across it, and the area W * H / L.  RECT_EDGE is the j that minimises the area, compared exactly as
 * W_a H_a L_b < W_b H_b L_a in 128 bits, on a tie the smallest j; RECT_W, RECT_H, RECT_L are that edge's.  COUNT' = 1 gives zeros.
 * PER VALUE, `value_rows` rows of INFUR_SHAPE_WORDS words, optional: for every loop with VALUE < value_rows, the row of its value
 * receives the sums of the seven measures (so AREA2 / 2 is the value's pixel count and the moments are the region's);
 * INFUR_SHAPE_HULL_AREA2 is summed over the outer loops (AREA2 > 0); INFUR_SHAPE_OUTER and INFUR_SHAPE_HOLES count the loops with
 * AREA2 > 0 and AREA2 < 0 (their difference is the Euler number); INFUR_SHAPE_LOOP is the index of the value's outer loop with the
 * largest AREA2, on a tie the smallest index, and -1 for a value without one: the region's hull and rectangle are that loop's.
 * Word 11 is 0.  Every one of the value_rows rows is written.
 * OUTPUTS, each optional (NULL or no rows = not wanted; nothing wanted is INFUR_E_INVALID_ARG), none needs initialisation; a
 * rejected call touches no output: loops_out and vertices_out as above; `shapes`, the first min(n_loops, shape_rows) per-loop
 * records; `values`; counts_out, INFUR_SHAPES_COUNT_WORDS uint32_t {n_loops, n_hull_vertices, status, largest COUNT'}, always
 * complete.
 * STATUS.  INFUR_SHAPES_TRUNCATED: counts[0] > loops_rows_in or counts[1] > vertex_rows_in.  Only counts_out, as {counts[0], 0,
 * 1, 0}, and the per-value table, as for a plane without loops, are written.  INFUR_SHAPES_MALFORMED: some record had COUNT < 2 or
 * OFFSET + COUNT > counts[1].  Such a loop gets COUNT' = 0, a record of zeros, and adds nothing to its value.  Every read is
 * clamped to the rows the caller declared: no value held in the input buffers can take a load or a store outside them.
 * EXAMPLE 1, the "C": a 24 x 24 plane, class 1 = [2:22, 2:22] minus [7:17, 7:22], class 0 skipped.  One loop of 8 vertices (2,2)
 * (22,2) (22,7) (7,7) (7,17) (22,17) (22,22) (2,22): AREA2 500, PERIMETER 110, M10_6 15750, M01_6 18000, M20_12 439000, M02_12
 * 577000, M11_24 756000.  The hull is (2,2) (22,2) (22,22) (2,22), HULL_AREA2 800 (solidity 0.625); the rectangle is edge 0 with
 * W = H = L = 400.  The centroid in pixel centres is 15750 / (3 * 500) - 1/2 = 10.0.
 * EXAMPLE 2, a slanted bar: a 12 x 16 plane, value 2 where |(x - 8) - (y - 6)| <= 1, 1 <= y <= 10 and 1 <= x <= 14, value 0
 * skipped.  One loop of 40 vertices: AREA2 60, PERIMETER 44, M10_6 1440, M01_6 1080, M20_12 26280, M02_12 15960, M11_24 40500.
 * The hull is (2,1) (5,1) (14,10) (14,11) (11,11) (2,2), HULL_AREA2 78; the rectangle is edge 1 with W 198, H 36, L 162: 15.56 x
 * 2.83 pixels, area 44.
 * COST.  A wave owns a loop: the measures read it once, the hull reads a range once per level of the recursion below it, 64
 * vertices a step; the rectangle is O(k^2 / 64) steps for a hull of k vertices (88 for a disc of radius 120).
 * WHAT IT DOES NOT DO.  No hull of a value with several outer loops, no Hu invariants, no least-squares ellipse, no Feret
 * diameters other than the rectangle's, no confidence-weighted moments, no input above 8191.  The stream ring, batch and group
 * calls produce RGBA only. */
enum {
    INFUR_SHAPE_AREA2 = 0,
    INFUR_SHAPE_PERIMETER = 1,
    INFUR_SHAPE_M10_6 = 2,
    INFUR_SHAPE_M01_6 = 3,
    INFUR_SHAPE_M20_12 = 4,
    INFUR_SHAPE_M02_12 = 5,
    INFUR_SHAPE_M11_24 = 6,
    INFUR_SHAPE_HULL_AREA2 = 7,
    INFUR_SHAPE_RECT_EDGE = 8,
    INFUR_SHAPE_RECT_W = 9,
    INFUR_SHAPE_RECT_H = 10,
    INFUR_SHAPE_RECT_L = 11,
    INFUR_SHAPE_WORDS = 12
};
enum { INFUR_SHAPE_OUTER = 8, INFUR_SHAPE_HOLES = 9, INFUR_SHAPE_LOOP = 10 }; /* words 8 .. 10 of a per-value row */
enum { INFUR_SHAPES_LOOPS = 0, INFUR_SHAPES_VERTICES = 1, INFUR_SHAPES_STATUS = 2, INFUR_SHAPES_LARGEST = 3, INFUR_SHAPES_COUNT_WORDS = 4 };
enum { INFUR_SHAPES_TRUNCATED = 1, INFUR_SHAPES_MALFORMED = 2 };
enum { INFUR_FEATURE_SHAPES = 2048 };

/* host pointers, with Simplify's copy rules: counts is read first, min(counts[0], loops_rows_in) records and min(counts[1],
 * vertex_rows_in) vertices travel to the device; then counts_out is read and what it says there is comes back */
int32_t infur_shapes(infur_ctx* ctx, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices,
                     uint32_t vertex_rows_in, const uint32_t* counts, uint32_t h, uint32_t w, uint32_t* loops_out,
                     uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out, uint64_t* shapes,
                     uint32_t shape_rows, uint64_t* values, uint32_t value_rows, uint32_t* counts_out);
/* device pointers throughout; enqueued on the context's stream as at most two memsets and 6 launches, a number fixed by the
 * arguments: the call never synchronises, so its grids are sized by loops_rows_in and vertex_rows_in -- declare the rows Outlines
 * was given, not more.  Capturable after one call outside the capture, which allocates the scratch: 9 bytes per vertex row, one
 * per loop row and the scan's sums, owned by the context.  The outputs must not overlap the inputs. */
int32_t infur_shapes_dev(infur_ctx* ctx, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices,
                         uint32_t vertex_rows_in, const void* d_counts, uint32_t h, uint32_t w, void* d_loops_out,
                         uint32_t loops_rows_out, void* d_vertices_out, uint32_t vertex_rows_out, void* d_shapes,
                         uint32_t shape_rows, void* d_values, uint32_t value_rows, void* d_counts_out);
/* The fused frame path with a descriptor per object: scale -> model -> Segments decode(out[0]) -> Regions -> Outlines of the label
 * plane (INFUR_REGION_NONE skipped, the caller's connectivity) -> Shapes, in one call.  The arguments are infur_frame_regions'
 * own, then Outlines' max_edges and Shapes' outputs; `values` has table_rows rows and row i is region i, table or no table.
 * Every output is optional, and at least one must be given; the label plane goes to scratch of the library's own when the caller
 * does not want it.  When a Shapes output is wanted the scaled frame must be at most 8191 x 8191 (INFUR_E_INVALID_ARG, before the
 * model runs).  A plane with more edges than max_edges (0: the worst case) reads counts = {0, 0, 0, 0} and a per-value table
 * without loops.  The calls inherit infur_frame_regions' checks, errors and order: with no model loaded the Scale stage still
 * runs and the call returns INFUR_E_MODEL_NOT_LOADED.  They always enqueue eagerly and leave the graphs cached for
 * infur_frame_advance_dev alone. */
int32_t infur_frame_shapes(infur_ctx* ctx, const uint8_t* bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                           uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, uint8_t* klass, uint8_t* conf,
                           size_t plane_capacity, uint32_t* labels, size_t labels_capacity, uint64_t* table, uint32_t table_rows,
                           uint32_t* n_regions, uint8_t* scaled_bgr, uint32_t* ow, uint32_t* oh, uint32_t max_edges,
                           uint32_t* loops_out, uint32_t loops_rows_out, uint32_t* vertices_out, uint32_t vertex_rows_out,
                           uint64_t* shapes, uint32_t shape_rows, uint64_t* values, uint32_t* counts_out);
int32_t infur_frame_shapes_dev(infur_ctx* ctx, const void* d_bgr, uint32_t w, uint32_t h, float factor, uint32_t scale_mode,
                               uint32_t decode, uint32_t connectivity, uint32_t min_pixels, uint32_t flags, void* d_klass,
                               void* d_conf, size_t plane_capacity, void* d_labels, size_t labels_capacity, void* d_table,
                               uint32_t table_rows, void* d_n_regions, void* d_scaled_bgr, uint32_t* ow, uint32_t* oh,
                               uint32_t max_edges, void* d_loops_out, uint32_t loops_rows_out, void* d_vertices_out,
                               uint32_t vertex_rows_out, void* d_shapes, uint32_t shape_rows, void* d_values, void* d_counts_out);

/* ---- Raster: polygon loops and run-length records filled back into a plane ----
 * Every stage above turns a dense plane into something smaller; Raster goes the other way, on the device: the loops Outlines,
 * Simplify, Coverage or Shapes (its hulls) left in device memory, or the records Runs left, become a class, label or track plane
 * again, so that Compare can grade against ground truth that exists as polygons or run-length records, and so that what a
 * tolerance costs can be counted in pixels.  Everything is an exact integer function of the input: identical bytes from run to
 * run and no tolerance anywhere.  Raster(Outlines(plane)) == plane and RasterRuns(Runs(plane)) == plane, byte for byte, for any
 * plane, connectivity and skip value (fill_value = skip_value).  Presence of this group is announced by infur_features() &
 * INFUR_FEATURE_RASTER (INFUR_ABI_VERSION does not move).
 *
 * THE PLANE is h x w, both in 1 .. 8191 (otherwise INFUR_E_INVALID_ARG), of elem_bytes 1 or 4; fill_value > 255 on a byte plane is
 * INFUR_E_INVALID_ARG.  Pixel (x, y) has its centre at (x + 1/2, y + 1/2).
 * INPUT, LOOPS.  Simplify's exactly: `loops`, `vertices` and `counts` with loops_rows_in and vertex_rows_in; a NULL counts, or a
 * NULL array with rows declared, is INFUR_E_INVALID_ARG.  A record (OFFSET, COUNT, VALUE, START) with lattice vertices v_0 ..
 * v_{n-1}, v_n := v_0, is a closed polygon of value V.
 * CROSSINGS.  Take a segment a -> b with y_a != y_b and each row y with min(y_a, y_b) <= y < max(y_a, y_b).  The segment crosses
 * the centre line of that row at x* = x_a + (x_b - x_a)(2y + 1 - 2 y_a) / (2 (y_b - y_a)); the CROSSING COLUMN c is the smallest x
 * with x + 1/2 >= x*: with the segment oriented so that dy > 0, c = ceil((num - dy) / (2 dy)), num = 2 x_0 dy + (x_1 - x_0)(2y + 1 -
 * 2 y_0), clamped to 0 from below; a crossing with c >= w has no effect.  Horizontal segments contribute nothing.  Centres have
 * half-integer y and vertices integer y: no vertex lies on a scan line.  The one tie, a centre exactly on a slanted segment, goes
 * to the right-hand side for every loop alike, so a border two loops share with the same vertices gives each such pixel to
 * exactly one of them.
 * SIGN.  A segment heading north (y_b < y_a) adds +1 to the winding of the pixels x >= c of that row and +V to their value sum; a
 * segment heading south adds -1 and -V.  This is Outlines' orientation: the pixel on the right hand, outer loops clockwise on a
 * y-down screen, holes counter-clockwise.
 * RESOLVE.  Pixel (x, y) then has a winding k and a value sum S modulo 2^32:
 *   OUTSIDE    k = 0 and S = 0                                  fill_value is written
 *   PAINTED    k = 1, and S <= 255 on a byte plane              S is written
 *   CONFLICT   anything else                                    fill_value is written
 * CONFLICT covers overlapping loops, a hole with no outer loop, crossed arcs, and a byte plane asked to hold more than 255.
 * Three or more loops stacked so that k = 1 again (two outer loops and a hole, say) are PAINTED with their signed value sum: that
 * is a property of the rule, not a defect.  There is no painter's order.
 * INPUT, RUNS.  `runs` holds Runs' records (START, END, VALUE), runs_rows_in of them declared, n_runs of them there.  A record
 * with START < END <= h*w and START / w == (END - 1) / w is +1, +V at START and -1, -V at END unless END is the end of its row:
 * overlapping runs are CONFLICT, deterministically, not "whichever wrote last".  Any other record is skipped and sets MALFORMED.
 * OUTPUTS, each optional (NULL = not wanted; neither wanted is INFUR_E_INVALID_ARG), neither needs initialisation; a rejected call
 * touches no output: plane_out, h*w elements, every one written; counts_out, INFUR_RASTER_COUNT_WORDS uint32_t {n_loops (for
 * runs: the number of records), PAINTED, CONFLICT, status}.  PAINTED + CONFLICT + the OUTSIDE pixels = h*w.
 * STATUS.  INFUR_RASTER_TRUNCATED: counts[0] > loops_rows_in or counts[1] > vertex_rows_in (runs: n_runs > runs_rows_in).  Only
 * counts_out is written, as {counts[0], 0, 0, INFUR_RASTER_TRUNCATED}; the plane is left alone.  INFUR_RASTER_MALFORMED: some
 * loop record had COUNT < 2 or OFFSET + COUNT > counts[1], or some run record was not a run of one row; it was skipped.
 * INFUR_RASTER_OUTSIDE: some vertex id had Y > h (X > w cannot be written as an id); it was clamped onto the lattice.  Every read
 * is clamped to the rows the caller declared: no value held in the input buffers can take a load, a store or an atomic outside
 * them, the library's scratch and the plane.
 * EXAMPLE.  The diamond (4,0) (8,4) (4,8) (0,4) of value 7 on an 8 x 8 plane, fill 0: rows 0 .. 7 are painted from column 3, 2, 1,
 * 0, 0, 1, 2, 3 up to but not including column 4, 5, 6, 7, 7, 6, 5, 4: every centre on the two left-hand sides belongs to the
 * diamond, no centre on the two right-hand sides does, PAINTED = 32 = the area.
 * COST.  8 bytes of accumulator per pixel, cleared on every call; one 64-bit atomic add per crossing (one per pixel side heading
 * north or south: scattered, one address per row and segment); one pass over the accumulator that also writes the plane.
 * WHAT IT DOES NOT DO.  No painter's order for overlapping instances, no anti-aliased coverage, no column-major COCO RLE, no frame,
 * stream, batch or group call: the input is not a product of the frame, and the stage composes through the _dev calls. */
enum { INFUR_RASTER_LOOPS = 0, INFUR_RASTER_PAINTED = 1, INFUR_RASTER_CONFLICT = 2, INFUR_RASTER_STATUS = 3, INFUR_RASTER_COUNT_WORDS = 4 };
enum { INFUR_RASTER_TRUNCATED = 1, INFUR_RASTER_MALFORMED = 2, INFUR_RASTER_OUTSIDE = 4 };
enum { INFUR_FEATURE_RASTER = 4096 };

/* host pointers, with Simplify's copy rules: counts is read first, min(counts[0], loops_rows_in) records and min(counts[1],
 * vertex_rows_in) vertices travel to the device; the plane comes back unless the status says INFUR_RASTER_TRUNCATED */
int32_t infur_raster(infur_ctx* ctx, const uint32_t* loops, uint32_t loops_rows_in, const uint32_t* vertices,
                     uint32_t vertex_rows_in, const uint32_t* counts, uint32_t h, uint32_t w, uint32_t elem_bytes,
                     uint32_t fill_value, void* plane_out, uint32_t* counts_out);
/* device pointers throughout; enqueued on the context's stream as one memset and at most 3 launches, a number fixed by the
 * arguments: the call never synchronises, so its grid is sized by loops_rows_in -- declare the rows Outlines was given, not more.
 * Capturable after one call outside the capture, which allocates the scratch: 8 bytes per pixel, owned by the context; it grows
 * only with a larger plane than any before.  The outputs must not overlap the inputs. */
int32_t infur_raster_dev(infur_ctx* ctx, const void* d_loops, uint32_t loops_rows_in, const void* d_vertices,
                         uint32_t vertex_rows_in, const void* d_counts, uint32_t h, uint32_t w, uint32_t elem_bytes,
                         uint32_t fill_value, void* d_plane_out, void* d_counts_out);
/* the runs front end, host pointers: min(n_runs, runs_rows_in) records travel to the device */
int32_t infur_raster_runs(infur_ctx* ctx, const uint32_t* runs, uint32_t runs_rows_in, uint32_t n_runs, uint32_t h, uint32_t w,
                          uint32_t elem_bytes, uint32_t fill_value, void* plane_out, uint32_t* counts_out);
/* device pointers throughout; d_n_runs is the device word Runs left (a NULL d_n_runs, or a NULL d_runs with rows declared, is
 * INFUR_E_INVALID_ARG).  One memset and at most 3 launches, the grid sized by runs_rows_in; otherwise as infur_raster_dev. */
int32_t infur_raster_runs_dev(infur_ctx* ctx, const void* d_runs, uint32_t runs_rows_in, const void* d_n_runs, uint32_t h,
                              uint32_t w, uint32_t elem_bytes, uint32_t fill_value, void* d_plane_out, void* d_counts_out);

/* ---- streaming (infur/src/main.rs:27-99,105): bounded queue, copies overlapped with compute ----
 * The reference back-pressures its producer with sync_channel(2) (main.rs:105); a stream
 * here is a ring of `depth` pinned + device slots.  submit() copies the caller's frame into a
 * pinned slot and enqueues H2D -> scale/model/decode -> D2H on three HIP streams (so frame
 * i+1's upload and frame i-1's download overlap frame i's kernels); it blocks only when all
 * `depth` slots are in flight.  collect() returns finished masks strictly in submission
 * order.  Frames are packed bgr24 exactly as `ffmpeg -f image2pipe -pix_fmt bgr24` emits them
 * (ff-video/src/decoder.rs:53-64,156-165). */
typedef struct infur_stream infur_stream;
int32_t infur_stream_create(infur_ctx* ctx, uint32_t depth, infur_stream** out);
/* Lifetime: a stream belongs to its context.  infur_ctx_destroy releases the resources of the streams still
 * alive and leaves them as empty handles (every call on them then returns INFUR_E_INVALID_ARG); such a handle
 * must still be passed to infur_stream_destroy.  Either destroy order is therefore safe. */
void infur_stream_destroy(infur_stream* st);
/* Optional second (third ...) compute lane: `other` is another context of the SAME device with a model loaded (e.g.
 * replicated by infur_group_weights_broadcast).  Frame i then runs on lane i % n: frames are independent, so the
 * kernels of consecutive frames overlap where one of them leaves CUs idle (+3..5 % frames/s with two lanes; results
 * and their order are unchanged).  Call while nothing is pending.  Either context may be destroyed first (the stream
 * is orphaned, see above). */
int32_t infur_stream_add_lane(infur_stream* st, infur_ctx* other);
/* INFUR_OK, or an error of infur_frame_advance; frame_id is returned by collect */
int32_t infur_stream_submit(infur_stream* st, const uint8_t* bgr, uint32_t w, uint32_t h, float factor,
                            uint32_t scale_mode, uint64_t frame_id);
/* number of submitted-but-not-collected frames */
uint32_t infur_stream_pending(const infur_stream* st);
/* mask dimensions and id of the oldest pending frame (no waiting), to size collect()'s buffers */
int32_t infur_stream_next_dims(const infur_stream* st, uint64_t* frame_id, uint32_t* ow, uint32_t* oh);
/* waits for the oldest pending frame.  rgba: ow*oh*4 bytes; scaled_bgr optional (ow*oh*3).
 * INFUR_E_INVALID_ARG when nothing is pending. */
int32_t infur_stream_collect(infur_stream* st, uint8_t* rgba, size_t rgba_capacity, uint8_t* scaled_bgr,
                             uint64_t* frame_id, uint32_t* ow, uint32_t* oh);

/* ---- zero-copy ingest / egress (ABI 5) ----
 * The reference's decoder fills a caller-owned, REUSED frame buffer in place (ff-video/src/decoder.rs:156-165,
 * infur/src/processing.rs:121-131); submit() / collect() above each add one pageable <-> pinned memcpy per frame instead (6.2 MB in,
 * 8.3 + 6.2 MB out at 1080p).  These four calls lend the ring's own PINNED slots to the caller:
 *   acquire   sizes the next slot for a w x h frame (scaled by `factor`) and returns its pinned input buffer, w*h*3 bytes: the
 *             producer read()s the next frame straight into it.  INFUR_E_CAPACITY when every slot is in flight (collect / release
 *             one first).  Acquiring again before commit returns the same slot, re-sized.
 *   commit    enqueues H2D -> scale / model / decode -> D2H for the acquired slot, exactly what submit() enqueues after its copy;
 *             w, h, factor must be the acquired ones.  submit() while a slot is acquired is INFUR_E_INVALID_ARG.
 *   abandon   (ABI 6) gives an acquired slot back UNCOMMITTED -- the producer hit end of input or a read error after acquiring
 *             (every pump acquires first and only then learns there is no frame).  Idempotent.  A failed acquire leaves nothing
 *             acquired, whatever was acquired before it.
 *   collect_view  waits for the oldest pending frame and returns pointers INTO its pinned output slot (mask ow*oh*4 bytes, scaled
 *             frame ow*oh*3 bytes); they stay valid -- and the slot stays out of circulation -- until
 *   release   (or a copying collect() of the same frame) gives the slot back.
 * Copying and zero-copy calls may be mixed frame by frame; results and their order are the same. */
int32_t infur_stream_acquire(infur_stream* st, uint32_t w, uint32_t h, float factor, uint8_t** bgr_slot);
int32_t infur_stream_commit(infur_stream* st, uint32_t w, uint32_t h, float factor, uint32_t scale_mode, uint64_t frame_id);
int32_t infur_stream_abandon(infur_stream* st);
int32_t infur_stream_collect_view(infur_stream* st, const uint8_t** rgba, const uint8_t** scaled_bgr, uint64_t* frame_id,
                                  uint32_t* ow, uint32_t* oh);
int32_t infur_stream_release(infur_stream* st);

/* Pinned host memory for buffers the CALLER owns and reuses (frames it decodes into, masks it displays from): the batch calls
 * (infur_batch_advance, infur_group_batch_advance, infur_batch_advance_multi) recognise such buffers and move them by DMA
 * directly -- no staging copy on either side; they return only when every frame is done, so nothing is read or written behind
 * the caller's back.  Pageable buffers keep working (staged through the ring).  Portable: usable with every device of the process. */
int32_t infur_host_alloc(size_t bytes, void** p);
int32_t infur_host_free(void* p);
uint32_t infur_host_is_pinned(const void* p); /* 1: hipHostMalloc / hipHostRegister memory */

/* ---- frame batch (BASELINE configs[3]: a batch of independent frames; across GPUs the host
 * layer gives each rank a contiguous slice, infur_amd/dist.py) ----
 * n frames through the fused path on this context, masks written in frame order.  Internally a
 * depth-3 ring, so uploads / kernels / downloads of neighbouring frames overlap.  frames[i] is
 * ws[i] x hs[i] packed BGR; rgba[i] has caps[i] bytes; ows/ohs (optional) receive mask dims. */
int32_t infur_batch_advance(infur_ctx* ctx, const uint8_t* const* frames, const uint32_t* ws,
                            const uint32_t* hs, uint32_t n, float factor, uint32_t scale_mode,
                            uint8_t* const* rgba, const size_t* caps, uint32_t* ows, uint32_t* ohs);

/* ---- several GPUs from ONE host process (BASELINE configs[3]; north_star: "a frame-batch mode shards independent
 * frames across the 8 GPUs of one node with RCCL broadcast of weights over xGMI and no cross-GPU dependence") ----
 * The reference runs all processors on one `Proc` thread of one process (infur/src/main.rs:38-40,110-112); a Rust
 * host reaches N GPUs through a GROUP: n contexts (normally one per device; several on one device are allowed),
 * one persistent worker thread per context, and -- when the contexts span >= 2 devices -- one RCCL communicator
 * over those devices (ncclCommInitAll).  Frames are independent (app.rs:107-153), so the only collective is the
 * one-off replication of the weights.  A group and its contexts are used from one thread at a time.
 * RCCL itself is resolved when the first such group is created (dlopen of librccl.so.1; INFUR_RCCL_LIB overrides the name):
 * the library does not link it, so the single-GPU entry points work on hosts without RCCL, and a group that needs it where
 * it is missing fails with INFUR_E_RCCL. */
typedef struct infur_group infur_group;
int32_t infur_group_create(infur_ctx* const* ctxs, uint32_t n_ctx, infur_group** out);
void infur_group_destroy(infur_group* g); /* the contexts stay alive and remain the caller's */
const char* infur_group_last_error(const infur_group* g);
uint32_t infur_group_size(const infur_group* g);
/* 1 when the group holds an RCCL communicator (its contexts span >= 2 devices, or INFUR_FORCE_RCCL=1 in the
 * environment: then a single-device group routes its copies through a one-rank communicator -- a test hook) */
uint32_t infur_group_uses_rccl(const infur_group* g);
/* NUMA node worker i is pinned to (the node of its GPU's PCIe root, from sysfs), or -1: every worker thread moves its slice
 * of a batch through pageable -> pinned copies, so it runs on the socket its GPU hangs off.  INFUR_NO_NUMA_PIN=1 in the
 * environment (read at infur_group_create) disables the pinning; hosts without the sysfs files are left alone. */
int32_t infur_group_worker_numa_node(const infur_group* g, uint32_t i);
/* Replicates the model loaded in context `root` (index into the group) to every other context: ONE
 * ncclBroadcast of the repacked weight arena (141 MB for FCN-ResNet50 f32) over xGMI, no
 * per-GPU re-upload or repack; contexts sharing a device with an already served one get a device-to-device copy.
 * All contexts must have been created with the same compute_dtype / winograd options (the arena layout depends
 * on them).  INFUR_E_MODEL_NOT_LOADED if `root` has no model; INFUR_E_RCCL on a collective error. */
int32_t infur_group_weights_broadcast(infur_group* g, uint32_t root);
/* infur_batch_advance over the whole group: frames [0, n) are split into contiguous slices, slice r (sizes differ
 * by at most one) runs on context r's worker thread through that context's depth-3 ring; masks land in rgba[i]
 * in frame order.  No data-path collective.  Returns the first failing context's status. */
int32_t infur_group_batch_advance(infur_group* g, const uint8_t* const* frames, const uint32_t* ws,
                                  const uint32_t* hs, uint32_t n, float factor, uint32_t scale_mode,
                                  uint8_t* const* rgba, const size_t* caps, uint32_t* ows, uint32_t* ohs);
/* One-shot forms (SURVEY section 8b's names): build a temporary group around the call.  ctxs[0] is the root.  Use a
 * persistent infur_group when calling repeatedly: communicator and thread set-up then happen once. */
int32_t infur_weights_broadcast(infur_ctx* const* ctxs, uint32_t n_ctx);
int32_t infur_batch_advance_multi(infur_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* const* frames,
                                  const uint32_t* ws, const uint32_t* hs, uint32_t n, float factor,
                                  uint32_t scale_mode, uint8_t* const* rgba, const size_t* caps,
                                  uint32_t* ows, uint32_t* ohs);

/* ---- INFUR_DTYPE_F32_SPLIT range monitor ----
 * The split mode carries every GEMM operand as an f16 pair of x * 2^k with static k (LAB_NOTES.md 3.3a): exact to
 * 22 bits while |x * 2^k| <= 65504, saturating beyond.  Every forward records the largest |activation| fed to a
 * GEMM and the largest |Winograd-domain input|; this call returns them for the last forward and whether either
 * left the exact range (the logits of that frame are then not f32-grade: re-run it on an INFUR_DTYPE_F32 context).
 * Synchronises the stream.  INFUR_E_INVALID_ARG in the other modes. */
int32_t infur_split_range(infur_ctx* ctx, float* act_amax, float* wino_amax, uint32_t* saturated);

/* ---- INFUR_DTYPE_F16_HL range monitor (ABI 7) ----
 * The three-byte mode stores every activation as an f16 hi + e5m2 lo pair, exact while |x| <= 65520; every split first clamps to
 * that range (silently: a larger value is stored as the f16 maximum, a NaN as the layer's lower bound -- 0 after a ReLU).  While the
 * monitor is on (opt-in; off by default, when every kernel runs as without it), the kernels that write three-byte tensors record what
 * their splits saw, ACCUMULATED over every forward of the context since it was enabled or last read: the largest |activation| (a
 * ReLU layer's max(x, 0); the f32 logits are not split and not included), the largest |Winograd-domain input| (unscaled), whether
 * any value was changed by the upper clamp, and whether any split received a NaN (+inf counts as saturation).  Read after each
 * infur_frame_advance for per-frame values, after a batch / ring for all its frames; a frame that saturated is not f16hl-grade:
 * re-run it on an INFUR_DTYPE_F32 or INFUR_DTYPE_F32_SPLIT context.  Each lane of a stream / member of a group is queried on its own.
 *   infur_hl_monitor_enable: INFUR_E_INVALID_ARG (nothing changed) unless compute_dtype is INFUR_DTYPE_F16_HL; enabling allocates
 *     and zeroes the monitor's words; switching drops the context's cached graphs.
 *   infur_hl_range: INFUR_E_INVALID_ARG while the monitor is off.  Synchronises the stream, returns the values and queues their
 *     clear on the stream.  Any out-pointer may be NULL.  A quantised model (or none) reads zeros. */
int32_t infur_hl_monitor_enable(infur_ctx* ctx, uint32_t on);
int32_t infur_hl_range(infur_ctx* ctx, float* act_amax, float* wino_amax, uint32_t* saturated, uint32_t* nan_seen);

/* ---- tuning database (tile configuration per conv shape, see options.no_autotune) ----
 * Text form: one line per shape, 13 shape integers + the configuration index.  Importing a
 * database makes the kernel mix reproducible from run to run and skips the trial launches of
 * the first frame; shapes it does not list are still measured on first use.  Results never
 * depend on it (all configurations are bit-identical). */
int32_t infur_tune_export(infur_ctx* ctx, char* buf, size_t cap, size_t* len);
int32_t infur_tune_import(infur_ctx* ctx, const char* text, size_t len);

/* ---- profiling (options.profile = 1) ---- */
/* switch per-kernel event recording on/off at run time (e.g. only for the last frame of a timed run) */
int32_t infur_profile_enable(infur_ctx* ctx, uint32_t on);
/* number of kernel records of the last advance (synchronises the stream) */
int32_t infur_profile_count(infur_ctx* ctx, uint32_t* n);
int32_t infur_profile_get(infur_ctx* ctx, uint32_t i, infur_kernel_record* rec);
/* debug (additive, no ABI change): which of a configuration's size-picked kernels ran for record i of the last advance, as a short
 * NUL-terminated tag ("bm256", "nsplit4", "bn128,mixed,na2", "lds", "form3,dma2", "f32stem"); "" where the launch has one form.
 * The record's `kernel` names the configuration, this names the kernel inside it.  INFUR_E_CAPACITY when cap is too small (24 is
 * always enough), INFUR_E_INVALID_ARG for i >= infur_profile_count. */
int32_t infur_debug_profile_variant(infur_ctx* ctx, uint32_t i, char* buf, size_t cap);

/* ---- device memory helpers for bindings without a HIP runtime of their own ----
 * Device pointers passed to any *_dev entry point need only the natural alignment of their element type (1 byte for frames, byte
 * planes and masks' sources, 4 for f32 tensors and RGBA words, 8 for the statistics table): no call requires more. */
int32_t infur_dev_alloc(infur_ctx* ctx, size_t bytes, void** d_ptr);
int32_t infur_dev_free(infur_ctx* ctx, void* d_ptr);
int32_t infur_memcpy_h2d(infur_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int32_t infur_memcpy_d2h(infur_ctx* ctx, void* dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* INFUR_HIP_H */
