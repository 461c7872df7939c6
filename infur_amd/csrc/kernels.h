// Internal launcher interface between the host runtime (infur_capi.cpp) and the
// gfx950 kernels.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_forms.h"

namespace infur {

// NHWC activations (f32 or f16); weights OHWI ([Cout][KH][KW][Cin], K contiguous per output
// channel) in the same element type; bias always f32.
struct ConvArgs {
    const void* in;     // [H][W][Cin]
    const void* wt;     // [Cout][KH*KW*Cin]
    const float* bias;  // [Cout], may be null (no bias)
    const void* res;    // optional residual, same shape and type as the input activations
    void* out;          // [OH][OW][Cout]
    int H, W, Cin;
    int OH, OW, Cout;
    int KH, KW, stride, pad, dil;
    int relu;
    // batched use (Winograd-domain GEMMs): `batch` independent problems of the same shape,
    // operand b starts at base + b * stride (bytes).  batch <= 1: plain convolution.
    int batch = 1;
    size_t in_bs = 0, wt_bs = 0, out_bs = 0;
    // mode 2 (f32 split into f16 pairs) only: activations are multiplied by a_scale (a power of two
    // that centres them in the f16 range) while they are staged, the weights were scaled and split at
    // load time (launch_split_weights), and the accumulators are multiplied by acc_scale =
    // 1 / (a_scale * weight scale) before bias / residual / ReLU.  Powers of two: exact.
    float a_scale = 1.0f, acc_scale = 1.0f;
    // batched use in the split modes: one accumulator scale PER PROBLEM (device array of `batch` floats) instead of acc_scale --
    // the (m+2)^2 Winograd-domain weight planes differ by orders of magnitude (G's entries run from 1/180 to 1), so each
    // plane is scaled into the f16 pair's range on its own
    const float* acc_scale_b = nullptr;
    // mode 2, optional: atomicMax target (bit pattern of a non-negative float) for max |output| of this launch --
    // the range monitor of the split mode (infur_split_range)
    unsigned* amax = nullptr;
    // mode 4 (quantised models: u8 activations, s8 weights, exact i32 accumulation on v_mfma_i32_32x32x32_i8): the requantisation
    // of ONNX QLinearConv in the epilogue -- y = sat_u8(round(f32(acc + q_bias[o]) * q_mult[o]) + q_yzp) -- then, with `res`, the
    // com.microsoft QLinearAdd of the residual sum -- c = sat_u8(round(f32(y - q_yzp) * q_ra + f32(res - q_bzp) * q_rb) + q_czp)
    // -- and, for an f32 output (the logits), DequantizeLinear: f32(y - q_yzp) * q_dq.  q_bias already holds the operator's
    // bias + (128 - x_zp) * sum_k w[o][k]: the kernel feeds the MFMA x - 128 (one XOR per fragment; an out-of-range tap loads 0,
    // i.e. x = 0 = the zero point of every padded tensor).
    const float* q_mult = nullptr;
    const int32_t* q_bias = nullptr;
    int q_yzp = 0, q_bzp = 0, q_czp = 0;
    float q_ra = 0.f, q_rb = 0.f, q_dq = 0.f;
    // f32 output: (y - q_yzp + q_dq_off) * q_dq.  DequantizeLinear: off 0, dq = y_scale; the codes themselves (models that Resize
    // before they dequantise): off = q_yzp, dq = 1
    float q_dq_off = 0.f;
    // two-source 1x1 GEMM (a bottleneck's conv3 and its downsample branch as ONE launch, no residual tensor):
    // out = W[:, :Cin] * in  +  W[:, Cin:] * in2(stride2)  + bias.  in2 == nullptr: ordinary convolution.
    // Requires KH = KW = 1, pad = 0, stride = 1; wt rows are Cin + Cin2 long; OH x OW = ceil(H2/stride2) x ...
    const void* in2 = nullptr;  // [H2][W2][Cin2]
    int H2 = 0, W2 = 0, Cin2 = 0, stride2 = 1;
    // mode 5 (INFUR_DTYPE_F16_HL, conv_hl.hip): every tensor is an f16 hi plane (in / wt / res / out above) plus an e5m2 lo plane of
    // the same shape (hl_format.h); batched use: lo plane b starts at base + b * (in_bs / 2).  out_f32 launches write plain f32.
    const void* in_lo = nullptr;
    const void* wt_lo = nullptr;
    const void* res_lo = nullptr;
    void* out_lo = nullptr;
    const void* in2_lo = nullptr;
    // mode 5, optional: the range monitor's device words (hl_format.h: kHlMon*) -- non-null selects the monitored form of the epilogue
    // (hi / lo output only; an f32 output is never split)
    unsigned* hl_mon = nullptr;
};

// conv as implicit GEMM on the matrix cores in one of the arithmetic modes of conv_forms.h (ConvMode; also ConvCfg and the table of forms).
// cfg: a configuration that conv_igemm_config_valid admits for the launch (what pick_cfg returns).  Every configuration of a mode
// produces bit-identical results; only the speed differs.
hipError_t launch_conv_igemm(const ConvArgs& a, ConvMode mode, int out_f32, int cfg, hipStream_t s);
ConvCfg conv_igemm_default_config(const ConvArgs& a);  // the configuration of a shape nobody has measured
bool conv_igemm_config_valid(const ConvArgs& a, int cfg, ConvMode mode, int out_f32);
const char* conv_igemm_config_name(int cfg, ConvMode mode);
// The sub-form of configuration `cfg` that launch_conv_igemm runs for this launch, as a short static tag of conv_forms.h's
// kVariantWords ("bm256", "nsplit4", "bn128,mixed,na2"); "" where the configuration has one form.  Evaluates the launchers' own
// selectors (size rules of conv_forms.h and their environment hooks), so it says what runs, whatever the reason.
const char* conv_variant_name(const ConvArgs& a, ConvMode mode, int cfg, int out_f32);

// mode 5 (conv_hl.hip)
bool conv_hl_config_valid(const ConvArgs& a, const ConvForm& f, int out_f32);  // f: a kFamHL / kFamHLAreg row
hipError_t launch_conv_hl(const ConvArgs& a, int out_f32, int cfg, hipStream_t s);
bool conv_hl_pipe_on();  // false under INFUR_HL_PIPE=0 (the plain K loop): conv_igemm_config_name then ends the tiled forms' names in ",plain"
// kCfgAreg of mode 5 (conv_hl_areg.hip): 1x1 expansions (Cin 64 / 128 / 256, Cout a multiple of 128) with the activation
// fragment in registers, weights and residual streamed by LDS-DMA; bit-identical to the tiled forms
bool conv_hl_areg_valid(const ConvArgs& a, int out_f32);
hipError_t launch_conv_hl_areg(const ConvArgs& a, hipStream_t s);
// weights of mode 5, one-off at load: f32 [n] (kernel K order) * scale -> f16 hi [n], e5m2 lo [n] (n % 4 == 0)
hipError_t launch_hl_pack_weights(const float* w, size_t rows, size_t cols, float scale, void* hi, void* lo, hipStream_t s);  // K-block-major planes
hipError_t launch_hl_pack_weights_planes(const float* w, size_t rows, size_t cols, int planes, const float* scales, void* hi, void* lo, hipStream_t s);  // <= 64 planes back to back, one launch

// 1x1 convolution with Cin in {64, 128, 256}, f16 operands (mode 1), f16 output: the activation tile stays in registers
// while the workgroup walks all N tiles (conv1x1_areg.hip).  Reached through launch_conv_igemm as one more configuration.
bool conv1x1_areg_valid(const ConvArgs& a, int mode, int out_f32);
hipError_t launch_conv1x1_areg(const ConvArgs& a, hipStream_t s);
const char* conv1x1_areg_variant(const ConvArgs& a);  // "bm128" / "bm256": the workgroup's pixels
// quantised models (mode 4, u8 output): activation tile in registers, 16 consecutive channels per lane straight from the
// accumulators (conv1x1_q8.hip): kCfgAreg in that mode
bool conv1x1_q8_valid(const ConvArgs& a, int mode, int out_f32);
hipError_t launch_conv1x1_q8(const ConvArgs& a, int nsplit, hipStream_t s);
const char* conv1x1_q8_variant(const ConvArgs& a);  // "nsplit<conv1x1_q8_nsplit>"
int conv1x1_q8_nsplit(const ConvArgs& a);  // kCfgAregNsplit: N tiles shared out over this many workgroups per M tile (0: not a candidate)

// stride-1 3x3 convolutions (pad = dilation 1 / 2 / 4), f16 operands and output, no residual: the input patch of a 16 x 16 output
// tile stays in LDS for all nine taps (conv3x3_halo.hip).  kCfgHalo128, kCfgHalo256 and kCfgHalo4 (the 4-wave form) of kModeF16.
bool conv3x3_halo_valid(const ConvArgs& a, int mode, int out_f32, int bn);
hipError_t launch_conv3x3_halo(const ConvArgs& a, int bn, hipStream_t s);
// the same kernel on the quantised model's tensors (mode 4, u8 out): kCfgHalo128 / kCfgHalo256 of that mode
hipError_t launch_conv3x3_halo_q(const ConvArgs& a, int bn, hipStream_t s);
// the 4-wave form (kCfgHalo4): BN = 256, one wave per SIMD with a 128 x 128 wave tile, dilation 1 / 2
bool conv3x3_halo4_valid(const ConvArgs& a, int mode, int out_f32);
hipError_t launch_conv3x3_halo4(const ConvArgs& a, hipStream_t s);
// N tile, tiling of the map and patch images of a launch the functions above take ("bn64,16x16,na1"); mode: 1 or 4
const char* conv3x3_halo_variant(const ConvArgs& a, int mode, int bn);
const char* conv3x3_halo4_variant(const ConvArgs& a);

// Two 1x1 convolutions back to back on the same pixels, f16 (conv1x1_b2b.hip): y = ReLU(w3 * in + b3 + res) -- a
// bottleneck's conv3 + residual -- is written once and immediately multiplied by the NEXT bottleneck's conv1 weights:
// out2 = ReLU(w1 * y + b1).  C2 = channels of `in` = channels of out2 (128 or 256); y and res have 4 * C2 channels.
// Bit-identical to the two launches it replaces.
struct B2bArgs {
    const void* in;    // [M][C2] f16
    const void* w3;    // [4*C2][C2] f16 in the step-interleaved row order of launch_b2b_pack_w3
    const float* b3;   // [4*C2]
    const void* res;   // [M][4*C2] f16
    void* y;           // [M][4*C2] f16
    const void* w1;    // [C2][4*C2] f16
    const float* b1;   // [C2]
    void* out2;        // [M][C2] f16
    int M, C2, relu1, relu2;
};
bool conv1x1_b2b_valid(const B2bArgs& a);
// one-off at model load: the conv3 weight matrix ([4*C2][C2] f16, plain row order) in the row order the kernel streams
hipError_t launch_b2b_pack_w3(const void* w3, void* w3i, int C2, hipStream_t s);
hipError_t launch_conv1x1_b2b(const B2bArgs& a, hipStream_t s);
const char* conv1x1_b2b_variant(const B2bArgs& a);  // workgroup form and DMA phase ("form3,dma2")

// Winograd F(mt x mt, 3x3), mt = 2 or 4, for stride-1 3x3 convs (f32, any dilation d with pad = d);
// (mt+2)^2 transform planes; see winograd.hip
int wino_num_tiles(int H, int W, int d, int mt);
// amax (optional): atomicMax target for max |V| / max |out| (range monitor of the split mode)
hipError_t launch_wino_input(const float* in, int H, int W, int C, int d, int mt, float* V, unsigned* amax, hipStream_t s);
hipError_t launch_wino_output(const float* M, int H, int W, int Cout, int d, int mt, const float* bias, int relu,
                              float* out, unsigned* amax, hipStream_t s);
hipError_t launch_wino_weights(const float* w_oihw, int O, int I, int mt, float* U, hipStream_t s);
// the form of launch_wino_input (C = Cin) / launch_wino_output (C = Cout): "lds", "f32x1", "f32x2", "f32x4w"
const char* wino_variant(int C, int mt);
// the same transforms on three-byte tensors (mode 5; C, Cout % 128 == 0): input hi / lo planes -> V * v_scale as hi / lo planes
// [(mt+2)^2][T][C]; f32 M -> the conv's output as hi / lo planes.  hl_mon (optional): the range monitor's words (hl_format.h), the
// monitored form of the kernel -- max |V * v_scale| to [kHlMonWino], max |out| to [kHlMonAct]
hipError_t launch_wino_input_hl(const void* in_hi, const void* in_lo, int H, int W, int C, int d, int mt, float v_scale, void* V_hi, void* V_lo,
                                unsigned* hl_mon, hipStream_t s);
hipError_t launch_wino_output_hl(const float* M, int H, int W, int Cout, int d, int mt, const float* bias, int relu, void* out_hi, void* out_lo,
                                 unsigned* hl_mon, hipStream_t s);

// three-byte tensors (hl_format.h): the lo plane of an [elems] tensor starts hl_lo_offset(elems) bytes after the hi plane
__host__ __device__ inline size_t hl_lo_offset(size_t elems) { return (elems * 2 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t hl_tensor_bytes(size_t elems) { return hl_lo_offset(elems) + ((elems + 255) & ~(size_t)255); }
// f32 [n] -> hi / lo planes (n % 8 == 0; hl_mon: optional range monitor words, max |in| to [kHlMonAct]); NHWC hi / lo planes ->
// planar f32 [C][H][W] (read-back)
hipError_t launch_hl_from_f32(const float* in, size_t n, void* hi, void* lo, unsigned* hl_mon, hipStream_t s);
hipError_t launch_hl_nhwc_to_planar(const void* hi, const void* lo, int H, int W, int C, float* out, hipStream_t s);

// stem: packed BGR u8 -> (LUT normalise, BGR->RGB) -> conv 7x7/2 pad 3 (3->64) + bias + ReLU,
// NHWC out (f32, or f16 when f16 != 0; the arithmetic is f32 either way).
// wt: [7][7][3][64] (ky,kx,c,cout) f32, lut: [3][256] in RGB order.
hipError_t launch_stem_conv7x7(const uint8_t* bgr, int H, int W, const float* wt,
                               const float* bias, const float* lut, void* out, int f16, int OH, int OW,
                               hipStream_t s);

// stem + maxpool 3x3/2 pad 1 in one kernel: out = pooled [PH][PW][64]; the SH x SW stem tensor is never written.
// mode 0: exact f32 MFMA, bit-identical to launch_stem_conv7x7 -> launch_maxpool3x3s2 (f32 out).  mode 1 (f16 out): f16
// operands on the f16 MFMA.  mode 2 (f32 out): operands as f16 hi + lo pairs of value * a_scale / weight * w_scale (powers
// of two), three MFMAs per product, f32-grade.
// quantised model: QuantizeLinear + QLinearConv 7x7/2 + u8 max-pool in one launch, exact on the f16 MFMA (stem_pool.hip).
// wt: [147][64] f32 = the s8 weights, k = (ky * 7 + kx) * 3 + c; lut: [3][256] f32 = q - x_zp (RGB order); out: [PH][PW][128] u8
hipError_t launch_stem_pool_q(const uint8_t* bgr, int H, int W, const void* wimg, const float* lut, const int32_t* q_bias, const float* q_mult,
                              int y_zp, uint8_t* out, int cstride, int SH, int SW, int PH, int PW, hipStream_t s);
// the f16-rate stems' weights as their finished LDS image (f16 hi (, lo) planes, pads zero), built once per model from wt[147][64] f32
size_t stem16_image_bytes();
hipError_t launch_stem16_pack(const float* wt, float w_scale, int split, void* img, hipStream_t s);
hipError_t launch_stem_pool(const uint8_t* bgr, int H, int W, const float* wt, const void* wimg, const float* bias, const float* lut, void* out,
                            int mode, int SH, int SW, int PH, int PW, float a_scale, float w_scale, unsigned* amax, hipStream_t s);
const char* stem_pool_variant(int mode);  // "f16stem" / "f32stem" (INFUR_STEM_F32=1: the f32 MFMA stem in modes 1 and 2 as well)

// maxpool 3x3 stride 2 pad 1, NHWC f32 / f16 (C % 4 == 0)
hipError_t launch_maxpool3x3s2(const void* in, int H, int W, int C, void* out, int f16, int OH, int OW,
                               unsigned* amax, hipStream_t s);

// OIHW f32 -> OHWI f32 / f16 weight repack (one-off at model load)
hipError_t launch_repack_oihw_to_ohwi(const float* src, void* dst, int f16, int O, int I, int KH, int KW,
                                      hipStream_t s);
// mode 2 weight preparation (one-off at model load).  absmax: *out = max |w[i]| (out must be zeroed).
// split: in place, every 32 consecutive f32 (one 128-byte K-step row chunk) become
// [32 x f16 hi][32 x f16 lo] of w * scale, hi = rne(w*scale), lo = rne(w*scale - hi).
hipError_t launch_absmax(const float* w, size_t n, float* out, hipStream_t s);
// out[p] = max |plane p| for `planes` tensors of `per` elements back to back, one launch (out must be zeroed)
hipError_t launch_absmax_planes(const float* w, size_t per, int planes, float* out, hipStream_t s);
// fp8_cross: the [f16 hi][e5m2 lo * 2^11][e5m2 hi] row form of conv_igemm mode 3 instead of [f16 hi][f16 lo]
hipError_t launch_split_weights(float* w, size_t n, float scale, int fp8_cross, hipStream_t s);
// two-source GEMM weights (one-off at load): out[r] = a[r] ++ b[r] for `rows` rows of a_bytes / b_bytes
// (multiples of 16); sum[i] = x[i] + y[i]
hipError_t launch_concat_rows(const void* a, size_t a_bytes, const void* b, size_t b_bytes, void* out, int rows, hipStream_t s);
hipError_t launch_add_f32(const float* x, const float* y, float* sum, int n, hipStream_t s);
// OIHW (O=64,I=3,7x7) -> [ky][kx][c][o] for the stem kernel
// reverse_c: the kernels read a pixel's channels as (p[2], p[1], p[0]); a model whose channel 0 is B (Uint8 input:
// BGR kept, predict_onnx.rs:296-301) gets its stem weights stored with the input-channel axis reversed instead
hipError_t launch_repack_stem(const float* src, float* dst, int reverse_c, hipStream_t s);

// ---- quantised models (quant.hip) ----
// stem: packed BGR u8 frame -> QuantizeLinear of the normalised image through a [3][256] u8 table (RGB order; out-of-frame
// taps take x_zp) -> QLinearConv 7x7/2 pad 3 (wq: [64][7][7] dwords = (r, g, b, 0) s8; q_bias / q_mult per channel) -> u8
// NHWC [SH][SW][64]
hipError_t launch_stem_q(const uint8_t* bgr, int H, int W, const uint8_t* qlut, int x_zp, const int32_t* wq, const int32_t* q_bias,
                         const float* q_mult, int y_zp, uint8_t* out, int SH, int SW, hipStream_t s);
// max-pool 3x3/2 pad 1 on u8 NHWC [H][W][C] -> [OH][OW][CP] (CP >= C: channels C..CP-1 are written as 0; C, CP % 16 == 0)
hipError_t launch_maxpool_q(const uint8_t* in, int H, int W, int C, uint8_t* out, int OH, int OW, int CP, hipStream_t s);
// OIHW s8 -> OHWI s8 with the input-channel axis zero-padded to IP and `OP - O` zero rows appended; also sums every row
// (wsum[o] = sum_k w[o][k], i32; rows O..OP-1: 0)
hipError_t launch_repack_q(const int8_t* src, int8_t* dst, int32_t* wsum, int O, int I, int KH, int KW, int OP, int IP, hipStream_t s);
// u8 NHWC -> planar f32 [C][H][W] (debug read-back of a quantised activation: the byte values)
hipError_t launch_u8_nhwc_to_planar(const uint8_t* in, int H, int W, int C, float* out, hipStream_t s);

// Scale: packed BGR u8 resize.  mode 0 nearest, 1 bilinear (definitions: oracle/infur_oracle.c)
hipError_t launch_scale_bgr(const uint8_t* in, int W, int H, uint8_t* out, int OW, int OH,
                            int mode, hipStream_t s);

// pre-proc only (used when the stem is not fused): BGR u8 HWC -> RGB f32 CHW via LUT
hipError_t launch_pack_normalize(const uint8_t* bgr, int W, int H, const float* lut, float* chw,
                                 hipStream_t s);

// display conversion (app.rs:132-144): packed BGR -> [r,g,b,255]
hipError_t launch_bgr_to_rgba(const uint8_t* bgr, int W, int H, uint32_t* rgba, hipStream_t s);

// NHWC (f32 or f16) -> planar f32 [C][H][W] (low-res logits, debug activation read-back)
hipError_t launch_nhwc_to_planar(const void* in, int f16, int H, int W, int C, float* out,
                                 hipStream_t s);

// quantised models that Resize their u8 logits before DequantizeLinear (prepost.hip: up_post): the low-res tensor holds the
// codes, every interpolated value v becomes (trunc(v) - zp) * scale.  on == 0: plain float interpolation.
struct UpQuant {
    int on = 0;
    float zp = 0.f, scale = 1.f;
};

// bilinear up-sample (ONNX Resize linear / pytorch_half_pixel) of NHWC low-res logits to
// planar [K][OH][OW] f32
hipError_t launch_upsample_planar(const float* low, int LH, int LW, int K, float* out, int OH,
                                  int OW, hipStream_t s, const UpQuant uq = UpQuant());

// ColorCode over planar [K][H][W] f32 -> premultiplied RGBA8.  lut: [20][256] uchar4
hipError_t launch_colorcode_planar(const float* khw, int K, int H, int W, const uint32_t* lut,
                                   uint32_t* rgba, hipStream_t s);

// fused: bilinear up-sample of NHWC low-res logits + argmax + shade -> RGBA8; never
// materialises the full-resolution logits.  Bit-identical to upsample_planar -> colorcode.
hipError_t launch_upsample_argmax_shade(const float* low, int LH, int LW, int K,
                                        const uint32_t* lut, uint32_t* rgba, int OH, int OW,
                                        hipStream_t s, const UpQuant uq = UpQuant());

// Segments (prepost.hip): ColorCode's sibling -- class byte, confidence byte, RGBA shaded by that confidence and per-class
// statistics, any subset (null = not wanted).  softmax: 0 = INFUR_DECODE_RAW, 1 = INFUR_DECODE_SOFTMAX.
// shards: kSegShards zeroed tables [K][8] u64 the kernels accumulate into; launch_segments_stats_finalize folds them into
// the caller's K x INFUR_STAT_WORDS table (which needs no initialisation).  K <= kSegMaxClasses.
constexpr int kSegShards = 16, kSegMaxClasses = 256;
constexpr size_t kSegShardBytes = (size_t)kSegShards * kSegMaxClasses * 8 * sizeof(unsigned long long);
struct SegOut {
    uint8_t* klass = nullptr;
    uint8_t* conf = nullptr;
    uint32_t* rgba = nullptr;
    unsigned long long* shards = nullptr;
};
// unfused, over planar [K][H][W] f32
hipError_t launch_segments_planar(const float* khw, int K, int H, int W, int softmax, const uint32_t* lut, const SegOut& o,
                                  hipStream_t s);
// fused with the bilinear up-sample of the NHWC low-res logits; bit-identical to upsample_planar -> segments_planar
hipError_t launch_upsample_argmax_segments(const float* low, int LH, int LW, int K, int softmax, const uint32_t* lut,
                                           const SegOut& o, int OH, int OW, hipStream_t s, const UpQuant uq = UpQuant());
hipError_t launch_segments_stats_finalize(const unsigned long long* shards, int K, unsigned long long* stats, hipStream_t s);

// Regions (regions.hip): connected components of a class plane -- u32 label plane, rows x kRegWords u64 table, region count
// (each optional; d_n is a device word).  scratch: regions_scratch_bytes(H * W) bytes the launches own for the call.
// conn8: 0 = 4-connectivity.  Stream-ordered; no workgroup waits for another.  H * W in [1, 2^32 - 2].
constexpr int kRegWords = 10;
size_t regions_scratch_bytes(size_t npix);
hipError_t launch_regions(const uint8_t* klass, const uint8_t* conf, unsigned H, unsigned W, int conn8, unsigned min_pixels, int skip_bg,
                          void* scratch, unsigned* labels, unsigned long long* table, unsigned rows, unsigned* d_n, hipStream_t s);

// Tracks (tracks.hip): region identities from frame to frame.  Everything a tracker remembers lives on the device: the scalars
// in TrkState, the arrays in TrkMem (M = max_regions entries each; keys / cnts: `slots` entries, a power of two; prev: the
// remembered label plane, at least H * W words).  The step reads *d_n on the device and is stream-ordered throughout.
constexpr int kTrkWords = 8;
constexpr unsigned kTrkTruncated = 1, kTrkOverflow = 2, kTrkExhausted = 4;
struct TrkState {
    unsigned next_id, frame, valid, ph, pw, pT;             // across steps: id and frame counters, the remembered frame's shape
    unsigned T, nrows, trunc, fresh, R, exhausted, base;    // of the running step
};
struct TrkMem {
    TrkState* st;
    unsigned long long* keys;  // pair table: (c << 32) | p, all ones = empty
    unsigned* cnts;            //             overlap pixels of the pair
    unsigned long long *best, *claim;      // per current / per remembered region: (overlap << 32) | (0xFFFFFFFF - partner)
    unsigned long long *ppix, *psx, *psy;  // remembered regions: PIXELS, SUM_X, SUM_Y
    unsigned *pclass, *ptrack, *page, *pborn;
    unsigned *ctrack, *cage, *cborn;  // current regions, until the save launch
    unsigned* partial;                // block sums of the scan: M / kScanBlock + 1 words (wave_scan.h)
    unsigned* prev;
    unsigned slots, M;
};
// one step on an H x W plane, H * W in [1, 2^32 - 2]; outputs optional
hipError_t launch_tracks(const TrkMem& m, const unsigned* labels, const unsigned long long* table, unsigned rows, const unsigned* d_n, unsigned H,
                         unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane, unsigned long long* track_table,
                         unsigned* summary, hipStream_t s);
// forget the remembered frame; step: advance the frame counter (an empty frame); set_id: next_id = first_id; summary (optional) zeroed
hipError_t launch_tracks_forget(TrkState* st, int step, int set_id, unsigned first_id, unsigned* summary, hipStream_t s);

// Tracks' memory (tracks.hip, DESIGN 4c'): a gallery of lost tracks, an allocation of its own made by infur_tracker_set_memory.
// The gallery is a list of at most G entries in structure-of-arrays form, held twice: a step compacts buf[cur] into
// buf[cur ^ 1] and its last launch flips cur.
constexpr int kLostWords = 12;
constexpr unsigned kTrkGalleryFull = 8;
struct TrkGalState {
    unsigned held, cur, T;                        // across steps: entries in buf[cur]; the last step's tracked regions
    unsigned revived, ended, drop, new_held;      // of the running step
    unsigned sum[4];                              // the last step's memory summary: REVIVED, LOST, EXPIRED, HELD
};
struct TrkLost {
    unsigned long long *pix, *sx, *sy;
    unsigned *id, *age, *born, *klass, *x0, *y0, *x1, *y1, *seen;
};
struct TrkGal {
    TrkGalState* gs;
    TrkLost buf[2];
    unsigned *px0, *py0, *px1, *py1;     // remembered regions: bounding box (M words each)
    unsigned* cgap;                      // current regions: gap_of_region
    unsigned long long *rbest, *rclaim;  // per current region / per entry: (score << 32) | (0xFFFFFFFF - partner)
    unsigned *rpart, *gpart;             // block sums: revived regions (as TrkMem::partial); the gallery scan over G + M flags
    unsigned max_lost, reach, G;
};
// launch_tracks on a tracker with memory: the same step, with the revival launches between keep and assign and the gallery
// update before save.  g.gs is zeroed by whoever allocates it
hipError_t launch_tracks_memory(const TrkMem& m, const TrkGal& g, const unsigned* labels, const unsigned long long* table, unsigned rows,
                                const unsigned* d_n, unsigned H, unsigned W, unsigned min_overlap, unsigned* track_of_region, unsigned* track_plane,
                                unsigned long long* track_table, unsigned* summary, hipStream_t s);
// empty the gallery (reset, empty frame): the memory summary reads all zero, gap_of_region too
hipError_t launch_tracks_memory_forget(const TrkGal& g, hipStream_t s);
// what the last step left, each output optional: gap_of_region[rows], memory summary[4], the first min(HELD, lost_rows) entries
hipError_t launch_tracks_memory_read(const TrkGal& g, unsigned* gap_of_region, unsigned rows, unsigned* memory_summary,
                                     unsigned long long* lost_table, unsigned lost_rows, hipStream_t s);

// Runs (runs.hip): an H x W plane of 1- or 4-byte elements as raster-ordered runs -- rows x kRunWords u32 records (START, END,
// VALUE), the per-row index row_start[H + 1] and the count (each optional; d_n is a device word).  skip: runs of skip_value are
// neither emitted nor counted.  scratch: runs_scratch_bytes(H * W) bytes the launches own for the call.  Stream-ordered; no
// workgroup waits for another.  H * W in [1, 2^32 - 2].
constexpr int kRunWords = 3;
size_t runs_scratch_bytes(size_t npix);
hipError_t launch_runs(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, void* scratch, unsigned* runs,
                       unsigned rows, unsigned* row_start, unsigned* d_n, hipStream_t s);

// Anchors (anchors.hip): the exact squared Euclidean distance transform by value of an H x W plane (both at most 65535) of 1- or
// 4-byte elements, the frame counting as a differing value -- dist2[H * W] u32 -- and per value v < rows the pixel of largest dist2,
// ties to the smallest index -- anchors[rows x kAnchorWords] u32 (PIXEL, DIST2), (0xFFFFFFFF, 0) where no pixel holds v (each
// optional; device memory; every one of the rows is written).  skip: pixels of skip_value belong to no region and read dist2 = 0.
// scratch: anchors_scratch_bytes(H * W, rows) bytes the launches own for the call.  Stream-ordered; one memset and three launches,
// no workgroup waits for another.  H * W == 0 writes the NONE rows and needs no scratch.
constexpr int kAnchorWords = 2;
size_t anchors_scratch_bytes(size_t npix, unsigned rows);
hipError_t launch_anchors(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, void* scratch, unsigned* dist2,
                          unsigned* anchors, unsigned rows, hipStream_t s);

// Compare (compare.hip): two H x W planes (both sides at most 65535) of 1- or 4-byte elements against each other.  A pixel whose
// a equals ignore_a (ign_a set) or whose b equals ignore_b (ign_b set) is ignored; a compared pixel with a >= rows_a or
// b >= rows_b is outside; the rest are inside.  matrix[rows_a x rows_b] u32 counts the inside pixels per (a, b); rows_a_out and
// rows_b_out hold kCompareWords u32 per value (PIXELS, PARTNER, INTER, UNION), (0, 0xFFFFFFFF, 0, 0) where no inside pixel holds
// it; counts[kCompareCountWords] = {COMPARED, EQUAL, IGNORED, OUTSIDE, PAIRS, MATCHED, RUNS, STATUS} (each optional; device
// memory; everything wanted is written in full).  compare_dense(rows_a, rows_b) says which form runs: the matrix in LDS, or an
// open-addressing pair table of pair_slots slots (a power of two >= 64; kCmpOverflow in STATUS when 2 * RUNS exceeds it: then
// no partner is reported and PIXELS, the matrix and the other counts are still exact).  scratch: compare_scratch_bytes(..)
// bytes the launches own for the call.  Stream-ordered; dense: one memset and four launches, table: two memsets (three with a
// matrix) and five launches, one launch fewer without counts; no workgroup waits for another.  H * W == 0 writes zeros and
// NONE rows and needs no scratch.
constexpr int kCompareWords = 4;
constexpr int kCompareCountWords = 8;
constexpr unsigned kCmpDenseMax = 4096;
constexpr unsigned kCmpOverflow = 1u, kCmpTable = 2u;
bool compare_dense(unsigned rows_a, unsigned rows_b);
size_t compare_scratch_bytes(unsigned rows_a, unsigned rows_b, unsigned pair_slots);
hipError_t launch_compare(const void* a, int elem_a, const void* b, int elem_b, unsigned H, unsigned W, int ign_a, unsigned ignore_a, int ign_b,
                          unsigned ignore_b, unsigned rows_a, unsigned rows_b, void* scratch, unsigned pair_slots, unsigned* matrix, unsigned* rows_a_out,
                          unsigned* rows_b_out, unsigned* counts, hipStream_t s);

// Adjacency (sieve.hip): which values of an H x W plane (H * W below 2^31) of 1- or 4-byte elements touch, and along how many pixel
// edges.  A pixel is inside when its value is below `rows` and is not skip_value (skip set).  pairs: pair_rows x kAdjPairWords u32
// (A, B, BORDER, FIRST) in ascending FIRST, min(PAIRS, pair_rows) of them; rows_out: rows x kAdjRowWords u32 (DEGREE, LONGEST,
// BORDER, PERIMETER); counts[kAdjCountWords] = {PAIRS, EDGES, SKIPPED, OUTSIDE, RUNS, WRITTEN, 0, STATUS} (each optional; device
// memory).  pair_slots: a power of two >= 64; 2 * RUNS above it sets kAdjOverflow: no record, rows (0, NONE, 0, PERIMETER).
// scratch: adjacency_scratch_bytes(..) bytes the launches own for the call (want_pairs: pairs wanted with pair_rows > 0).
// Stream-ordered; two memsets and at most nine launches; no workgroup waits for another.
constexpr int kAdjPairWords = 4;
constexpr int kAdjRowWords = 4;
constexpr int kAdjCountWords = 8;
constexpr unsigned kAdjOverflow = 1u, kAdjTruncated = 2u;
size_t adjacency_scratch_bytes(size_t npix, unsigned rows, unsigned pair_slots, bool want_rows, bool want_pairs);
hipError_t launch_adjacency(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, unsigned rows, void* scratch,
                            unsigned pair_slots, unsigned* pairs, unsigned pair_rows, unsigned* rows_out, unsigned* counts, hipStream_t s);

// Sieve (sieve.hip): every region of fewer than min_pixels pixels takes the class of the resolved neighbour with the longest
// border, round by round (max_rounds of 1 to 64), over the adjacency pairs of the label plane.  klass, labels, table (table_rows
// rows of kRegWords u64) and the device word d_n are what launch_regions left; n = min(*d_n, table_rows), a pixel with a label
// >= n keeps its class.  klass_out: H * W bytes; rows_out: n x kSieveRowWords u32 (CLASS, INTO, ROUND, BORDER); counts
// [kSieveCountWords] = {REGIONS, SMALL, ABSORBED, STRANDED, ROUNDS, PIXELS_CHANGED, PAIRS, STATUS} (each optional).  scratch:
// sieve_scratch_bytes(..).  Stream-ordered; three memsets, 4 + 2 * max_rounds launches and one per wanted output; a round behind
// one that resolved nothing exits on a device flag; nothing is read back.
constexpr int kSieveRowWords = 4;
constexpr int kSieveCountWords = 8;
constexpr unsigned kSieveOverflow = 1u, kSieveRoundsExhausted = 2u, kSieveTableShort = 4u;
size_t sieve_scratch_bytes(size_t npix, unsigned table_rows, unsigned pair_slots);
hipError_t launch_sieve(const uint8_t* klass, const unsigned* labels, const unsigned long long* table, unsigned table_rows, const unsigned* d_n, unsigned H,
                        unsigned W, unsigned min_pixels, unsigned max_rounds, void* scratch, unsigned pair_slots, uint8_t* klass_out, unsigned* rows_out,
                        unsigned* counts, hipStream_t s);

// Outlines (outlines.hip): the boundaries of the value-regions of an H x W plane of 1- or 4-byte elements as closed loops --
// loops_rows x kLoopWords u32 records (OFFSET, COUNT, VALUE, START), vertex_rows u32 vertex ids Y * (W + 1) + X, and counts[3] =
// {n_loops, n_vertices, n_edges} (each optional; device memory).  skip: pixels of skip_value belong to no region; conn8: the
// saddle turns left.  cap: the edge capacity, in [1, 4 * H * W]; with more edges counts = {0, 0, n_edges} and nothing else is
// written.  scratch: outlines_scratch_bytes(H * W, cap) bytes the launches own for the call.  Stream-ordered; 9 + ceil(log2(cap))
// launches, no workgroup waits for another.  4 * H * W in [4, 2^32 - 2].
constexpr int kLoopWords = 4;
size_t outlines_scratch_bytes(size_t npix, size_t cap);
hipError_t launch_outlines(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, int conn8, unsigned skip_value, size_t cap,
                           void* scratch, unsigned* loops, unsigned loops_rows, unsigned* vertices, unsigned vertex_rows, unsigned* counts,
                           hipStream_t s);

// Simplify (simplify.hip): Douglas-Peucker on the loops Outlines left in device memory -- loops_rows_in records, vertex_rows_in
// vertex ids and counts[2] = {n_loops, n_vertices, ..} of a plane of width W in [1, 8191] -- with the tolerance tol16 / 16 pixels,
// tol16 <= 65535.  Outputs, each optional: loops_rows_out records (OFFSET', COUNT', VALUE, START), vertex_rows_out vertex ids and
// counts_out[4] = {n_loops, n_vertices', n_degenerate, status}.  scratch: simplify_scratch_bytes(loops_rows_in, vertex_rows_in)
// bytes the launches own for the call.  Stream-ordered; one memset and at most 6 launches, no workgroup waits for another.  No
// value held in the input buffers takes a load or a store outside the declared rows.
size_t simplify_scratch_bytes(size_t loops_rows, size_t vertex_rows);
hipError_t launch_simplify(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                           unsigned W, unsigned tol16, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out,
                           unsigned vertex_rows_out, unsigned* counts_out, hipStream_t s);

// Shapes (shapes.hip): per loop of launch_simplify's input its measures (AREA2, PERIMETER and five moment sums), its convex hull in
// Simplify's output layout, the hull's area and the minimum rectangle over the hull's edges; per value the sums.  Outputs, each
// optional: loops_rows_out records (OFFSET', COUNT', VALUE, START), vertex_rows_out hull vertex ids, shape_rows x kShapeWords
// signed 64-bit words per loop, value_rows x kShapeWords per value (every row written) and counts_out[4] = {n_loops,
// n_hull_vertices, status, largest COUNT'}.  scratch: shapes_scratch_bytes(loops_rows_in, vertex_rows_in) bytes.  Stream-ordered;
// two memsets and at most 6 launches, no workgroup waits for another.  No value held in the input buffers takes a load or a
// store outside the declared rows.
constexpr int kShapeMeasures = 7;
constexpr int kShapeWords = 12;
constexpr int kShapesCountWords = 4;
constexpr unsigned kShapesTruncated = 1u, kShapesMalformed = 2u;
size_t shapes_scratch_bytes(size_t loops_rows, size_t vertex_rows);
hipError_t launch_shapes(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                         unsigned W, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out, unsigned vertex_rows_out,
                         long long* shapes, unsigned shape_rows, long long* values, unsigned value_rows, unsigned* counts_out, hipStream_t s);

// Raster (raster.hip): the way back -- launch_simplify's input (loops of any polygon stage), or launch_runs' records, filled into an
// H x W plane (both in [1, 8191]) of 1- or 4-byte elements.  A pixel inside exactly one loop (winding 1) reads that loop's VALUE,
// a pixel inside none reads fill_value, every other pixel is a CONFLICT and reads fill_value.  Outputs, each optional: the plane
// (every pixel written) and counts_out[4] = {n_loops or n_runs, painted, conflict, status}.  scratch: raster_scratch_bytes(H * W)
// bytes.  Stream-ordered; one memset and at most 3 launches, no workgroup waits for another.  No value held in the input buffers
// takes a load, a store or an atomic outside the declared rows, the scratch and the plane.
constexpr int kRasterCountWords = 4;
constexpr unsigned kRasterTruncated = 1u, kRasterMalformed = 2u, kRasterOutside = 4u;
size_t raster_scratch_bytes(size_t npix);
hipError_t launch_raster(const unsigned* loops, unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts,
                         unsigned H, unsigned W, int elem_bytes, unsigned fill_value, void* scratch, void* plane, unsigned* counts_out, hipStream_t s);
hipError_t launch_raster_runs(const unsigned* runs, unsigned runs_rows_in, const unsigned* d_n, unsigned H, unsigned W, int elem_bytes,
                              unsigned fill_value, void* scratch, void* plane, unsigned* counts_out, hipStream_t s);

// Coverage (coverage.hip): Outlines' loops of an H x W plane (both in [1, 8191]) of 1- or 4-byte elements, simplified within
// tol16 / 16 pixels so that neighbouring polygons still fit: the loops are cut at the plane's junctions and every arc between
// two of them is simplified by a rule that does not depend on the direction of travel.  Inputs as launch_simplify's plus the
// plane (skip: pixels of skip_value belong to no region); aug_rows >= 1: the capacity in augmented vertices.  Outputs, each
// optional: loops_rows_out records, vertex_rows_out vertex ids and counts_out[6] = {n_loops, n_vertices', n_degenerate, status,
// n_aug, n_arcs}.  scratch: coverage_scratch_bytes(H, W, loops_rows_in, aug_rows) bytes the launches own for the call.
// Stream-ordered; one memset and at most 13 launches, no workgroup waits for another.  No value held in the input buffers takes
// a load or a store outside the declared rows, the plane or the scratch.
size_t coverage_scratch_bytes(size_t H, size_t W, size_t loops_rows, size_t aug_rows);
hipError_t launch_coverage(const void* plane, int elem_bytes, unsigned H, unsigned W, int skip, unsigned skip_value, const unsigned* loops,
                           unsigned loops_rows_in, const unsigned* vertices, unsigned vertex_rows_in, const unsigned* counts, unsigned tol16,
                           unsigned aug_rows, void* scratch, unsigned* loops_out, unsigned loops_rows_out, unsigned* vertices_out,
                           unsigned vertex_rows_out, unsigned* counts_out, hipStream_t s);

}  // namespace infur
