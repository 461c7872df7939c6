// conv_forms.h -- the ONE table of the convolution kernels' forms: what a configuration number means in each arithmetic mode -- kernel
// family, tile, staging, profile name, the modes it can be a candidate in, whether the tuner times it, its tie-break area.  Read by
// the name / validity / launch dispatch (conv_igemm.hip, conv_igemm_kernel.h: launch_t, conv_hl.hip: launch_conv_hl) and the tuner
// (infur_tuner.cpp).  Plain C++17, no HIP header: tests/cpp/conv_forms_test.cpp prints it (tests/test_conv_forms_cpu.py).
// All forms of a mode accumulate k in the same order for every output element: the choice changes speed, never a bit of the result.
#pragma once
#include <initializer_list>
#include <type_traits>

namespace infur {

// GEMM arithmetic of launch_conv_igemm.  0 / 1 / 2 / 3 / 5 are the INFUR_DTYPE_* values of a context (infur_rt.h asserts it);
// 4 is no option value: the integer arithmetic of a quantised model is selected by the model file.
enum ConvMode : int {
    kModeF32 = 0,    // f32 operands on the f32 MFMA (Cin % 32 == 0)
    kModeF16 = 1,    // f16 operands, f32 accumulation (Cin % 64 == 0), output f16 or (out_f32) f32
    kModeSplit = 2,  // f32 tensors, each value split into an f16 hi + lo pair while it is staged, three f16 MFMAs per product, f32
                     // accumulation (Cin % 32 == 0) -- f32-grade results at f16 matrix rate / 3
    // as kModeSplit, but the two cross terms hi * lo run on the bf8 (OCP e5m2) MX MFMA: 2 MFMA units per product instead of 3,
    // products exact to ~2^-13 whatever the tensors' dynamic range (e5m2 has f16's exponent range: no scales; round 3 used e4m3
    // under per-tensor scales, which heavy-tailed weights broke); weights prepared with launch_split_weights(fp8_cross = 1)
    kModeSplitFp8 = 3,
    kModeI8 = 4,  // quantised (ConvArgs::q_*): u8 NHWC activations, s8 OHWI weights (Cin % 128 == 0), output u8 or (out_f32) dequantised f32
    // three-byte tensors (f16 hi + e5m2 lo planes, ConvArgs::*_lo), hi * hi on the f16 MFMA + both cross terms on the bf8 MX MFMA,
    // every operand staged by LDS-DMA (conv_hl.hip); Cin % 32 == 0
    kModeHL = 5,
};
constexpr int kNumConvModes = 6;

// Configuration numbers: the on-disk format of the tuning database (infur_amd/conv_tune_gfx950.txt, infur_tune_import / _export),
// the value of INFUR_CONV_CFG and the numbers in scripts/ -- they never change.  Named after the kModeF16 form; kModeHL runs its own
// kernels under ten of the numbers (the second block of kConvForms), not always on the tile of the name.
enum ConvCfg : int {
    kCfg128x128 = 0, kCfg64x128, kCfg128x64, kCfg64x64, kCfg256x32, kCfg128x256, kCfg256x128,
    kCfg128x128_1buf, kCfg128x64_1buf, kCfg64x128_1buf, kCfg64x64_1buf, kCfg256x256_1frag, kCfg256x128_1frag,
    kCfg256x256_dma, kCfg256x128_dma, kCfgAreg, kCfg256x256_dmai, kCfg256x128_dmai, kCfgAregNsplit,
    kCfgHalo128, kCfgHalo256, kCfgHalo4,
};
constexpr int kNumConvCfgs = 22;

enum ConvFamily : int {
    kFamTiled,       // conv_igemm_kernel.h; stage = NBUF: 1 / 2 register-staged LDS buffers, 3 one fragment set, 4 LDS-DMA, 5 LDS-DMA issued between the slices
    kFamAreg,        // 1x1, activation tile in registers: conv1x1_areg.hip (kModeF16), conv1x1_q8.hip (kModeI8)
    kFamAregNsplit,  // conv1x1_q8.hip with the N tiles of an M tile shared out over several workgroups
    kFamHalo,        // stride-1 3x3, input patch of a 16 x 16 output tile in LDS for all nine taps: conv3x3_halo.hip
    kFamHalo4,       // its 4-wave form
    kFamHL,          // conv_hl.hip; stage = NIMG, the ring of LDS images
    kFamHLAreg,      // conv_hl_areg.hip
};

constexpr unsigned mode_bit(ConvMode m) { return 1u << m; }
constexpr unsigned kInAllTiled = mode_bit(kModeF32) | mode_bit(kModeF16) | mode_bit(kModeSplit) | mode_bit(kModeSplitFp8) | mode_bit(kModeI8);
constexpr unsigned kInBytes = mode_bit(kModeF16) | mode_bit(kModeI8);  // byte operands that need no conversion: what LDS-DMA can stage
constexpr unsigned kInHL = mode_bit(kModeHL);

struct ConvForm {
    ConvCfg cfg;
    ConvFamily family;
    int bm, bn, wm, wn;  // workgroup tile and its waves (kFamTiled, kFamHL: the kernel's template arguments; otherwise bm x bn only)
    int stage;           // NBUF / NIMG
    const char* suffix;  // name = family prefix + mode tag + suffix
    unsigned modes;      // mode_bit()s in which the form can ever be a candidate; the shape decides the rest (conv_igemm_config_valid)
    bool tunable;        // the tuner times it
    // What the tuner's tie-break compares (infur_tuner.cpp: the larger area among the forms within 2 % of the fastest).  STORED, not
    // bm * bn: it is the area of the kModeF16 form of the same NUMBER in every mode, as it always was -- for kModeHL's 15 and 16
    // that is twice the tile that runs (128 x 128, 128 x 256).  Correcting those two changes which form the tuner picks: a speed
    // change that needs its own measurements.
    int tie_area;
};

constexpr ConvForm kConvForms[] = {
    // ---- modes 0-4: row index == configuration number ----
    {kCfg128x128, kFamTiled, 128, 128, 2, 2, 2, "<128,128>", kInAllTiled, true, 128 * 128},
    {kCfg64x128, kFamTiled, 64, 128, 2, 2, 2, "<64,128>", kInAllTiled, true, 64 * 128},
    {kCfg128x64, kFamTiled, 128, 64, 2, 2, 2, "<128,64>", kInAllTiled, true, 128 * 64},
    {kCfg64x64, kFamTiled, 64, 64, 2, 2, 2, "<64,64>", kInAllTiled, true, 64 * 64},
    {kCfg256x32, kFamTiled, 256, 32, 4, 1, 2, "<256,32>", kInAllTiled, true, 256 * 32},
    {kCfg128x256, kFamTiled, 128, 256, 2, 4, 2, "<128,256>", kInAllTiled, true, 128 * 256},
    {kCfg256x128, kFamTiled, 256, 128, 4, 2, 2, "<256,128>", kInAllTiled, true, 256 * 128},
    {kCfg128x128_1buf, kFamTiled, 128, 128, 2, 2, 1, "<128,128,1buf>", kInAllTiled, true, 128 * 128},
    {kCfg128x64_1buf, kFamTiled, 128, 64, 2, 2, 1, "<128,64,1buf>", kInAllTiled, true, 128 * 64},
    {kCfg64x128_1buf, kFamTiled, 64, 128, 2, 2, 1, "<64,128,1buf>", kInAllTiled, true, 64 * 128},
    {kCfg64x64_1buf, kFamTiled, 64, 64, 2, 2, 1, "<64,64,1buf>", kInAllTiled, true, 64 * 64},
    {kCfg256x256_1frag, kFamTiled, 256, 256, 2, 4, 3, "<256,256,1frag>", kInAllTiled, true, 256 * 256},  // 8 waves of 128x64, one fragment set
    {kCfg256x128_1frag, kFamTiled, 256, 128, 4, 2, 3, "<256,128,1frag>", kInAllTiled, true, 256 * 128},  // 8 waves of 64x64, one fragment set
    // LDS-DMA staging (the kernel is written in bytes and the DMA forms were built and measured for f32 too: 134-138 TFLOP/s against
    // 139-144 for the tuned register forms at 1080p -- the 64-cycle f32 MFMAs hide the register staging anyway and 256-row tiles
    // are too coarse for M = 32400)
    {kCfg256x256_dma, kFamTiled, 256, 256, 2, 4, 4, "<256,256,dma>", kInBytes, true, 256 * 256},
    {kCfg256x128_dma, kFamTiled, 256, 128, 4, 2, 4, "<256,128,dma>", kInBytes, true, 256 * 128},
    // short-K 1x1 convs: activation tile in registers, all N tiles walked by one workgroup (never the f32 logits)
    {kCfgAreg, kFamAreg, 256, 128, 0, 0, 0, "<256,areg>", kInBytes, true, 256 * 128},
    // LDS-DMA staging with the DMA instructions issued between the slices (the MFMA-bound layers)
    {kCfg256x256_dmai, kFamTiled, 256, 256, 2, 4, 5, "<256,256,dmai>", kInBytes, true, 256 * 256},
    {kCfg256x128_dmai, kFamTiled, 256, 128, 4, 2, 5, "<256,128,dmai>", kInBytes, true, 256 * 128},
    // kCfgAreg of the quantised mode with the N tiles of an M tile shared out over several workgroups: M = 32400 alone gives 254
    // workgroups for 256 CUs
    {kCfgAregNsplit, kFamAregNsplit, 256, 128, 0, 0, 0, "<256,areg,nsplit>", mode_bit(kModeI8), true, 256 * 128},
    // round 4: stride-1 3x3 convs with the input patch of a 16 x 16 output tile resident in LDS for all nine taps: a fifth of the
    // activation ingest of the tiled forms -- for M = 32400, where one tile per CU is bound by the L2 -> LDS path, not by the MFMA.
    // (kCfgHalo256 is not a tuning candidate: timed in isolation, with its operands warm in the Infinity Cache, it beats the tiled
    //  `dmai` form on the long-K head convs by 2-4 %; inside a frame, where its one-patch-image chunk boundaries meet HBM latency, it
    //  is 5-12 % slower (classifier.0 at 1080p 535 against 477 us).  It stays selectable -- INFUR_CONV_CFG=20, INFUR_TUNE_HALO256=1
    //  -- and bit-identical: tests/test_gpu_halo.py.)
    {kCfgHalo128, kFamHalo, 256, 128, 0, 0, 0, "<16x16,128,halo>", kInBytes, true, 256 * 128},
    {kCfgHalo256, kFamHalo, 256, 256, 0, 0, 0, "<16x16,256,halo>", kInBytes, false, 256 * 256},
    // the same with ONE wave per SIMD and a 128 x 128 wave tile (two thirds of the fragment reads per MFMA), software-pipelined across
    // the weight steps ("the 4-wave form")
    {kCfgHalo4, kFamHalo4, 256, 256, 0, 0, 0, "<16x16,256,halo4>", mode_bit(kModeF16), true, 256 * 256},
    // ---- mode 5: its own kernels under ten of the numbers ----
    {kCfg128x128, kFamHL, 128, 128, 2, 2, 3, "<128,128>", kInHL, true, 128 * 128},  // 4 waves of 64x64
    {kCfg128x256, kFamHL, 128, 256, 2, 4, 3, "<128,256>", kInHL, true, 128 * 256},  // 8 waves of 64x64
    {kCfg256x128, kFamHL, 256, 128, 4, 2, 3, "<256,128>", kInHL, true, 256 * 128},  // 8 waves of 64x64
    {kCfg256x256_1frag, kFamHL, 256, 256, 2, 4, 3, "<256,256>", kInHL, true, 256 * 256},  // 8 waves of 128x64
    // FOUR waves of 128x64 with a ring of two images: two workgroups per CU
    {kCfg256x128_1frag, kFamHL, 256, 128, 2, 2, 2, "<256,128,4w>", kInHL, true, 256 * 128},
    {kCfg256x256_dma, kFamHL, 256, 256, 4, 2, 3, "<256,256,wn2>", kInHL, true, 256 * 256},  // 8 waves of 64 x 128: a wave's epilogue rows are 128 channels wide
    {kCfg256x128_dma, kFamHL, 128, 256, 1, 4, 2, "<128,256,4w>", kInHL, true, 256 * 128},
    // the activation fragment in registers (1x1 expansions); tie_area: see ConvForm
    {kCfgAreg, kFamHLAreg, 128, 128, 0, 0, 0, "<128,areg>", kInHL, true, 256 * 128},
    // round 6: the two-workgroups-per-CU forms with 64 x 128 wave tiles (the expansions' epilogue moves whole 256 / 128-byte rows of
    // the hi / lo planes per pixel instead of 128 / 64); tie_area of the first: see ConvForm
    {kCfg256x256_dmai, kFamHL, 128, 256, 2, 2, 2, "<128,256,4w,wn2>", kInHL, true, 256 * 256},
    {kCfg256x128_dmai, kFamHL, 256, 128, 4, 1, 2, "<256,128,4w,wn2>", kInHL, true, 256 * 128},
    // (forms that were measured and not shipped, with their numbers: LAB_NOTES.md, "Conv forms: one table")
};
constexpr int kNumConvForms = (int)(sizeof(kConvForms) / sizeof(kConvForms[0]));
constexpr int kFirstHLForm = kNumConvCfgs;

constexpr bool conv_forms_in_order() {  // rows 0-21 are configurations 0-21 of modes 0-4, the rest is mode 5
    for (int i = 0; i < kNumConvForms; i++)
        if (i < kNumConvCfgs ? (kConvForms[i].cfg != i || (kConvForms[i].modes & kInHL)) : kConvForms[i].modes != kInHL) return false;
    return true;
}
static_assert(conv_forms_in_order(), "");

// the form that configuration `cfg` is in `mode`; null: there is none
constexpr const ConvForm* conv_form(int cfg, int mode) {
    if (mode < 0 || mode >= kNumConvModes) return nullptr;
    for (const ConvForm& f : kConvForms)
        if (f.cfg == cfg && (f.modes >> mode & 1)) return &f;
    return nullptr;
}

// ---- names: family prefix + mode tag + suffix, built once, at compile time ----
constexpr int kConvNameLen = 32;  // infur_kernel_record::kernel
struct ConvFormNames {
    char name[kNumConvModes][kNumConvCfgs][kConvNameLen];
    char plain[kNumConvCfgs][kConvNameLen];  // kModeHL under INFUR_HL_PIPE=0
};
constexpr const char* conv_family_prefix(ConvFamily f) {
    return f == kFamTiled ? "conv_igemm_" : f == kFamAreg || f == kFamAregNsplit ? "conv1x1_" : f == kFamHalo || f == kFamHalo4 ? "conv3x3_" : "conv_hl";
}
constexpr const char* kConvModeTag[kNumConvModes] = {"f32", "f16", "f32s", "f32x", "i8", ""};
constexpr void conv_name_join(char* dst, const char* a, const char* b, const char* c, const char* d) {
    int n = 0;
    for (const char* s : {a, b, c, d})
        for (; *s; s++) dst[n++] = *s;  // (a name of kConvNameLen or more characters does not compile: dst[n] out of bounds)
    dst[n] = 0;
}
constexpr ConvFormNames conv_form_names() {
    ConvFormNames t{};
    for (int k = 0; k < kNumConvCfgs; k++) {
        conv_name_join(t.name[kModeHL][k], "conv_hl<?>", "", "", "");
        conv_name_join(t.plain[k], "conv_hl<?>", "", "", "");
    }
    for (const ConvForm& f : kConvForms) {
        const char* pre = conv_family_prefix(f.family);
        if (f.modes & kInHL) {  // the tiled forms run their plain K loop and say so (conv_hl_areg.hip has one loop only)
            conv_name_join(t.name[kModeHL][f.cfg], pre, f.suffix, "", "");
            conv_name_join(t.plain[f.cfg], pre, f.suffix, f.family == kFamHL ? ",plain" : "", "");
        } else {
            for (int m = 0; m < kModeHL; m++) conv_name_join(t.name[m][f.cfg], pre, kConvModeTag[m], f.suffix, "");  // (also where it is no candidate)
        }
    }
    return t;
}
inline constexpr ConvFormNames kConvFormNames = conv_form_names();

// the profile's kernel name of configuration `cfg` in `mode`; hl_plain: INFUR_HL_PIPE=0.  The pointer is valid for the process' life.
inline const char* conv_form_name(int cfg, int mode, bool hl_plain) {
    const bool known = cfg >= 0 && cfg < kNumConvCfgs && mode >= 0 && mode < kNumConvModes;
    if (!known) return mode == kModeHL ? "conv_hl<?>" : "conv_igemm<?>";
    return mode == kModeHL && hl_plain ? kConvFormNames.plain[cfg] : kConvFormNames.name[mode][cfg];
}

// ---- sub-forms: the kernels WITHIN a configuration, picked from the size of the map ----
// Several launchers choose among two to four kernels from M (pixels) and Cout.  The pure size rules live here, so that the launcher,
// the name function (conv_variant_name, kernels.h) and tests/cpp/conv_forms_test.cpp all evaluate the same expression; the
// environment hooks that override a rule stay with their launcher.  All sub-forms of a configuration give the same bits.
constexpr int kTwoThirdsOfCUs = 170;  // of 256: a launch of no more workgroups than this leaves over a third of the chip idle
constexpr long cdiv_l(long a, long b) { return (a + b - 1) / b; }
// conv1x1_areg.hip (kModeF16, kCfgAreg): the 128-pixel 4-wave form where 256-pixel workgroups would leave more than a third of the
// CUs without one
constexpr bool areg_small_rule(long M) { return cdiv_l(M, 256) <= kTwoThirdsOfCUs; }
// conv1x1_b2b.hip: INFUR_B2B_FORM's default -- 3 (the 128-pixel workgroup) by the same rule, else 1 (two waves per SIMD x 32 pixels)
constexpr int b2b_form_rule(long M) { return cdiv_l(M, 256) <= kTwoThirdsOfCUs ? 3 : 1; }
// conv3x3_halo.hip (kModeF16, kCfgHalo128): N tiles of 64 on the 64-channel convs and wherever 128-wide tiles over 16 x 16 pixel tiles
// would leave more than a third of the CUs without a workgroup (a Cout that 128 does not divide keeps 128 and is then no candidate)
constexpr long halo_tiles16(int OH, int OW) { return cdiv_l(OH, 16) * cdiv_l(OW, 16); }
constexpr int halo_bn_rule(long tiles16, int Cout) {
    if (Cout == 64) return 64;
    return (Cout % 128 == 0 && tiles16 * (Cout / 128) <= kTwoThirdsOfCUs) ? 64 : 128;
}
// conv1x1_q8.hip (kModeI8, kCfgAregNsplit; M tiles of 128 pixels, N tiles of 128 channels): the smallest divisor of the N tile count
// that brings the launch to about two workgroups per CU; 0: the plain form already has them, or Cout is a single N tile
constexpr int kQ8TilePixels = 128, kQ8TileChannels = 128, kQ8TwoPerCU = 480, kQ8MaxSplit = 16;
constexpr int q8_nsplit_rule(long mtiles, int ntiles) {
    if (mtiles >= kQ8TwoPerCU || ntiles < 2) return 0;
    for (int d = 2; d <= ntiles; d++)
        if (ntiles % d == 0 && (mtiles * d >= kQ8TwoPerCU || d == ntiles)) return d;
    return 0;
}

// ---- variant tags: what a profile record says about the sub-form that ran (ProfRec::variant, infur_debug_profile_variant) ----
// A tag is a comma-separated list of the words below, "" where a launch has one form only.  The halo forms say three things:
// the N tile, the tiling of the map (uniform 16 x 16, uniform 8 x 32, or 16 x 16 with an (H mod 16) x 32 strip) and the number of
// patch images.  EVERY word the library can say is in kVariantWords: tests/test_conv_forms_cpu.py holds tests/forms.py against it,
// so that a new sub-form without a forced case fails there.
constexpr const char* kVariantWords[] = {
    "bm128", "bm256",                                // conv1x1_areg.hip
    "nsplit2", "nsplit4", "nsplit8", "nsplit16",     // conv1x1_q8.hip (N tile counts of 2^k: every Cout the kernel is built for)
    "bn64", "bn128", "bn256",                        // conv3x3_halo.hip
    "16x16", "8x32", "mixed", "na1", "na2",          //   halo_plan / halo4_plan
    "lds", "f32x1", "f32x2", "f32x4w",               // winograd.hip: the transforms' forms
    "form1", "form2", "form3", "dma0", "dma1", "dma2",  // conv1x1_b2b.hip: workgroup form, which waves issue the DMA pieces
    "f16stem", "f32stem",                            // stem_pool.hip: the fused stem's arithmetic (split modes: f16stem = its f16 hi + lo pairs)
};
constexpr int kNumVariantWords = (int)(sizeof(kVariantWords) / sizeof(kVariantWords[0]));

constexpr const char* q8_nsplit_tag(int nsplit) {
    constexpr const char* t[kQ8MaxSplit + 1] = {"", "", "nsplit2", "nsplit3", "nsplit4", "nsplit5", "nsplit6", "nsplit7", "nsplit8",
                                                "nsplit9", "nsplit10", "nsplit11", "nsplit12", "nsplit13", "nsplit14", "nsplit15", "nsplit16"};
    return nsplit >= 0 && nsplit <= kQ8MaxSplit ? t[nsplit] : "nsplit?";
}

// the halo forms' tags, built once: [bn 64 / 128 / 256][tiling 16x16 / 8x32 / mixed][patch images 1 / 2]
constexpr int kVariantLen = 24;
struct HaloTags {
    char tag[3][3][2][kVariantLen];
};
constexpr HaloTags halo_tags() {
    HaloTags t{};
    constexpr const char* bn[3] = {"bn64", "bn128", "bn256"};
    constexpr const char* geom[3] = {",16x16", ",8x32", ",mixed"};
    constexpr const char* na[2] = {",na1", ",na2"};
    for (int b = 0; b < 3; b++)
        for (int g = 0; g < 3; g++)
            for (int n = 0; n < 2; n++) conv_name_join(t.tag[b][g][n], bn[b], geom[g], na[n], "");
    return t;
}
inline constexpr HaloTags kHaloTags = halo_tags();
// th1 x tw1 = the first region's tile, th2 = rows of the strip region (0: none): HaloGeom of conv3x3_halo.hip
inline const char* halo_variant_tag(int bn, int th1, int tw1, int th2, int na) {
    const int b = bn == 64 ? 0 : bn == 128 ? 1 : bn == 256 ? 2 : -1;
    if (b < 0 || na < 1 || na > 2) return "halo?";
    return kHaloTags.tag[b][th2 ? 2 : (th1 == 8 && tw1 == 32) ? 1 : 0][na - 1];
}

// conv1x1_b2b.hip: [form 1 / 2 / 3][dma phase 0 / 1 / 2]
struct B2bTags {
    char tag[3][3][kVariantLen];
};
constexpr B2bTags b2b_tags() {
    B2bTags t{};
    constexpr const char* form[3] = {"form1", "form2", "form3"};
    constexpr const char* dma[3] = {",dma0", ",dma1", ",dma2"};
    for (int f = 0; f < 3; f++)
        for (int d = 0; d < 3; d++) conv_name_join(t.tag[f][d], form[f], dma[d], "", "");
    return t;
}
inline constexpr B2bTags kB2bTags = b2b_tags();
inline const char* b2b_variant_tag(int form, int dma_phase) {
    return form >= 1 && form <= 3 && dma_phase >= 0 && dma_phase <= 2 ? kB2bTags.tag[form - 1][dma_phase] : "b2b?";
}

// f(std::integral_constant<int, I>) for the row I of [I, End) that holds configuration `cfg`, `none` without one: how a launcher turns
// the run-time number into the row's template arguments
template <int I, int End, class R, class F>
R conv_form_visit(int cfg, R none, F&& f) {
    if constexpr (I < End) return kConvForms[I].cfg == cfg ? f(std::integral_constant<int, I>()) : conv_form_visit<I + 1, End>(cfg, none, f);
    else return none;
}

}  // namespace infur
