// conv_igemm.hip -- name, validity and launch of a conv configuration (the table: conv_forms.h): the dispatch to the kernel families and
// to the per-mode translation units of the implicit-GEMM convolution (conv_igemm_kernel.h).
#include "kernels.h"

namespace infur {

// one launcher per arithmetic mode, each in its own translation unit (conv_igemm_<mode>.hip)
hipError_t conv_igemm_launch_f32(const ConvArgs& a, int cfg, hipStream_t s);
hipError_t conv_igemm_launch_f16(const ConvArgs& a, int out_f32, int cfg, hipStream_t s);
hipError_t conv_igemm_launch_split(const ConvArgs& a, int fp8_cross, int cfg, hipStream_t s);
hipError_t conv_igemm_launch_i8(const ConvArgs& a, int out_f32, int cfg, hipStream_t s);
#ifdef KTRACE
hipError_t ktrace_read_f32(unsigned long long* out);
hipError_t ktrace_read_f16(unsigned long long* out);
hipError_t ktrace_read_split(unsigned long long* out);
hipError_t ktrace_read_i8(unsigned long long* out);
hipError_t ktrace_read(unsigned long long* out) {  // the buffer of the mode that traced something
    hipError_t (*const rd[4])(unsigned long long*) = {ktrace_read_f32, ktrace_read_f16, ktrace_read_split, ktrace_read_i8};
    unsigned long long tmp[8 * 8 * 4];
    bool any = false;
    for (auto f : rd) {
        const hipError_t e = f(tmp);
        if (e != hipSuccess) return e;
        bool nz = false;
        for (auto v : tmp) nz |= v != 0;
        if (nz || !any) {
            for (int i = 0; i < 8 * 8 * 4; i++) out[i] = tmp[i];
            any |= nz;
        }
    }
    return hipSuccess;
}
#endif

const char* conv_igemm_config_name(int cfg, ConvMode mode) { return conv_form_name(cfg, mode, !conv_hl_pipe_on()); }

const char* conv_variant_name(const ConvArgs& a, ConvMode mode, int cfg, int out_f32) {
    const ConvForm* f = conv_form(cfg, mode);
    if (!f || !conv_igemm_config_valid(a, cfg, mode, out_f32)) return "";
    switch (f->family) {
        case kFamAreg: return mode == kModeI8 ? "" : conv1x1_areg_variant(a);
        case kFamAregNsplit: return conv1x1_q8_variant(a);
        case kFamHalo: return conv3x3_halo_variant(a, mode, f->bn);
        case kFamHalo4: return conv3x3_halo4_variant(a);
        default: return "";
    }
}

// the configuration of a shape nobody has measured (pick_cfg without a tuning entry)
ConvCfg conv_igemm_default_config(const ConvArgs& a) {
    if (a.Cout >= 128) return kCfg128x128;
    if (a.Cout > 32) return kCfg128x64;
    return kCfg256x32;
}

// A configuration is a candidate when the table has a form of it for the mode (conv_form) and the form's kernel takes the shape: the
// kernel families' own predicates; a tiled form's N tile must not be mostly padding.
bool conv_igemm_config_valid(const ConvArgs& a, int cfg, ConvMode mode, int out_f32) {
    const ConvForm* f = conv_form(cfg, mode);
    if (!f) return false;
    switch (f->family) {
        case kFamHL:
        case kFamHLAreg: return conv_hl_config_valid(a, *f, out_f32);
        case kFamHalo: return conv3x3_halo_valid(a, mode, out_f32, f->bn);
        case kFamHalo4: return conv3x3_halo4_valid(a, mode, out_f32);
        case kFamAregNsplit: return conv1x1_q8_valid(a, mode, out_f32) && conv1x1_q8_nsplit(a) > 1;
        case kFamAreg: return mode == kModeI8 ? conv1x1_q8_valid(a, mode, out_f32) : conv1x1_areg_valid(a, mode, out_f32);
        case kFamTiled: break;
    }
    if (a.Cout <= 32) return f->bn == 32;
    if (f->bn == 32) return false;
    return f->bn <= a.Cout || f->bn == 64;  // Cout = 64 -> BN 64 only; Cout >= 128 -> 64 and 128 (and 256 when Cout >= 256)
}

hipError_t launch_conv_igemm(const ConvArgs& a, ConvMode mode, int out_f32, int cfg, hipStream_t s) {
    switch (mode) {
        case kModeHL: return launch_conv_hl(a, out_f32, cfg, s);
        case kModeF32: return conv_igemm_launch_f32(a, cfg, s);
        case kModeF16: return conv_igemm_launch_f16(a, out_f32, cfg, s);
        case kModeSplit: return conv_igemm_launch_split(a, 0, cfg, s);
        case kModeSplitFp8: return conv_igemm_launch_split(a, 1, cfg, s);
        case kModeI8: return a.q_mult && a.q_bias ? conv_igemm_launch_i8(a, out_f32, cfg, s) : hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

}  // namespace infur
