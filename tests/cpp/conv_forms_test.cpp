// conv_forms_test.cpp -- prints the table of infur_amd/csrc/conv_forms.h, one line per (mode, configuration) it admits:
//   mode cfg name plain_name bm bn tie_area tunable
// plain_name: what the profile says under INFUR_HL_PIPE=0.  tests/test_conv_forms_cpu.py holds it against tests/forms.py.  g++ only.
#include <cstdio>
#include <cstring>

#include "conv_forms.h"

using namespace infur;

static_assert(kModeF32 == 0 && kModeF16 == 1 && kModeSplit == 2 && kModeSplitFp8 == 3 && kModeI8 == 4 && kModeHL == 5 && kNumConvModes == 6, "");
// the numbers of the tuning database and of INFUR_CONV_CFG
static_assert(kCfg128x128 == 0 && kCfg64x128 == 1 && kCfg128x64 == 2 && kCfg64x64 == 3 && kCfg256x32 == 4 && kCfg128x256 == 5 && kCfg256x128 == 6, "");
static_assert(kCfg128x128_1buf == 7 && kCfg128x64_1buf == 8 && kCfg64x128_1buf == 9 && kCfg64x64_1buf == 10, "");
static_assert(kCfg256x256_1frag == 11 && kCfg256x128_1frag == 12 && kCfg256x256_dma == 13 && kCfg256x128_dma == 14 && kCfgAreg == 15, "");
static_assert(kCfg256x256_dmai == 16 && kCfg256x128_dmai == 17 && kCfgAregNsplit == 18 && kCfgHalo128 == 19 && kCfgHalo256 == 20 && kCfgHalo4 == 21, "");
static_assert(kNumConvCfgs == 22 && kNumConvForms == 32 && kFirstHLForm == 22, "");

constexpr int len(const char* s) {
    int n = 0;
    while (s[n]) n++;
    return n;
}
// every name, with the ",plain" of the forms that can carry one, fits infur_kernel_record::kernel (char[32])
constexpr bool names_fit() {
    for (const ConvForm& f : kConvForms)
        for (int m = 0; m < kNumConvModes; m++)
            if ((f.modes >> m & 1) && len(conv_family_prefix(f.family)) + len(kConvModeTag[m]) + len(f.suffix) + (f.family == kFamHL ? len(",plain") : 0) >= 32)
                return false;
    return true;
}
static_assert(names_fit() && kConvNameLen == 32, "");

int main() {
    for (int m = -1; m <= kNumConvModes; m++)
        for (int k = -1; k <= kNumConvCfgs; k++) {
            const ConvForm* f = conv_form(k, m);
            const char *name = conv_form_name(k, m, false), *plain = conv_form_name(k, m, true);
            if (strlen(name) >= 32 || strlen(plain) >= 32) return 1;
            if (f) printf("%d %d %s %s %d %d %d %d\n", m, k, name, plain, f->bm, f->bn, f->tie_area, f->tunable ? 1 : 0);
            else printf("# %d %d %s %s\n", m, k, name, plain);  // no form: the name the library would still report
        }
    return 0;
}
