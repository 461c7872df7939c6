// conv_forms_test.cpp -- prints the table of infur_amd/csrc/conv_forms.h, one line per (mode, configuration) it admits:
//   mode cfg name plain_name bm bn tie_area tunable
// plain_name: what the profile says under INFUR_HL_PIPE=0.  tests/test_conv_forms_cpu.py holds it against tests/forms.py.  g++ only.
// Then the sub-forms inside a configuration: one line "V word" per word a variant tag can hold, "T tag" per composed tag, and one line
// "R rule arguments... value" per size rule at the values the sources' comments state and at each threshold +- 1 (pinned here by
// static_assert as well: a rule that moves does not compile).
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

// ---- the size rules (conv_forms.h, "sub-forms") at the values the code comments state ----
// conv1x1_areg.hip: M = 43,520 = 170 tiles of 256 pixels is small, 43,521 is big; the back-to-back launch follows the same rule
static_assert(areg_small_rule(1) && areg_small_rule(43519) && areg_small_rule(43520) && !areg_small_rule(43521) && !areg_small_rule(135 * 240 * 4), "");
static_assert(b2b_form_rule(1) == 3 && b2b_form_rule(43520) == 3 && b2b_form_rule(43521) == 1, "");
// conv3x3_halo.hip: 1080p layer2 conv2 (135 x 240, 128 channels: 135 tiles x ONE N tile) runs BN = 64, Cout 256 there BN = 128
static_assert(halo_tiles16(135, 240) == 135 && halo_bn_rule(135, 128) == 64 && halo_bn_rule(135, 256) == 128, "");
static_assert(halo_bn_rule(170, 128) == 64 && halo_bn_rule(171, 128) == 128 && halo_bn_rule(169, 128) == 64, "");
static_assert(halo_bn_rule(85, 256) == 64 && halo_bn_rule(86, 256) == 128 && halo_bn_rule(84, 256) == 64, "");
static_assert(halo_bn_rule(1, 64) == 64 && halo_bn_rule(100000, 64) == 64 && halo_bn_rule(1, 192) == 128 && halo_bn_rule(1, 2048) == 64, "");
static_assert(halo_tiles16(1, 1) == 1 && halo_tiles16(16, 16) == 1 && halo_tiles16(17, 16) == 2 && halo_tiles16(17, 31) == 4, "");
// conv1x1_q8.hip: M = 32,400 = 254 M tiles with Cout 2048 gives split 2; 480 workgroups are "two per CU"
static_assert(cdiv_l(32400, kQ8TilePixels) == 254 && q8_nsplit_rule(254, 2048 / kQ8TileChannels) == 2, "");
static_assert(q8_nsplit_rule(480, 16) == 0 && q8_nsplit_rule(479, 16) == 2 && q8_nsplit_rule(481, 16) == 0, "");
static_assert(q8_nsplit_rule(240, 16) == 2 && q8_nsplit_rule(239, 16) == 4 && q8_nsplit_rule(241, 16) == 2, "");
static_assert(q8_nsplit_rule(120, 16) == 4 && q8_nsplit_rule(119, 16) == 8 && q8_nsplit_rule(60, 16) == 8 && q8_nsplit_rule(59, 16) == 16, "");
static_assert(q8_nsplit_rule(1, 16) == 16 && q8_nsplit_rule(1, 8) == 8 && q8_nsplit_rule(1, 4) == 4 && q8_nsplit_rule(1, 2) == 2, "");
static_assert(q8_nsplit_rule(1, 1) == 0 && q8_nsplit_rule(479, 1) == 0 && q8_nsplit_rule(239, 2) == 2 && q8_nsplit_rule(240, 6) == 2 && q8_nsplit_rule(100, 6) == 6, "");

static void print_rules() {
    for (long m : {1L, 104L, 4096L, 34L * 61, 43519L, 43520L, 43521L, 195L * 225, 98L * 113, 135L * 240, 270L * 480})
        printf("R areg_small %ld %d\nR b2b_form %ld %d\n", m, areg_small_rule(m) ? 1 : 0, m, b2b_form_rule(m));
    const int maps[][2] = {{1, 1}, {17, 31}, {34, 61}, {98, 113}, {195, 225}, {135, 240}};
    for (const auto& hw : maps)
        for (int cout : {64, 128, 256, 512})
            printf("R halo_bn %d %d %d %d\n", hw[0], hw[1], cout, halo_bn_rule(halo_tiles16(hw[0], hw[1]), cout));
    for (long m : {1L, 17L * 31, 98L * 113, 30592L, 30593L, 32400L, 61312L, 61313L})
        for (int cout : {128, 256, 512, 1024, 2048})
            printf("R q8_nsplit %ld %d %d\n", m, cout, q8_nsplit_rule(cdiv_l(m, kQ8TilePixels), cout / kQ8TileChannels));
}

static int print_tags() {
    for (const char* w : kVariantWords) printf("V %s\n", w);
    for (int bn : {64, 128, 256})
        for (int geom = 0; geom < 3; geom++)
            for (int na = 1; na <= 2; na++) {
                const char* t = halo_variant_tag(bn, geom == 1 ? 8 : 16, geom == 1 ? 32 : 16, geom == 2 ? 1 : 0, na);
                if (strlen(t) >= (size_t)kVariantLen) return 1;
                printf("T %s\n", t);
            }
    for (int form = 1; form <= 3; form++)
        for (int dma = 0; dma <= 2; dma++) printf("T %s\n", b2b_variant_tag(form, dma));
    for (int d = 2; d <= kQ8MaxSplit; d++) printf("T %s\n", q8_nsplit_tag(d));
    if (strcmp(halo_variant_tag(32, 16, 16, 0, 1), "halo?") || strcmp(halo_variant_tag(64, 16, 16, 0, 3), "halo?")) return 1;
    if (strcmp(b2b_variant_tag(0, 0), "b2b?") || strcmp(b2b_variant_tag(1, 3), "b2b?") || strcmp(q8_nsplit_tag(17), "nsplit?") || *q8_nsplit_tag(0)) return 1;
    return 0;
}

int main() {
    for (int m = -1; m <= kNumConvModes; m++)
        for (int k = -1; k <= kNumConvCfgs; k++) {
            const ConvForm* f = conv_form(k, m);
            const char *name = conv_form_name(k, m, false), *plain = conv_form_name(k, m, true);
            if (strlen(name) >= 32 || strlen(plain) >= 32) return 1;
            if (f) printf("%d %d %s %s %d %d %d %d\n", m, k, name, plain, f->bm, f->bn, f->tie_area, f->tunable ? 1 : 0);
            else printf("# %d %d %s %s\n", m, k, name, plain);  // no form: the name the library would still report
        }
    print_rules();
    return print_tags();
}
