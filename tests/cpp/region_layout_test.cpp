// region_layout_test.cpp -- sweeps infur_amd/csrc/region_layout.h, where the frame calls behind Regions stage Regions' and
// Anchors' products: these numbers decide where a kernel writes and how many bytes a copy moves into a caller's array.
// Stand-alone and HIP-free: tests/test_region_layout_cpu.py builds it with plain g++, once more under the address and
// undefined-behaviour sanitizers, and requires the same output of both.  A property that does not hold is printed and makes the
// exit status 1.
#include <cstdint>
#include <cstdio>

#include "region_layout.h"

using namespace infur;

static_assert(sizeof(size_t) == 8, "the layout arithmetic is 64-bit");

static unsigned long long g_checks = 0, g_failed = 0;

#define CHECK(cond, ...)                               \
    do {                                               \
        g_checks++;                                    \
        if (!(cond)) {                                 \
            if (g_failed++ < 20) {                     \
                std::printf("FAILED %s: ", #cond);     \
                std::printf(__VA_ARGS__);              \
                std::printf("\n");                     \
            }                                          \
        }                                              \
    } while (0)

// slots in order, aligned, disjoint, each large enough for `need` and with less than one boundary of padding
static void check_slots(const size_t* off, const size_t* need, int slots, size_t at) {
    CHECK(off[0] == at, "the first slot at %zu, wanted %zu", off[0], at);
    size_t sum = 0;
    for (int i = 0; i < slots; i++) {
        CHECK(off[i] % 256 == 0, "slot %d at %zu", i, off[i]);
        CHECK(off[i + 1] >= off[i] && off[i + 1] - off[i] >= need[i], "slot %d: %zu .. %zu holds %zu", i, off[i], off[i + 1], need[i]);
        CHECK(off[i + 1] - off[i] < need[i] + 256, "slot %d: %zu .. %zu for %zu", i, off[i], off[i + 1], need[i]);
        CHECK(off[i + 1] >= at, "slot %d wrapped: %zu", i, off[i + 1]);
        sum += align_up(need[i], 256);
    }
    // the padding bound: the whole is the sum of the parts' aligned sizes
    CHECK(off[slots] % 256 == 0 && off[slots] - at == sum, "%zu bytes from %zu, parts %zu", off[slots] - at, at, sum);
}

// every property of Regions' slots: tr the table rows asked for, reg_end where the confidence plane's slot ends
static void check_reg(const RegLayout& r, size_t reg_end, size_t at, size_t npix, uint32_t tr) {
    const size_t rows = tr < npix ? tr : npix;
    CHECK(r.rows == rows && r.rows == min_rows(tr, npix), "rows %zu of %u asked, %zu pixels", r.rows, tr, npix);
    // n is one word in a slot of its own; the table's slot takes every staged row, the planes every pixel
    const size_t off[6] = {r.n, r.table, r.labels, r.klass, r.conf, reg_end};
    const size_t need[5] = {4, rows * 80, npix * 4, npix, npix};
    check_slots(off, need, 5, at);
    CHECK(r.table - r.n == 256, "the count's slot: %zu", r.table - r.n);
    // rows copied back: min(n, rows), whatever the device counted, and never past the slot
    const uint32_t ns[] = {0, 1, (uint32_t)(rows ? rows - 1 : 0), (uint32_t)rows, (uint32_t)(rows < 0xFFFFFFFFu ? rows + 1 : rows), 0xFFFFFFFFu};
    for (uint32_t n : ns) {
        const size_t got = copy_rows(n, r.rows);
        CHECK(got == (n < rows ? n : rows) && r.table + got * kRegionRowBytes <= r.labels, "n %u rows %zu: %zu copied", n, rows, got);
    }
}

int main() {
    const uint32_t kTop = 0xFFFFFFFFu;
    const struct { size_t w, h; } dims[] = {{0, 0}, {1, 1}, {1, 63}, {63, 1}, {1, 64}, {1, 65}, {61, 97}, {1, 4097}};
    const size_t starts[] = {0, 256, (size_t)1 << 40};
    const uint32_t arows[] = {0, 1, kTop};
    CHECK(kRegionRowBytes == 80 && kAnchorRowBytes == 8 && kSlotAlign == 256, "constants");
    for (const auto& d : dims) {
        const size_t npix = d.w * d.h;
        const size_t trs[] = {0, 1, npix, npix + 1, kTop};
        unsigned long long layouts = 0, sum = 0;
        for (size_t at : starts)
            for (size_t tr : trs) {
                const RegLayout r(at, npix, (uint32_t)tr);
                check_reg(r, r.end, at, npix, (uint32_t)tr);
                layouts++;
                sum += r.end - at;
                for (uint32_t ar : arows) {
                    const RegAnchLayout a(at, npix, (uint32_t)tr, ar);
                    check_reg(a, a.dist2, at, npix, (uint32_t)tr);  // (`end` is the anchors': checked below)
                    // Regions' slots are where RegLayout alone puts them, and Anchors' follow: every anchor row is written and copied
                    CHECK(a.n == r.n && a.table == r.table && a.labels == r.labels && a.klass == r.klass && a.conf == r.conf && a.dist2 == r.end,
                          "the extension moved a slot: %zu %zu", a.conf, a.dist2);
                    const size_t off[3] = {a.dist2, a.anchors, a.end};
                    const size_t need[2] = {npix * 4, (size_t)ar * 8};
                    check_slots(off, need, 2, r.end);
                    layouts++;
                    sum += a.end - at;
                }
            }
        std::printf("%zux%zu: %llu layouts, %llu bytes in all\n", d.w, d.h, layouts, sum);
    }
    // nothing wraps: the largest plane Regions takes (2^32 - 2 pixels), every row asked for, from the large start
    {
        const size_t npix = 0xFFFFFFFEull, at = (size_t)1 << 40;
        const RegAnchLayout a(at, npix, kTop, kTop);
        CHECK(a.rows == npix && a.end > a.anchors && a.anchors > a.dist2 && a.dist2 > a.conf && a.conf > a.klass && a.klass > a.labels &&
                  a.labels > a.table && a.table > a.n,
              "largest: %zu", a.end);
        CHECK(a.end - at == 256 + align_up(npix * 80, 256) + 2 * align_up(npix * 4, 256) + 2 * align_up(npix, 256) + align_up((size_t)kTop * 8, 256),
              "largest: %zu bytes", a.end - at);
        std::printf("largest: %zu bytes\n", a.end - at);
    }

    std::printf("%llu checks, %llu failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
