// egress_layout_test.cpp -- sweeps infur_amd/csrc/egress_layout.h, the staging layout and the row rules of the egress stages'
// host-pointer calls: these numbers decide how many bytes a copy moves into a caller's array.  Stand-alone and HIP-free:
// tests/test_egress_layout_cpu.py builds it with plain g++, once more under the address and undefined-behaviour sanitizers,
// and requires the same output of both.  A property that does not hold is printed and makes the exit status 1.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "egress_layout.h"

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

// every property of one layout: lr, vr the staged rows, k the staged classes, li, vi the input rows, pb the plane's bytes
static void check_layout(const PolyStage& st, size_t lr, size_t vr, uint32_t k, size_t li, size_t vi, size_t pb) {
    const size_t off[9] = {st.counts_out, st.counts_in, st.stats, st.loops, st.vertices, st.loops_in, st.vertices_in, st.plane, st.bytes};
    const size_t need[8] = {24, 8, (size_t)k * 64, lr * 16, vr * 4, li * 16, vi * 4, pb};
    CHECK(st.loops_rows == lr && st.vertex_rows == vr, "rows %zu %zu, wanted %zu %zu", st.loops_rows, st.vertex_rows, lr, vr);
    CHECK(off[0] == 0, "counts_out at %zu", off[0]);
    for (int i = 0; i < 8; i++) {
        CHECK(off[i] % 256 == 0, "slot %d at %zu", i, off[i]);
        CHECK(off[i + 1] >= off[i] && off[i + 1] - off[i] >= need[i], "slot %d: %zu .. %zu holds %zu", i, off[i], off[i + 1], need[i]);
        CHECK(off[i + 1] - off[i] < need[i] + 256, "slot %d: %zu .. %zu for %zu", i, off[i], off[i + 1], need[i]);  // zero costs nothing
    }
    CHECK(st.bytes % 256 == 0, "bytes %zu", st.bytes);
}

int main() {
    const uint32_t kTop = 0xFFFFFFFFu;
    const struct { size_t w, h; } dims[] = {{0, 0}, {0, 5}, {5, 0}, {1, 1}, {1, 63}, {63, 1}, {7, 9}, {1, 64}, {64, 1}, {8, 8},
                                            {1, 65}, {65, 1}, {5, 13}, {1, 4097}, {4097, 1}, {17, 241}};
    const uint32_t ks[] = {0, 1, 21, 256, 257}, rows_in[] = {0, 1, 1000};
    const size_t sizes[6] = {0, 1, 63, 64, 65, 4097};  // the products of `dims`
    size_t seen[6] = {0, 0, 0, 0, 0, 0};
    for (const auto& d : dims) {
        const size_t npix = d.w * d.h, lattice = (d.w + 1) * (d.h + 1);
        // the three per-frame maxima
        CHECK(frame_max_loops(npix) == npix && frame_max_vertices(npix) == 4 * npix, "npix %zu", npix);
        CHECK(frame_max_vertices_coverage(npix, d.w, d.h) == 4 * npix + lattice, "%zux%zu", d.w, d.h);
        unsigned long long sum = 0, layouts = 0;
        for (int cov = 0; cov < 2; cov++) {
            const size_t most_l = frame_max_loops(npix), most_v = cov ? frame_max_vertices_coverage(npix, d.w, d.h) : frame_max_vertices(npix);
            const size_t asked_l[] = {0, 1, most_l, most_l + 1, kTop}, asked_v[] = {0, 1, most_v, most_v + 1, kTop};
            for (size_t al : asked_l)
                for (size_t av : asked_v) {
                    if (al > kTop || av > kTop) continue;  // (a request is a u32)
                    const size_t lr = stage_rows(true, (uint32_t)al, most_l), vr = stage_rows(true, (uint32_t)av, most_v);
                    // a request above the maximum is clamped to the maximum, one below it is kept; no array, no rows
                    CHECK(lr == (al < most_l ? al : most_l) && vr == (av < most_v ? av : most_v), "asked %zu %zu of %zu %zu: %zu %zu", al, av, most_l, most_v, lr, vr);
                    CHECK(stage_rows(false, (uint32_t)al, most_l) == 0 && stage_rows(false, (uint32_t)av, most_v) == 0, "unwanted rows");
                    for (uint32_t k : ks) {
                        const uint32_t kc = staged_classes(true, k);
                        CHECK(kc == (k < 256 ? k : 256) && staged_classes(false, k) == 0, "k %u -> %u", k, kc);
                        for (uint32_t li : rows_in)
                            for (uint32_t vi : rows_in)
                                for (size_t pb : {(size_t)0, npix, 4 * npix}) {
                                    const PolyStage st(lr, vr, kc, li, vi, pb);
                                    check_layout(st, lr, vr, kc, li, vi, pb);
                                    sum += st.bytes;
                                    layouts++;
                                }
                    }
                }
        }
        std::printf("%zux%zu: %llu layouts, %llu bytes in all\n", d.w, d.h, layouts, sum);
        for (int i = 0; i < 6; i++)
            if (npix == sizes[i]) seen[i]++;
    }
    for (int i = 0; i < 6; i++) CHECK(seen[i] >= 1, "no plane of the %d-th size", i);

    // nothing wraps: the largest plane Outlines takes, and the largest lattice Coverage takes, with every slot at its maximum
    {
        const size_t npix = ((size_t)1 << 30) - 1, side = 8191;
        const size_t most_v = frame_max_vertices_coverage(npix, side, side);
        CHECK(most_v == 4 * npix + 8192 * 8192 && most_v > 4 * npix, "most_v %zu", most_v);
        const PolyStage st(npix, most_v, 256, npix, kTop, 4 * npix);
        check_layout(st, npix, most_v, 256, npix, kTop, 4 * npix);
        std::printf("largest: %zu bytes\n", st.bytes);
        const PolyScratch at(edge_capacity(npix, 0));
        CHECK(at.loops_rows == npix && at.vertex_rows == 4 * npix && at.loops == 256 && at.vertices >= at.loops + at.loops_rows * 16 &&
                  at.vertices % 256 == 0 && at.bytes >= at.vertices + at.vertex_rows * 4 && at.bytes % 256 == 0,
              "scratch %zu %zu %zu", at.loops, at.vertices, at.bytes);
    }
    // what Outlines leaves behind it: at least one record, a quarter of the edges, every edge's tail
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)3, (size_t)4, (size_t)7, (size_t)260, (size_t)16388}) {
        const PolyScratch at(cap);
        CHECK(at.loops_rows == (cap / 4 ? cap / 4 : 1) && at.vertex_rows == cap, "cap %zu", cap);
        CHECK(at.loops == 256 && at.vertices % 256 == 0 && at.vertices - at.loops >= at.loops_rows * 16 && at.bytes % 256 == 0 &&
                  at.bytes - at.vertices >= cap * 4,
              "cap %zu: %zu %zu %zu", cap, at.loops, at.vertices, at.bytes);
    }

    // rows to copy back
    for (size_t rows : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000, (size_t)kTop - 1}) {
        const uint32_t ns[] = {0, (uint32_t)(rows ? rows - 1 : 0), (uint32_t)rows, (uint32_t)(rows + 1), kTop};
        for (uint32_t n : ns) {
            CHECK(copy_rows(n, rows, true) == 0, "nothing: n %u rows %zu", n, rows);
            CHECK(copy_rows(n, rows, false) == (n < rows ? n : rows) && copy_rows(n, rows) == copy_rows(n, rows, false), "n %u rows %zu", n, rows);
            CHECK(copy_rows(n, rows) <= rows && copy_rows(n, rows) <= n, "n %u rows %zu", n, rows);
        }
    }
    // the edge capacity: 0 and anything above the worst case are the worst case
    for (size_t hw : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)4097, ((size_t)1 << 30) - 1}) {
        CHECK(edge_capacity(hw, 0) == 4 * hw, "hw %zu", hw);
        if (4 * hw + 1 <= kTop) CHECK(edge_capacity(hw, (uint32_t)(4 * hw + 1)) == 4 * hw, "hw %zu", hw);
        CHECK(edge_capacity(hw, kTop) == 4 * hw, "hw %zu", hw);
        if (hw >= 2) CHECK(edge_capacity(hw, 7) == 7, "hw %zu", hw);
        CHECK(edge_capacity(hw, (uint32_t)(4 * hw - 1)) == 4 * hw - 1 && edge_capacity(hw, (uint32_t)(4 * hw)) == 4 * hw, "hw %zu", hw);
    }
    CHECK(align_up(0, 256) == 0 && align_up(1, 256) == 256 && align_up(256, 256) == 256 && align_up(257, 256) == 512, "align_up");
    CHECK(kMaxSide == 8191 && kStatsMaxClasses == 256 && kSlotAlign == 256, "constants");

    std::printf("%llu checks, %llu failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
