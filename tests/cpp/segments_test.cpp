// Exercises infur::Segments of include/infur_processor.hpp (ColorCode's sibling: class / confidence planes, statistics).
//   segments_test cpu   -- the surface that needs no GPU: feature bit, class names, command validation
//   segments_test gpu   -- the RAW decode on the decode_0to1 input (decode_predict.rs:100-116) against an in-file restatement
//                          of decode_predict.rs:67-78, and the statistics table of a two-class image
#include <cstdio>
#include <cstring>
#include <vector>

#include "infur_processor.hpp"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int cpu_tests() {
    CHECK(infur_abi_version() == INFUR_ABI_VERSION);
    CHECK(infur_features() & INFUR_FEATURE_SEGMENTS);
    CHECK(!std::strcmp(infur_voc_class_name(0), "__background__") && !std::strcmp(infur_voc_class_name(15), "person"));
    CHECK(infur_voc_class_name(21) == nullptr);
    CHECK(INFUR_STAT_WORDS == 8 && INFUR_STAT_MAX_Y == 7);
    uint8_t b[16] = {0};
    CHECK(infur_segments(nullptr, nullptr, 1, 4, 4, INFUR_DECODE_RAW, b, nullptr, nullptr, nullptr) == INFUR_E_INVALID_ARG);
    std::printf("cpu ok\n");
    return 0;
}

// decode_predict.rs:67-78 for one pixel: k_max = 0, c_max = 0.0, strict '>'; (c_max * 255.0) as u8
static void raw_rule(const infur::Tensor3& t, size_t p, int* k_max, int* conf) {
    *k_max = 0;
    float c_max = 0.0f;
    const size_t hw = (size_t)t.h * t.w;
    for (uint32_t k = 0; k < t.k; k++) {
        const float c = t.data[k * hw + p];
        if (c > c_max) {
            *k_max = (int)k;
            c_max = c;
        }
    }
    volatile float a = c_max * 255.0f;
    *conf = a >= 255.0f ? 255 : (int)a;
}

static int gpu_tests() {
    infur::Context c(0);
    CHECK(c.ok());
    infur::Segments seg(c);
    CHECK(seg.is_dirty());
    CHECK(seg.control(2) == INFUR_E_INVALID_ARG);
    CHECK(seg.control(INFUR_DECODE_RAW) == INFUR_OK && !seg.is_dirty());
    // decode_0to1
    {
        infur::Tensor3 hm;
        hm.k = 22; hm.h = 24; hm.w = 32;
        const size_t n = (size_t)22 * 24 * 32, hw = (size_t)24 * 32;
        hm.data.resize(n);
        for (size_t i = 0; i < n; i++) hm.data[i] = (float)((double)i / (double)(n - 1));
        infur::SegmentsOut out;
        out.want_rgba = true;
        CHECK(seg.advance(hm, out) == INFUR_OK && !seg.is_dirty());
        CHECK(out.width == 32 && out.height == 24 && out.classes == 22);
        CHECK(out.klass.size() == hw && out.conf.size() == hw && out.rgba.size() == hw * 4 && out.stats.size() == 22u * INFUR_STAT_WORDS);
        std::optional<infur::ColorImage> img;
        CHECK(infur::ColorCode(c).advance(hm, img) == INFUR_OK);
        CHECK(img->rgba == out.rgba);  // RAW mode: exactly ColorCode's bytes
        uint64_t sum_conf = 0;
        int last = 0;
        for (size_t p = 0; p < hw; p++) {
            int k, a;
            raw_rule(hm, p, &k, &a);
            CHECK(out.klass[p] == k && out.conf[p] == a);
            CHECK(k == 21 && a >= last);
            last = a;
            sum_conf += (uint64_t)a;
        }
        CHECK(last == 255);
        CHECK(out.stat(21, INFUR_STAT_PIXELS) == hw && out.stat(21, INFUR_STAT_SUM_CONF) == sum_conf);
        CHECK(out.stat(21, INFUR_STAT_MIN_X) == 0 && out.stat(21, INFUR_STAT_MAX_X) == 31 && out.stat(21, INFUR_STAT_MAX_Y) == 23);
        CHECK(out.stat(3, INFUR_STAT_PIXELS) == 0 && out.stat(3, INFUR_STAT_MIN_X) == UINT64_MAX && out.stat(3, INFUR_STAT_MAX_X) == 0);
    }
    // two classes: class 2 fills the rectangle x 70..99, y 5..11 of a 130 x 20 image (two tiles wide), class 0 the rest
    {
        infur::Tensor3 t;
        t.k = 3; t.h = 20; t.w = 130;
        const size_t hw = (size_t)t.h * t.w;
        t.data.assign(3 * hw, 0.0f);
        uint64_t n2 = 0, sx = 0, sy = 0;
        for (uint32_t y = 5; y <= 11; y++)
            for (uint32_t x = 70; x <= 99; x++) {
                t.data[2 * hw + (size_t)y * t.w + x] = 0.5f;
                n2++;
                sx += x;
                sy += y;
            }
        infur::SegmentsOut out;
        CHECK(seg.advance(t, out) == INFUR_OK);
        CHECK(out.rgba.empty());
        CHECK(out.stat(2, INFUR_STAT_PIXELS) == n2 && out.stat(2, INFUR_STAT_SUM_X) == sx && out.stat(2, INFUR_STAT_SUM_Y) == sy);
        CHECK(out.stat(2, INFUR_STAT_SUM_CONF) == 127 * n2);
        CHECK(out.stat(2, INFUR_STAT_MIN_X) == 70 && out.stat(2, INFUR_STAT_MAX_X) == 99);
        CHECK(out.stat(2, INFUR_STAT_MIN_Y) == 5 && out.stat(2, INFUR_STAT_MAX_Y) == 11);
        CHECK(out.stat(0, INFUR_STAT_PIXELS) == hw - n2 && out.stat(0, INFUR_STAT_SUM_CONF) == 0);
        CHECK(out.stat(0, INFUR_STAT_MIN_X) == 0 && out.stat(0, INFUR_STAT_MAX_X) == 129 && out.stat(0, INFUR_STAT_MAX_Y) == 19);
        CHECK(out.stat(1, INFUR_STAT_PIXELS) == 0 && out.stat(1, INFUR_STAT_MIN_Y) == UINT64_MAX);
        CHECK(out.klass[(size_t)5 * t.w + 70] == 2 && out.conf[(size_t)5 * t.w + 70] == 127 && out.klass[0] == 0 && out.conf[0] == 0);
        // the softmax of (0, 0, 0.5) and of (0, 0, 0): class 2 wins inside, the first maximum (0) outside, p = 1/3 -> 85
        CHECK(seg.control(INFUR_DECODE_SOFTMAX) == INFUR_OK && seg.is_dirty());
        CHECK(seg.advance(t, out) == INFUR_OK);
        CHECK(out.klass[(size_t)5 * t.w + 70] == 2 && out.klass[0] == 0 && out.conf[0] == 85);
        CHECK(out.stat(2, INFUR_STAT_PIXELS) == n2 && out.stat(0, INFUR_STAT_SUM_CONF) == 85 * (hw - n2));
    }
    std::printf("gpu ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "gpu")) return gpu_tests();
    return cpu_tests();
}
