// infur_tuner.cpp -- which tile configuration of the conv kernels runs a layer shape: measured on first use (pick_cfg), kept per
// context, pre-loadable from / exportable to text (infur_tune_import / _export; infur_amd/conv_tune_gfx950.txt holds the decisions
// for the BASELINE shapes).  Every configuration of a mode gives bit-identical results (tests/test_gpu_forms.py,
// test_gpu_conv_configs.py, test_gpu_hl.py), so the choice is a speed knob only.  Split out of infur_capi.cpp in round 5.
#include "../../include/infur_hip.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "infur_rt.h"

using namespace infur;

namespace infur {

// ---- tile configuration of the conv kernel for one problem shape ----
// The first time a shape is seen (a new frame size), every candidate configuration is launched
// for real on the actual operands and timed with HIP events; the fastest is remembered for the
// context's lifetime.  All configurations give bit-identical outputs, so the trial launches are
// simply redundant evaluations of the layer.

int32_t pick_cfg(infur_ctx* c, const ConvArgs& a, ConvMode mode, int out_f32, int* cfg) {
    *cfg = conv_igemm_default_config(a);
    if (mode == kModeHL && !conv_igemm_config_valid(a, *cfg, mode, out_f32)) *cfg = kCfg128x128;  // (valid for every mode-5 shape)
    // test hook: INFUR_CONV_CFG=<k> forces configuration k wherever it is a candidate.  A forced configuration that is NOT a
    // candidate for the shape falls back to the default silently; tests/test_gpu_forms.py is what checks, from the profile's kernel
    // names, that the forced form really ran.
    static const int forced = getenv("INFUR_CONV_CFG") ? atoi(getenv("INFUR_CONV_CFG")) : -1;
    if (forced >= 0) {
        if (conv_igemm_config_valid(a, forced, mode, out_f32)) *cfg = forced;
        return INFUR_OK;
    }
    if (c->opt.no_autotune) return INFUR_OK;
    const TuneKey key = tune_key(a, mode, out_f32);
    auto it = c->tuned.find(key);
    if (it != c->tuned.end() && conv_igemm_config_valid(a, it->second, mode, out_f32)) {
        *cfg = it->second;
        return INFUR_OK;
    }
    EventPair ev;
    HIPCHK(c, ev.create());
    if (!c->tune_warm) {  // bring clocks and caches to their steady state before the first measurement
        for (int r = 0; r < 12; r++) HIPCHK(c, launch_conv_igemm(a, mode, out_f32, *cfg, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->tune_warm = true;
    }
    float best = 1e30f;
    std::vector<std::pair<int, float>> timed;
    static const bool tune_halo256 = getenv("INFUR_TUNE_HALO256") != nullptr;  // times what the table marks untunable (kCfgHalo256)
    for (int k = 0; k < kNumConvCfgs; k++) {
        if (!conv_igemm_config_valid(a, k, mode, out_f32)) continue;
        if (!conv_form(k, mode)->tunable && !tune_halo256) continue;
        // a candidate that cannot launch on this shape after all (invalid value) is skipped, not fatal: the layer still
        // has the other configurations; anything else (a fault, a lost device) is an error of the frame
        const hipError_t le = launch_conv_igemm(a, mode, out_f32, k, c->stream);  // warm-up (attributes, caches)
        if (le == hipErrorInvalidValue) continue;
        HIPCHK(c, le);
        float fastest;  // minimum of 4 single-launch timings
        RETIF(min_launch_ms(c, ev, 0, 4, &fastest, [&] { return launch_conv_igemm(a, mode, out_f32, k, c->stream); }));
        timed.emplace_back(k, fastest);
        if (fastest < best) {
            best = fastest;
            *cfg = k;
        }
    }
    // Tie-break towards the larger tile: among the configurations within 2 % of the fastest, the one with the largest
    // BM x BN re-reads its operands least (A once per N tile, B once per M tile) -- the same speed for less L2 / Infinity
    // Cache / HBM traffic, which is also what leaves room for a second frame in flight.  (ConvForm::tie_area: not always the tile)
    for (const auto& kt : timed)
        if (kt.second <= best * 1.02f && conv_form(kt.first, mode)->tie_area > conv_form(*cfg, mode)->tie_area) *cfg = kt.first;
    c->tuned[key] = *cfg;
    c->mem_gen++;  // (a new decision: frames captured as graphs before it are stale)
    return INFUR_OK;
}

int32_t run_tuned(infur_ctx* c, const std::string& layer, const ConvArgs& a, ConvMode mode, int out_f32, double flops, double bytes, double algo_flops) {
    int cfg = -1;
    RETIF(pick_cfg(c, a, mode, out_f32, &cfg));
    ProfScope ps(c, layer, conv_igemm_config_name(cfg, mode), flops, bytes, algo_flops);
    if (ps.on) ps.r.variant = conv_variant_name(a, mode, cfg, out_f32);
    HIPCHK(c, launch_conv_igemm(a, mode, out_f32, cfg, c->stream));
    return INFUR_OK;
}

}  // namespace infur

extern "C" {

// ---- tuning database ----
int32_t infur_tune_export(infur_ctx* c, char* buf, size_t cap, size_t* len) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || !len) return INFUR_E_INVALID_ARG;
        std::string out;
        char line[256];
        for (const auto& kv : c->tuned) {
            int n = 0;
            for (int v : kv.first) n += snprintf(line + n, sizeof line - n, "%d ", v);
            snprintf(line + n, sizeof line - n, "%d\n", kv.second);
            out += line;
        }
        *len = out.size();
        if (!buf) return INFUR_OK;
        if (cap < out.size()) return fail(c, INFUR_E_CAPACITY, "tuning text needs %zu bytes", out.size());
        memcpy(buf, out.data(), out.size());
        return INFUR_OK;
    });
}

int32_t infur_tune_import(infur_ctx* c, const char* text, size_t len) {
    return abi_call(c, [&]() -> int32_t {
        if (!c || (!text && len)) return INFUR_E_INVALID_ARG;
        std::string t(text ? text : "", len);
        size_t pos = 0;
        while (pos < t.size()) {
            size_t eol = t.find('\n', pos);
            if (eol == std::string::npos) eol = t.size();
            const std::string ln = t.substr(pos, eol - pos);
            pos = eol + 1;
            if (ln.empty() || ln[0] == '#') continue;
            TuneKey key;
            int cfg = -1, off = 0, n = 0;
            bool ok = true;
            for (int i = 0; i < 13 && ok; i++) {
                ok = sscanf(ln.c_str() + off, "%d%n", &key[i], &n) == 1;
                off += n;
            }
            ok = ok && sscanf(ln.c_str() + off, "%d", &cfg) == 1;
            if (!ok || cfg < 0 || cfg >= kNumConvCfgs) return fail(c, INFUR_E_INVALID_ARG, "bad tuning line: %s", ln.c_str());
            c->tuned[key] = cfg;
            c->mem_gen++;
        }
        return INFUR_OK;
    });
}

}  // extern "C"
