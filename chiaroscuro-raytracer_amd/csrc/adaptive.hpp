// adaptive.hpp -- the host plan of the adaptive render (cr_render_adaptive, cr_render_layers_list_device), as pure
// functions in the style of wfplan.hpp: when the noise is checked, and how a group of layers over a pixel list is
// cut into render passes.  Nothing here calls the HIP runtime; tests/native/adaptive_check.cpp runs all of it on
// the CPU.
#pragma once
#include "wfplan.hpp"

#include <vector>

namespace cr {

// ---- the check schedule ----
// One step of cr_render_adaptive from L layers done: render n = min(check_every, max_layers - L) layers, then check
// iff L + n >= min_layers.  Checks so happen at the multiples of check_every that are >= min_layers, and at
// max_layers; the schedule is a function of the three parameters alone -- never of what fits a pass, or a pixel's
// layer count would depend on free memory.
struct AdStep {
    uint32_t n;
    bool check;
};
inline AdStep ad_step(uint32_t L, uint32_t min_layers, uint32_t max_layers, uint32_t check_every) {
    const uint32_t n = std::min(check_every, max_layers - L);
    return {n, L + n >= min_layers};
}
// the layers at which a render that never runs out of active pixels checks, ascending (the last is max_layers)
inline std::vector<uint32_t> ad_checks(uint32_t min_layers, uint32_t max_layers, uint32_t check_every) {
    std::vector<uint32_t> at;
    for (uint32_t L = 0; L < max_layers;) {
        const AdStep s = ad_step(L, min_layers, max_layers, check_every);
        L += s.n;
        if (s.check) at.push_back(L);
    }
    return at;
}

// ---- the passes of a list render ----
// A pass renders layers [layer0, layer0 + nl) (offsets from the group's first layer) for list entries
// [first, first + count).  Its work items are the entries padded with skipped ones to a multiple of tile * tile
// (ad_padded): every place that takes n_items % (tile * tile) == 0 -- wf_plan's nkeys, the pixel sort keys -- keeps
// its invariant.
struct AdPass {
    uint32_t first, count, layer0, nl;
};
struct AdPlanIn {
    uint32_t m = 0;          // list entries
    uint32_t n = 0;          // layers of the group
    uint32_t spp = 1, tile = 32;
    uint32_t max_nl = 32;    // the most layers of one pass (1: the counting build, two lanes)
    uint64_t paths_cap = ~0ull, sample_buf = 0; // wf_layers_fit's: the ctx's path cap and sample buffer
};
inline uint64_t ad_padded(uint32_t count, uint32_t tile) {
    const uint64_t TT = (uint64_t)tile * tile;
    return ((uint64_t)count + TT - 1) / TT * TT;
}
// true: the pass is one path chunk and one sample buffer (wf_layers_fit).  The one pass that need not be: a single
// layer of at most tile * tile entries, the smallest there is -- run_render cuts it into sample and path chunks.
inline bool ad_pass_fits(const AdPlanIn &in, const AdPass &p) {
    return wf_layers_fit(ad_padded(p.count, in.tile), in.spp, p.nl, in.paths_cap, in.sample_buf);
}
// The plan: the list in the fewest contiguous ranges whose single layer fits (whole tiles of entries; the whole list
// when it fits), each range's layers in the fewest groups that fit, range after range -- every (entry, layer) once,
// a pixel's layers ascending.
inline std::vector<AdPass> ad_plan(const AdPlanIn &in) {
    std::vector<AdPass> plan;
    if (!in.m || !in.n) return plan;
    const uint64_t TT = (uint64_t)in.tile * in.tile;
    auto fits = [&](uint64_t items, uint32_t nl) { return wf_layers_fit(items, in.spp, nl, in.paths_cap, in.sample_buf); };
    // entries per range: the most whole tiles whose single layer fits, at least one tile
    uint64_t range = ad_padded(in.m, in.tile);
    if (!fits(range, 1)) {
        uint64_t lo = 1, hi = range / TT; // tiles: lo fits or is the minimum, hi does not fit
        while (lo + 1 < hi) {
            const uint64_t mid = (lo + hi) / 2;
            (fits(mid * TT, 1) ? lo : hi) = mid;
        }
        range = lo * TT;
    }
    for (uint64_t first = 0; first < in.m; first += range) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(range, in.m - first);
        const uint64_t items = ad_padded(count, in.tile);
        for (uint32_t l = 0; l < in.n;) {
            uint32_t nl = std::min(std::max(in.max_nl, 1u), in.n - l);
            while (nl > 1 && !fits(items, nl)) nl--;
            plan.push_back({(uint32_t)first, count, l, nl});
            l += nl;
        }
    }
    return plan;
}

} // namespace cr
