// denoise.hpp -- the host plan of the guide buffers and the a-trous filter (cr_guides*, cr_denoise*; include/chiaro_hip.h
// "guide buffers and denoiser"), as pure functions in the style of adaptive.hpp / wfplan.hpp: parameter validation, the
// level schedule and the scratch layout.  Nothing here calls the HIP runtime; tests/test_denoise_abi.py compiles and
// runs all of it on the CPU.
#pragma once
#include "chiaro_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cr {

enum : uint32_t { DN_MAX_LEVELS = 8, DN_MAX_SQUARINGS = 8 };
// the a-trous kernel's tile (one 256-thread block) and the largest step whose tile plus halo is staged in LDS:
// (32 + 4 s) x (8 + 4 s) pixels of 48 B -- 20.25 KiB at step 1, 30 KiB at step 2 (what won: DESIGN.md §3.25)
enum : uint32_t { DN_TILE_X = 32, DN_TILE_Y = 8, DN_LDS_MAX_STEP = 2 };

inline void dn_defaults(cr_denoise_params &p) {
    p.levels = 4;
    p.sigma_l = 4.0f;
    p.sigma_z = 0.1f;
    p.sigma_a = 0.1f;
    p.normal_squarings = 5;
}

// ---- validation ----
// null: the parameters and the shape are usable; else the message of the CR_E_INVALID they earn.  All of it is
// arithmetic on the arguments: it is answered before any device is looked at.
inline const char *dn_check_params(const cr_denoise_params *p) {
    if (!p) return "null denoise params";
    if (p->levels > DN_MAX_LEVELS) return "denoise levels must be <= 8";
    if (p->normal_squarings > DN_MAX_SQUARINGS) return "denoise normal_squarings must be <= 8";
    for (float s : {p->sigma_l, p->sigma_z, p->sigma_a})
        if (!(s > 0.f) || std::isinf(s)) return "denoise sigmas must be > 0 and finite";
    return nullptr;
}
inline const char *dn_check_shape(uint32_t xres, uint32_t yres, uint32_t layers, uint32_t spp) {
    if (!xres || !yres) return "xres/yres must be > 0";
    if ((uint64_t)xres * yres > (1ull << 31)) return "image too large";
    if ((uint64_t)layers * spp == 0) return "layers * spp must be > 0";
    if ((uint64_t)layers * spp > 0xFFFFFFFFull) return "layers * spp must fit 32 bits";
    return nullptr;
}

// ---- the level schedule ----
// Level i filters with step 1 << i from ping-pong frame `src` into `dst` (0 / 1: the scratch's two frames); the
// last level writes the caller's outputs instead (dst -1).  The initial variance goes into frame 0 -- or, with no
// level at all, straight to the outputs (dn_levels then is empty and var_init is the whole filter).
struct DnLevel {
    uint32_t step;
    int src, dst; // dst -1: the outputs
    bool lds;     // the tile plus halo staged in LDS (steps <= DN_LDS_MAX_STEP), else every tap through L2
};
inline std::vector<DnLevel> dn_levels(uint32_t levels) {
    std::vector<DnLevel> v;
    for (uint32_t i = 0; i < levels; i++) {
        const uint32_t s = 1u << i;
        v.push_back({s, (int)(i & 1u), i + 1 == levels ? -1 : (int)((i + 1) & 1u), s <= DN_LDS_MAX_STEP});
    }
    return v;
}

// ---- scratch ----
// One grow-only buffer of the ctx, 256-B aligned parts: the packed guide record (2 float4 per pixel:
// {albedo, depth}, {normal, 0}) and the ping-pong frames (float4 per pixel: {colour, variance}; the second only
// when more than one level runs, none without a level).
struct DnScratch {
    size_t guide = 0, frame[2] = {0, 0}, bytes = 0;
};
inline size_t dn_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline DnScratch dn_scratch(uint64_t npix, uint32_t levels) {
    DnScratch s;
    s.guide = 0;
    s.bytes = levels ? dn_align((size_t)npix * 32) : 0;
    for (uint32_t i = 0; i < 2; i++) {
        s.frame[i] = s.bytes;
        if (levels > i) s.bytes += dn_align((size_t)npix * 16);
    }
    return s;
}
// cr_guides_device's rays and hits for npix pixels: origins and directions [npix][3], hit and triangle [npix],
// barycentrics [npix][2], distance [npix]
struct GuideScratch {
    size_t orig = 0, dir = 0, hit = 0, tri = 0, bary = 0, dist = 0, bytes = 0;
};
inline GuideScratch guide_scratch(uint64_t npix) {
    GuideScratch g;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t at = off; off += dn_align(b); return at; };
    g.orig = take((size_t)npix * 12);
    g.dir = take((size_t)npix * 12);
    g.hit = take((size_t)npix * 4);
    g.tri = take((size_t)npix * 4);
    g.bary = take((size_t)npix * 8);
    g.dist = take((size_t)npix * 4);
    g.bytes = off;
    return g;
}

} // namespace cr
