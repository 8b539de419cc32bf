// temporal.hpp -- the host plan of temporal reprojection (cr_reproject_device, cr_render_temporal; include/chiaro_hip.h
// "temporal reprojection"), as pure functions in the style of denoise.hpp: the parameter checks, the projector of the
// previous camera and the layout of the ctx's history.  Nothing here calls the HIP runtime;
// tests/test_temporal_abi.py compiles and runs all of it on the CPU.
#pragma once
#include "chiaro_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace cr {

// The layout of the history cr_render_temporal keeps between frames: the five planar arrays alone (0), or beside
// them the packed record the kernel then taps -- 3 float4 per pixel, {H, K bits}, {H2, Zp}, {Np, 0} (1).  Both
// write the same bits; what was measured and why this one is kept: DESIGN.md §3.27.
enum : uint32_t { TP_CTX_PACKED = 0 };

inline void tp_defaults(cr_temporal_params &p) {
    p.depth_tol = 0.05f;
    p.normal_min = 0.9f;
    p.max_history = 65536;
}

// ---- validation ----
// null: usable; else the message of the CR_E_INVALID they earn (arithmetic on the arguments only)
inline const char *tp_check_params(const cr_temporal_params *p) {
    if (!p) return "null temporal params";
    if (!(p->depth_tol > 0.f) || std::isinf(p->depth_tol)) return "temporal depth_tol must be > 0 and finite";
    if (!std::isfinite(p->normal_min)) return "temporal normal_min must be finite";
    if (!p->max_history) return "temporal max_history must be > 0";
    return nullptr;
}
inline const char *tp_check_shape(uint32_t xres, uint32_t yres) {
    if (!xres || !yres) return "xres/yres must be > 0";
    if ((uint64_t)xres * yres > (1ull << 31)) return "image too large";
    return nullptr;
}

// ---- the projector of the previous camera ----
// P = eye_p + t * (lu_p + u * dx_p + v * dy_p) solved for (t, t u, t v) by Cramer's rule: with q = P - eye_p,
// t = dot(q, ra) / det, u = dot(q, rb) / dot(q, ra), v = dot(q, rc) / dot(q, ra).  float32, the operations in the
// header's order (the build has no contraction).
struct TpProjector {
    float ra[3], rb[3], rc[3], det;
};
inline void tp_cross(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
inline float tp_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// false: det is not finite or is 0 (CR_E_INVALID)
inline bool tp_projector(const cr_camera &prev, TpProjector &o) {
    tp_cross(prev.dx, prev.dy, o.ra);
    tp_cross(prev.dy, prev.left_upper, o.rb);
    tp_cross(prev.left_upper, prev.dx, o.rc);
    o.det = tp_dot(prev.left_upper, o.ra);
    return std::isfinite(o.det) && o.det != 0.f;
}

// ---- the ctx's history ----
// One side of the double buffer, 256-B aligned parts of one allocation: frame and m2 [npix][3], count [npix],
// normal [npix][3], depth [npix], and (packed) the record [npix][3] float4.  The current frame's own buffers --
// frame, m2, albedo (the filter's guide) -- follow the two sides.
struct TpScratch {
    size_t frame = 0, m2 = 0, count = 0, normal = 0, depth = 0, rec = 0, side = 0; // offsets in a side, its bytes
    size_t cur_frame = 0, cur_m2 = 0, cur_albedo = 0, bytes = 0;                   // offsets in the whole
};
inline size_t tp_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline TpScratch tp_scratch(uint64_t npix, bool packed) {
    TpScratch s;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t at = off; off += tp_align(b); return at; };
    s.frame = take((size_t)npix * 12);
    s.m2 = take((size_t)npix * 12);
    s.count = take((size_t)npix * 4);
    s.normal = take((size_t)npix * 12);
    s.depth = take((size_t)npix * 4);
    s.rec = off;
    if (packed) take((size_t)npix * 48);
    s.side = off;
    off = 2 * s.side;
    s.cur_frame = take((size_t)npix * 12);
    s.cur_m2 = take((size_t)npix * 12);
    s.cur_albedo = take((size_t)npix * 12);
    s.bytes = off;
    return s;
}

} // namespace cr
