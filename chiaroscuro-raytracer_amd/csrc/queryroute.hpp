// queryroute.hpp -- which kernels answer a caller's ray query (cr_intersect_device /
// cr_intersect_shadow_device), and the key its queue is sorted by.
//
// The render feeds the trace kernels only rays it made itself: origins at hit points inside the
// padded scene box, unit directions, finite everything.  A caller's rays promise none of that, so
// every query is routed by what each build's exactness rests on (DESIGN.md §3.18 lists where each
// precondition was read):
//   QR_DEFAULT  the scene's default trace build (59 at or above the leaf-cull triangle threshold,
//               else 44).  Its leaf cull records are exact only for origins inside the padded root
//               box widened by 1 per side: leaf_cull_fixed (leafcull.hpp) bakes the per-ray term
//               S = max |o_i - box_i| of the bound in as smax = the box's largest extent + 2
//               (cabi.cpp cr_upload_scene), and pads the boxes for |o_i| <= db (S.db; lc_grid_make
//               too) -- origins the render's hit points + 0.001 n always satisfy.  Unit directions
//               are checked per ray by the kernels themselves (lc_unit: any other direction tests
//               every reference).
//   QR_FAT      the fat-record kernels of build 44 without the leaf cull (tc::ClosestFat,
//               tc::ShadowFatFd): the reference's arithmetic step by step, for any finite ray --
//               the short division (FD) guards its own ranges (device_math.hpp rcp_for_div /
//               div_by_rcp_wave: out of range takes the full division).
//   QR_LEGACY   the per-thread traverse<> kernel (kernels.hip), which is what cr_intersect runs:
//               anything else, any non-finite component included, behaves as cr_intersect does by
//               construction.
// A zero direction is finite: it is routed by its origin like any other ray, every slab parameter
// is then +-inf or NaN, the traversal takes the near child at every node and ends at one leaf
// whose tests all reject (aa = 0) -- a miss on every route.
// Host and device, in the style of leafcull.hpp.
#pragma once
#include <math.h>
#include <stdint.h>

#include "leafcull.hpp"

namespace cr {

enum { QR_DEFAULT = 0, QR_FAT = 1, QR_LEGACY = 2 };

CR_LC_HD inline bool qr_finite(float v) { return fabsf(v) <= 3.402823466e+38f; } // false for NaN and +-inf

// o, d: the query's origin and direction; shadow queries also carry their limit (the distance up to
// which an occluder counts, in units of d) and the light triangle they ignore; bmin, bmax: the padded
// root box (DevScene::bmin / bmax, what cr_upload_scene derived smax from); db: DevScene::db.
// A light id with bit 31 set goes to QR_LEGACY: the shadow trace keeps a flag of the render's in that
// bit of its queue entry (wavefront.hip SEXCL_CONT) and masks it off the id it compares.
CR_LC_HD inline int query_route(const float o[3], const float d[3], bool shadow, float limit, uint32_t light,
                                const float bmin[3], const float bmax[3], float db) {
    for (int i = 0; i < 3; i++)
        if (!qr_finite(o[i]) || !qr_finite(d[i])) return QR_LEGACY;
    if (shadow && (!qr_finite(limit) || (light & 0x80000000u))) return QR_LEGACY;
    for (int i = 0; i < 3; i++)
        if (!(fabsf(o[i]) <= db) || !(o[i] >= bmin[i] - 1.f) || !(o[i] <= bmax[i] + 1.f)) return QR_FAT;
    return QR_DEFAULT;
}

// Octahedral direction bin, Morton order (wavefront.hip dir_bin's arithmetic); res: a power of two.
CR_LC_HD inline uint32_t query_dir_bin(const float d[3], uint32_t res) {
    const float s = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]);
    if (!(s > 0.f) || !qr_finite(s)) return 0u;
    float u = d[0] / s, v = d[2] / s;
    if (d[1] < 0.f) {
        const float uu = (1.f - fabsf(v)) * (u >= 0.f ? 1.f : -1.f), vv = (1.f - fabsf(u)) * (v >= 0.f ? 1.f : -1.f);
        u = uu;
        v = vv;
    }
    const float h = 0.5f * (float)res, top = (float)(res - 1u);
    const uint32_t bu = (uint32_t)fminf(top, fmaxf(0.f, (u + 1.f) * h));
    const uint32_t bv = (uint32_t)fminf(top, fmaxf(0.f, (v + 1.f) * h));
    uint32_t m = 0;
    for (uint32_t b = 0; (1u << b) < res; b++) m |= ((bu >> b) & 1u) << (2 * b + 1) | ((bv >> b) & 1u) << (2 * b);
    return m;
}

// The queue sort key of a finite query (wavefront.hip world_key's): a Morton code of the origin in
// the scene box [bmin, bmax], world_bits per axis, then the direction bin.  The cell is clamped as a
// float, before the conversion, so an origin far outside the box keeps a key below
// 2^(3 world_bits) * dir_res^2.  Any deterministic key is exact: it only orders the work.
CR_LC_HD inline uint32_t query_key(const float o[3], const float d[3], const float bmin[3], const float bmax[3],
                                   uint32_t world_bits, uint32_t dir_res) {
    const float sc = (float)(1u << world_bits);
    uint32_t q[3];
    for (int i = 0; i < 3; i++) {
        const float v = (o[i] - bmin[i]) / (bmax[i] - bmin[i]) * sc;
        q[i] = v == v ? (uint32_t)fminf(sc - 1.f, fmaxf(0.f, v)) : 0u; // (NaN: a flat box)
    }
    uint32_t m = 0;
    for (uint32_t b = 0; b < world_bits; b++)
        m |= ((q[0] >> b) & 1u) << (3 * b + 2) | ((q[1] >> b) & 1u) << (3 * b + 1) | ((q[2] >> b) & 1u) << (3 * b);
    return m * (dir_res * dir_res) + query_dir_bin(d, dir_res);
}

} // namespace cr
