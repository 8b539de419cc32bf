// probe.hpp -- SH irradiance probes (cr_probe_sh* / cr_probe_eval* / cr_probe_sample*; include/chiaro_hip.h "probes",
// DESIGN.md §3.30), as pure functions in the style of bake.hpp: the argument checks, and the one C++ statement of the
// definition -- the sphere direction, the L2 basis, the projection's fold and blend, the evaluation and the grid
// lookup -- that probe.hip's and wavefront.hip's kernels and the host restatement below both compile.  Nothing here
// calls the HIP runtime; tests/native/probe_check.cpp runs all of it on the CPU.  float32, every operation rounded
// once, in the order written, no contraction; the two steps marked double are double.
//
// What include/chiaro_hip.h leaves to this file:
//   max(0, v)      is v > 0 ? v : 0 (a NaN or -0 gives +0), in the direction's radius and the evaluation's clamp
//   the clamp      of the grid coordinate is f > 0 ? f : 0 first (a NaN gives 0), then f < hi ? f : hi, with
//                  hi = (float)(dims - 1)
//   every sum      starts from +0 and adds its terms one by one (so a lone -0 term gives +0)
//   the sine       is the host libm's sinf / cosf on the CPU and device_math.hpp's restatement of it in a kernel
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "device_math.hpp"
#define PROBE_FN __host__ __device__ __forceinline__
#else
#define PROBE_FN inline
#endif

namespace cr {

enum : uint32_t { PROBE_K = 9, PROBE_F = 27 }; // coefficients per channel, floats per probe: sh[k][c]

// cr_probe_grid's layout (include/chiaro_hip.h; cabi.cpp asserts the two agree)
struct ProbeGrid {
    float origin[3], step[3];
    uint32_t dims[3];
};

// ---- validation (arithmetic on the arguments: answered before any device is looked at) ----
PROBE_FN bool probe_finite(float v) {
    return v - v == 0.f; // (inf - inf and NaN - NaN are NaN)
}
// cr_probe_sh / cr_probe_sh_device, after radiance.hpp's rad_check of (n, params, layers): the size of the 27 n floats;
// max_floats: the most floats an array may hold (the platform's, a parameter so that the CPU check can reach it)
inline const char *probe_check_size(uint32_t n, uint64_t max_floats = SIZE_MAX / sizeof(float)) {
    if ((uint64_t)n > max_floats / PROBE_F) return "27 * n floats overflow a size";
    return nullptr;
}
inline const char *probe_check_grid(const ProbeGrid *g) {
    if (!g) return "null probe grid";
    uint64_t count = 1;
    for (int a = 0; a < 3; a++) {
        if (!g->dims[a]) return "probe grid dims must be > 0";
        count *= g->dims[a];
        if (count > 0xffffffffull) return "probe grid too large (more than 0xffffffff probes)";
    }
    for (int a = 0; a < 3; a++)
        if (!probe_finite(g->origin[a])) return "probe grid origin must be finite";
    for (int a = 0; a < 3; a++)
        if (g->dims[a] > 1 && !(probe_finite(g->step[a]) && g->step[a] > 0.f))
            return "probe grid step must be finite and > 0 on every axis with dims > 1";
    return nullptr;
}
inline uint64_t probe_grid_count(const ProbeGrid &g) { return (uint64_t)g.dims[0] * g.dims[1] * g.dims[2]; }
// true: [a, a + na) and [b, b + nb) bytes share a byte
inline bool probe_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}
// cr_probe_eval*: arrays = sh, probe, nrm and out are given (m == 0 needs none); sh is taken as one probe at least
inline const char *probe_check_eval(uint32_t m, bool arrays, const void *sh, uint64_t n_probes, const void *out) {
    if (m && !arrays) return "null sh / probe / normal / output arrays";
    if (m && probe_overlap(out, (uint64_t)m * 3 * sizeof(float), sh, (n_probes ? n_probes : 1) * PROBE_F * sizeof(float)))
        return "probe output must not alias the coefficients";
    return nullptr;
}
// cr_probe_sample*: the grid first, then the arrays
inline const char *probe_check_sample(const ProbeGrid *g, uint32_t m, bool arrays, const void *sh, const void *out) {
    if (const char *msg = probe_check_grid(g)) return msg;
    if (m && !arrays) return "null sh / position / normal / output arrays";
    if (m && probe_overlap(out, (uint64_t)m * 3 * sizeof(float), sh, probe_grid_count(*g) * PROBE_F * sizeof(float)))
        return "probe output must not alias the coefficients";
    return nullptr;
}

// ---- the sphere direction ----
// rng_uniform(rng, 0, 1) of one raw 32-bit draw (device_math.hpp rng_uniform: generate_canonical, then c (b - a) + a)
PROBE_FN float probe_uniform(uint32_t raw) {
    float c = (float)raw / 4294967296.0f;
    if (c >= 1.0f) c = 0x1.fffffep-1f;
    return c * (1.f - 0.f) + 0.f;
}
PROBE_FN float probe_max0(float v) { return v > 0.f ? v : 0.f; }
PROBE_FN void probe_sincos(float phi, float &sn, float &cs) {
#if defined(__HIP_DEVICE_COMPILE__)
    cr_sincosf(phi, sn, cs);
#else
    sn = sinf(phi);
    cs = cosf(phi);
#endif
}
// draws 0 and 1 of the sample's stream -> d[3], uniform over the sphere (density 1 / 4 pi), not renormalised
PROBE_FN void probe_dir(uint32_t raw0, uint32_t raw1, float *d) {
    const float u0 = probe_uniform(raw0), u1 = probe_uniform(raw1);
    const float z = u0 * 2.f + (-1.f);
    const float r = sqrtf(probe_max0(1.f - z * z));
    const float phi = (float)((double)u1 * 6.283185307179586);
    float sn, cs;
    probe_sincos(phi, sn, cs);
    d[0] = r * cs;
    d[1] = r * sn;
    d[2] = z;
}

// ---- the basis: the real L2 set, constants as float32 ----
PROBE_FN void probe_basis(float x, float y, float z, float *Y) {
    const float K0 = 0.28209479f, K1 = 0.48860251f, K2 = 1.0925484f, K3 = 0.31539157f, K4 = 0.54627422f;
    Y[0] = K0;
    Y[1] = K1 * y;
    Y[2] = K1 * z;
    Y[3] = K1 * x;
    Y[4] = K2 * (x * y);
    Y[5] = K2 * (y * z);
    Y[6] = K3 * (3.f * (z * z) - 1.f);
    Y[7] = K2 * (x * z);
    Y[8] = K4 * (x * x - y * y);
}
// the cosine lobe's band factors A_l / pi: 1, 2/3, 1/4
PROBE_FN float probe_band(int k) { return k == 0 ? 1.f : k < 4 ? (float)(2.0 / 3.0) : 0.25f; }

// ---- the projection ----
// one sample: t[k][c] += p, q[k][c] += p p with p = Y_k r[c] rounded (q null: no moments)
PROBE_FN void probe_accum(const float *Y, const float *r, float *t, float *q) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < (int)PROBE_K; k++)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int c = 0; c < 3; c++) {
            const float p = Y[k] * r[c];
            t[3 * k + c] = t[3 * k + c] + p;
            if (q) q[3 * k + c] = q[3 * k + c] + p * p;
        }
}
// a layer's sum t blended onto the stored value (sum_samples' write_pixel; write_moment for q): old is not read --
// taken as 0 -- for layer 1
PROBE_FN float probe_blend(float old, float t, float inv_spp, uint32_t layer) {
    const float o = layer > 1 ? old : 0.f;
    return (o * (float)(layer - 1) + t * inv_spp) / (float)layer;
}

// ---- the evaluation: the mean incoming radiance under the cosine density about n (irradiance / pi) ----
PROBE_FN void probe_eval(const float *sh, const float *n, float *out) {
    const float FOURPI = 12.566371f;
    float Y[PROBE_K];
    probe_basis(n[0], n[1], n[2], Y);
    float e[3] = {0.f, 0.f, 0.f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < (int)PROBE_K; k++) {
        const float w = probe_band(k) * Y[k];
        for (int c = 0; c < 3; c++) e[c] = e[c] + w * sh[3 * k + c];
    }
    for (int c = 0; c < 3; c++) out[c] = probe_max0(FOURPI * e[c]);
}

// ---- the grid ----
PROBE_FN uint32_t probe_index(const ProbeGrid &g, uint32_t x, uint32_t y, uint32_t z) {
    return (z * g.dims[1] + y) * g.dims[0] + x;
}
PROBE_FN float probe_position(const ProbeGrid &g, int a, uint32_t i) { return g.origin[a] + (float)i * g.step[a]; }
// one axis of a lookup at coordinate p: the cell's lower and upper probe and the weight t of the upper
PROBE_FN void probe_axis(float p, float origin, float step, uint32_t dim, uint32_t &i0, uint32_t &i1, float &t) {
    if (dim == 1) {
        i0 = i1 = 0;
        t = 0.f;
        return;
    }
    float f = (p - origin) / step;
#ifndef PROBE_NO_CLAMP
    const float hi = (float)(dim - 1);
    f = f > 0.f ? f : 0.f;
    f = f < hi ? f : hi;
    const uint32_t i = (uint32_t)f;
#else // (tests/native/probe_check.cpp builds this form to show that its comparison notices; the conversion stays defined)
    const uint32_t i = f > 0.f ? (f < 4e9f ? (uint32_t)f : 0xffffffffu) : 0u;
#endif
    i0 = i < dim - 2 ? i : dim - 2;
    t = f - (float)i0;
    i1 = i0 + 1;
}
// The lookup at p for normal n over sh [count][27]: each coefficient is the sum over the cell's eight corners of
// w sh, w = (wx wy) wz, corners in z, y, x order with x fastest; the evaluation's sum takes it as it is formed
PROBE_FN void probe_sample(const ProbeGrid &g, const float *sh, const float *p, const float *n, float *out) {
    const float FOURPI = 12.566371f;
    uint32_t i0[3], i1[3];
    float t[3];
    for (int a = 0; a < 3; a++) probe_axis(p[a], g.origin[a], g.step[a], g.dims[a], i0[a], i1[a], t[a]);
    const float *corner[8];
    float w[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; j++) {
        const bool ux = j & 1, uy = j & 2, uz = j & 4;
        const float wx = ux ? t[0] : 1.f - t[0], wy = uy ? t[1] : 1.f - t[1], wz = uz ? t[2] : 1.f - t[2];
        w[j] = (wx * wy) * wz;
        corner[j] = sh + (size_t)PROBE_F * probe_index(g, ux ? i1[0] : i0[0], uy ? i1[1] : i0[1], uz ? i1[2] : i0[2]);
    }
    float Y[PROBE_K];
    probe_basis(n[0], n[1], n[2], Y);
    float e[3] = {0.f, 0.f, 0.f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < (int)PROBE_K; k++) {
        const float a = probe_band(k) * Y[k];
        for (int c = 0; c < 3; c++) {
            float s = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int j = 0; j < 8; j++) s = s + w[j] * corner[j][3 * k + c];
            e[c] = e[c] + a * s;
        }
    }
    for (int c = 0; c < 3; c++) out[c] = probe_max0(FOURPI * e[c]);
}

// ---- the host restatement (tests/native/probe_check.cpp; cr_probe_grid_positions) ----
inline void probe_grid_positions(const ProbeGrid &g, float *pos) {
    size_t i = 0;
    for (uint32_t z = 0; z < g.dims[2]; z++)
        for (uint32_t y = 0; y < g.dims[1]; y++)
            for (uint32_t x = 0; x < g.dims[0]; x++, i++) {
                pos[3 * i] = probe_position(g, 0, x);
                pos[3 * i + 1] = probe_position(g, 1, y);
                pos[3 * i + 2] = probe_position(g, 2, z);
            }
}
// One probe's projection over `layers` layers from layer0 on: raw [layers][spp][2] draws, rad [layers][spp][3] the
// samples' radiance; sh (and m2, may be null) [27] are blended onto
inline void probe_fold_host(uint32_t layer0, uint32_t layers, uint32_t spp, const uint32_t *raw, const float *rad,
                            float *sh, float *m2) {
    const float inv = 1.f / (float)spp;
    for (uint32_t j = 0; j < layers; j++) {
        float t[PROBE_F] = {}, q[PROBE_F] = {};
        for (uint32_t s = 0; s < spp; s++) {
            const size_t i = (size_t)j * spp + s;
            float d[3], Y[PROBE_K];
            probe_dir(raw[2 * i], raw[2 * i + 1], d);
            probe_basis(d[0], d[1], d[2], Y);
            probe_accum(Y, rad + 3 * i, t, m2 ? q : nullptr);
        }
        for (uint32_t f = 0; f < PROBE_F; f++) {
            sh[f] = probe_blend(sh[f], t[f], inv, layer0 + j);
            if (m2) m2[f] = probe_blend(m2[f], q[f], inv, layer0 + j);
        }
    }
}

} // namespace cr
