// bake.hpp -- the texture-space side of a lightmap bake (cr_bake_surface_device / cr_bake_dilate_device / cr_bake;
// include/chiaro_hip.h "lightmap baking"), as pure functions in the style of adaptive.hpp: the
// argument checks, the coverage arithmetic -- the one statement that texbake.hip's kernels and the host restatement
// below both compile -- and the grid atlas.  Nothing here calls the HIP runtime; tests/native/bake_check.cpp runs all
// of it on the CPU.  float32, the operations in the order written, no contraction.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define BAKE_FN __host__ __device__ inline
#else
#define BAKE_FN inline
#endif
// The edge rule: a weight on the edge counts (inclusive, so a shared edge loses no texel).  A macro so that
// tests/native/bake_check.cpp can build the exclusive rule and show that its comparison notices.
#ifndef BAKE_EDGE_IN
#define BAKE_EDGE_IN(w) ((w) >= 0.f)
#endif

namespace cr {

enum : uint32_t { BAKE_NONE = 0xffffffffu }; // an unowned texel of the owner map

// ---- validation (arithmetic on the arguments: answered before any device is looked at) ----
inline const char *bake_check_map(uint32_t W, uint32_t H) {
    if (!W || !H) return "lightmap width/height must be > 0";
    if ((uint64_t)W * H > (1ull << 31)) return "lightmap too large (width * height > 2^31)";
    return nullptr;
}
// cr_bake_params of the surface call (spp, k and seed are the gather's, checked by bake_check_sampling)
inline const char *bake_check_surface(bool have_params, uint32_t W, uint32_t H, float offset, bool outputs) {
    if (!have_params) return "null bake params";
    if (const char *m = bake_check_map(W, H)) return m;
    if (!(offset == offset) || std::isinf(offset)) return "bake offset must be finite";
    if (!outputs) return "null owner / pos / nrm / list / count";
    return nullptr;
}
inline const char *bake_check_sampling(uint32_t spp, int32_t k, uint64_t layers) {
    if (spp == 0) return "spp must be > 0";
    if (k < 1 || k > 64) return "k must be in [1, 64]";
    if (layers < 1) return "no layers";
    if (layers * spp > 0xFFFFFFFFull) return "layers * spp must fit 32 bits";
    return nullptr;
}
inline const char *bake_check_dilate(uint32_t W, uint32_t H, bool arrays, bool alias) {
    if (const char *m = bake_check_map(W, H)) return m;
    if (!arrays) return "null owner / input / output";
    if (alias) return "dilation output must not alias its input";
    return nullptr;
}
// passes beyond max(W, H) change nothing: a map with one filled texel is full after max(W, H) - 1
inline uint32_t bake_dilate_passes(uint32_t W, uint32_t H, uint32_t passes) {
    const uint32_t m = W > H ? W : H;
    return passes < m ? passes : m;
}

// ---- coverage ----
BAKE_FN bool bake_finite(float v) {
    return v - v == 0.f; // (inf - inf and NaN - NaN are NaN)
}
BAKE_FN float bake_edge(float ax, float ay, float bx, float by, float cx, float cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}
// A triangle in texel space: q_k = (u_k * W, v_k * H), A = edge(q0, q1, q2), its bounding box; ok false: it covers
// nothing (a UV that is not finite, or A == 0)
struct BakeTri {
    float qx[3], qy[3], A;
    float minx, maxx, miny, maxy;
    bool ok;
};
BAKE_FN BakeTri bake_tri(const float *uv, float fW, float fH) {
    BakeTri t;
    bool fin = true;
    for (int k = 0; k < 3; k++) {
        fin = fin && bake_finite(uv[2 * k]) && bake_finite(uv[2 * k + 1]);
        t.qx[k] = uv[2 * k] * fW;
        t.qy[k] = uv[2 * k + 1] * fH;
    }
    t.A = bake_edge(t.qx[0], t.qy[0], t.qx[1], t.qy[1], t.qx[2], t.qy[2]);
    t.minx = fminf(fminf(t.qx[0], t.qx[1]), t.qx[2]);
    t.maxx = fmaxf(fmaxf(t.qx[0], t.qx[1]), t.qx[2]);
    t.miny = fminf(fminf(t.qy[0], t.qy[1]), t.qy[2]);
    t.maxy = fmaxf(fmaxf(t.qy[0], t.qy[1]), t.qy[2]);
    t.ok = fin && !(t.A == 0.f);
    return t;
}
// The weights of q1 and q2 at texel (x, y)'s centre and A, all negated for A < 0; covered: the centre is inside the
// triangle's bounding box (inclusive; exact comparisons, so the owner pass may walk any box of texels that holds
// these) and no weight is outside the edge rule
struct BakeWeights {
    float w1, w2, A;
    bool covered;
};
BAKE_FN BakeWeights bake_weights(const BakeTri &t, uint32_t x, uint32_t y) {
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    float w0 = bake_edge(t.qx[1], t.qy[1], t.qx[2], t.qy[2], cx, cy);
    float w1 = bake_edge(t.qx[2], t.qy[2], t.qx[0], t.qy[0], cx, cy);
    float w2 = bake_edge(t.qx[0], t.qy[0], t.qx[1], t.qy[1], cx, cy);
    float A = t.A;
    if (A < 0.f) w0 = -w0, w1 = -w1, w2 = -w2, A = -A;
    const bool in_box = cx >= t.minx && cx <= t.maxx && cy >= t.miny && cy <= t.maxy;
    return {w1, w2, A, t.ok && in_box && BAKE_EDGE_IN(w0) && BAKE_EDGE_IN(w1) && BAKE_EDGE_IN(w2)};
}
// The texels [x0, x1] x [y0, y1] of the W x H map that hold every centre inside t's bounding box (one texel of
// slack each way, then clipped); false: none
BAKE_FN bool bake_box(const BakeTri &t, uint32_t W, uint32_t H, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1) {
    if (!t.ok) return false;
    const float top = 2147483648.f; // 2^31 >= W, H
    const float ax = fminf(fmaxf(floorf(t.minx) - 1.f, 0.f), top), bx = fminf(floorf(t.maxx) + 1.f, top);
    const float ay = fminf(fmaxf(floorf(t.miny) - 1.f, 0.f), top), by = fminf(floorf(t.maxy) + 1.f, top);
    if (!(bx >= 0.f) || !(by >= 0.f) || !(ax <= bx) || !(ay <= by)) return false; // (a NaN bound: nothing)
    x0 = (uint32_t)ax, y0 = (uint32_t)ay;
    if (x0 >= W || y0 >= H) return false;
    x1 = (uint32_t)bx, y1 = (uint32_t)by;
    x1 = x1 < W - 1 ? x1 : W - 1;
    y1 = y1 < H - 1 ? y1 : H - 1;
    return true;
}
// The surface point of a covered texel: b1 = w1 / A, b2 = w2 / A, P = p0 (1 - b1 - b2) + p1 b1 + p2 b2 per component,
// nrm = n + 0, pos = P + offset nrm.  p: the triangle's vertices [3][stride] floats, n its normal.
BAKE_FN void bake_point(const BakeWeights &w, const float *p, int stride, const float *n, float offset, float *pos,
                        float *nrm) {
    const float b1 = w.w1 / w.A, b2 = w.w2 / w.A, b0 = 1.f - b1 - b2;
    for (int i = 0; i < 3; i++) {
        const float P = p[i] * b0 + p[stride + i] * b1 + p[2 * stride + i] * b2;
        nrm[i] = n[i] + 0.0f;
        pos[i] = P + offset * nrm[i];
    }
}

// ---- the host restatement (tests/native/bake_check.cpp; nothing in the library calls it) ----
// owner [H][W], pos / nrm [H][W][3], list (room W * H): returns the covered count
inline uint32_t bake_surface_host(uint32_t n_tris, const float *uv, const float *tri_pos, const float *tri_normal,
                                  uint32_t W, uint32_t H, float offset, uint32_t *owner, float *pos, float *nrm,
                                  uint32_t *list) {
    const size_t n = (size_t)W * H;
    const float fW = (float)W, fH = (float)H;
    for (size_t i = 0; i < n; i++) owner[i] = BAKE_NONE;
    std::memset(pos, 0, n * 3 * sizeof(float));
    std::memset(nrm, 0, n * 3 * sizeof(float));
    for (uint32_t t = 0; t < n_tris; t++) {
        const BakeTri T = bake_tri(uv + 6 * (size_t)t, fW, fH);
        uint32_t x0, x1, y0, y1;
        if (!bake_box(T, W, H, x0, x1, y0, y1)) continue;
        for (uint32_t y = y0; y <= y1; y++)
            for (uint32_t x = x0; x <= x1; x++)
                if (bake_weights(T, x, y).covered && t < owner[(size_t)y * W + x]) owner[(size_t)y * W + x] = t;
    }
    uint32_t count = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t t = owner[i];
        if (t == BAKE_NONE) continue;
        const BakeTri T = bake_tri(uv + 6 * (size_t)t, fW, fH);
        bake_point(bake_weights(T, (uint32_t)(i % W), (uint32_t)(i / W)), tri_pos + 9 * (size_t)t, 3,
                   tri_normal + 3 * (size_t)t, offset, pos + 3 * i, nrm + 3 * i);
        list[count++] = (uint32_t)i;
    }
    return count;
}

// ---- dilation ----
// The eight neighbours in the order their values are summed
BAKE_FN void bake_neighbour(int j, int &dx, int &dy) {
    // (-1,0) (+1,0) (0,-1) (0,+1) (-1,-1) (+1,-1) (-1,+1) (+1,+1), without a table a kernel would index
    if (j < 4) {
        dx = j == 0 ? -1 : j == 1 ? 1 : 0;
        dy = j == 2 ? -1 : j == 3 ? 1 : 0;
    } else {
        dx = (j & 1) ? 1 : -1;
        dy = j < 6 ? -1 : 1;
    }
}
// level [H][W]: 0 an owned texel, p a texel filled by pass p, BAKE_NONE not filled.  Pass p gives every unfilled
// texel with neighbours of level < p their mean; it reads values and levels of earlier passes only, so it runs in
// place: what it writes (level p) is nothing it reads.
inline void bake_dilate_host(uint32_t W, uint32_t H, const uint32_t *owner, uint32_t passes, const float *in,
                             float *out) {
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> level(n);
    for (size_t i = 0; i < n; i++) level[i] = owner[i] == BAKE_NONE ? (uint32_t)BAKE_NONE : 0u;
    std::memcpy(out, in, n * 3 * sizeof(float));
    passes = bake_dilate_passes(W, H, passes);
    for (uint32_t p = 1; p <= passes; p++)
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                if (level[i] != BAKE_NONE) continue;
                float s[3] = {0.f, 0.f, 0.f};
                uint32_t cnt = 0;
                for (int j = 0; j < 8; j++) {
                    int dx, dy;
                    bake_neighbour(j, dx, dy);
                    const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy;
                    if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
                    const size_t q = (size_t)ny * W + (size_t)nx;
                    if (level[q] >= p) continue;
                    for (int c = 0; c < 3; c++) s[c] = s[c] + out[3 * q + c];
                    cnt++;
                }
                if (!cnt) continue;
                for (int c = 0; c < 3; c++) out[3 * i + c] = s[c] / (float)cnt;
                level[i] = p;
            }
}

// ---- the grid atlas ----
// Triangle t in cell (t % cols, t / cols) of a cols = ceil(sqrt(n_tris)) grid of cell x cell texels, its vertices at
// texel offsets (g, g), (cell - g, g), (g, cell - g) of the cell, divided by W = cols * cell and H = rows * cell.
inline const char *bake_atlas_check(uint32_t n_tris, uint32_t cell, float gutter) {
    if (!n_tris) return "atlas of no triangles";
    if (cell < 1) return "atlas cell must be >= 1";
    if (!(gutter >= 0.f) || !(gutter < 0.5f * (float)cell)) return "atlas gutter must be in [0, cell / 2)";
    uint64_t cols = (uint64_t)std::ceil(std::sqrt((double)n_tris));
    while (cols * cols < n_tris) cols++;
    const uint64_t rows = (n_tris + cols - 1) / cols;
    if (cols * cell > 0xffffffffull || rows * cell > 0xffffffffull || cols * cell * rows * cell > (1ull << 31))
        return "atlas too large (width * height > 2^31)";
    return nullptr;
}
inline void bake_atlas_grid(uint32_t n_tris, uint32_t cell, float gutter, uint32_t *W, uint32_t *H, float *uv_out) {
    uint32_t cols = (uint32_t)std::ceil(std::sqrt((double)n_tris));
    while ((uint64_t)cols * cols < n_tris) cols++;
    while (cols > 1 && (uint64_t)(cols - 1) * (cols - 1) >= n_tris) cols--;
    const uint32_t rows = (n_tris + cols - 1) / cols;
    const uint32_t w = cols * cell, h = rows * cell;
    if (W) *W = w;
    if (H) *H = h;
    if (!uv_out) return;
    const float fw = (float)w, fh = (float)h, lo = gutter, hi = (float)cell - gutter;
    for (uint32_t t = 0; t < n_tris; t++) {
        const float cx = (float)((t % cols) * cell), cy = (float)((t / cols) * cell);
        float *o = uv_out + 6 * (size_t)t;
        o[0] = (cx + lo) / fw, o[1] = (cy + lo) / fh;
        o[2] = (cx + hi) / fw, o[3] = (cy + lo) / fh;
        o[4] = (cx + lo) / fw, o[5] = (cy + hi) / fh;
    }
}

} // namespace cr
