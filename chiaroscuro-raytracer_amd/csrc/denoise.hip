// denoise.hip -- the guide buffers of the first hit and the variance-guided a-trous filter (cr_guides_device,
// cr_denoise_device; include/chiaro_hip.h "guide buffers and denoiser").  Image-space work behind
// the noise block: float32, no contraction, IEEE division and square root, the operations exactly in the order the
// header writes them -- tests/denoise_model.py restates them in numpy and the results agree bit for bit.
#include "chiaro_hip.h"
#include "denoise.hpp"
#include "render_common.hpp"

namespace cr {

enum : uint32_t { DN_BLOCKS = 4096 }; // of the per-pixel kernels: the blocks stride over frames of more pixels

static inline uint32_t dn_grid(uint64_t npix) {
    const uint64_t need = (npix + 255) / 256;
    return (uint32_t)(need < DN_BLOCKS ? need : (uint64_t)DN_BLOCKS);
}

// ---- guide buffers ----
// One ray per pixel through its centre: camera_dir's affine form (render_common.hpp) at sx = x + 0.5, sy = y + 0.5,
// without the RNG, unnormalised.
__global__ void __launch_bounds__(256) guide_rays(GuideArgs G) {
    const uint64_t npix = (uint64_t)G.xres * G.yres;
    const f3 eye = mk(G.cam[0], G.cam[1], G.cam[2]), lu = mk(G.cam[3], G.cam[4], G.cam[5]),
             dx = mk(G.cam[6], G.cam[7], G.cam[8]), dy = mk(G.cam[9], G.cam[10], G.cam[11]);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t y = (uint32_t)(i / G.xres), x = (uint32_t)(i - (uint64_t)y * G.xres);
        const float sx = (float)x + 0.5f, sy = (float)y + 0.5f;
        const f3 d = add(add(lu, muls(dx, sx)), muls(dy, sy));
        float *o = G.orig + 3 * i, *q = G.dir + 3 * i;
        o[0] = eye.x, o[1] = eye.y, o[2] = eye.z;
        q[0] = d.x, q[1] = d.y, q[2] = d.z;
    }
}
// The hit (tri, bx, by, dist) of pixel i -> albedo (Kd, or the texture at shade_hit's uv), the normalised material
// normal, the distance; a miss: zeros and depth -1.
__global__ void __launch_bounds__(256) guide_shade(GuideArgs G) {
    const uint64_t npix = (uint64_t)G.xres * G.yres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        f3 kd = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f);
        float z = -1.0f;
        if (G.hit[i]) {
            const uint32_t t = G.tri[i];
            const float bx = G.bary[2 * i], by = G.bary[2 * i + 1];
            const float bz = (1.f - bx - by);
            const float4 kd4 = G.S.mat_kd[t];
            kd = ld3(kd4);
            const int ti = __float_as_int(kd4.w);
            if (ti >= 0) {
                const float2 ua = G.S.mat_uv[3 * t], ub = G.S.mat_uv[3 * t + 1], uc = G.S.mat_uv[3 * t + 2];
                kd = tex_lookup(G.S, ti, (ua.x * bz + ub.x * bx) + uc.x * by, (ua.y * bz + ub.y * bx) + uc.y * by);
            }
            nrm = normalize(ld3(G.S.mat_n[t]));
            z = G.dist[i];
        }
        if (G.albedo) G.albedo[3 * i] = kd.x, G.albedo[3 * i + 1] = kd.y, G.albedo[3 * i + 2] = kd.z;
        if (G.normal) G.normal[3 * i] = nrm.x, G.normal[3 * i + 1] = nrm.y, G.normal[3 * i + 2] = nrm.z;
        if (G.depth) G.depth[i] = z;
        if (G.rec) {
            G.rec[2 * i] = make_float4(kd.x, kd.y, kd.z, z);
            G.rec[2 * i + 1] = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
        }
    }
}
int launch_guide_rays(const GuideArgs &G, hipStream_t st) {
    const uint32_t blocks = dn_grid((uint64_t)G.xres * G.yres);
    if (blocks) hipLaunchKernelGGL(guide_rays, dim3(blocks), dim3(256), 0, st, G);
    return (int)hipGetLastError();
}
int launch_guide_shade(const GuideArgs &G, hipStream_t st) {
    const uint32_t blocks = dn_grid((uint64_t)G.xres * G.yres);
    if (blocks) hipLaunchKernelGGL(guide_shade, dim3(blocks), dim3(256), 0, st, G);
    return (int)hipGetLastError();
}

// ---- the filter ----
__global__ void __launch_bounds__(256) guide_pack(DnArgs D) {
    const uint64_t npix = (uint64_t)D.xres * D.yres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const float *a = D.albedo + 3 * i, *n = D.normal + 3 * i;
        D.rec[2 * i] = make_float4(a[0], a[1], a[2], D.depth[i]);
        D.rec[2 * i + 1] = make_float4(n[0], n[1], n[2], 0.f);
    }
}
// The variance of the pixel's mean: the noise block's per-channel variance over n, summed.
__global__ void __launch_bounds__(256) var_init(DnArgs D) {
    const uint64_t npix = (uint64_t)D.xres * D.yres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const float *f = D.frame + 3 * i, *q = D.m2 + 3 * i;
        const float n = D.layer_map ? (float)(D.layer_map[i] * D.spp) : D.n;
        const float cr = f[0], cg = f[1], cb = f[2];
        float vr = q[0] - cr * cr, vg = q[1] - cg * cg, vb = q[2] - cb * cb;
        vr = (vr > 0.f) ? vr : 0.f; // (a NaN or negative variance: 0)
        vg = (vg > 0.f) ? vg : 0.f;
        vb = (vb > 0.f) ? vb : 0.f;
        vr = vr / n, vg = vg / n, vb = vb / n;
        const float var = (vr + vg) + vb;
        if (D.dst) {
            D.dst[i] = make_float4(cr, cg, cb, var);
        } else {
            D.out[3 * i] = cr, D.out[3 * i + 1] = cg, D.out[3 * i + 2] = cb;
            if (D.var_out) D.var_out[i] = var;
        }
    }
}

// One level.  A block is a DN_TILE_X x DN_TILE_Y tile of pixels, a thread one pixel; the tiles are numbered row-major
// in a one-dimensional grid.  LDS: the tile plus its halo of 2 * step pixels is staged first -- three float4 planes
// (colour and variance, albedo and depth, normal), consecutive lanes at consecutive 16-B slots -- and every tap and
// the 3x3 variance blur (whose +-1 neighbours, clamped to the frame, lie inside the halo) read it; else they read
// global memory.  Slots of the staged tile that lie outside the frame are never written and never read: a tap
// outside the frame is skipped before its fetch.
struct DnPix {
    float4 c, a, n; // {colour, variance}, {albedo, depth}, {normal, 0}
};
template <bool LDS> struct DnFetch {
    const DnArgs &D;
    const float4 *sm;
    int x0, y0, W, plane;
    __device__ __forceinline__ size_t at(int qx, int qy) const {
        return LDS ? (size_t)((qy - y0) * W + (qx - x0)) : (size_t)qy * D.xres + (size_t)qx;
    }
    __device__ __forceinline__ float4 colour(int qx, int qy) const { return LDS ? sm[at(qx, qy)] : D.src[at(qx, qy)]; }
    __device__ __forceinline__ DnPix pixel(int qx, int qy) const {
        const size_t i = at(qx, qy);
        if (LDS) return DnPix{sm[i], sm[plane + i], sm[2 * plane + i]};
        return DnPix{D.src[i], D.rec[2 * i], D.rec[2 * i + 1]};
    }
};
template <bool LDS> __global__ void __launch_bounds__(256) atrous(DnArgs D) {
    extern __shared__ float4 dn_sm[];
    const int s = (int)D.step, xres = (int)D.xres, yres = (int)D.yres;
    const uint32_t tiles_x = (D.xres + DN_TILE_X - 1) / DN_TILE_X;
    const int by = (int)(blockIdx.x / tiles_x), bx = (int)(blockIdx.x - (uint32_t)by * tiles_x);
    const int x = bx * (int)DN_TILE_X + (int)(threadIdx.x % DN_TILE_X), y = by * (int)DN_TILE_Y + (int)(threadIdx.x / DN_TILE_X);
    DnFetch<LDS> F{D, dn_sm, bx * (int)DN_TILE_X - 2 * s, by * (int)DN_TILE_Y - 2 * s, (int)DN_TILE_X + 4 * s, 0};
    if (LDS) {
        const int H = (int)DN_TILE_Y + 4 * s;
        F.plane = F.W * H;
        for (int e = (int)threadIdx.x; e < F.plane; e += 256) {
            const int gy = F.y0 + e / F.W, gx = F.x0 + e % F.W;
            if (gx >= 0 && gy >= 0 && gx < xres && gy < yres) {
                const size_t p = (size_t)gy * D.xres + (size_t)gx;
                dn_sm[e] = D.src[p];
                dn_sm[F.plane + e] = D.rec[2 * p];
                dn_sm[2 * F.plane + e] = D.rec[2 * p + 1];
            }
        }
        __syncthreads();
    }
    if (x >= xres || y >= yres) return;
    // the 3x3 blur of the variance, coordinates clamped to the frame, row-major from 0
    float vb = 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float g = (j == 1 ? 0.5f : 0.25f) * (i == 1 ? 0.5f : 0.25f);
            int qx = x + i - 1, qy = y + j - 1;
            qx = qx < 0 ? 0 : (qx > xres - 1 ? xres - 1 : qx);
            qy = qy < 0 ? 0 : (qy > yres - 1 ? yres - 1 : qy);
            vb = vb + g * F.colour(qx, qy).w;
        }
    }
    const float den = D.sl2 * vb + 1e-8f;
    const DnPix P = F.pixel(x, y);
    const float bp = (P.c.x + P.c.y) + P.c.z;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int j = 0; j < 5; j++) {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const float hj = j == 2 ? 0.375f : ((j == 1 || j == 3) ? 0.25f : 0.0625f);
            const float hi = i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f);
            const float w0 = hj * hi;
            const int qx = x + s * (i - 2), qy = y + s * (j - 2);
            if (qx < 0 || qy < 0 || qx >= xres || qy >= yres) continue;
            float w = w0;
            float4 cq = P.c;
            if (!(i == 2 && j == 2)) {
                const DnPix Q = F.pixel(qx, qy);
                cq = Q.c;
                const float bq = (Q.c.x + Q.c.y) + Q.c.z;
                const float dl = bq - bp;
                float t = 1.f / (1.f + (dl * dl) / den);
                w = w0 * (t * t);
                const float dr = Q.a.x - P.a.x, dg = Q.a.y - P.a.y, db = Q.a.z - P.a.z;
                const float d2 = ((dr * dr + dg * dg) + db * db) * D.inv_sa2;
                t = 1.f / (1.f + d2);
                w = w * (t * t);
                const bool hp = P.a.w >= 0.f, hq = Q.a.w >= 0.f;
                if (hp != hq) continue; // exactly one of the two is a hit
                if (hp) {
                    float dn = (P.n.x * Q.n.x + P.n.y * Q.n.y) + P.n.z * Q.n.z;
                    dn = dn > 0.f ? dn : 0.f;
                    for (uint32_t k = 0; k < D.squarings; k++) dn = dn * dn;
                    const float zm = P.a.w > Q.a.w ? P.a.w : Q.a.w;
                    const float dz = (Q.a.w - P.a.w) / (D.sz_step * zm);
                    t = 1.f / (1.f + dz * dz);
                    w = w * (dn * (t * t));
                }
                if (!(w > 0.f)) continue; // zero, negative, NaN: the tap adds nothing
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    const float r = sr / sw, g = sg / sw, b = sb / sw, var = sv / (sw * sw);
    const size_t p = (size_t)y * D.xres + (size_t)x;
    if (D.dst) {
        D.dst[p] = make_float4(r, g, b, var);
    } else {
        D.out[3 * p] = r, D.out[3 * p + 1] = g, D.out[3 * p + 2] = b;
        if (D.var_out) D.var_out[p] = var;
    }
}

int launch_guide_pack(const DnArgs &D, hipStream_t st) {
    const uint32_t blocks = dn_grid((uint64_t)D.xres * D.yres);
    if (blocks) hipLaunchKernelGGL(guide_pack, dim3(blocks), dim3(256), 0, st, D);
    return (int)hipGetLastError();
}
int launch_var_init(const DnArgs &D, hipStream_t st) {
    const uint32_t blocks = dn_grid((uint64_t)D.xres * D.yres);
    if (blocks) hipLaunchKernelGGL(var_init, dim3(blocks), dim3(256), 0, st, D);
    return (int)hipGetLastError();
}
int launch_atrous(const DnArgs &D, bool lds, hipStream_t st) {
    static_assert(DN_TILE_X * DN_TILE_Y == 256, "one thread per pixel of a tile");
    const uint64_t tiles = (uint64_t)((D.xres + DN_TILE_X - 1) / DN_TILE_X) * ((D.yres + DN_TILE_Y - 1) / DN_TILE_Y);
    if (!tiles) return (int)hipGetLastError();
    if (lds && D.step <= DN_LDS_MAX_STEP) {
        const size_t bytes = 3 * sizeof(float4) * (size_t)(DN_TILE_X + 4 * D.step) * (DN_TILE_Y + 4 * D.step);
        hipLaunchKernelGGL(atrous<true>, dim3((uint32_t)tiles), dim3(256), bytes, st, D);
    } else {
        hipLaunchKernelGGL(atrous<false>, dim3((uint32_t)tiles), dim3(256), 0, st, D);
    }
    return (int)hipGetLastError();
}

} // namespace cr
