// temporal.hip -- temporal reprojection (cr_reproject_device, cr_render_temporal; include/chiaro_hip.h "temporal
// reprojection"): a (frame, moments, count) history of the previous camera carried to the current
// one and merged with the current samples.  float32, no contraction, IEEE division, the operations exactly in the
// order the header writes them -- tests/temporal_model.py restates them in numpy and the results agree bit for bit.
#include "chiaro_hip.h"
#include "temporal.hpp"
#include "render_common.hpp"

namespace cr {

enum : uint32_t { TP_BLOCKS = 4096 }; // the blocks stride over frames of more pixels

static inline uint32_t tp_grid(uint64_t npix) {
    const uint64_t need = (npix + 255) / 256;
    return (uint32_t)(need < TP_BLOCKS ? need : (uint64_t)TP_BLOCKS);
}

// One tap of the history at pixel q: its frame, moments, count, normal and depth, from the planar arrays or from
// the packed record (three 16-B loads).
struct TpTap {
    f3 h, h2, n;
    uint32_t k;
    float z;
};
template <bool PACKED> __device__ __forceinline__ TpTap tp_fetch(const TpArgs &T, size_t q) {
    TpTap t;
    if (PACKED) {
        const float4 a = T.hist_rec[3 * q], b = T.hist_rec[3 * q + 1], c = T.hist_rec[3 * q + 2];
        t.h = ld3(a), t.h2 = ld3(b), t.n = ld3(c);
        t.k = __float_as_uint(a.w);
        t.z = b.w;
    } else {
        const float *f = T.hist_frame + 3 * q, *m = T.hist_m2 + 3 * q, *n = T.hist_normal + 3 * q;
        t.h = mk(f[0], f[1], f[2]), t.h2 = mk(m[0], m[1], m[2]), t.n = mk(n[0], n[1], n[2]);
        t.k = T.hist_count[q];
        t.z = T.hist_depth[q];
    }
    return t;
}

template <bool PACKED> __global__ void __launch_bounds__(256) reproject(TpArgs T) {
    const uint64_t npix = (uint64_t)T.xres * T.yres;
    const f3 eye = mk(T.cam[0], T.cam[1], T.cam[2]), lu = mk(T.cam[3], T.cam[4], T.cam[5]),
             dx = mk(T.cam[6], T.cam[7], T.cam[8]), dy = mk(T.cam[9], T.cam[10], T.cam[11]);
    const f3 eye_p = mk(T.eye_p[0], T.eye_p[1], T.eye_p[2]), ra = mk(T.ra[0], T.ra[1], T.ra[2]),
             rb = mk(T.rb[0], T.rb[1], T.rb[2]), rc = mk(T.rc[0], T.rc[1], T.rc[2]);
    const float fxres = (float)T.xres, fyres = (float)T.yres;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t y = (uint32_t)(i / T.xres), x = (uint32_t)(i - (uint64_t)y * T.xres);
        const uint32_t n_u = T.layer_map ? T.layer_map[i] * T.spp : T.n_u;
        const f3 C = mk(T.frame[3 * i], T.frame[3 * i + 1], T.frame[3 * i + 2]);
        const f3 M = mk(T.m2[3 * i], T.m2[3 * i + 1], T.m2[3 * i + 2]);
        const f3 Nc = mk(T.normal[3 * i], T.normal[3 * i + 1], T.normal[3 * i + 2]);
        const float Zc = T.depth[i];
        uint32_t h = 0;
        f3 R = mk(0.f, 0.f, 0.f), R2 = mk(0.f, 0.f, 0.f);
        if (Zc >= 0.f) {
            const float sx = (float)x + 0.5f, sy = (float)y + 0.5f;
            const f3 d = add(add(lu, muls(dx, sx)), muls(dy, sy));
            const f3 P = add(eye, muls(d, Zc));
            const f3 q = sub(P, eye_p);
            const float a = dot(q, ra), b = dot(q, rb), c = dot(q, rc);
            const float u = b / a, v = c / a;
            const float ze = a / T.det;
            if (ze > 0.f) {
                const float fx = u - 0.5f, fy = v - 0.5f;
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float wx = fx - x0, wy = fy - y0;
                const float omx = 1.f - wx, omy = 1.f - wy;
                const float ztol = T.depth_tol * ze;
                float sw = 0.f;
                f3 sr = mk(0.f, 0.f, 0.f), s2 = mk(0.f, 0.f, 0.f);
                uint32_t kmin = 0xFFFFFFFFu;
                bool any = false;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int ti = t & 1, tj = t >> 1;
                    const float tx = x0 + (float)ti, ty = y0 + (float)tj;
                    // in float, before any integer conversion: a NaN or an infinity fails
                    if (!(tx >= 0.f && tx < fxres && ty >= 0.f && ty < fyres)) continue;
                    const float w = (ti ? wx : omx) * (tj ? wy : omy);
                    const size_t qi = (size_t)(uint32_t)ty * T.xres + (size_t)(uint32_t)tx;
                    const TpTap Q = tp_fetch<PACKED>(T, qi);
                    if (!(Q.k > 0u)) continue;
                    if (!(Q.z >= 0.f)) continue;
                    if (!(fabsf(Q.z - ze) <= ztol)) continue;
                    if (!(dot(Nc, Q.n) >= T.normal_min)) continue;
                    if (Q.h.x != Q.h.x || Q.h.y != Q.h.y || Q.h.z != Q.h.z || Q.h2.x != Q.h2.x || Q.h2.y != Q.h2.y ||
                        Q.h2.z != Q.h2.z)
                        continue;
                    if (!(w > 0.f)) continue;
                    sw = sw + w;
                    sr = add(sr, muls(Q.h, w));
                    s2 = add(s2, muls(Q.h2, w));
                    kmin = Q.k < kmin ? Q.k : kmin;
                    any = true;
                }
                if (any) {
                    R = divs(sr, sw);
                    R2 = divs(s2, sw);
                    h = kmin < T.max_history ? kmin : T.max_history;
                }
            }
        }
        f3 o = mk(0.f, 0.f, 0.f), o2 = mk(0.f, 0.f, 0.f);
        uint32_t cnt = 0;
        if (h == 0) {
            if (n_u) o = C, o2 = M, cnt = n_u; // the bits, no arithmetic
        } else if (n_u == 0) {
            o = R, o2 = R2, cnt = h;
        } else {
            const float hf = (float)h, nf = (float)n_u;
            const float tot = hf + nf;
            o = divs(add(muls(R, hf), muls(C, nf)), tot);
            o2 = divs(add(muls(R2, hf), muls(M, nf)), tot);
            const uint64_t s = (uint64_t)h + n_u;
            cnt = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
        }
        T.out[3 * i] = o.x, T.out[3 * i + 1] = o.y, T.out[3 * i + 2] = o.z;
        T.m2_out[3 * i] = o2.x, T.m2_out[3 * i + 1] = o2.y, T.m2_out[3 * i + 2] = o2.z;
        T.count_out[i] = cnt;
        if (T.rec_out) {
            T.rec_out[3 * i] = make_float4(o.x, o.y, o.z, __uint_as_float(cnt));
            T.rec_out[3 * i + 1] = make_float4(o2.x, o2.y, o2.z, Zc);
            T.rec_out[3 * i + 2] = make_float4(Nc.x, Nc.y, Nc.z, 0.f);
        }
    }
}

__global__ void __launch_bounds__(256) temporal_pack(uint32_t npix, const float *frame, const float *m2,
                                                     const uint32_t *count, const float *normal, const float *depth,
                                                     float4 *rec) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const float *f = frame + 3 * i, *m = m2 + 3 * i, *n = normal + 3 * i;
        rec[3 * i] = make_float4(f[0], f[1], f[2], __uint_as_float(count[i]));
        rec[3 * i + 1] = make_float4(m[0], m[1], m[2], depth[i]);
        rec[3 * i + 2] = make_float4(n[0], n[1], n[2], 0.f);
    }
}

int launch_reproject(const TpArgs &T, bool packed, hipStream_t st) {
    const uint32_t blocks = tp_grid((uint64_t)T.xres * T.yres);
    if (blocks) {
        if (packed) hipLaunchKernelGGL(reproject<true>, dim3(blocks), dim3(256), 0, st, T);
        else hipLaunchKernelGGL(reproject<false>, dim3(blocks), dim3(256), 0, st, T);
    }
    return (int)hipGetLastError();
}
int launch_temporal_pack(uint32_t npix, const float *frame, const float *m2, const uint32_t *count, const float *normal,
                         const float *depth, float4 *rec, hipStream_t st) {
    const uint32_t blocks = tp_grid(npix);
    if (blocks) hipLaunchKernelGGL(temporal_pack, dim3(blocks), dim3(256), 0, st, npix, frame, m2, count, normal, depth, rec);
    return (int)hipGetLastError();
}

} // namespace cr
