// probe.hip -- SH irradiance probes (cr_probe_sh_device / cr_probe_eval_device / cr_probe_sample_device;
// include/chiaro_hip.h "probes"): the sum of an SH pass, which projects every path's radiance onto
// the L2 basis of the direction its sample was aimed along, and the two lookups.  The arithmetic is probe.hpp's, the
// same functions the host restatement compiles: float32, no contraction, IEEE division and square root.
#include "probe.hpp"
#include "traverse.hpp"

namespace cr {

// The sum of an SH pass: the list form of sum_samples (samples.hip) with 27 chains per item instead of 3.  A thread
// per work item; entry e = list[item] of the pass owns probe e of H.sh.  Sample s of the launch is sample
// A.s0 + s of the pass, so its direction is recomputed from the stream wf_camera_sphere drew it from --
// (seed, layer, id0 + e, sample), draws 0 and 1 -- and nothing is stored per path but the radiance.  The chains are
// folded in sample order, carried across sample chunks in H.run / H.run2 [n_items][27] (A.run has room for 3), and
// blended per layer of a pass group as sum_samples blends: a pass of A.nl > 1 layers is never sample-chunked.
// Every index into t, q and Y is a constant after unrolling: the 27 (54) chains live in registers, no scratch.
template <bool M2>
__global__ void __launch_bounds__(256) sum_samples_sh(RenderArgs A, int first, int last, ShOut H) {
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t e = 0, ey = 0;
    const bool valid = item < A.n_items && item_pixel_of<true>(A, item, e, ey); // (a frame of n entries x 1)
    if (valid) {
        float t[PROBE_F], q[PROBE_F];
        const float *r1 = H.run + (size_t)PROBE_F * item, *r2 = H.run2 + (size_t)PROBE_F * item;
#pragma unroll
        for (int f = 0; f < (int)PROBE_F; f++) {
            t[f] = first ? 0.f : r1[f];
            q[f] = (M2 && !first) ? r2[f] : 0.f;
        }
        const float inv = 1.f / (float)A.spp;
        float *o = H.sh + (size_t)PROBE_F * e, *o2 = H.m2 + (size_t)PROBE_F * e;
        const float *sm = A.samples + 3 * (size_t)item * A.s_count;
        uint32_t lj = 0; // the layer of the pass
        for (uint32_t s = 0; s < A.s_count; s++) {
            Rng rng = path_rng(A, H.id0 + e, A.s0 + s);
            const uint32_t raw0 = rng_u32(rng), raw1 = rng_u32(rng);
            float d[3], Y[PROBE_K];
            probe_dir(raw0, raw1, d);
            probe_basis(d[0], d[1], d[2], Y);
            const float v[3] = {sm[3 * s], sm[3 * s + 1], sm[3 * s + 2]};
            probe_accum(Y, v, t, M2 ? q : nullptr);
            // A.nl layers in one pass: a layer's run ends -> blend it and start the next from 0
            if (A.nl > 1 && s + 1 < A.s_count && (s + 1) % A.spp == 0) {
#pragma unroll
                for (int f = 0; f < (int)PROBE_F; f++) {
                    o[f] = probe_blend(o[f], t[f], inv, A.layer + lj);
                    t[f] = 0.f;
                    if (M2) {
                        o2[f] = probe_blend(o2[f], q[f], inv, A.layer + lj);
                        q[f] = 0.f;
                    }
                }
                lj++;
            }
        }
        if (last) {
#pragma unroll
            for (int f = 0; f < (int)PROBE_F; f++) {
                o[f] = probe_blend(o[f], t[f], inv, A.layer + A.nl - 1);
                if (M2) o2[f] = probe_blend(o2[f], q[f], inv, A.layer + A.nl - 1);
            }
        } else {
            float *w1 = H.run + (size_t)PROBE_F * item, *w2 = H.run2 + (size_t)PROBE_F * item;
#pragma unroll
            for (int f = 0; f < (int)PROBE_F; f++) {
                w1[f] = t[f];
                if (M2) w2[f] = q[f];
            }
        }
    }
    const uint64_t b = __ballot(valid && last);
    // (pixels written: one per layer of the pass, as sum_samples counts them)
    if (b && (threadIdx.x & 63u) == 0) atomicAdd(&A.counters[T_PIXELS], (unsigned long long)__popcll(b) * A.nl);
}

int launch_sum_samples_sh(const RenderArgs &A, bool first, bool last, const ShOut &H, hipStream_t st) {
    const uint32_t blocks = (A.n_items + 255) / 256;
    if (!blocks) return (int)hipGetLastError();
    if (!A.list || !H.sh) return (int)hipErrorInvalidValue; // (an SH pass is a list pass)
    const int f = first ? 1 : 0, l = last ? 1 : 0;
    if (H.m2) hipLaunchKernelGGL(sum_samples_sh<true>, dim3(blocks), dim3(256), 0, st, A, f, l, H);
    else hipLaunchKernelGGL(sum_samples_sh<false>, dim3(blocks), dim3(256), 0, st, A, f, l, H);
    return (int)hipGetLastError();
}

// ---- the lookups: a thread per query ----
__global__ void __launch_bounds__(256) probe_eval_kernel(const float *sh, const uint32_t *probe, const float *nrm,
                                                         float *out, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const float n[3] = {nrm[3 * (size_t)j], nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2]};
    float v[3];
    probe_eval(sh + (size_t)PROBE_F * probe[j], n, v);
    out[3 * (size_t)j] = v[0];
    out[3 * (size_t)j + 1] = v[1];
    out[3 * (size_t)j + 2] = v[2];
}
__global__ void __launch_bounds__(256) probe_sample_kernel(ProbeGrid G, const float *sh, const float *pos,
                                                           const float *nrm, float *out, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const float p[3] = {pos[3 * (size_t)j], pos[3 * (size_t)j + 1], pos[3 * (size_t)j + 2]};
    const float n[3] = {nrm[3 * (size_t)j], nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2]};
    float v[3];
    probe_sample(G, sh, p, n, v);
    out[3 * (size_t)j] = v[0];
    out[3 * (size_t)j + 1] = v[1];
    out[3 * (size_t)j + 2] = v[2];
}

int launch_probe_eval(const float *sh, const uint32_t *probe, const float *nrm, float *out, uint32_t m, hipStream_t st) {
    if (m) hipLaunchKernelGGL(probe_eval_kernel, dim3((uint32_t)(((uint64_t)m + 255) / 256)), dim3(256), 0, st, sh, probe, nrm, out, m);
    return (int)hipGetLastError();
}
int launch_probe_sample(const ProbeGrid &G, const float *sh, const float *pos, const float *nrm, float *out, uint32_t m,
                        hipStream_t st) {
    if (m) hipLaunchKernelGGL(probe_sample_kernel, dim3((uint32_t)(((uint64_t)m + 255) / 256)), dim3(256), 0, st, G, sh, pos, nrm, out, m);
    return (int)hipGetLastError();
}

} // namespace cr
