// noise.hip -- how noisy a progressive frame still is (cr_noise_device): from the frame (the
// mean of layers * spp samples per pixel, src/rayTracer.cpp:18-33,59-64) and the moment frame the sum kernels
// keep beside it (samples.hip), the standard error of each pixel's mean relative to its brightness, and an
// exact frame statistic -- two integer counts and a maximum, which no reduction order can change.
// float32, no contraction, IEEE division and square root: the operations are exactly the ones written here.
#include "chiaro_hip.h"
#include "kernels.hpp"

namespace cr {

// One thread per pixel, the blocks striding over the frame when it has more pixels than NOISE_BLOCKS blocks hold.
// A block's `above` count goes to the statistic with one atomic per block (the ballots' popcounts summed per
// wave, then through LDS) and so does its maximum: same-address device atomics serialise at ~5.7 ns each
//  -- one pair per 256 pixels was 16200 of them at 1080p, 196 us for a kernel whose 50 MB of
// reads take a tenth of that; with at most NOISE_BLOCKS blocks it is 2048, and 36 us.  The maximum is an atomicMax on the
// floats' bits, which order as the floats do for err >= +0; a negative or -0 err (a negative mean, which no
// render produces) leaves the maximum at 0.
enum : uint32_t { NOISE_BLOCKS = 1024 };
__global__ void __launch_bounds__(256) noise_eval(NoiseArgs N) {
    __shared__ uint32_t s_above[4], s_max[4];
    uint32_t above = 0, bits = 0; // (above: the wave's count, the same in every lane)
    for (uint32_t base = blockIdx.x * 256u; base < N.npix; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < N.npix;
        float err = 0.f;
        if (valid) {
            const float *f = N.frame + 3 * (size_t)i, *q = N.m2 + 3 * (size_t)i;
            const float mr = f[0], mg = f[1], mb = f[2];
            float vr = q[0] - mr * mr, vg = q[1] - mg * mg, vb = q[2] - mb * mb;
            vr = (vr > 0.f) ? vr : 0.f; // (a NaN or negative variance: 0)
            vg = (vg > 0.f) ? vg : 0.f;
            vb = (vb > 0.f) ? vb : 0.f;
            const float sr = sqrtf(vr / N.n), sg = sqrtf(vg / N.n), sb = sqrtf(vb / N.n);
            err = ((sr + sg) + sb) / (((mr + mg) + mb) + N.floor);
            if (err != err) err = 0.f;
            if (N.err) N.err[i] = err;
        }
        above += (uint32_t)__popcll(__ballot(valid && err > N.threshold));
        const uint32_t eb = (err > 0.f) ? __float_as_uint(err) : 0u;
        bits = bits > eb ? bits : eb;
    }
    for (int o = 32; o; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bits, o);
        bits = bits > other ? bits : other;
    }
    if ((threadIdx.x & 63u) == 0) {
        s_above[threadIdx.x >> 6] = above;
        s_max[threadIdx.x >> 6] = bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cr_noise_stats *S = (cr_noise_stats *)N.stats;
        uint32_t a = 0, m = 0;
        for (int w = 0; w < 4; w++) {
            a += s_above[w];
            m = m > s_max[w] ? m : s_max[w];
        }
        if (a) atomicAdd((unsigned long long *)&S->above, (unsigned long long)a);
        if (m) atomicMax((uint32_t *)&S->max_err, m);
        if (blockIdx.x == 0) {
            S->pixels = N.npix;
            S->layers = N.layers;
        }
    }
}

int launch_noise_eval(const NoiseArgs &N, hipStream_t st) {
    const uint32_t need = (N.npix + 255) / 256, blocks = need < NOISE_BLOCKS ? need : (uint32_t)NOISE_BLOCKS;
    if (!blocks) return (int)hipGetLastError();
    hipLaunchKernelGGL(noise_eval, dim3(blocks), dim3(256), 0, st, N);
    return (int)hipGetLastError();
}

} // namespace cr
