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
// The error of pixel i (chiaro_hip.h "noise estimate"): the one statement of the formula, for the frame's map and
// statistic (noise_eval) and for the selection (select_count / select_scatter, which must agree on every pixel).
__device__ __forceinline__ float pixel_err(const float *frame, const float *m2, uint32_t i, float n, float floor) {
    const float *f = frame + 3 * (size_t)i, *q = m2 + 3 * (size_t)i;
    const float mr = f[0], mg = f[1], mb = f[2];
    float vr = q[0] - mr * mr, vg = q[1] - mg * mg, vb = q[2] - mb * mb;
    vr = (vr > 0.f) ? vr : 0.f; // (a NaN or negative variance: 0)
    vg = (vg > 0.f) ? vg : 0.f;
    vb = (vb > 0.f) ? vb : 0.f;
    const float sr = sqrtf(vr / n), sg = sqrtf(vg / n), sb = sqrtf(vb / n);
    float err = ((sr + sg) + sb) / (((mr + mg) + mb) + floor);
    if (err != err) err = 0.f;
    return err;
}
__global__ void __launch_bounds__(256) noise_eval(NoiseArgs N) {
    __shared__ uint32_t s_above[4], s_max[4];
    uint32_t above = 0, bits = 0; // (above: the wave's count, the same in every lane)
    for (uint32_t base = blockIdx.x * 256u; base < N.npix; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < N.npix;
        float err = 0.f;
        if (valid) {
            err = pixel_err(N.frame, N.m2, i, N.n, N.floor);
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

// ---- selection (cr_noise_select_device) ----
// The listed pixels whose error is above the threshold, in input order.  The sort's shape, without a wait between
// blocks: block b owns entries [b * per_block, (b + 1) * per_block) of the list -- at most SELECT_BLOCKS blocks, each
// walking its range 256 entries at a time, as noise_eval strides the frame -- and
//   select_count    writes its range's count of selected entries, of evaluated entries and its maximum to scratch;
//   select_scan     (one block) turns the counts into each block's first output slot and writes the statistic: integer
//                   sums and a maximum on the floats' bits, exact in any order;
//   select_scatter  evaluates its range again -- pixel_err, the same operations on the same inputs -- and writes each
//                   selected entry at the block's slot + the entry's rank among the range's selected ones: the ballot's
//                   bits below the lane inside a wave (mbcnt), the waves' counts through LDS inside a block.
// The per-block results meet in scratch, so nothing here is a global atomic.
struct SelectEntry {
    uint32_t pix;
    bool evaluated, selected;
    float err;
};
__device__ __forceinline__ SelectEntry select_entry(const SelectArgs &N, uint32_t i, uint32_t end) {
    SelectEntry e{LIST_SKIP, false, false, 0.f};
    if (i < end) e.pix = N.in[i];
    e.evaluated = e.pix < N.npix; // (LIST_SKIP, and an index outside the frame, is skipped)
    if (e.evaluated) e.err = pixel_err(N.frame, N.m2, e.pix, N.n, N.floor);
    e.selected = e.evaluated && e.err > N.threshold;
    return e;
}
__device__ __forceinline__ void select_range(const SelectArgs &N, uint32_t &begin, uint32_t &end) {
    const uint64_t b = (uint64_t)blockIdx.x * N.per_block;
    begin = (uint32_t)(b < N.n_in ? b : N.n_in);
    end = (uint32_t)(b + N.per_block < N.n_in ? b + N.per_block : N.n_in);
}
__global__ void __launch_bounds__(256) select_count(SelectArgs N) {
    __shared__ uint32_t s_sel[4], s_ev[4], s_max[4];
    uint32_t begin, end, sel = 0, ev = 0, bits = 0; // (sel, ev: the wave's counts, the same in every lane)
    select_range(N, begin, end);
    for (uint32_t base = begin; base < end; base += 256u) {
        const SelectEntry e = select_entry(N, base + threadIdx.x, end);
        sel += (uint32_t)__popcll(__ballot(e.selected));
        ev += (uint32_t)__popcll(__ballot(e.evaluated));
        const uint32_t eb = (e.err > 0.f) ? __float_as_uint(e.err) : 0u;
        bits = bits > eb ? bits : eb;
    }
    for (int o = 32; o; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bits, o);
        bits = bits > other ? bits : other;
    }
    if ((threadIdx.x & 63u) == 0) {
        s_sel[threadIdx.x >> 6] = sel;
        s_ev[threadIdx.x >> 6] = ev;
        s_max[threadIdx.x >> 6] = bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, v = 0, m = 0;
        for (int w = 0; w < 4; w++) {
            a += s_sel[w];
            v += s_ev[w];
            m = m > s_max[w] ? m : s_max[w];
        }
        N.scratch[blockIdx.x] = a;
        N.scratch[SELECT_BLOCKS + blockIdx.x] = v;
        N.scratch[2 * SELECT_BLOCKS + blockIdx.x] = m;
    }
}
// One block of SELECT_BLOCKS threads over the `blocks` blocks' results: scratch[3 * SELECT_BLOCKS + b] = the
// selected entries before block b's.
__global__ void __launch_bounds__(SELECT_BLOCKS) select_scan(SelectArgs N, uint32_t blocks) {
    __shared__ uint32_t a[2][SELECT_BLOCKS];
    __shared__ uint32_t s_ev, s_max;
    const uint32_t t = threadIdx.x, live = t < blocks;
    const uint32_t sel = live ? N.scratch[t] : 0u;
    if (t == 0) s_ev = 0u, s_max = 0u;
    a[0][t] = sel;
    __syncthreads();
    if (live) {
        atomicAdd(&s_ev, N.scratch[SELECT_BLOCKS + t]); // (LDS: integer sum and maximum, exact in any order)
        atomicMax(&s_max, N.scratch[2 * SELECT_BLOCKS + t]);
    }
    int cur = 0;
    for (uint32_t o = 1; o < SELECT_BLOCKS; o <<= 1) { // inclusive scan
        uint32_t v = a[cur][t];
        if (t >= o) v += a[cur][t - o];
        a[cur ^ 1][t] = v;
        __syncthreads();
        cur ^= 1;
    }
    N.scratch[3 * SELECT_BLOCKS + t] = a[cur][t] - sel;
    if (t == SELECT_BLOCKS - 1) {
        cr_select_stats *S = (cr_select_stats *)N.stats;
        S->evaluated = s_ev;
        S->above = a[cur][t];
        S->max_err = __uint_as_float(s_max);
        S->layers = N.layers;
    }
}
__global__ void __launch_bounds__(256) select_scatter(SelectArgs N) {
    __shared__ uint32_t s_cnt[4];
    uint32_t begin, end;
    select_range(N, begin, end);
    uint32_t slot = N.scratch[3 * SELECT_BLOCKS + blockIdx.x]; // of the next selected entry of this block
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t base = begin; base < end; base += 256u) {
        const SelectEntry e = select_entry(N, base + threadIdx.x, end);
        const uint64_t b = __ballot(e.selected);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if ((threadIdx.x & 63u) == 0) s_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) {
            before += w < wave ? s_cnt[w] : 0u;
            total += s_cnt[w];
        }
        if (e.selected) N.out[slot + before + rank] = e.pix;
        slot += total;
        __syncthreads(); // (s_cnt is read: the next round may write it)
    }
}

int launch_noise_select(SelectArgs N, hipStream_t st) {
    const uint32_t chunks = (uint32_t)(((uint64_t)N.n_in + 255) / 256);
    const uint32_t blocks = chunks < SELECT_BLOCKS ? chunks : (uint32_t)SELECT_BLOCKS;
    N.per_block = blocks ? (chunks + blocks - 1) / blocks * 256u : 256u;
    if (blocks) hipLaunchKernelGGL(select_count, dim3(blocks), dim3(256), 0, st, N);
    hipLaunchKernelGGL(select_scan, dim3(1), dim3(SELECT_BLOCKS), 0, st, N, blocks); // (an empty list: the zero statistic)
    if (blocks) hipLaunchKernelGGL(select_scatter, dim3(blocks), dim3(256), 0, st, N);
    return (int)hipGetLastError();
}

// ---- the lists of the adaptive render ----
__global__ void __launch_bounds__(256) tile_list(uint32_t xres, uint32_t yres, uint32_t tile, uint32_t n, uint32_t *out) {
    const uint32_t tiles_x = (xres + tile - 1) / tile, TT = tile * tile;
    for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < n; item += gridDim.x * 256u) {
        const uint32_t lt = item / TT, o = item - lt * TT; // (item_pixel's map for the whole frame, nranks 1)
        const uint32_t x = lt % tiles_x * tile + o % tile, y = lt / tiles_x * tile + o / tile;
        out[item] = x < xres && y < yres ? y * xres + x : (uint32_t)LIST_SKIP;
    }
}
int launch_tile_list(uint32_t xres, uint32_t yres, uint32_t tile, uint32_t *out, hipStream_t st) {
    const uint32_t n = ((xres + tile - 1) / tile) * ((yres + tile - 1) / tile) * tile * tile;
    const uint32_t need = (n + 255) / 256, blocks = need < NOISE_BLOCKS ? need : (uint32_t)NOISE_BLOCKS;
    if (blocks) hipLaunchKernelGGL(tile_list, dim3(blocks), dim3(256), 0, st, xres, yres, tile, n, out);
    return (int)hipGetLastError();
}
__global__ void __launch_bounds__(256) list_fill(uint32_t *map, const uint32_t *list, uint32_t n, uint32_t npix,
                                                 uint32_t value) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t pix = list ? list[i] : i;
        if (pix < npix) map[pix] = value;
    }
}
int launch_list_fill(uint32_t *map, const uint32_t *list, uint32_t n, uint32_t npix, uint32_t value, hipStream_t st) {
    const uint32_t need = (n + 255) / 256, blocks = need < NOISE_BLOCKS ? need : (uint32_t)NOISE_BLOCKS;
    if (blocks) hipLaunchKernelGGL(list_fill, dim3(blocks), dim3(256), 0, st, map, list, n, npix, value);
    return (int)hipGetLastError();
}

} // namespace cr
