// samples.hip -- the per-pixel sample sum and layer blend of a render pass (rayTracer.cpp:59-64):
// every path of the pass wrote its radiance to samples[item][sample]; these kernels add each pixel's
// samples in sample order -- the reference's order -- and blend the layer into the frame (or write the
// tile mean), so the result is bit-identical to the sequential loop whatever order the paths were
// traced in.
#include "traverse.hpp"

namespace cr {

// The moment frame's blend of one layer (MODE_BLEND): q, the in-order sum of the layer's squared samples, blended
// into m2 [yres][xres][3] exactly as write_pixel blends the radiance sum into the frame (rayTracer.cpp:64).
__device__ __forceinline__ void write_moment(const RenderArgs &A, float *m2, uint32_t x, uint32_t y, f3 q,
                                             uint32_t lj) {
    const float inv = 1.f / (float)A.spp;
    const uint32_t layer = A.layer + lj;
    float *o = m2 + 3 * ((size_t)y * A.xres + x);
    const f3 old = (layer > 1) ? mk(o[0], o[1], o[2]) : mk(0.f, 0.f, 0.f);
    const f3 nw = divs(add(muls(old, (float)(layer - 1)), muls(q, inv)), (float)layer);
    o[0] = nw.x;
    o[1] = nw.y;
    o[2] = nw.z;
}

// Per pixel: add this launch's samples in sample order onto the running sum
// (A.run, carried across sample chunks), then on the last chunk blend the
// layer into the frame / write the tile mean (write_pixel).
// M2 (cr_render_layers_noise_device, MODE_BLEND): a second accumulator takes each sample's square (the product
// rounded, then added, in the same order; carried across sample chunks in run2) and is blended into the moment
// frame m2 wherever the sum is blended into the frame.  Without M2 the two pointers are unused and the
// kernel's operations are the ones it always had.
// LIST (cr_render_layers_list_device): the item's pixel is the entry of A.list, not the tile mapping's
// (item_pixel_of); the sums, their order and the blends are the same.
template <bool M2, bool LIST = false>
__global__ void __launch_bounds__(256) sum_samples(RenderArgs A, int first, int last, float *m2, float *run2) {
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t px = 0, py = 0;
    const bool valid = item < A.n_items && item_pixel_of<LIST>(A, item, px, py);
    if (valid) {
        f3 temp = mk(0.f, 0.f, 0.f);
        if (!first) temp = mk(A.run[3 * (size_t)item], A.run[3 * (size_t)item + 1], A.run[3 * (size_t)item + 2]);
        f3 sq = mk(0.f, 0.f, 0.f);
        if (M2 && !first) sq = mk(run2[3 * (size_t)item], run2[3 * (size_t)item + 1], run2[3 * (size_t)item + 2]);
        const float *sm = A.samples + 3 * (size_t)item * A.s_count;
        // A.nl layers in one pass (never sample-chunked): each layer's run of A.spp samples is
        // summed in sample order and blended / written as its own layer, in layer order
        for (uint32_t j = 0; j + 1 < A.nl; j++) {
            for (uint32_t s = j * A.spp; s < (j + 1) * A.spp; s++) {
                const f3 v = mk(sm[3 * s], sm[3 * s + 1], sm[3 * s + 2]);
                temp = add(temp, v);
                if (M2) sq = add(sq, mul(v, v));
            }
            write_pixel(A, px, py, item, temp, j);
            temp = mk(0.f, 0.f, 0.f);
            if (M2) {
                write_moment(A, m2, px, py, sq, j);
                sq = mk(0.f, 0.f, 0.f);
            }
        }
        const uint32_t s_first = (A.nl - 1) * A.spp;
        for (uint32_t s = s_first; s < A.s_count; s++) {
            const f3 v = mk(sm[3 * s], sm[3 * s + 1], sm[3 * s + 2]);
            temp = add(temp, v);
            if (M2) sq = add(sq, mul(v, v));
        }
        if (last) {
            write_pixel(A, px, py, item, temp, A.nl - 1);
            if (M2) write_moment(A, m2, px, py, sq, A.nl - 1);
        } else {
            A.run[3 * (size_t)item] = temp.x;
            A.run[3 * (size_t)item + 1] = temp.y;
            A.run[3 * (size_t)item + 2] = temp.z;
            if (M2) {
                run2[3 * (size_t)item] = sq.x;
                run2[3 * (size_t)item + 1] = sq.y;
                run2[3 * (size_t)item + 2] = sq.z;
            }
        }
    }
    const uint64_t b = __ballot(valid && last);
    // (pixels written: one per layer of the pass)
    if (b && (threadIdx.x & 63u) == 0) atomicAdd(&A.counters[T_PIXELS], (unsigned long long)__popcll(b) * A.nl);
}

// sum_samples with the sample runs staged through LDS: a block's 256 pixels read their next SUM_C samples
// together (each pixel's run of SUM_C x 12 B read by consecutive lanes, 16 B each), then each thread adds
// its pixel's from LDS -- the same adds in the same order as sum_samples.  The thread-per-pixel reads of
// sum_samples touch 64 lines per wave-load and re-read each line ~10 loads later, by which time the many
// waves streaming beside it have evicted it from L2 (2-3x the sample bytes at the fabric).  Needs
// s_count % 4 == 0 (16-B aligned runs).
enum : uint32_t { SUM_C = 16, SUM_ROW = 3 * SUM_C + 1 }; // (+1: the rows of consecutive pixels start in other banks)
template <bool M2, bool LIST = false>
__global__ void __launch_bounds__(256) sum_samples_lds(RenderArgs A, int first, int last, float *m2, float *run2) {
    __shared__ float buf[256 * SUM_ROW];
    const uint32_t item0 = blockIdx.x * blockDim.x, item = item0 + threadIdx.x;
    const uint32_t nitems = min((uint32_t)blockDim.x, A.n_items - item0);
    uint32_t px = 0, py = 0;
    const bool valid = item < A.n_items && item_pixel_of<LIST>(A, item, px, py);
    f3 temp = mk(0.f, 0.f, 0.f);
    if (valid && !first) temp = mk(A.run[3 * (size_t)item], A.run[3 * (size_t)item + 1], A.run[3 * (size_t)item + 2]);
    f3 sq = mk(0.f, 0.f, 0.f); // (M2: the squares' sum, fed from the same staged values)
    if (M2 && valid && !first) sq = mk(run2[3 * (size_t)item], run2[3 * (size_t)item + 1], run2[3 * (size_t)item + 2]);
    const uint32_t S = A.s_count;
    const float4 *run4 = (const float4 *)(A.samples + 3 * (size_t)item0 * S); // S % 4 == 0: 16-B aligned
    const size_t stride4 = 3 * (size_t)S / 4;                                   // float4 per pixel run
    uint32_t lj = 0;                                                            // the layer of the pass
    for (uint32_t s0 = 0; s0 < S; s0 += SUM_C) {
        const uint32_t cs = min((uint32_t)SUM_C, S - s0), q = 3 * cs / 4; // samples and float4 per pixel this chunk
        __syncthreads(); // (the previous chunk is consumed)
        for (uint32_t k = threadIdx.x; k < nitems * q; k += blockDim.x) {
            const uint32_t pix = k / q, part = k - pix * q;
            const float4 v = run4[pix * stride4 + 3 * (size_t)s0 / 4 + part];
            float *d = buf + pix * SUM_ROW + 4 * part;
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
        __syncthreads();
        if (valid) {
            const float *b = buf + threadIdx.x * SUM_ROW;
            for (uint32_t t = 0; t < cs; t++) {
                const f3 v = mk(b[3 * t], b[3 * t + 1], b[3 * t + 2]);
                temp = add(temp, v);
                if (M2) sq = add(sq, mul(v, v));
                // A.nl layers in one pass (never sample-chunked): a layer's run ends -> blend / write it
                const uint32_t s = s0 + t + 1;
                if (A.nl > 1 && s < S && s % A.spp == 0) {
                    write_pixel(A, px, py, item, temp, lj);
                    temp = mk(0.f, 0.f, 0.f);
                    if (M2) {
                        write_moment(A, m2, px, py, sq, lj);
                        sq = mk(0.f, 0.f, 0.f);
                    }
                    lj++;
                }
            }
        }
    }
    if (valid) {
        if (last) {
            write_pixel(A, px, py, item, temp, A.nl - 1);
            if (M2) write_moment(A, m2, px, py, sq, A.nl - 1);
        } else {
            A.run[3 * (size_t)item] = temp.x;
            A.run[3 * (size_t)item + 1] = temp.y;
            A.run[3 * (size_t)item + 2] = temp.z;
            if (M2) {
                run2[3 * (size_t)item] = sq.x;
                run2[3 * (size_t)item + 1] = sq.y;
                run2[3 * (size_t)item + 2] = sq.z;
            }
        }
    }
    const uint64_t bl = __ballot(valid && last);
    if (bl && (threadIdx.x & 63u) == 0) atomicAdd(&A.counters[T_PIXELS], (unsigned long long)__popcll(bl) * A.nl);
}

// lds: dynamic LDS reserved per block (unused: it only caps the blocks per CU, so fewer waves share
// each CU's slice of L2 while they stream their pixels' sample runs; option "sum_lds")
// staged: sum_samples_lds when the runs are 16-B aligned (option "sum_staged", default)
// m2: the moment-tracking instantiations (MODE_BLEND), blending into the moment frame m2; run2 carries the
// squares' running sum across sample chunks ([n_items][3], as A.run); null: the plain kernels
int launch_sum_samples(const RenderArgs &A, bool first, bool last, hipStream_t st, uint32_t lds, bool staged,
                       float *m2, float *run2) {
    const uint32_t blocks = (A.n_items + 255) / 256;
    if (!blocks) return (int)hipGetLastError();
    const int f = first ? 1 : 0, l = last ? 1 : 0;
    const bool lds_kernel = staged && A.s_count % 4 == 0;
    if (A.list) { // a list pass: the same four kernels with the list's pixels
        if (m2 && lds_kernel)
            hipLaunchKernelGGL((sum_samples_lds<true, true>), dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
        else if (m2)
            hipLaunchKernelGGL((sum_samples<true, true>), dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
        else if (lds_kernel)
            hipLaunchKernelGGL((sum_samples_lds<false, true>), dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
        else
            hipLaunchKernelGGL((sum_samples<false, true>), dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
    } else if (m2 && lds_kernel)
        hipLaunchKernelGGL(sum_samples_lds<true>, dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
    else if (m2)
        hipLaunchKernelGGL(sum_samples<true>, dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
    else if (lds_kernel)
        hipLaunchKernelGGL(sum_samples_lds<false>, dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
    else
        hipLaunchKernelGGL(sum_samples<false>, dim3(blocks), dim3(256), lds, st, A, f, l, m2, run2);
    return (int)hipGetLastError();
}

} // namespace cr
