// append.hpp -- block-aggregated queue appends shared by the wavefront kernels (wavefront.hip) and the
// ray-query ingest (queries.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cr {

// Block-aggregated appends (call with the whole block, uniformly): one global atomicAdd per block and
// queue instead of one per wave -- same-address atomics from every wave of the grid serialise in one L2
// slice.  Slots keep lane order within a wave and wave order within the block.
// (lds: one word per wave of the block, up to 16, then the base)
enum : uint32_t { APP_W = 16 };
// N appends of one block at once (wf_shade's shadow and closest queues): one barrier round and
// the N global atomics in flight together instead of one after another.  lds: [2][4 N + N] words,
// the half `buf` alternating between consecutive calls (so no barrier is needed before the next
// call writes it: the one after that is separated from this one by the next call's barriers).
template <int N>
__device__ __forceinline__ void block_append_n(uint32_t *const (&counter)[N], const bool (&pred)[N], uint32_t *lds,
                                               uint32_t buf, uint32_t (&slot)[N]) {
    uint32_t *L = lds + buf * (APP_W + 1u) * N;
    const uint32_t wave = threadIdx.x >> 6;
    uint64_t m[N];
#pragma unroll
    for (int q = 0; q < N; q++) {
        m[q] = __ballot(pred[q]);
        if ((threadIdx.x & 63u) == 0) L[APP_W * q + wave] = (uint32_t)__popcll(m[q]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot[N];
#pragma unroll
        for (int q = 0; q < N; q++) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < (blockDim.x >> 6); w++) {
                const uint32_t c = L[APP_W * q + w];
                L[APP_W * q + w] = s;
                s += c;
            }
            tot[q] = s;
        }
        uint32_t base[N];
#pragma unroll
        for (int q = 0; q < N; q++) base[q] = tot[q] ? atomicAdd(counter[q], tot[q]) : 0u;
#pragma unroll
        for (int q = 0; q < N; q++) L[APP_W * N + q] = base[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; q++)
        slot[q] = L[APP_W * N + q] + L[APP_W * q + wave] +
                  __builtin_amdgcn_mbcnt_hi((uint32_t)(m[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[q], 0u));
}

} // namespace cr
