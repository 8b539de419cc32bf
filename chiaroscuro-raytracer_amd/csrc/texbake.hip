// texbake.hip -- the texture-space side of a lightmap bake (cr_bake_surface_device / cr_bake_dilate_device;
// include/chiaro_hip.h "lightmap baking"): which triangle owns each texel of a W x H map, the
// surface point and normal under the texel's centre, the owned texels as an ascending list, and the dilation that
// fills the gutters of the baked map.  The arithmetic is bake.hpp's, the same functions the host restatement
// compiles: float32, no contraction, IEEE division.
#include "bake.hpp"
#include "kernels.hpp"

namespace cr {

enum : uint32_t { BAKE_BLOCKS = 2048 }; // the most blocks of a grid-striding per-texel kernel

// ---- owner pass ----
// One wave per triangle: its six UVs, A and box are wave-uniform (the triangle id goes through readfirstlane, so the
// loads are scalar), and the lanes stride over the texels of the box clipped to the map -- a triangle that spans the
// map is 64 lanes wide, not one.  A covered texel takes the lowest id that covers it: atomicMin on the map preset
// to BAKE_NONE, one vector atomic per covered texel, each at its own address (no two lanes of a wave share one).
__global__ void __launch_bounds__(256) bake_owner(BakeArgs B) {
    const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (t >= B.n_tris) return;
    float uv[6];
    for (int k = 0; k < 6; k++) uv[k] = B.uv[6 * (size_t)t + k];
    const BakeTri T = bake_tri(uv, (float)B.W, (float)B.H);
    uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    if (!bake_box(T, B.W, B.H, x0, x1, y0, y1)) return;
    const uint32_t bw = x1 - x0 + 1u, n = bw * (y1 - y0 + 1u); // (<= W * H <= 2^31)
    for (uint32_t i = threadIdx.x & 63u; i < n; i += 64u) {
        const uint32_t r = i / bw, x = x0 + (i - r * bw), y = y0 + r; // (x <= x1 < W, y <= y1 < H)
        if (bake_weights(T, x, y).covered) atomicMin(&B.owner[(size_t)y * B.W + x], t);
    }
}

// ---- surface pass and the covered list ----
// The compaction has the selection's shape (noise.hip): block b owns texels [b * per_block, (b + 1) * per_block),
//   bake_surface  writes each texel's point and normal (zeros where unowned) and its range's count of owned texels,
//   bake_scan     (one block) turns the counts into each block's first slot and writes the total to *count,
//   bake_scatter  writes each owned texel's index at the block's slot + its rank among the range's owned texels.
// The per-block counts meet in scratch: no same-address atomic, and the list ascends.
__device__ __forceinline__ void bake_range(const BakeArgs &B, uint32_t &begin, uint32_t &end) {
    const uint64_t b = (uint64_t)blockIdx.x * B.per_block;
    begin = (uint32_t)(b < B.npix ? b : B.npix);
    end = (uint32_t)(b + B.per_block < B.npix ? b + B.per_block : B.npix);
}
__global__ void __launch_bounds__(256) bake_surface(BakeArgs B) {
    __shared__ uint32_t s_cnt[4];
    uint32_t begin, end, cnt = 0; // (cnt: the wave's count, the same in every lane)
    bake_range(B, begin, end);
    const float fW = (float)B.W, fH = (float)B.H;
    for (uint32_t base = begin; base < end; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        bool owned = false;
        if (i < end) {
            const uint32_t t = B.owner[i];
            owned = t < B.n_tris; // (BAKE_NONE is no triangle)
            float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
            if (owned) {
                float uv[6];
                for (int k = 0; k < 6; k++) uv[k] = B.uv[6 * (size_t)t + k];
                const BakeTri T = bake_tri(uv, fW, fH);
                const uint32_t y = i / B.W, x = i - y * B.W;
                const float4 n = B.mat_n[t];
                const float nn[3] = {n.x, n.y, n.z};
                bake_point(bake_weights(T, x, y), (const float *)(B.tri + 3 * (size_t)t), 4, nn, B.offset, pos, nrm);
            }
            float *po = B.pos + 3 * (size_t)i, *no = B.nrm + 3 * (size_t)i;
            po[0] = pos[0], po[1] = pos[1], po[2] = pos[2];
            no[0] = nrm[0], no[1] = nrm[1], no[2] = nrm[2];
        }
        cnt += (uint32_t)__popcll(__ballot(owned));
    }
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) B.scratch[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}
// One block of SELECT_BLOCKS threads over the `blocks` blocks' counts: scratch[SELECT_BLOCKS + b] = the owned texels
// before block b's
__global__ void __launch_bounds__(SELECT_BLOCKS) bake_scan(BakeArgs B, uint32_t blocks) {
    __shared__ uint32_t a[2][SELECT_BLOCKS];
    const uint32_t t = threadIdx.x;
    const uint32_t own = t < blocks ? B.scratch[t] : 0u;
    a[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (uint32_t o = 1; o < SELECT_BLOCKS; o <<= 1) { // inclusive scan
        uint32_t v = a[cur][t];
        if (t >= o) v += a[cur][t - o];
        a[cur ^ 1][t] = v;
        __syncthreads();
        cur ^= 1;
    }
    B.scratch[SELECT_BLOCKS + t] = a[cur][t] - own;
    if (t == SELECT_BLOCKS - 1) *B.count = a[cur][t];
}
__global__ void __launch_bounds__(256) bake_scatter(BakeArgs B) {
    __shared__ uint32_t s_cnt[4];
    uint32_t begin, end;
    bake_range(B, begin, end);
    uint32_t slot = B.scratch[SELECT_BLOCKS + blockIdx.x]; // of the next owned texel of this block
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t base = begin; base < end; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool owned = i < end && B.owner[i] < B.n_tris;
        const uint64_t b = __ballot(owned);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if ((threadIdx.x & 63u) == 0) s_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) {
            before += w < wave ? s_cnt[w] : 0u;
            total += s_cnt[w];
        }
        if (owned) B.list[slot + before + rank] = i; // (slot + before + rank < the total <= npix: room W * H)
        slot += total;
        __syncthreads(); // (s_cnt is read: the next round may write it)
    }
}

int launch_bake_surface(BakeArgs B, hipStream_t st) {
    B.npix = B.W * B.H;
    if (hipError_t e = hipMemsetAsync(B.owner, 0xff, (size_t)B.npix * sizeof(uint32_t), st)) return (int)e; // BAKE_NONE
    if (B.n_tris) hipLaunchKernelGGL(bake_owner, dim3((B.n_tris + 3u) / 4u), dim3(256), 0, st, B);
    const uint32_t chunks = (uint32_t)(((uint64_t)B.npix + 255) / 256);
    const uint32_t blocks = chunks < SELECT_BLOCKS ? chunks : (uint32_t)SELECT_BLOCKS;
    B.per_block = (chunks + blocks - 1) / blocks * 256u;
    hipLaunchKernelGGL(bake_surface, dim3(blocks), dim3(256), 0, st, B);
    hipLaunchKernelGGL(bake_scan, dim3(1), dim3(SELECT_BLOCKS), 0, st, B, blocks);
    hipLaunchKernelGGL(bake_scatter, dim3(blocks), dim3(256), 0, st, B);
    return (int)hipGetLastError();
}

// ---- dilation ----
// level [H][W] (bake.hpp bake_dilate_host): 0 an owned texel, p one filled by pass p, BAKE_NONE not filled.  Pass p
// reads the neighbours of level < p -- values and levels that earlier passes wrote -- and writes level p, which
// nothing in pass p reads: the passes ping-pong between "before p" and "p" inside one value array and one level map.
__global__ void __launch_bounds__(256) dilate_init(DilateArgs D) {
    const uint32_t npix = D.W * D.H;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        const float *s = D.in + 3 * (size_t)i;
        float *o = D.out + 3 * (size_t)i;
        o[0] = s[0], o[1] = s[1], o[2] = s[2];
        if (D.level) D.level[i] = D.owner[i] == BAKE_NONE ? (uint32_t)BAKE_NONE : 0u;
    }
}
__global__ void __launch_bounds__(256) dilate_pass(DilateArgs D, uint32_t p) {
    const uint32_t npix = D.W * D.H;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        if (D.level[i] != BAKE_NONE) continue;
        const uint32_t y = i / D.W, x = i - y * D.W;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            int dx, dy;
            bake_neighbour(j, dx, dy);
            const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy; // (x - 1 of x == 0 wraps above W)
            if (nx >= D.W || ny >= D.H) continue;
            const uint32_t q = ny * D.W + nx;
            if (D.level[q] >= p) continue;
            const float *v = D.out + 3 * (size_t)q;
            s0 = s0 + v[0], s1 = s1 + v[1], s2 = s2 + v[2];
            cnt++;
        }
        if (!cnt) continue;
        const float fc = (float)cnt;
        float *o = D.out + 3 * (size_t)i;
        o[0] = s0 / fc, o[1] = s1 / fc, o[2] = s2 / fc;
        D.level[i] = p;
    }
}
int launch_bake_dilate(const DilateArgs &D, uint32_t passes, hipStream_t st) {
    const uint32_t npix = D.W * D.H, need = (npix + 255u) / 256u;
    const uint32_t blocks = need < BAKE_BLOCKS ? need : (uint32_t)BAKE_BLOCKS;
    hipLaunchKernelGGL(dilate_init, dim3(blocks), dim3(256), 0, st, D);
    for (uint32_t p = 1; p <= passes; p++) hipLaunchKernelGGL(dilate_pass, dim3(blocks), dim3(256), 0, st, D, p);
    return (int)hipGetLastError();
}

} // namespace cr
