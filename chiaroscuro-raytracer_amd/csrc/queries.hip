// queries.hip -- the kernels around the trace launches of a device-resident ray-query batch
// (cr_intersect_device / cr_intersect_shadow_device):
//   query_ingest   one thread per query: route it (queryroute.hpp), append it to the trace queue (the
//                  records wf_trace reads, the light to ignore, the sort key) or to the index list of
//                  the per-thread kernel; block-aggregated appends (append.hpp)
//   query_finish   one thread: the append counters become the queue counts and work counters of the
//                  two trace launches
//   query_scatter  one thread per queue slot: the slot's answer written at the query's index, the hit
//                  distance re-evaluated from the hit triangle's record with tri_test's expressions
// Nothing here reads a count on the host: the grids cover the chunk and test against the counters.
#include "append.hpp"
#include "queryroute.hpp"
#include "render_common.hpp"

namespace cr {

__global__ void __launch_bounds__(256) query_ingest(QueryDevArgs Q) {
    __shared__ uint32_t app_lds[2 * (APP_W + 1u) * 3u];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < Q.n;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f}, limit = 0.f;
    uint32_t light = 0u;
    int route = -1;
    const float bmin[3] = {Q.S.bmin.x, Q.S.bmin.y, Q.S.bmin.z}, bmax[3] = {Q.S.bmax.x, Q.S.bmax.y, Q.S.bmax.z};
    if (live) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            o[a] = Q.orig[3 * (size_t)i + a];
            d[a] = Q.dir[3 * (size_t)i + a];
        }
        if (Q.shadow) {
            limit = Q.dist[i];
            light = Q.light[i];
        }
        route = Q.route == 1u ? (int)QR_LEGACY : query_route(o, d, Q.shadow != 0u, limit, light, bmin, bmax, Q.S.db);
        if (route == QR_DEFAULT && Q.route == 2u) route = QR_FAT;
        if (route == QR_FAT && Q.no_cull && Q.route != 2u) route = QR_DEFAULT;
    }
    const bool traced = route == QR_DEFAULT || route == QR_FAT;
    uint32_t *const counter[3] = {Q.qc + QC_TRACED, Q.qc + QC_LEGACY, Q.qc + QC_DEFAULT};
    const bool pred[3] = {traced, route == QR_LEGACY, route == QR_DEFAULT};
    uint32_t slot[3];
    block_append_n<3>(counter, pred, app_lds, 0u, slot);
    if (traced) {
        const uint32_t s = slot[0];
        // (w = the query's index in the chunk: below the chunk's capacity, never NO_PATH)
        Q.ray[2 * (size_t)s] = make_float4(o[0], o[1], o[2], __uint_as_float(i));
        Q.ray[2 * (size_t)s + 1] = make_float4(d[0], d[1], d[2], limit);
        if (Q.shadow) Q.sexcl[s] = light;
        const uint32_t k = Q.sort ? query_key(o, d, bmin, bmax, QUERY_WORLD_BITS, QUERY_DIR_RES) : 0u;
        Q.key[s] = Q.sort ? (k | (route == QR_FAT ? 1u << QUERY_ROUTE_BIT : 0u)) : (route == QR_FAT ? 1u : 0u);
    } else if (route == QR_LEGACY) {
        Q.list[slot[1]] = i;
    }
}

// The default build's launch takes entries [0, na) of the (sorted) order, the fat kernels' [na, na + nb):
// its count is na + nb and its work counter starts at na.
__global__ void query_finish(QueryDevArgs Q) {
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t nab = Q.qc[QC_TRACED], na = Q.qc[QC_DEFAULT];
    const uint32_t cq = Q.shadow ? WF_G : 0u, wq = Q.shadow ? 3u * WF_G : 2u * WF_G;
    Q.cnt[cq + QUERY_G_DEFAULT] = na;
    Q.cnt[wq + QUERY_G_DEFAULT] = 0u;
    Q.cnt[cq + QUERY_G_FAT] = nab;
    Q.cnt[wq + QUERY_G_FAT] = na;
}

__global__ void __launch_bounds__(256) query_scatter(QueryDevArgs Q) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= Q.n || s >= Q.qc[QC_TRACED]) return;
    const float4 r0 = Q.ray[2 * (size_t)s];
    const uint32_t i = __float_as_uint(r0.w);
    if (i >= Q.n) return;
    if (Q.shadow) {
        Q.hit[i] = Q.occ[s];
        return;
    }
    // {tri, bx, by, leaf + 1}; a miss is the all-zero record (w tells it from triangle 0 at (0, 0))
    const uint4 h = Q.hits[s];
    Q.hit[i] = h.w ? 1u : 0u;
    if (!h.w) return;
    if (Q.tri) Q.tri[i] = h.x;
    if (Q.bary) {
        Q.bary[2 * (size_t)i] = __uint_as_float(h.y);
        Q.bary[2 * (size_t)i + 1] = __uint_as_float(h.z);
    }
    if (Q.dist_out) {
        // the hit record carries no distance: tri_test on the hit triangle's record in its leaf gives the
        // bits the trace compared (the same expressions on the same operands, no contraction)
        const f3 o = ld3(r0), d = ld3(Q.ray[2 * (size_t)s + 1]);
        const uint2 nd = h.w - 1u < Q.S.n_nodes ? Q.S.nodes[h.w - 1u] : make_uint2(0u, 3u);
        const uint32_t first = nd.x, count = (nd.y & 3u) == 3u ? nd.y >> 2 : 0u;
        float t = __builtin_nanf(""); // (never stored as it is: the hit's record is in the hit's leaf)
        for (uint32_t j = 0; j < count; j++) {
            const TriRec r = load_rec(Q.S, first + j);
            if (rec_id(r) != h.x) continue;
            float ux, uy, tt = 0.f;
            if (tri_test(o, d, r, __builtin_inff(), ux, uy, tt)) t = tt;
            break;
        }
        Q.dist_out[i] = t;
    }
}

int launch_query_ingest(const QueryDevArgs &Q, hipStream_t st) {
    if (Q.n == 0) return 0;
    hipLaunchKernelGGL(query_ingest, dim3((Q.n + 255u) / 256u), dim3(256), 0, st, Q);
    hipLaunchKernelGGL(query_finish, dim3(1), dim3(64), 0, st, Q);
    return (int)hipGetLastError();
}

int launch_query_scatter(const QueryDevArgs &Q, hipStream_t st) {
    if (Q.n == 0) return 0;
    hipLaunchKernelGGL(query_scatter, dim3((Q.n + 255u) / 256u), dim3(256), 0, st, Q);
    return (int)hipGetLastError();
}

} // namespace cr
