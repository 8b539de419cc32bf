// scenelayout.hpp -- the device layout of a scene as one pure host function: what cr_upload_scene (cabi.cpp)
// validates, renumbers and builds from a cr_scene_desc before it uploads anything.  Every address the trace kernels
// compute assumes this layout, so it runs without a device (tests/native/scenelayout_check.cpp).  No HIP runtime
// call; kernels.hpp for the vector types and constants.
#pragma once
#include "chiaro_hip.h"
#include "kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace cr {

struct SceneLayout {
    // DevScene's arrays; levels: the inner nodes by depth, deepest first; level_off: each level's [offset, count)
    std::vector<uint32_t> levels;
    std::vector<uint2> nodes, lights;
    std::vector<uint4> fat, lcullc, texs;
    std::vector<float4> recs, lcullp, tri, mat_n, mat_kd, mat_ke;
    std::vector<float2> mat_uv;
    std::vector<uint8_t> texels;
    std::vector<std::pair<uint32_t, uint32_t>> level_off;
    std::vector<float> splits[3]; // split positions of the inner nodes per axis, sorted
    DevScene S{}; // its scalars (lcg, db, nlights, n_nodes, the box); the pointers stay null: the upload's
    uint32_t tree_depth = 0, stack_depth = 1, n_refs = 0, n_tris = 0;
};

// The layout of *d with the first node_bfs nodes numbered breadth-first; CR_OK, or the code with its message in err.
inline int scene_layout(const cr_scene_desc *d, uint32_t node_bfs, SceneLayout &out, std::string &err) {
    auto fail = [&err](int code, const char *msg) { return err = msg, code; };
    const uint32_t nt = d->n_tris;
    // nodes -> {split bits | first, axis | child<<2}, validated first
    const uint32_t NN = d->n_nodes;
    for (uint32_t i = 0; i < NN; i++) {
        const cr_kdnode &n = d->nodes[i];
        if (n.axis == 3) {
            if (n.count >= (1u << 30) || (uint64_t)n.child_or_first + n.count > d->n_refs)
                return fail(CR_E_INVALID, "bad leaf range");
        } else if (n.axis > 2 || (uint64_t)n.child_or_first + 1 >= NN || n.child_or_first >= (1u << 30)) {
            return fail(CR_E_INVALID, "bad inner node");
        }
    }
    // node numbering: the first NODE_BFS nodes breadth-first from the root (each inner
    // node's two children take consecutive ids, as KDTree::build allocates them), the
    // rest in the reference's depth-first order -- the top of the tree is nodes
    // 0..NODE_BFS-1 for the LDS node tile; only addresses change, not the traversal
    std::vector<uint32_t> newid(NN, 0xffffffffu), order;
    order.reserve(NN);
    order.push_back(0);
    newid[0] = 0;
    for (size_t h = 0; h < order.size() && order.size() + 2 <= node_bfs; h++) {
        const cr_kdnode &n = d->nodes[order[h]];
        if (n.axis == 3) continue;
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t ch = n.child_or_first + k;
            if (newid[ch] != 0xffffffffu) return fail(CR_E_INVALID, "kd node with two parents");
            newid[ch] = (uint32_t)order.size();
            order.push_back(ch);
        }
    }
    for (uint32_t i = 0; i < NN; i++)
        if (newid[i] == 0xffffffffu) {
            newid[i] = (uint32_t)order.size();
            order.push_back(i);
        }
    std::vector<uint2> nodes(NN);
    for (uint32_t i = 0; i < NN; i++) {
        const cr_kdnode &n = d->nodes[i];
        if (n.axis == 3) {
            nodes[newid[i]] = make_uint2(n.child_or_first, 3u | (n.count << 2));
        } else {
            const uint32_t ch = newid[n.child_or_first];
            if (newid[n.child_or_first + 1] != ch + 1) return fail(CR_E_INVALID, "kd siblings not adjacent");
            uint32_t sb;
            std::memcpy(&sb, &n.split, 4);
            nodes[newid[i]] = make_uint2(sb, n.axis | (ch << 2));
        }
    }
    // fat node records: a node's own record followed by both children's
    if ((uint64_t)32 * d->n_nodes > 0xFFFFFFFFull) return fail(CR_E_INVALID, "more than 134 M kd nodes");
    std::vector<uint4> fat((size_t)2 * d->n_nodes, make_uint4(0u, 0u, 0u, 0u));
    for (uint32_t i = 0; i < d->n_nodes; i++) {
        const uint2 n = nodes[i];
        fat[2 * (size_t)i].x = n.x;
        fat[2 * (size_t)i].y = n.y;
        if ((n.y & 3u) != 3u) {
            const uint32_t ch = n.y >> 2;
            fat[2 * (size_t)i].z = nodes[ch].x;
            fat[2 * (size_t)i].w = nodes[ch].y;
            fat[2 * (size_t)i + 1] = make_uint4(nodes[ch + 1].x, nodes[ch + 1].y, 0u, 0u);
        }
    }
    // leaf-ordered triangle records {A,id},{B-A},{C-A}: e1/e2 computed exactly as
    // intersectRayTriangle does each time (kdtree.cpp:222-223), so bit-identical.
    // load_rec addresses records with a 32-bit byte offset
    if ((uint64_t)16 * cr::REC_STRIDE * ((uint64_t)d->n_refs + 1) > 0xFFFFFFFFull)
        return fail(CR_E_INVALID, "more than 89 M leaf references (triangle records exceed 4 GiB)");
    // + one zero record past the last (an empty leaf's `first` may be n_refs)
    std::vector<float4> recs((size_t)cr::REC_STRIDE * ((size_t)d->n_refs + 1), make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint32_t r = 0; r < d->n_refs; r++) {
        const uint32_t t = d->refs[r];
        if (t >= nt) return fail(CR_E_INVALID, "leaf ref out of range");
        const float *p = d->tri_pos + 9 * (size_t)t;
        float idf;
        std::memcpy(&idf, &t, 4);
        float4 *q = recs.data() + (size_t)cr::REC_STRIDE * r;
        q[0] = make_float4(p[0], p[1], p[2], idf);
        q[1] = make_float4(p[3] - p[0], p[4] - p[1], p[5] - p[2], 0.f);
        q[2] = make_float4(p[6] - p[0], p[7] - p[1], p[8] - p[2], 0.f);
    }
    // leaf cull records (leafcull.hpp), per node of the new numbering; host threads.  The per-ray and
    // fixed-pad forms stay on the host: they are the steps from which the packed (LC 4) and the
    // compressed (LC 5) records the traces read are derived
    std::vector<float4> lcull((size_t)cr::LC_REC * NN, make_float4(0.f, 0.f, 0.f, 0.f));
    {
        const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        for (unsigned w = 0; w < nth; w++)
            th.emplace_back([&, w] {
                float A[cr::LC_MAXREFS][3], e1[cr::LC_MAXREFS][3], e2[cr::LC_MAXREFS][3];
                for (uint32_t i = w; i < NN; i += nth) {
                    if ((nodes[i].y & 3u) != 3u) continue;
                    const uint32_t first = nodes[i].x, cnt = nodes[i].y >> 2;
                    const uint32_t m = std::min(cnt, (uint32_t)cr::LC_MAXREFS);
                    for (uint32_t j = 0; j < m; j++) {
                        const float4 *q = recs.data() + (size_t)cr::REC_STRIDE * (first + j);
                        A[j][0] = q[0].x, A[j][1] = q[0].y, A[j][2] = q[0].z;
                        e1[j][0] = q[1].x, e1[j][1] = q[1].y, e1[j][2] = q[1].z;
                        e2[j][0] = q[2].x, e2[j][1] = q[2].y, e2[j][2] = q[2].z;
                    }
                    cr::leaf_cull_record(A, e1, e2, cnt, (cr::LcFloat4 *)(lcull.data() + (size_t)cr::LC_REC * i));
                }
            });
        for (auto &t : th) t.join();
    }
    // ... and in the fixed-pad form: origins and vertices inside the padded box (+1: the 0.001 n offsets)
    std::vector<float4> lcullf((size_t)cr::LC_REC * NN, make_float4(0.f, 0.f, 0.f, 0.f));
    double lc_db = 1.0;
    {
        double &db = lc_db, smax = 0.0;
        for (int i = 0; i < 3; i++) {
            db = std::max(db, std::max(std::fabs((double)d->box_min[i]), std::fabs((double)d->box_max[i])) + 1.0);
            smax = std::max(smax, (double)d->box_max[i] - (double)d->box_min[i] + 2.0);
        }
        db *= 1.0001;
        for (uint32_t i = 0; i < NN; i++)
            cr::leaf_cull_fixed((const cr::LcFloat4 *)(lcull.data() + (size_t)cr::LC_REC * i), db, smax,
                                (cr::LcFloat4 *)(lcullf.data() + (size_t)cr::LC_REC * i));
    }
    std::vector<float4> lcullp((size_t)cr::LC_RECP * NN, make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint32_t i = 0; i < NN; i++)
        cr::leaf_cull_pack((const cr::LcFloat4 *)(lcullf.data() + (size_t)cr::LC_REC * i),
                           (nodes[i].y & 3u) == 3u ? nodes[i].y >> 2 : 0u,
                           (cr::LcFloat4 *)(lcullp.data() + (size_t)cr::LC_RECP * i));
    // ... and compressed on the scene's grid (48 B per node, LC 5)
    cr::LcGrid lcg = cr::lc_grid_make((const cr::LcFloat4 *)lcullf.data(), NN, lc_db);
    cr::lc_grid_dt(lcg, (const cr::LcFloat4 *)lcullf.data(), NN);
    std::vector<uint4> lcullc((size_t)cr::LC_RECC * NN, make_uint4(0u, 0u, 0u, 0u));
    for (uint32_t i = 0; i < NN; i++)
        cr::leaf_cull_compress((const cr::LcFloat4 *)(lcull.data() + (size_t)cr::LC_REC * i),
                               (const cr::LcFloat4 *)(lcullf.data() + (size_t)cr::LC_REC * i),
                               (nodes[i].y & 3u) == 3u ? nodes[i].y >> 2 : 0u, lcg,
                               (uint32_t *)(lcullc.data() + (size_t)cr::LC_RECC * i));
    std::vector<float4> tri((size_t)3 * nt), mn(nt), mkd(nt), mke(nt);
    std::vector<float2> muv((size_t)3 * nt);
    for (uint32_t t = 0; t < nt; t++) {
        const float *p = d->tri_pos + 9 * (size_t)t;
        for (int v = 0; v < 3; v++) tri[3 * (size_t)t + v] = make_float4(p[3 * v], p[3 * v + 1], p[3 * v + 2], 0.f);
        const uint32_t em = d->tri_emissive ? (d->tri_emissive[t] ? 1u : 0u)
                                            : ((d->tri_ke[3 * t] > 0.f || d->tri_ke[3 * t + 1] > 0.f ||
                                                d->tri_ke[3 * t + 2] > 0.f) ? 1u : 0u);
        float emf;
        std::memcpy(&emf, &em, 4);
        mn[t] = make_float4(d->tri_normal[3 * t], d->tri_normal[3 * t + 1], d->tri_normal[3 * t + 2], emf);
        int32_t ti = d->tri_tex ? d->tri_tex[t] : -1;
        if (ti >= (int32_t)d->n_textures) return fail(CR_E_INVALID, "texture index out of range");
        float tif;
        std::memcpy(&tif, &ti, 4);
        mkd[t] = make_float4(d->tri_kd[3 * t], d->tri_kd[3 * t + 1], d->tri_kd[3 * t + 2], tif);
        mke[t] = make_float4(d->tri_ke[3 * t], d->tri_ke[3 * t + 1], d->tri_ke[3 * t + 2], 0.f);
        for (int v = 0; v < 3; v++)
            muv[3 * (size_t)t + v] = make_float2(d->tri_uv[6 * t + 2 * v], d->tri_uv[6 * t + 2 * v + 1]);
    }
    std::vector<uint2> lights(d->n_lights);
    for (uint32_t i = 0; i < d->n_lights; i++) {
        if (d->light_id[i] >= nt) return fail(CR_E_INVALID, "light id out of range");
        uint32_t sb;
        std::memcpy(&sb, &d->light_surface[i], 4);
        lights[i] = make_uint2(d->light_id[i], sb);
    }
    std::vector<uint4> texs(d->n_textures);
    std::vector<uint8_t> texels;
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const cr_texture &t = d->textures[i];
        if (t.width <= 0 || t.height <= 0 || t.components <= 0 || !t.data)
            return fail(CR_E_INVALID, "bad texture");
        size_t off = (texels.size() + 15) & ~(size_t)15;
        size_t bytes = (size_t)t.width * t.height * t.components;
        texels.resize(off + bytes + cr::tex_pad(t.width, t.components), 0);
        std::memcpy(texels.data() + off, t.data, bytes);
        if (off > 0xffffffffull) return fail(CR_E_INVALID, "texture atlas > 4 GiB");
        texs[i] = make_uint4((uint32_t)t.width, (uint32_t)t.height, (uint32_t)t.components, (uint32_t)off);
    }
    // inner nodes grouped by depth, deepest level first (children have larger ids than
    // their parent in this numbering: one forward pass gives the depths)
    std::vector<uint32_t> depth(NN, 0), levels;
    std::vector<std::pair<uint32_t, uint32_t>> level_off;
    uint32_t tree_depth = 0; // deepest node (root = 0): the most entries a traversal stack holds
    {
        uint32_t maxd = 0;
        for (uint32_t i = 0; i < NN; i++) {
            tree_depth = std::max(tree_depth, depth[i]);
            if ((nodes[i].y & 3u) == 3u) continue;
            const uint32_t ch = nodes[i].y >> 2;
            if (ch <= i) return fail(CR_E_INVALID, "kd child numbered before its parent");
            depth[ch] = depth[ch + 1] = depth[i] + 1;
            maxd = std::max(maxd, depth[i]);
        }
        // the stacks (LDS rings, gstack, the packet trace's PACKET_DEPTH node stack) are sized
        // from the tree itself, never from the caller's declared max_depth
        if (tree_depth > 256) return fail(CR_E_DEPTH, "kd tree deeper than 256");
        std::vector<uint32_t> cnt(maxd + 1, 0);
        for (uint32_t i = 0; i < NN; i++)
            if ((nodes[i].y & 3u) != 3u) cnt[depth[i]]++;
        uint32_t off = 0;
        for (int dd = (int)maxd; dd >= 0; dd--) {
            level_off.emplace_back(off, cnt[dd]);
            off += cnt[dd];
        }
        levels.resize(off);
        std::vector<uint32_t> pos(maxd + 1);
        for (uint32_t dd = 0; dd <= maxd; dd++) pos[dd] = level_off[maxd - dd].first;
        for (uint32_t i = 0; i < NN; i++)
            if ((nodes[i].y & 3u) != 3u) levels[pos[depth[i]]++] = i;
    }
    out.S.lcg = lcg;
    out.S.nlights = d->n_lights;
    out.S.n_nodes = d->n_nodes;
    out.S.bmin = make_float3(d->box_min[0], d->box_min[1], d->box_min[2]);
    out.S.bmax = make_float3(d->box_max[0], d->box_max[1], d->box_max[2]);
    // every origin (a hit point + 0.001 n) and vertex lies in the padded box.  db <= 2^19: a split distance's
    // dividend split - o_a is at most 2 db <= 2^20, the domain of the fixed trace kernels' one-sided short
    // division (wfbuilds.hpp wf_short_division_scene, which the launchers check per render)
    out.S.db = (float)lc_db;
    out.tree_depth = tree_depth;
    out.stack_depth = std::max(tree_depth, std::max(d->max_depth, 1u));
    out.n_refs = d->n_refs;
    out.n_tris = d->n_tris;
    for (int a = 0; a < 3; a++) out.splits[a].clear();
    for (uint32_t i = 0; i < NN; i++)
        if (d->nodes[i].axis < 3) out.splits[d->nodes[i].axis].push_back(d->nodes[i].split);
    for (int a = 0; a < 3; a++) std::sort(out.splits[a].begin(), out.splits[a].end());
    // (the intermediate forms -- lcull, lcullf, depth, newid, order -- end here)
    out.levels = std::move(levels), out.level_off = std::move(level_off);
    out.nodes = std::move(nodes), out.fat = std::move(fat), out.recs = std::move(recs);
    out.lcullp = std::move(lcullp), out.lcullc = std::move(lcullc), out.tri = std::move(tri);
    out.mat_n = std::move(mn), out.mat_kd = std::move(mkd), out.mat_ke = std::move(mke), out.mat_uv = std::move(muv);
    out.lights = std::move(lights), out.texs = std::move(texs), out.texels = std::move(texels);
    return CR_OK;
}

} // namespace cr
