// traverse.hpp -- the resumable kd traversal of the wavefront trace kernels and the tail kernel
// (wavefront.hip): the loads (sload_*, load_*, leaf_mask), the stack's pop (trav_pop), one kd decision
// (kd_step), one triangle test (tri_one), the round that runs them (trav_round: descent, leaf references,
// one leaf tester, the round's end) and the leaf exchange of the LX builds (leaf_exchange).  What only counts
// or pads is behind Probe<C> (travprobe.hpp).  DESIGN.md §3.24 maps the round's stages to the C:: knobs and
// the builds, and says how a change here is held to the parent's code (scripts/kernel_regs.py --diff).
#pragma once
#include "leafcull.hpp"
#include "travprobe.hpp"
#include "wfbuilds.hpp"

namespace cr {

enum : uint32_t {
    ST_NEED_WORK = 0, // lane has no query: take the next item / ray
    ST_CLOSEST = 2,   // closest-hit query in flight
    ST_SHADOW = 3,    // NEE shadow query in flight
    ST_DONE = 4,      // no work left
    ST_HIT = 5,       // query results
    ST_MISS = 6,
    ST_OCCLUDED = 7,
    ST_VISIBLE = 8,
    ST_LEAFX = 9,     // LX builds: the lane's leaf tests wait for the wave's leaf exchange (leaf_exchange)
};

// Traversal registers of a query in flight.  r = per-axis rcp_for_div(d) for
// the exact short split-distance division (FD builds, device_math.hpp).
struct Trav {
    uint32_t node, sp, nl;
    float tmin, tmax;
    f3 r;
};

// A lane's stack-overflow entry at `depth` ([depth][gstride] rows): a 32-bit byte offset from the
// wave-uniform base, so the access uses scalar-base addressing and no 64-bit per-lane pointer is kept
// live (the compiler spilled one); cr_render checks that an area stays below 4 GiB.
__device__ __forceinline__ uint2 &gstack_at(uint2 *gstk, uint32_t depth, uint32_t gstride, uint32_t gid) {
    return *(uint2 *)((char *)gstk + (depth * gstride + gid) * 8u);
}

// Root-box clip (kdtree.cpp:196-208, 276-283); false: the query ends without a hit.
__device__ __forceinline__ bool trav_begin(const DevScene &S, f3 o, f3 d, bool shadow, float limit, Trav &T) {
    const f3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
    ray_box_inv(S, o, inv, T.tmin, T.tmax);
    if (T.tmax < 0 || T.tmax < T.tmin) return false;
    if (shadow) {
        if (T.tmin > limit) return false;
        T.tmax = std_min(T.tmax, limit);
    }
    const float nan = __builtin_nanf("");
    T.r = mk(fabsf(d.x) >= 0x1p-40f && fabsf(d.x) <= 0x1p40f ? inv.x : nan,
             fabsf(d.y) >= 0x1p-40f && fabsf(d.y) <= 0x1p40f ? inv.y : nan,
             fabsf(d.z) >= 0x1p-40f && fabsf(d.z) <= 0x1p40f ? inv.z : nan);
    T.node = T.sp = T.nl = 0;
    return true;
}

// Measured and dropped forms of the round (trav_round, below):
// (A wave-level mailbox -- per wave in LDS, the lanes for which a triangle was
// a geometric miss in their current query, so a uniform leaf skips it when all
// active lanes know it -- is exact too and measured 3% slower: the LDS lookup
// serialises behind every scalar record load.)
// (Speculative descent -- lanes that reached their leaf early descending toward
// the next one, Aila & Laine's postponed leaves -- is exact here too but
// measured slower: the merged descent loop costs more than the idle lanes.)
// Scalar-memory loads for wave-uniform addresses (SC builds): when every active
// lane wants the same node / leaf, one s_load serves the wave and the vector
// memory address path -- the measured bottleneck -- is not used at all.  The
// data is read-only for the whole launch, so the scalar cache is coherent.
// Every block that issues more than one load marks its outputs early-clobber
// ("=&s"): without it the register allocator may give a later load's base the
// registers an earlier load of the same block is filling, and a scalar load
// that returns before the next one issues then rewrites that base (the
// full-size-only illegal address of the grandchild-prefetch builds).
typedef unsigned int cr_v2u __attribute__((ext_vector_type(2)));
typedef float cr_v4f __attribute__((ext_vector_type(4)));
typedef float cr_v8f __attribute__((ext_vector_type(8)));
typedef unsigned int cr_v8u __attribute__((ext_vector_type(8)));
typedef unsigned int cr_v4u __attribute__((ext_vector_type(4)));
typedef float cr_v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ uint2 sload_node(const uint2 *p) {
    cr_v2u r;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p));
    return make_uint2(r.x, r.y);
}
__device__ __forceinline__ TriRec sload_rec(const float4 *p) {
    cr_v8f a;
    cr_v4f b;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b)
                 : "s"(p));
    return TriRec{make_float4(a[0], a[1], a[2], a[3]), make_float4(a[4], a[5], a[6], a[7]),
                  make_float4(b[0], b[1], b[2], b[3])};
}
// Four consecutive cull boxes (64 B; cull buffers carry three padding boxes).
__device__ __forceinline__ cr_v16f sload_box4(const float4 *p) {
    cr_v16f r;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p));
    return r;
}
__device__ __forceinline__ float4 sload_box(const float4 *p) {
    cr_v4f r;
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p));
    return make_float4(r[0], r[1], r[2], r[3]);
}
// A fat record and its subtree box (camera cull) under one scalar-load wait.
__device__ __forceinline__ void sload_fat_box(const uint4 *p, const float4 *q, uint4 &a, uint4 &b, float4 &box) {
    cr_v8u r;
    cr_v4f x;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(r), "=&s"(x)
                 : "s"(p), "s"(q));
    a = make_uint4(r[0], r[1], r[2], r[3]);
    b = make_uint4(r[4], r[5], r[6], r[7]);
    box = make_float4(x[0], x[1], x[2], x[3]);
}
// The same for node n with the byte offsets in SGPRs (s_load's soffset form): no 64-bit
// address arithmetic on the scalar unit, which bounds the packet trace.
__device__ __forceinline__ void sload_fat_box_n(const uint4 *fat, const float4 *boxes, uint32_t n, uint4 &a, uint4 &b,
                                                float4 &box) {
    cr_v8u r;
    cr_v4f x;
    asm volatile("s_load_dwordx8 %0, %2, %4\n\ts_load_dwordx4 %1, %3, %5\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(r), "=&s"(x)
                 : "s"(fat), "s"(boxes), "s"(n * 32u), "s"(n * 16u));
    a = make_uint4(r[0], r[1], r[2], r[3]);
    b = make_uint4(r[4], r[5], r[6], r[7]);
    box = make_float4(x[0], x[1], x[2], x[3]);
}
// A packed leaf cull record (LC_RECP float4, 96 B) under one scalar-load wait.
__device__ __forceinline__ void sload_lcullp(const float4 *p, LcFloat4 (&r)[LC_REC]) {
    cr_v16f a;
    cr_v8f b;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx8 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b)
                 : "s"(p));
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = LcFloat4{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]};
    r[4] = LcFloat4{b[0], b[1], b[2], b[3]};
    r[5] = LcFloat4{b[4], b[5], b[6], b[7]};
}
// A compressed leaf cull record (S.lcullc, 48 B: three 16-B loads, or one 48-B scalar load pair)
__device__ __forceinline__ void sload_lcullc(const uint4 *p, uint32_t (&w)[12]) {
    cr_v8u a;
    cr_v4u b;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b)
                 : "s"(p));
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = a[i];
#pragma unroll
    for (int i = 0; i < 4; i++) w[8 + i] = b[i];
}
// The references of the leaf at `node` that the lane's ray (o, d: unit, segment [0, tmax]) must test
// (leafcull.hpp); bits < count.  LC (the build's C::LC) 4: packed fixed-pad records (S.lcullp), 5: compressed
// (S.lcullc).
constexpr uint32_t lc_rec_bytes(int LC) { return 16u * (LC == 5 ? LC_RECC : LC_RECP); }
template <bool SC, int LC>
__device__ __forceinline__ uint32_t leaf_mask(const DevScene &S, uint32_t node, uint32_t count, f3 o, f3 d, float tmax) {
    if (LC == 5) {
        uint32_t w[12];
        if (SC && wave_uniform(node)) {
            sload_lcullc(S.lcullc + (size_t)LC_RECC * __builtin_amdgcn_readfirstlane(node), w);
        } else {
            const uint4 *p = (const uint4 *)((const char *)S.lcullc + node * (uint32_t)(16 * LC_RECC));
#pragma unroll
            for (int i = 0; i < LC_RECC; i++) {
                const uint4 v = p[i];
                w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
            }
        }
        const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
        const float inv[3] = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z)};
        return leaf_cull_mask_c(ov, dv, inv, lc_unit(d.x, d.y, d.z), tmax, w, count, S.lcg);
    }
    static_assert(LC == 4 || LC == 5, "leaf cull record forms: 4 (packed) or 5 (compressed)");
    LcFloat4 rec[LC_REC];
    constexpr int NR = LC_RECP;
    const float4 *recs = S.lcullp;
    if (SC && wave_uniform(node)) {
        sload_lcullp(recs + (size_t)NR * __builtin_amdgcn_readfirstlane(node), rec);
    } else {
        const float4 *p = (const float4 *)((const char *)recs + node * (uint32_t)(16 * NR));
#pragma unroll
        for (int i = 0; i < NR; i++) {
            const float4 v = p[i];
            rec[i] = LcFloat4{v.x, v.y, v.z, v.w};
        }
#ifdef CR_PAD_LC
        pad_loads<CR_PAD_LC, -1>(p);
#endif
    }
    const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
    // v_rcp_f32: within 1 ulp of 1/d (the check allows 2, tests/native/leafcull_check.cpp)
    const float inv[3] = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z)};
    return leaf_cull_mask_packed(ov, dv, inv, lc_unit(d.x, d.y, d.z), tmax, rec, count);
}

template <bool SC> __device__ __forceinline__ float4 load_box(const float4 *b, uint32_t i) {
    if (SC && wave_uniform(i)) return sload_box(b + __builtin_amdgcn_readfirstlane(i));
    return b[i];
}
template <bool SC> __device__ __forceinline__ uint2 load_node(const DevScene &S, uint32_t node) {
    if (SC && wave_uniform(node)) return sload_node(S.nodes + __builtin_amdgcn_readfirstlane(node));
    return S.nodes[node];
}

// Fat node records (DevScene::fat): 32 B per node, {self, child 0, child 1}, so
// one dependent load serves two descent levels.
__device__ __forceinline__ void sload_fat(const uint4 *p, uint4 &a, uint4 &b) {
    cr_v8u r;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p));
    a = make_uint4(r[0], r[1], r[2], r[3]);
    b = make_uint4(r[4], r[5], r[6], r[7]);
}
template <bool SC> __device__ __forceinline__ void load_fat(const DevScene &S, uint32_t node, uint4 &a, uint4 &b) {
    if (SC && wave_uniform(node)) return sload_fat(S.fat + 2u * __builtin_amdgcn_readfirstlane(node), a, b);
    const uint4 *p = (const uint4 *)((const char *)S.fat + node * 32u);
    a = p[0];
    b = p[1];
#ifdef CR_PAD_FETCH
    pad_loads<CR_PAD_FETCH, 1>(p);
#endif
}

// The leaf loop is software-pipelined (triangle j+1's loads issued before j is
// tested).  Measured and dropped: the same unrolled by two with unconditional
// loads (no register rotation copies, but count-1 leaves fetch a second record:
// -2.3%), and compiler-scheduled, pipelined scalar loads for uniform leaves
// (address_space(4): -2.5% against the asm s_load + wait below).  The other measured
// and dropped knobs (DESIGN.md keeps their numbers): the top of the tree in LDS, a
// uniform leaf's records two per wait, per-reference plane records, two-level 16-B node
// records, the per-ray, fixed-pad and short leaf cull record forms, the phase clock.
// BF: the decisions as selects instead of divergent branches (the trace kernels
// are bound by the scalar unit's exec-mask bookkeeping, SURVEY §8d / DESIGN §3.3):
// a descent step branches only around its stack push, and a uniform leaf's
// triangle tests keep their result by select (tri_test_wave).
// CULL (camera rays; BF + SC): a triangle test runs only when the lane's sample
// position (csx, csy) lies in the reference's cull box (camcull.hpp) -- outside it the
// test cannot accept, so skipping it changes nothing.  A uniform leaf reads four boxes
// per scalar load and tests a triangle only if some lane is inside its box; a divergent
// lane reads its box (16 B) and, inside, the record (48 B).
// LC (secondary closest / shadow rays, unit directions; BF + SC): a leaf's tests run only
// for the references its cull record (leafcull.hpp) cannot exclude for this ray and segment.
// (a trace build's configuration type C -- TraceDefaults and the builds deriving from it: wfbuilds.hpp)

// A lane's deferred leaf (LX builds): the references of the leaf whose first record is `first` that its
// cull mask keeps (bit j: first + j).
struct LeafX {
    uint32_t mask, first;
};

// The stack's top entry becomes the query's node and interval (stack invariant).
// ring: the LDS ring [slot][blockDim.x]; gstk / gid: the stack-overflow area and the lane's global index.
template <int R>
__device__ __forceinline__ void trav_pop(uint2 *ring, uint2 *gstk, uint32_t gstride, uint32_t gid, Trav &T,
                                         Pc *pc = nullptr) {
    T.sp--;
    uint2 e;
    if (T.nl) {
        e = ring[(T.sp & (R - 1)) * blockDim.x + threadIdx.x];
        T.nl--;
    } else {
        e = gstack_at(gstk, T.sp, gstride, gid);
        pc_load(pc, false, 8);
    }
    T.node = e.x;
    T.tmin = T.tmax; // == the popped entry's split distance (stack invariant)
    T.tmax = __uint_as_float(e.y);
}

// One kd decision at inner node nd (kdtree.cpp:258-275): T.node = the child to descend into (child + k,
// k returned), the far child pushed when both are crossed, the ring's oldest entry spilled when it is full.
// Reads C::FD (the split division; with C::FIX its one-sided form) and C::BF (the decision as selects, a
// branch only around the push).  The instruction stream of one decision, and why `below`, the child's index
// and the pushed child are written as they are: DESIGN.md §3.26.
// (o, d by reference and bdim = blockDim.x, tid = threadIdx.x read once by trav_round, as its lambdas hold
// them: by value, or read here, kernels came out changed -- DESIGN.md §3.24.)
template <class C>
__device__ __forceinline__ uint32_t kd_step(uint2 nd, uint2 *ring, uint32_t bdim, uint32_t tid, uint2 *gstk, uint32_t gstride,
                                            uint32_t gid, const f3 &o, const f3 &d, Trav &T, const Probe<C> &P) {
    constexpr int R = C::R;
    P.step(T.node, nd.x);
    const uint32_t a = nd.y & 3u;
    const float split = __uint_as_float(nd.x);
    const float oa = comp(o, a), da = comp(d, a);
    // (FIX: the launchers take such a kernel only for a scene inside wf_short_division_scene's bound)
    const float tsplit = !C::FD    ? split_distance(split, oa, da)
                         : C::FIX ? div_by_rcp_wave_bounded(split - oa, da, comp(T.r, a))
                                  : div_by_rcp_wave(split - oa, da, comp(T.r, a));
    const bool below = kd_below(split - oa, da);
    const uint32_t child = nd.y >> 2;
    uint32_t k;
    // the branching form keeps `below` as 0 / 1 in a register (the empty asm pins it there): as a lane mask it
    // would be merged over the three branches by exec arithmetic on the scalar unit, ~7 instructions a step
    uint32_t bw = below;
    if (!C::BF) asm("" : "+v"(bw));
    if (C::BF) { // (bitwise logic on the lane masks: no short-circuit exec branches)
        const bool near_only = (tsplit >= T.tmax) | (tsplit < 0);
        const bool far_only = !near_only & (tsplit <= T.tmin);
        const bool push = !near_only & !far_only;
        // far_only ? below : 1 - below, on the lane masks; the child's index here, in the block of the
        // compares, where the lane mask is the add's carry-in (past the push it is a select and an add)
        k = below ^ (near_only | !(tsplit <= T.tmin));
        T.node = child + k;
        if (push) {
            const uint32_t slot = (T.sp & (R - 1)) * bdim + tid;
            if (T.nl == R) P.load(false, 8);
            if (T.nl == R) gstack_at(gstk, T.sp - R, gstride, gid) = ring[slot]; // spill the oldest
            ring[slot] = make_uint2(2u * child + 1u - T.node, __float_as_uint(T.tmax)); // the other child
            T.sp++;
        }
        T.nl = push && T.nl < R ? T.nl + 1 : T.nl;
        T.tmax = push ? tsplit : T.tmax;
    } else if (tsplit >= T.tmax || tsplit < 0) {
        k = 1u - bw;
    } else if (tsplit <= T.tmin) {
        k = bw;
    } else {
        const uint2 e = make_uint2(child + bw, __float_as_uint(T.tmax));
        const uint32_t slot = (T.sp & (R - 1)) * bdim + tid;
        if (T.nl == R) gstack_at(gstk, T.sp - R, gstride, gid) = ring[slot]; // spill the oldest
        else T.nl++;
        ring[slot] = e;
        T.sp++;
        T.tmax = tsplit;
        k = 1u - bw;
    }
    if (!C::BF) T.node = child + k;
    return k;
}

// One triangle of the lane's leaf (kdtree.cpp:235-246 / 309-320); false: stop the leaf.  An accepted hit
// goes to found / tri / bx / by and T.tmax, an occluder (shadow) to occluded.  (Everything by reference, the
// scalars shadow and exclude too, as trav_round's lambda held them: by value the default kernels change.)
template <class C>
__device__ __forceinline__ bool tri_one(const f3 &o, const f3 &d, const bool &shadow, const uint32_t &exclude, const TriRec &r,
                                        Trav &T, bool &found, bool &occluded, uint32_t &tri, float &bx, float &by,
                                        const Probe<C> &P) {
    const uint32_t id = rec_id(r);
    if (shadow && id == exclude) return true;
    P.test(true);
    P.miss_census(o, d, r, id);
    float ux, uy, t;
    // BF: the lanes that failed an early test compute on (wave-uniform exits, no exec bookkeeping)
    if (C::BF ? tri_test_wave(o, d, r, T.tmax, ux, uy, t) : tri_test(o, d, r, T.tmax, ux, uy, t)) {
        if (shadow) {
            occluded = true;
            return false;
        }
        bx = ux;
        by = uy;
        T.tmax = t;
        tri = id;
        found = true;
    }
    return true;
}

// One traversal round (kdtree.cpp:250-330 as an explicit stack): descend to the next leaf, test it, pop.
// Returns the lane's new state: unchanged while the query continues, else its result (a closest hit leaves
// {bx, by, tri} in d: the direction is dead by then), or ST_LEAFX with the leaf's masked references in *lx
// (LX builds: wf_trace runs leaf_exchange with the whole wave and ends the round itself).
//   Stack: entries {far node, tmax at push}; the top R live in the LDS ring [slot][blockDim.x] (ring),
//   deeper ones spill to gstk [depth][gstride].  On pop the interval is [current tmax, entry.tmax]: the
//   current tmax equals the push-time tsplit (stack invariant).
// The body's stages in order -- the descent (kd_step per decision; C::FAT: two levels per fetch), the
// leaf's references (camera cull box, leaf cull mask), one leaf tester by the build and the leaf, the
// round's end -- with the C:: knobs each reads and the builds that reach it: DESIGN.md §3.24, which also
// records why the descent loop and the testers stay blocks of this function (csx, csy, cull, cull_node:
// camera cull only; lx: LX only; c, dg, pc: the probe's).
template <class C>
__device__ __forceinline__ uint32_t trav_round(int lc_debug, uint32_t lc_min, const DevScene &S, uint2 *ring, uint2 *gstk, uint32_t gstride,
                                               uint32_t gid, f3 o, f3 &d, bool shadow, uint32_t exclude, Trav &T,
                                               Ctr &c, float csx = 0.f, float csy = 0.f, const float4 *cull = nullptr,
                                               const float4 *cull_node = nullptr, Diag *dg = nullptr,
                                               Pc *pc = nullptr, uint32_t quorum = 0, LeafX *lx = nullptr) {
    static constexpr int R = C::R, CULL = C::CULL, LC = C::LC;
    static constexpr bool FULL = C::FULL, SC = C::SC, FAT = C::FAT, BF = C::BF;
    // quorum (lean FAT builds without the camera cull): the wave's descent stops at a fetch once at most
    // quorum / 64 of the lanes that entered the round still descend; those keep T.node (the node to fetch)
    // and their interval and go on next round -- the same node visits with the same intervals, so the
    // same answers -- while the others test their leaves now instead of idling
    const uint32_t nbusy = quorum ? (uint32_t)__popcll(__ballot(1)) : 0u;
    constexpr uint32_t PENDING_LEAF = 0xfffffffeu;
    bool pending = false;
    const Probe<C> P = {c, dg, pc};
    P.round();
    auto lrec = [&](uint32_t i) -> TriRec {
        P.load(false, 16u * REC_STRIDE);
        return load_rec(S, i);
    };
    auto srec = [&](const float4 *q) -> TriRec {
        P.load(true, 16u * REC_STRIDE);
        return sload_rec(q);
    };
    static_assert(CULL == 0 || CULL == 2, "camera cull: none, or references, leaves and subtrees");
    static_assert(!CULL || (FAT && BF && SC && !FULL), "cull: lean fat-record BF + SC builds");
    static_assert(!LC || ((LC == 4 || LC == 5) && !CULL && BF && SC && !FULL), "leaf cull: lean BF + SC builds, forms 4 / 5");
    static_assert(!C::LX || LC, "leaf exchange: leaf-cull builds");
    // (read once, here, and handed to kd_step: reading them at the push, or not at all, moves the registers
    // of 44 kernels -- DESIGN.md §3.24)
    const uint32_t bdim = blockDim.x, tid = threadIdx.x;
    auto step = [&](uint2 nd) -> uint32_t { return kd_step<C>(nd, ring, bdim, tid, gstk, gstride, gid, o, d, T, P); };
    uint2 nd;
    // CULL: a fetched node whose subtree box excludes the sample is treated as an
    // empty leaf -- none of its triangles can accept, so the traversal would leave it
    // without a hit and with tmax = its interval's end, which is exactly this state
    bool culled = false;
    uint32_t first, count, lmask;
    bool lin;
    auto pop_entry = [&]() { trav_pop<R>(ring, gstk, gstride, gid, T, pc); };
    if (FAT) { // two levels per dependent load: a node's record carries its children's
        uint4 f0, f1;
        auto fetch = [&](uint32_t node) {
            if (CULL) { // the record and the subtree box, loads issued together
                float4 b;
                P.load(SC && wave_uniform(node), 48);
                if (SC && wave_uniform(node)) {
                    const uint32_t un = __builtin_amdgcn_readfirstlane(node);
                    sload_fat_box(S.fat + 2u * un, cull_node + un, f0, f1, b);
                } else {
                    const uint4 *p = (const uint4 *)((const char *)S.fat + node * 32u);
                    f0 = p[0];
                    f1 = p[1];
                    b = cull_node[node];
                }
                nd = make_uint2(f0.x, f0.y);
                if (!(csx >= b.x && csx <= b.y && csy >= b.z && csy <= b.w)) {
                    culled = true;
                    nd = make_uint2(0xffffffffu, 3u); // an empty leaf no real leaf shares `first` with
                }
            } else {
                P.load(SC && wave_uniform(node), 32);
                load_fat<SC>(S, node, f0, f1);
                nd = make_uint2(f0.x, f0.y);
            }
        };
        fetch(T.node);
        // one exit: a lane whose level-1 node is a leaf skips the second step and leaves at the loop test
        // (a second exit would double the exec-mask bookkeeping of this divergent loop on the scalar
        // unit); the quorum leaves the same way
        while ((nd.y & 3u) != 3u) {
            const uint32_t k = step(nd);
            nd = k ? make_uint2(f1.x, f1.y) : make_uint2(f0.z, f0.w);
            if ((nd.y & 3u) != 3u) {
                step(nd);
                if (!FULL && !CULL && quorum && (uint32_t)__popcll(__ballot(1)) * 64u <= nbusy * quorum)
                    nd = make_uint2(PENDING_LEAF, 3u); // (an empty "leaf" no real leaf shares `first` with)
                else
                    fetch(T.node);
            }
        }
        pending = !FULL && !CULL && quorum && nd.x == PENDING_LEAF;
    } else {
        P.load(SC && wave_uniform(T.node), 8);
        nd = load_node<SC>(S, T.node);
        while ((nd.y & 3u) != 3u) {
            step(nd);
            P.load(SC && wave_uniform(T.node), 8);
            nd = load_node<SC>(S, T.node);
        }
    }
    if (pending) return shadow ? ST_SHADOW : ST_CLOSEST; // descends on next round from T.node
    P.leaf();
    first = nd.x;
    count = nd.y >> 2;
    lin = !culled; // CULL: the sample lies in the leaf's box (the union of its references')
    if (CULL && !culled) {
        P.load(SC && wave_uniform(T.node), 16);
        const float4 lb = load_box<SC>(cull_node, T.node);
        lin = csx >= lb.x && csx <= lb.y && csy >= lb.z && csy <= lb.w;
    }
    // LC: the references to test (bit j: first + j); count > LC_MAXREFS: every one (lmask unused)
    lmask = 0u;
    if constexpr (LC != 0) { // (leaf_mask has no form for LC 0)
        if (count && count <= (uint32_t)LC_MAXREFS) {
            // leaves below lc_min: every reference, no check
            const uint32_t lcid = T.node;
            if (count >= lc_min) P.mask(SC && wave_uniform(lcid), lc_rec_bytes(LC));
            lmask = count >= lc_min ? leaf_mask<SC, LC>(S, lcid, count, o, d, T.tmax)
                                    : (count >= 32 ? 0xffffffffu : (1u << count) - 1u);
            if (lc_debug) lmask = lc_debug == 1 ? (count >= 32 ? 0xffffffffu : (1u << count) - 1u) : 0u;
        }
    }
    bool found = false, occluded = false;
    uint32_t tri = 0;
    float bx = 0.f, by = 0.f;
    auto test = [&](const TriRec &r) -> bool {
        return tri_one<C>(o, d, shadow, exclude, r, T, found, occluded, tri, bx, by, P);
    };
    P.leaf_census(first, count);
    if (BF && SC && wave_uniform(first)) { // uniform leaf, results by select
        const uint32_t uf = __builtin_amdgcn_readfirstlane(first), uc = __builtin_amdgcn_readfirstlane(count);
        const float4 *base = S.recs + (size_t)REC_STRIDE * uf;
        // one triangle of the uniform leaf; false: every active lane occluded (stop)
        // in: the lane tests this triangle (LC: the bit of its own mask)
        auto utest = [&](const TriRec &r, uint32_t j, bool in = true) -> bool {
            P.tri_lines(uf + j);
            const uint32_t id = rec_id(r);
            const bool live = in & !(shadow & (occluded | (id == exclude)));
            P.test(live);
            float ux, uy, t;
            const bool acc = live & tri_test_wave(o, d, r, T.tmax, ux, uy, t);
            if (shadow) {
                occluded = occluded | acc;
                return __ballot(!occluded) != 0;
            }
            bx = acc ? ux : bx;
            by = acc ? uy : by;
            T.tmax = acc ? t : T.tmax;
            tri = acc ? id : tri;
            found = found | acc;
            return true;
        };
        if (CULL) {
            const float4 *cb = cull + uf;
            for (uint32_t j = 0; j < uc && __ballot(lin); j += 4) {
                P.load(true, 64);
                const cr_v16f bx = sload_box4(cb + j);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    if (j + k >= uc) break;
                    const bool in = csx >= bx[4 * k] && csx <= bx[4 * k + 1] && csy >= bx[4 * k + 2] &&
                                    csy <= bx[4 * k + 3];
                    if (__ballot(in)) utest(srec(base + (size_t)REC_STRIDE * (j + k)), j + k);
                }
            }
        } else if (LC && uc <= (uint32_t)LC_MAXREFS) {
            // a triangle runs when some lane's mask holds it (a lane tests only its own
            // references: utest's `in`); per-bit ballots, since a butterfly over the wave
            // would not see the bits of lanes whose partners are inactive
            for (uint32_t j = 0; j < uc; j++) {
                const bool in = (lmask >> j) & 1u;
                if (!__ballot(in)) continue;
                if (!utest(srec(base + (size_t)REC_STRIDE * j), j, in)) break;
            }
        } else {
            for (uint32_t j = 0; j < uc; j++)
                if (!utest(srec(base + (size_t)REC_STRIDE * j), j)) break;
        }
    } else if (SC && wave_uniform(first)) { // every lane at the same leaf: scalar loads
        const float4 *base = S.recs + (size_t)REC_STRIDE * __builtin_amdgcn_readfirstlane(first);
        for (uint32_t j = 0; j < count; j++) {
            P.tri_lines(first + j);
            if (!test(srec(base + (size_t)REC_STRIDE * j))) break;
        }
    } else if (C::LX && LC && count <= (uint32_t)LC_MAXREFS) { // tests deferred to the wave's leaf exchange
        if (lmask) {
            lx->mask = lmask;
            lx->first = first;
            return ST_LEAFX;
        }
    } else if (LC && count <= (uint32_t)LC_MAXREFS) { // the mask's references, pipelined one ahead
        uint32_t m = lmask;
        P.dloop(m);
        TriRec nx;
        if (m) nx = lrec(first + (uint32_t)__builtin_ctz(m));
        while (m) {
            m &= m - 1u;
            const TriRec r = nx;
            if (m) nx = lrec(first + (uint32_t)__builtin_ctz(m));
            if (!test(r)) break;
        }
    } else if (CULL) { // boxes pipelined one ahead; a record only for a sample inside its box
        if (!lin) count = 0;
        float4 nb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (count) nb = cull[first];
        if (count) P.load(false, 16);
        for (uint32_t j = 0; j < count; j++) {
            const float4 b = nb;
            if (j + 1 < count) nb = cull[first + j + 1];
            if (j + 1 < count) P.load(false, 16);
            if (csx >= b.x && csx <= b.y && csy >= b.z && csy <= b.w)
                if (!test(lrec(first + j))) break;
        }
    } else {
        TriRec nx;
        if (count) nx = lrec(first);
        for (uint32_t j = 0; j < count; j++) { // software pipeline: triangle j+1's loads before j's test
            P.tri_lines(first + j);
            const TriRec r = nx;
            if (j + 1 < count) nx = lrec(first + j + 1);
            if (!test(r)) break;
        }
    }
    if (occluded) return ST_OCCLUDED;
    if (found) {
        d = mk(bx, by, __uint_as_float(tri));
        return ST_HIT;
    }
    if (T.sp == 0) return shadow ? ST_VISIBLE : ST_MISS;
    pop_entry();
    return shadow ? ST_SHADOW : ST_CLOSEST;
}

// ------------------------------------------------------------ leaf exchange --
// LX builds.  In a divergent leaf round the leaf cull leaves tests in ~16 of a wave's lanes, ~5 each, and
// the per-lane loop runs as long as the longest mask: 6 iterations at 0.2 of the lanes.
// Here the whole wave (every lane, busy or idle) tests the round's (lane, reference) pairs 64 at a time:
// pair i belongs to the lane whose exclusive prefix of mask popcounts is the largest one <= i, and is that
// lane's (i - prefix)-th mask bit.  The answers are the per-lane loop's:
//   shadow: occluded == some masked reference other than the excluded one accepts (0 <= t < tmax) -- an OR,
//           whatever the order (kdtree.cpp:309-320);
//   closest: the loop keeps a hit when t < the current tmax, so it ends with the smallest t over the
//           accepting references and, among equal t (+0 == -0), the first in mask order
//           (kdtree.cpp:235-246); the pairs are reduced in ascending (window, lane) = mask order with a
//           strict <, which selects the same reference, and its own ux, uy, t are taken.
// Every lane of the wave must be active.  lx: 192 words of LDS owned by the wave (the window's start marks,
// every lane's mask and first record).

// the position of the q-th (from 0) set bit of m (q < popcount(m))
__device__ __forceinline__ uint32_t nth_bit(uint32_t m, uint32_t q) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t w = 16; w >= 1; w >>= 1) {
        const uint32_t c = (uint32_t)__builtin_popcount(m & ((1u << w) - 1u));
        const bool up = q >= c;
        q = up ? q - c : q;
        m = up ? m >> w : m;
        pos = up ? pos + w : pos;
    }
    return pos;
}
__device__ __forceinline__ uint32_t bperm(uint32_t addr, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr, (int)v);
}
__device__ __forceinline__ float bpermf(uint32_t addr, float v) { return __uint_as_float(bperm(addr, __float_as_uint(v))); }

typedef __attribute__((address_space(3))) uint32_t lds_u32;
// Inclusive prefix sum of x over the 64 lanes of a converged wave: row scans by DPP row shifts (out-of-row
// sources read 0), then rows 1 / 3 add lane 15 of the row below and rows 2 / 3 add lane 31.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true); // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true); // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true); // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true); // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false); // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false); // row_bcast:31
    return x;
}

// DPP: the prefix by wave_incl_scan instead of the six bit-sliced ballots
template <bool SHADOW, bool DPP = false>
__device__ __forceinline__ void leaf_exchange(const DevScene &S, volatile lds_u32 *lx, uint32_t m, uint32_t first,
                                              f3 o, f3 d, float tmax, uint32_t exclude, bool &occluded, bool &found,
                                              float &bx, float &by, float &bt, uint32_t &tri, Pc *pc = nullptr) {
    const uint32_t lane = lane_id();
    const uint32_t c = (uint32_t)__builtin_popcount(m);
    if (pc) { // the exchange's shape: rounds, windows (diters), owner lanes and their pairs
        const uint32_t owners = (uint32_t)__popcll(__ballot(c > 0u));
        if (wave_leader()) {
            pc->drounds++;
            pc->dlanes += owners;
        }
        pc->dtests += c;
    }
    // exclusive prefix P of c over the lanes and the total, bit-sliced (c <= 32)
    uint32_t P = 0, total = 0;
    if (DPP) {
        const uint32_t inc = wave_incl_scan(c);
        P = inc - c;
        total = __builtin_amdgcn_readlane(inc, 63);
    } else {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const uint64_t bal = __ballot((c >> b) & 1u);
            P += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u)) << b;
            total += (uint32_t)__popcll(bal) << b;
        }
    }
    // this lane's pairs: [P, E) (packed: one register through the exchange)
    const uint32_t pe = P | ((P + c) << 16);
    occluded = found = false;
    // lx: [0, 64) the window's start marks, [64, 128) every lane's mask, [128, 192) its leaf's first record
    // (read from LDS by the pairs' testers, so they hold no registers during the exchange)
    volatile lds_u32 *const marks = lx;
    lx[64 + lane] = m;
    lx[128 + lane] = first;
    uint32_t carry = 0, carry_q = 0; // the owner of the pair before the window, and its rank + 1
    for (uint32_t base = 0; base < total; base += 64u) {
        // the owner of pair base + lane: the last lane that starts at or before it
        const uint32_t ln = lane_id(); // (re-derived per window: values hoisted out of this loop hold registers)
        marks[ln] = 0u;
        const uint32_t P0 = pe & 0xffffu, E0 = pe >> 16;
        if (E0 > P0 && P0 >= base && P0 < base + 64u) marks[P0 - base] = ln + 1u;
        const uint32_t mv = marks[ln];
        // the last start at or before this lane: s = ln - (its distance below), none when the shifted mask is 0
        const uint64_t upto = __ballot(mv != 0u) << (63u - ln);
        const uint32_t back = upto ? (uint32_t)__builtin_clzll(upto) : 0u;
        const uint32_t sm = bperm((ln - back) << 2, mv);
        const uint32_t owner = upto ? sm - 1u : carry;
        // q: the pair's rank among its owner's (a carried owner started before the window)
        const uint32_t q = upto ? back : ln + carry_q;
        carry = __builtin_amdgcn_readlane(owner, 63);
        carry_q = __builtin_amdgcn_readlane(q, 63) + 1u;
        const bool live = base + ln < total;
        const uint32_t a = owner << 2;
        const uint32_t om = lx[64 + owner], of = lx[128 + owner];
        const uint32_t j = nth_bit(om, q);                    // (any value < 32 for a dead lane)
        const uint32_t ref = live ? of + j : 0u;              // (record 0: a dead lane's harmless load)
        const TriRec r = load_rec(S, ref);
        if (pc) {
            if (wave_leader()) pc->diters++;
            pc->tests += live ? 1u : 0u;
            pc->vb += live ? 16u * REC_STRIDE : 0u;
        }
        // tri_test_wave's arithmetic with the owner's ray fetched in stages (the direction, then the origin,
        // then tmax), each where it is first used: the scheduler keeps them apart (fewer live registers)
        float ux, uy, t;
        bool acc;
        {
            const f3 od = mk(bpermf(a, d.x), bpermf(a, d.y), bpermf(a, d.z));
            const f3 v0 = ld3(r.a), e1 = ld3(r.b), e2 = ld3(r.c);
            const f3 p = cross(od, e2);
            const float aa = dot(e1, p);
            bool ok = live & !((aa < 1.19209290e-7F) & (aa > -1.19209290e-7F));
            acc = false;
            if (__ballot(ok)) {
                __builtin_amdgcn_sched_barrier(0);
                const f3 oo = mk(bpermf(a, o.x), bpermf(a, o.y), bpermf(a, o.z));
                const float f = rcp_rn_wave(aa);
                const f3 sv = sub(oo, v0);
                ux = f * dot(sv, p);
                ok = ok & !((ux < 0.f) | (ux > 1.f));
                if (__ballot(ok)) {
                    const f3 qv = cross(sv, e1);
                    uy = f * dot(od, qv);
                    ok = ok & !((uy < 0.f) | (uy + ux > 1.f));
                    if (__ballot(ok)) {
                        __builtin_amdgcn_sched_barrier(0);
                        const float ot = bpermf(a, tmax);
                        t = f * dot(e2, qv);
                        acc = ok & (t >= 0.f) & (t < ot);
                    }
                }
            }
        }
        if (SHADOW) {
            acc = acc & (rec_id(r) != bperm(a, exclude));
            const uint64_t h = __ballot(acc);
            // this lane's pairs in the window: [lo, hi)
            const uint32_t P1 = pe & 0xffffu, E1 = pe >> 16;
            const int lo = (int)P1 - (int)base, hi = (int)E1 - (int)base;
            const int l = lo < 0 ? 0 : lo, e = hi > 64 ? 64 : hi;
            if (h && l < e) {
                const uint64_t bits = h >> l;
                occluded = occluded | ((e - l == 64 ? bits : bits & ((1ull << (e - l)) - 1ull)) != 0ull);
            }
            // every lane with pairs past the window is occluded already: done
            if (!__ballot(E1 > P1 && !occluded && E1 > base + 64u)) break;
        } else {
            uint64_t h = __ballot(acc);
            while (h) { // ascending lanes = ascending mask order within each owner
                const uint32_t w = (uint32_t)__builtin_ctzll(h);
                h &= h - 1ull;
                const uint32_t ow = __builtin_amdgcn_readlane(owner, w);
                const float tw = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(t), w));
                const float uxw = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ux), w));
                const float uyw = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(uy), w));
                const uint32_t idw = __builtin_amdgcn_readlane(rec_id(r), w);
                const bool take = lane_id() == ow && (!found || (__float_as_uint(tw) & 0x7fffffffu) <
                                                               (__float_as_uint(bt) & 0x7fffffffu));
                found = found | take;
                bt = take ? tw : bt;
                bx = take ? uxw : bx;
                by = take ? uyw : by;
                tri = take ? idw : tri;
            }
        }
    }
}

// Per-query tallies are wave-aggregated LDS atomics: the callers run in
// divergent code, so a wave total cannot be kept wave-uniform in registers.
enum : int { T_CLOSEST = 0, T_SHADOW = 1, T_HIT = 5, T_TEXHIT = 6, T_PATHS = 7, T_PIXELS = 8, T_NEE = 9, T_N = 10 };
// the device counter slot of tally i (T_NEE: CTR_NEE, past the cr_counters fields of the Ctr order)
__device__ __forceinline__ int tally_slot(int i) { return i == T_NEE ? CTR_NEE : i; }
__device__ __forceinline__ void tally(unsigned long long *tl, int i, bool pred) {
    const uint64_t b = __ballot(pred);
    if (b && wave_leader()) atomicAdd(&tl[i], (unsigned long long)__popcll(b));
}

__device__ __forceinline__ float4 pk(f3 v, uint32_t w) { return make_float4(v.x, v.y, v.z, __uint_as_float(w)); }

// Wave-aggregated append: one atomicAdd per wave, slots in lane order.
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool pred) {
    const uint64_t m = __ballot(pred);
    if (!m) return 0;
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader, 64);
    return base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

} // namespace cr
