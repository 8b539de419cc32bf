// travprobe.hpp -- everything the traversal (traverse.hpp) only counts or pads: the counting build's work
// counters (C::FULL, Ctr), its two censuses (Diag), the performed-work counters (Pc, C::PC builds) and the
// calibration pads (CR_PAD_*).  The traversal calls Probe<C> in one line per site; every method starts with
// `if (C::FULL)` or `if (pc)`, so a lean build compiles each to nothing.  (Ctr itself: render_common.hpp,
// shared with the megakernel.)  DESIGN.md §3.24 lists the methods against the counter slots.
#pragma once
#include "render_common.hpp"

namespace cr {

// True when every active lane holds the same x.
__device__ __forceinline__ bool wave_uniform(uint32_t x) {
    return __ballot(x == (uint32_t)__builtin_amdgcn_readfirstlane(x)) == __ballot(1);
}

// Distinct values of key over the active lanes (FULL-build diagnostics).
__device__ __forceinline__ uint32_t wave_distinct(uint32_t key) {
    uint64_t m = __ballot(1);
    uint32_t n = 0;
    while (m) {
        const uint32_t k = (uint32_t)__shfl((int)key, __ffsll((long long)m) - 1, 64);
        m &= ~__ballot(key == k);
        n++;
    }
    return n;
}

// Counting-build diagnostics of one lane (DIAG_* in kernels.hpp): the lane's last 8
// triangles that missed for any segment in its current query (a per-lane mailbox, as a
// census: no test is skipped), and its tallies (wave-level ones kept by the leader).
struct Diag {
    bool on;        // the trace kind is in RenderArgs::diag_kinds
    uint32_t n;     // misses recorded in this query (reset at each query start)
    uint32_t mb[8]; // mb[i & 7]: the i-th
    uint32_t v[DIAG_N];
};
__device__ __forceinline__ void diag_begin(Diag *dg) {
    if (dg) dg->n = 0;
}
__device__ __forceinline__ void diag_flush(unsigned long long *ctrs, const Diag &dg) {
    const uint32_t ln = lane_id();
#pragma unroll
    for (int i = 0; i < DIAG_N; i++) {
        unsigned long long s = dg.v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (ln == 0 && s) atomicAdd(&ctrs[CTR_DIAG + i], s);
    }
}

// Performed work of one lane (perf builds, PERF_* in kernels.hpp): what the kernel executes and
// the bytes its loads and stores move -- vector accesses per lane, scalar loads once per wave
// (counted by the wave's leader).
struct Pc {
    uint32_t q, steps, leaves, masks, tests, waves;
    uint64_t vb, sb;
    uint32_t drounds, diters, dlanes, dtests;
};
__device__ __forceinline__ void pc_load(Pc *pc, bool scalar, uint32_t bytes) {
    if (!pc) return;
    if (!scalar) pc->vb += bytes;
    else if (wave_leader()) pc->sb += bytes;
}
// Call with the whole wave converged: the lane sums go to ctrs[0 .. PERF_N).
__device__ __forceinline__ void pc_flush(unsigned long long *ctrs, const Pc &pc) {
    const uint32_t ln = lane_id();
    const unsigned long long v[PERF_N] = {pc.q,     pc.steps,   pc.leaves, pc.masks,  pc.tests,  pc.vb,
                                          pc.sb,    pc.waves,   pc.drounds, pc.diters, pc.dlanes, pc.dtests};
#pragma unroll
    for (int i = 0; i < PERF_N; i++) {
        unsigned long long x = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        if (ln == 0 && x) atomicAdd(&ctrs[i], x);
    }
}

// Address-path calibration only (CR_PAD_FETCH / CR_PAD_LC): N extra 16-B loads of the lines of the record at
// p, record word i & WRAP (a fat record has two such words, a leaf cull record at least N).
template <int N, int WRAP> __device__ __forceinline__ void pad_loads(const void *p) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u4 g_u4;
    g_u4 *q = (g_u4 *)p;
    asm volatile("" : "+v"(q));
#pragma unroll
    for (int i = 0; i < N; i++) {
        const u4 v = q[i & WRAP];
        asm volatile("" ::"v"(v));
    }
}

// The probe of one lane's rounds.  c: the counting build's counters; dg: its censuses (wf_trace's FULL
// builds, else null); pc: the performed-work counters (PC builds, else null).
template <class C> struct Probe {
    Ctr &c;
    Diag *dg;
    Pc *pc;

    // a round of the wave
    __device__ __forceinline__ void round() const {
        if (pc && wave_leader()) pc->waves++;
    }
    // a load of `bytes`: a scalar one counts once per wave, a vector one per lane
    __device__ __forceinline__ void load(bool scalar, uint32_t bytes) const { pc_load(pc, scalar, bytes); }
    // one kd decision at inner node `node`, whose record's first word is `word`
    __device__ __forceinline__ void step(uint32_t node, uint32_t word) const {
        if (pc) pc->steps++;
#ifdef CR_PAD_STEP // issue-cost calibration only: CR_PAD_STEP extra VALU per shadow descent step
        if (C::SHADOW) {
#pragma unroll
            for (int i = 0; i < CR_PAD_STEP; i++) asm volatile("v_mov_b32 %0, %0" : "+v"(word));
        }
#endif
        if (C::FULL) {
            c.inner++;
            const bool uni = wave_uniform(node);
            const uint32_t lines = wave_distinct(node >> (C::FAT ? 2 : 4)); // 32-B / 8-B node records
            if (wave_leader()) {
                c.wave_desc++;
                c.wave_desc_uniform += uni;
                c.wave_desc_lines += lines;
            }
        }
    }
    // a leaf reached: a leaf round of the lane (and of the wave)
    __device__ __forceinline__ void leaf() const {
        if (C::FULL) {
            c.leaf++;
            if (wave_leader()) c.wave_round++;
        }
        if (pc) pc->leaves++;
    }
    // a leaf cull record of `bytes` read
    __device__ __forceinline__ void mask(bool scalar, uint32_t bytes) const {
        if (pc) {
            pc->masks++;
            pc_load(pc, scalar, bytes);
        }
    }
    // a triangle test the lane runs (live) or only sits through
    __device__ __forceinline__ void test(bool live) const {
        if (C::FULL) c.tritest += live ? 1u : 0u;
        if (pc) pc->tests += live ? 1u : 0u;
    }
    // the wave's record loads of one leaf-loop iteration: uniform or not, and the 128-B lines they touch
    __device__ __forceinline__ void tri_lines(uint32_t ref) const {
        if (C::FULL) {
            const bool uni = wave_uniform(ref);
            const uint32_t lines = wave_distinct(ref * (16u * REC_STRIDE) >> 7);
            if (wave_leader()) {
                c.wave_tri++;
                c.wave_tri_uniform += uni;
                c.wave_tri_lines += lines;
            }
        }
    }
    // the leaf-round census: what staging a divergent round's leaves in LDS would take (the lanes at leaf
    // `first` with `count` references), or one more uniform round
    __device__ __forceinline__ void leaf_census(uint32_t first, uint32_t count) const {
        if (C::FULL && (!dg || dg->on) && !wave_uniform(first)) {
            uint64_t m = __ballot(count > 0);
            uint32_t nd = 0, nr = 0, mc = 0, lt = 0;
            const uint32_t lanes = (uint32_t)__popcll(m);
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                const uint32_t f = (uint32_t)__shfl((int)first, l, 64), n = (uint32_t)__shfl((int)count, l, 64);
                const uint64_t same = __ballot(first == f && count > 0);
                m &= ~same;
                nd++;
                nr += n;
                mc = max(mc, n);
                lt += n * (uint32_t)__popcll(same);
            }
            if (wave_leader()) {
                c.leaf_rounds++;
                c.leaf_distinct += nd;
                c.leaf_records += nr;
                c.leaf_fit21 += nr <= 21;
                c.leaf_fit56 += nr <= 56;
                if (dg) {
                    dg->v[DIAG_ROUNDS]++;
                    dg->v[DIAG_LANES] += lanes;
                    dg->v[DIAG_DISTINCT] += nd;
                    dg->v[DIAG_RECORDS] += nr;
                    dg->v[DIAG_MAXCOUNT] += mc;
                    dg->v[DIAG_LANETESTS] += lt;
                    dg->v[DIAG_FIT64] += nr <= 64;
                    dg->v[DIAG_FIT128] += nr <= 128;
                }
            }
        } else if (C::FULL && dg && dg->on && wave_leader()) {
            dg->v[DIAG_UROUNDS]++;
        }
    }
    // the repeated-miss census of one test (triangle `id`, record r): a miss for any segment is one for
    // every later segment of the query
    __device__ __forceinline__ void miss_census(f3 o, f3 d, const TriRec &r, uint32_t id) const {
        if (C::FULL && dg && dg->on) {
            dg->v[DIAG_TESTS]++;
            float gx, gy, gt;
            if (!tri_test(o, d, r, __builtin_inff(), gx, gy, gt)) {
                dg->v[DIAG_GEOMISS]++;
                const uint32_t n = dg->n;
                bool r1 = false, r4 = false, r8 = false;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const bool m = j < n && dg->mb[(n - 1 - j) & 7u] == id;
                    r1 = r1 | (m & (j < 1));
                    r4 = r4 | (m & (j < 4));
                    r8 = r8 | m;
                }
                dg->v[DIAG_REP1] += r1;
                dg->v[DIAG_REP4] += r4;
                dg->v[DIAG_REP8] += r8;
                dg->mb[n & 7u] = id;
                dg->n = n + 1;
            }
        }
    }
    // the divergent masked leaf loop's shape: iterations = the largest lane mask
    __device__ __forceinline__ void dloop(uint32_t mask) const {
        if (pc) {
            const uint32_t pop = (uint32_t)__builtin_popcount(mask);
            const uint32_t lanes = (uint32_t)__popcll(__ballot(pop > 0));
            uint32_t mx = 0;
            while (__ballot(pop > mx)) mx++;
            if (lanes && wave_leader()) {
                pc->drounds++;
                pc->diters += mx;
                pc->dlanes += lanes;
            }
            pc->dtests += pop;
        }
    }
};

} // namespace cr
