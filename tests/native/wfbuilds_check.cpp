// wfbuilds_check.cpp -- host run of the trace builds' table and kernel selection
// (chiaroscuro-raytracer_amd/csrc/wfbuilds.hpp), driven by tests/test_wfbuilds.py.
//   wfbuilds_check            every case; prints "checks N failures M" and one line per failure
// The expectations below are literal data: which kernel every build launches in every mode, written out by
// hand.  Nothing here is derived from the table under test -- a kernel is named by its configuration type
// (the index of a type in a kernel list is only how the header spells that name).
#include <cstdint>
#include <cstdio>
#include <string>

#include "wfbuilds.hpp"

using namespace cr;

static int checks = 0, failures = 0;
static void expect(bool ok, const char *what, long a = 0, long b = 0, long c = 0) {
    checks++;
    if (!ok) {
        failures++;
        std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    }
}

template <class C> constexpr int T() { return trace_id<C>(); }
template <bool PC, bool FD> constexpr int P() { return packet_id<tc::Packet<8, 2, PC, FD>>(); }
template <bool FULL, int W, int LC, bool PC> constexpr int TL() {
    return KernelIndex<tc::Tail<FULL, W, LC, PC>, TailKernels>::value;
}
template <int MINW, bool CH, int BS> constexpr int SH() { return KernelIndex<tc::Shade<MINW, CH, BS>, ShadeKernels>::value; }

enum { NONE = -1 };
struct Want {
    int id;
    int packet_fd; // NONE: the camera is `camera` (a wf_trace); 0 / 1: the packet camera, its FD
    int camera, closest, shadow;
    int dead, closest_fix, shadow_fix, dead_fix; // NONE: the build has no such flavour
    int perf_closest, perf_shadow;               // NONE: perf_counters refuses the build
    int ring, waves, cull, lc;
};
// the twelve builds (the issue's tables; ring, waves per SIMD, camera cull level, tail leaf-cull form)
static const Want kWant[] = {
    {0, NONE, T<tc::CameraRef>(), T<tc::ClosestRef>(), T<tc::ShadowRef>(), NONE, NONE, NONE, NONE, NONE, NONE, 4, 8, 0, 0},
    {15, NONE, T<tc::CameraCull>(), T<tc::ClosestFat>(), T<tc::ShadowFat>(), NONE, NONE, NONE, NONE, NONE, NONE, 8, 8, 2, 0},
    {18, 0, NONE, T<tc::ClosestFat>(), T<tc::ShadowFat>(), NONE, NONE, NONE, NONE, T<tc::ClosestFatPerf>(),
     T<tc::ShadowFatPerf>(), 8, 8, 2, 0},
    {26, 0, NONE, T<tc::ClosestFatLc>(), T<tc::ShadowFatLc>(), NONE, NONE, NONE, NONE, T<tc::ClosestFatLcPerf>(),
     T<tc::ShadowFatLcPerf>(), 8, 8, 2, 4},
    {40, 1, NONE, T<tc::ClosestFatLc>(), T<tc::ShadowFatLc>(), NONE, NONE, NONE, NONE, T<tc::ClosestFatLcPerf>(),
     T<tc::ShadowFatLcPerf>(), 8, 8, 2, 4},
    {42, 1, NONE, T<tc::ClosestFat>(), T<tc::ShadowFat>(), NONE, NONE, NONE, NONE, T<tc::ClosestFatPerf>(),
     T<tc::ShadowFatPerf>(), 8, 8, 2, 0},
    {43, 1, NONE, T<tc::ClosestFatLc>(), T<tc::ShadowFatLcFd>(), NONE, NONE, NONE, NONE, T<tc::ClosestFatLcPerf>(),
     T<tc::ShadowFatLcPerf>(), 8, 8, 2, 4},
    {44, 1, NONE, T<tc::ClosestFat>(), T<tc::ShadowFatFd>(), T<tc::ShadowFatFdDead>(), T<tc::Fixed<tc::ClosestFat>>(),
     T<tc::Fixed<tc::ShadowFatFd>>(), T<tc::Fixed<tc::ShadowFatFdDead>>(), T<tc::ClosestFatPerf>(), T<tc::ShadowFatPerf>(),
     8, 8, 2, 0},
    {49, 1, NONE, T<tc::ClosestFatLc5>(), T<tc::ShadowFatLc5Fd>(), T<tc::ShadowFatLc5FdDead>(), NONE, NONE, NONE,
     T<tc::ClosestFatLc5Perf>(), T<tc::ShadowFatLc5Perf>(), 8, 8, 2, 5},
    {53, 1, NONE, T<tc::ClosestFatLc5>(), T<tc::ShadowFatLc5FdLx>(), T<tc::ShadowFatLc5FdDeadLx>(), NONE, NONE, NONE,
     T<tc::ClosestFatLc5Perf>(), T<tc::ShadowFatLc5LxPerf>(), 8, 8, 2, 5},
    {54, 1, NONE, T<tc::ClosestFatLc5Lx>(), T<tc::ShadowFatLc5FdLx>(), T<tc::ShadowFatLc5FdDeadLx>(), NONE, NONE, NONE,
     T<tc::ClosestFatLc5LxPerf>(), T<tc::ShadowFatLc5LxPerf>(), 8, 8, 2, 5},
    {59, 1, NONE, T<tc::ClosestFatLc5LxD>(), T<tc::ShadowFatLc5FdLxD>(), T<tc::ShadowFatLc5FdDeadLxD>(),
     T<tc::Fixed<tc::ClosestFatLc5LxD>>(), T<tc::Fixed<tc::ShadowFatLc5FdLxD>>(), T<tc::Fixed<tc::ShadowFatLc5FdDeadLxD>>(),
     T<tc::ClosestFatLc5LxPerf>(), T<tc::ShadowFatLc5LxPerf>(), 8, 8, 2, 5},
};
static const int kNumWant = (int)(sizeof(kWant) / sizeof(kWant[0]));

static int lean_tail(int waves, int lc) { // wf_tail<false, 8, W, LC, false>
    const int t[3][3] = {{TL<false, 4, 0, false>(), TL<false, 5, 0, false>(), TL<false, 6, 0, false>()},
                         {TL<false, 4, 4, false>(), TL<false, 5, 4, false>(), TL<false, 6, 4, false>()},
                         {TL<false, 4, 5, false>(), TL<false, 5, 5, false>(), TL<false, 6, 5, false>()}};
    return t[lc == 5 ? 2 : lc == 4 ? 1 : 0][waves - 4];
}
static int perf_tail(int lc) { // wf_tail<false, 8, 4, LC, true>
    return lc == 5 ? TL<false, 4, 5, true>() : lc == 4 ? TL<false, 4, 4, true>() : TL<false, 4, 0, true>();
}

static bool used_trace[TraceKernels::N], used_packet[PacketKernels::N], used_tail[TailKernels::N], used_shade[ShadeKernels::N];
static void use(bool *set, int n, int id, const char *what) {
    expect(id >= 0 && id < n, what, id, n);
    if (id >= 0 && id < n) set[id] = true;
}

int main() {
    const int cus = 256;
    // ---- the lookups ----
    for (int v = -3; v < 80; v++) {
        const Want *w = nullptr;
        for (int i = 0; i < kNumWant; i++)
            if (kWant[i].id == v) w = &kWant[i];
        expect(wf_variant_available(v) == (w != nullptr), "wf_variant_available", v);
        expect(wf_variant_culls(v) == (w && w->cull != 0), "wf_variant_culls", v);
        expect(wf_variant_leaf_cull(v) == (w && w->lc != 0), "wf_variant_leaf_cull", v);
        expect(wf_perf_available(v) == (w && w->perf_closest != NONE), "wf_perf_available", v);
        // every build there is, the counting build (-1) and a number that does not exist (the reference build's):
        // 256 threads, 8 blocks per CU
        uint32_t blk = 0, blocks = 0;
        wf_trace_geometry(v, cus, blk, blocks);
        expect(blk == 256u && blocks == 8u * cus, "wf_trace_geometry", v, blk, blocks);
        wf_trace_geometry(v, 0, blk, blocks);
        expect(blk == 256u && blocks == 8u * 256u, "wf_trace_geometry without a CU count", v, blk, blocks);
    }
    expect(kNumWfBuilds == 12, "twelve builds", kNumWfBuilds);
    expect(num_wf_variants() == 60, "num_wf_variants", num_wf_variants());
    expect(wf_perf_builds_text() == "18, 26, 40, 42, 43, 44, 49, 53, 54 and 59", "wf_perf_builds_text");
    expect(wf_default_build(65536u) == 59 && wf_default_build(0xffffffffu) == 59, "default build of a large scene");
    expect(wf_default_build(65535u) == 44 && wf_default_build(0u) == 44, "default build of a small scene");
    expect(wf_ring_bytes(8) == 16384u && wf_ring_bytes(4) == 8192u, "ring bytes: R x 256 threads x 8");
    expect(wf_mode(true, true) == WF_COUNT && wf_mode(true, false) == WF_COUNT && wf_mode(false, true) == WF_PERF &&
               wf_mode(false, false) == WF_LEAN, "counting wins over perf_counters");

    // ---- trace and tail kernels: builds x mode x eye_on_split x the fixed options x dead x wf_tail_waves ----
    for (int bi = 0; bi < kNumWant; bi++) {
        const Want &w = kWant[bi];
        for (int mode = 0; mode < 3; mode++) {
            const WfMode m = mode == 0 ? WF_LEAN : mode == 1 ? WF_PERF : WF_COUNT;
            const WfBuild *b = wf_render_build(w.id, m);
            if (m == WF_PERF && w.perf_closest == NONE) { // builds 0 and 15: refused before any launch
                expect(b == nullptr, "no performed-work set", w.id);
                continue;
            }
            expect(b != nullptr, "render build", w.id, mode);
            if (!b) continue;
            // LDS ring, grid, cull level and leaf-cull form: the counting build's are 8 / 8 / 0 / 0 whatever the number
            expect(b->ring == (m == WF_COUNT ? 8 : w.ring), "ring", w.id, mode, b->ring);
            expect(b->waves == (m == WF_COUNT ? 8 : w.waves), "waves", w.id, mode, b->waves);
            expect(b->cull == (m == WF_COUNT ? 0 : w.cull), "cull", w.id, mode, b->cull);
            expect(b->lc == (m == WF_COUNT ? 0 : w.lc), "lc", w.id, mode, b->lc);
            expect(b->packet == (m != WF_COUNT && w.packet_fd != NONE ? 1 : 0), "packet", w.id, mode, b->packet);
            // chunked appends (dead entries): lean builds 44, 49, 53, 54, 59 only
            const bool has_dead = m == WF_LEAN && w.dead != NONE;
            expect(wf_appends_chunked(*b, m) == has_dead, "chunked appends", w.id, mode);
            for (int eye = 0; eye < 2; eye++) {
                const CameraSel c = wf_camera_kernel(*b, m, eye != 0);
                if (m == WF_COUNT) {
                    expect(!c.packet && c.id == T<tc::CameraCount>(), "counting camera", w.id, eye, c.id);
                } else if (w.packet_fd == NONE) {
                    expect(!c.packet && c.id == w.camera, "camera", w.id, eye, c.id);
                } else if (eye) { // build 15's camera trace, under perf_counters too
                    expect(!c.packet && c.id == T<tc::CameraCull>(), "eye-on-split camera", w.id, mode, c.id);
                } else {
                    const int want = m == WF_PERF ? (w.packet_fd ? P<true, true>() : P<true, false>())
                                                  : (w.packet_fd ? P<false, true>() : P<false, false>());
                    expect(c.packet && c.id == want, "packet camera", w.id, mode, c.id);
                }
                if (c.packet) use(used_packet, PacketKernels::N, c.id, "packet id in range");
                else use(used_trace, TraceKernels::N, c.id, "camera id in range");
            }
            for (int vis_mark = 0; vis_mark < 3; vis_mark++)
                for (uint32_t ended_only = 0; ended_only < 2; ended_only++)
                    for (int lc_debug = 0; lc_debug < 3; lc_debug++) {
                        const bool held = vis_mark == 1 && ended_only == 0 && lc_debug == 0;
                        const bool fo = wf_fixed_options(vis_mark, ended_only, lc_debug);
                        const int cl = wf_closest_kernel(*b, m, fo);
                        const int want_cl = m == WF_COUNT  ? T<tc::ClosestCount>()
                                            : m == WF_PERF ? w.perf_closest
                                                           : (held && w.closest_fix != NONE ? w.closest_fix : w.closest);
                        expect(cl == want_cl, "closest kernel", w.id, mode, cl);
                        use(used_trace, TraceKernels::N, cl, "closest id in range");
                        for (int dead = 0; dead < 2; dead++) {
                            const int sh = wf_shadow_kernel(*b, m, fo, dead != 0);
                            if (dead && !has_dead) { // never asked for: wf_shade appends per iteration
                                expect(sh == NONE, "no dead flavour", w.id, mode, sh);
                                continue;
                            }
                            const int want_sh =
                                m == WF_COUNT  ? T<tc::ShadowCount>()
                                : m == WF_PERF ? w.perf_shadow
                                : dead         ? (held && w.dead_fix != NONE ? w.dead_fix : w.dead)
                                               : (held && w.shadow_fix != NONE ? w.shadow_fix : w.shadow);
                            expect(sh == want_sh, "shadow kernel", w.id, mode * 2 + dead, sh);
                            use(used_trace, TraceKernels::N, sh, "shadow id in range");
                        }
                    }
            for (int tw = 3; tw <= 7; tw++) { // the option takes 4, 5, 6; anything else launches at 4
                const int t = wf_tail_kernel(*b, m, tw);
                const int eff = tw == 5 || tw == 6 ? tw : 4;
                const int want = m == WF_COUNT ? TL<true, 4, 0, false>() : m == WF_PERF ? perf_tail(w.lc) : lean_tail(eff, w.lc);
                expect(t == want, "tail kernel", w.id, mode, tw);
                use(used_tail, TailKernels::N, t, "tail id in range");
                if (t >= 0 && t < TailKernels::N) {
                    expect(wf_tail_blocks(t, cus) == (uint32_t)cus * (uint32_t)(m == WF_LEAN ? eff : 4), "tail grid", w.id, mode, tw);
                    expect(wf_ring_bytes(tail_desc(t).ring) == 16384u, "tail ring bytes", w.id, mode, tw);
                    // the stride that covers the trace grid covers the tail grid (ChunkLauncher::check)
                    expect(wf_tail_blocks(t, cus) <= wf_trace_blocks(m == WF_COUNT ? -1 : w.id, cus), "tail grid within the trace grid", w.id, mode, tw);
                }
            }
        }
    }
    // ---- ray queries: the default build's generic kernels (cull) or build 44's; never fixed, never dead ----
    for (int def : {59, 44})
        for (int cull = 0; cull < 2; cull++) {
            const WfBuild *b = wf_query_build(def, cull != 0);
            const bool lc = def == 59 && cull;
            expect(b && b->id == (lc ? 59 : 44), "query build", def, cull);
            if (!b) continue;
            expect(wf_query_kernel(*b, false) == (lc ? T<tc::ClosestFatLc5LxD>() : T<tc::ClosestFat>()), "query closest", def, cull);
            expect(wf_query_kernel(*b, true) == (lc ? T<tc::ShadowFatLc5FdLxD>() : T<tc::ShadowFatFd>()), "query shadow", def, cull);
            expect(b->ring == 8 && wf_trace_blocks(b->id, cus) == 8u * cus, "query launch geometry", def, cull);
        }
    expect(wf_query_build(7, true) == nullptr, "a query on a build that does not exist");

    // ---- wf_shade: wf_shade_waves x wf_shade_block x app_chunk ----
    struct ShadeWant {
        int waves, block;
        uint32_t chunk;
        int id, bs; // the kernel and its threads per block
    };
    const ShadeWant shade[] = {
        {8, 256, 0, SH<8, false, 256>(), 256},   {8, 256, 256, SH<8, true, 256>(), 256},  {8, 256, 1024, SH<8, true, 256>(), 256},
        {8, 512, 0, SH<8, false, 512>(), 512},   {8, 512, 256, SH<8, true, 256>(), 256},  {8, 512, 1024, SH<8, true, 256>(), 256},
        {8, 1024, 0, SH<8, false, 1024>(), 1024}, {8, 1024, 256, SH<8, true, 256>(), 256}, {8, 1024, 1024, SH<8, true, 1024>(), 1024},
        {6, 256, 0, SH<1, false, 256>(), 256},   {6, 256, 256, SH<1, true, 256>(), 256},  {6, 256, 1024, SH<1, true, 256>(), 256},
        {6, 512, 0, SH<1, false, 512>(), 512},   {6, 512, 256, SH<1, true, 256>(), 256},  {6, 512, 1024, SH<1, true, 256>(), 256},
        {6, 1024, 0, SH<1, false, 1024>(), 1024}, {6, 1024, 256, SH<1, true, 256>(), 256}, {6, 1024, 1024, SH<1, true, 256>(), 256},
        // (chunks the launcher picks itself: powers of two up to 4096)
        {8, 1024, 512, SH<8, true, 256>(), 256}, {8, 1024, 4096, SH<8, true, 1024>(), 1024}, {6, 1024, 4096, SH<1, true, 256>(), 256},
    };
    for (const ShadeWant &s : shade) {
        const int id = wf_shade_kernel(s.chunk, (uint32_t)s.block, s.waves);
        expect(id == s.id, "shade kernel", s.waves, s.block, (long)s.chunk);
        use(used_shade, ShadeKernels::N, id, "shade id in range");
        if (id >= 0 && id < ShadeKernels::N) expect(shade_desc(id).bs == s.bs, "shade block size", s.waves, s.block, (long)s.chunk);
    }
    // ---- what the selections reach is exactly what the lists instantiate ----
    expect(TraceKernels::N == 37 && PacketKernels::N == 4 && TailKernels::N == 13 && ShadeKernels::N == 9,
           "kernel counts: 37 wf_trace, 4 wf_trace_packet, 13 wf_tail, 9 wf_shade");
    for (int i = 0; i < TraceKernels::N; i++) expect(used_trace[i], "unreachable wf_trace instantiation", i);
    for (int i = 0; i < PacketKernels::N; i++) expect(used_packet[i], "unreachable wf_trace_packet instantiation", i);
    for (int i = 0; i < TailKernels::N; i++) expect(used_tail[i], "unreachable wf_tail instantiation", i);
    for (int i = 0; i < ShadeKernels::N; i++) expect(used_shade[i], "unreachable wf_shade instantiation", i);
    std::printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
