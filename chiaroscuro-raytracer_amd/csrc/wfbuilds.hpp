// wfbuilds.hpp -- the trace builds of the wavefront kernels, each declared once, and which kernel
// instantiation every launch takes.
//
// A trace build (cr_set_option "variant") is a camera trace, a secondary closest trace and a shadow
// trace, each a configuration type of namespace tc, plus the flavours derived from them (the shadow
// trace over queues with dead entries, the instantiations with the default options fixed, the
// performed-work counting set).  Everything else a launch needs to know about a build -- LDS ring
// depth, grid, camera cull level, packet camera or not, the tail kernel's leaf-cull form -- is read
// off those types here, and what has to agree between them is a static_assert.
//
// The kernels themselves are named by the four lists TraceKernels / PacketKernels / TailKernels /
// ShadeKernels: wavefront.hip expands each list once into the table of its kernel template's
// instantiations, so a list is both what exists in the binary and what a selection can return (an
// index into it).  The selection functions at the end are pure: build number and launch facts in,
// indices out.  Host-pure (no HIP headers); tests/native/wfbuilds_check.cpp walks every input.
#pragma once
#include <stdint.h>

#include <string>
#include <type_traits>

namespace cr {

// A trace build's configuration, every knob named.  Who reads which: R, FD, BF -- traverse.hpp kd_step;
// FAT, CULL, SC and the quorum's FULL / CULL guard -- trav_round's descent; CULL, LC, FIX -- its leaf
// references; BF, SC, LC, LX, CULL -- its choice of leaf tester; FULL, PC, SHADOW (pad) -- travprobe.hpp;
// SHADOW, CAM, DEAD, FIX, LX, LXD, MINW -- wf_trace (wavefront.hip).  DESIGN.md §3.24 has the map by stage.
// The defaults are the plain reference build; a build is a type deriving from this and restating what it
// changes (namespace tc below), so a kernel reads e.g. wf_trace<cr::tc::ShadowFatLc5Fd>.
struct TraceDefaults {
    static constexpr bool SHADOW = false; // shadow (any-hit) queries, else closest-hit
    static constexpr bool FULL = false;   // counting build: SURVEY §8d work counters and diagnostics
    static constexpr int R = 8;           // LDS ring entries of the traversal stack per lane
    static constexpr int MINW = 8;        // waves per SIMD the launch bounds ask for
    static constexpr bool SC = false;     // scalar loads of wave-uniform nodes and leaves
    static constexpr bool FD = false;     // exact short split division by the ray's RN(1/d)
    static constexpr bool FAT = false;    // fat node records (a node and its children per load)
    static constexpr bool CAM = false;    // the generation-1 closest (camera-ray) instantiation
    static constexpr bool BF = false;     // branch-light steps and uniform-leaf tests by select
    static constexpr int CULL = 0;        // camera cull boxes: 1 references and leaves, 2 also subtrees
    static constexpr int LC = 0;          // leaf cull records (4 packed, 5 compressed)
    static constexpr bool PC = false;     // performed-work counters (measurement only)
    static constexpr bool DEAD = false;   // shadow queues with dead entries (wf_shade's chunked appends) skipped
    static constexpr bool LX = false;     // a divergent leaf's masked tests spread over the wave (leaf_exchange)
    static constexpr bool LXD = false;    // LX builds: the exchange's prefix by a DPP scan
    // the options every real run leaves at their defaults fixed at compile time: WfArgs::vis_mark 1,
    // WfArgs::ended_only 0 (no overlapped tail), RenderArgs::lc_debug 0 -- the launchers take such an
    // instantiation only for a launch whose options have these values (tc::Fixed, wf_fixed_options).  It also
    // fixes a fact of the scene: |coordinate| <= 2^19 (wf_short_division_scene), under which the FD builds'
    // split division drops its upper range test (device_math.hpp div_by_rcp_wave_bounded)
    static constexpr bool FIX = false;
};

// Threads per block of wf_trace, wf_trace_packet and wf_tail: their launch bounds, the per-wave LDS of
// the leaf exchange and every grid below are written for it.
enum : uint32_t { WF_TRACE_BLOCK = 256, WF_TRACE_WAVES = WF_TRACE_BLOCK / 64 };
// Bytes of one entry of the traversal stack's LDS ring (a uint2: node, far distance); the dynamic LDS of
// a trace or tail launch is R entries per thread.
enum : uint32_t { WF_RING_ENTRY = 8 };

// The trace configurations of the builds, by what they restate.
namespace tc {
// build 0: the plain reference build (4-deep ring, vector loads, one level per load)
struct CameraRef : TraceDefaults { static constexpr int R = 4; static constexpr bool CAM = true; };
struct ClosestRef : TraceDefaults { static constexpr int R = 4; };
struct ShadowRef : TraceDefaults { static constexpr int R = 4; static constexpr bool SHADOW = true; };
// fat records, scalar loads of wave-uniform nodes / leaves, branch-light steps
struct Fat : TraceDefaults { static constexpr bool SC = true, FAT = true, BF = true; };
struct ClosestFat : Fat {};
struct ShadowFat : Fat { static constexpr bool SHADOW = true; };
// the camera trace with cull boxes of references, leaves and subtrees
struct CameraCull : Fat { static constexpr bool CAM = true; static constexpr int CULL = 2; };
// + packed fixed-pad leaf cull records
struct ClosestFatLc : Fat { static constexpr int LC = 4; };
struct ShadowFatLc : ClosestFatLc { static constexpr bool SHADOW = true; };
// + the exact short split division by the ray's RN(1/d) in the shadow trace
struct ShadowFatLcFd : ShadowFatLc { static constexpr bool FD = true; };
struct ShadowFatFd : ShadowFat { static constexpr bool FD = true; };
struct ShadowFatFdDead : ShadowFatFd { static constexpr bool DEAD = true; };
// the same with the compressed leaf cull records (48 B per leaf instead of 96: three loads, not six)
struct ClosestFatLc5 : Fat { static constexpr int LC = 5; };
struct ShadowFatLc5Fd : ClosestFatLc5 { static constexpr bool SHADOW = true, FD = true; };
struct ShadowFatLc5FdDead : ShadowFatLc5Fd { static constexpr bool DEAD = true; };
// + the leaf exchange (traverse.hpp leaf_exchange: a divergent leaf's masked tests spread over the wave)
struct ClosestFatLc5Lx : ClosestFatLc5 { static constexpr bool LX = true; };
struct ShadowFatLc5FdLx : ShadowFatLc5Fd { static constexpr bool LX = true; };
struct ShadowFatLc5FdDeadLx : ShadowFatLc5FdDead { static constexpr bool LX = true; };
struct ClosestFatLc5LxD : ClosestFatLc5Lx { static constexpr bool LXD = true; };
struct ShadowFatLc5FdLxD : ShadowFatLc5FdLx { static constexpr bool LXD = true; };
struct ShadowFatLc5FdDeadLxD : ShadowFatLc5FdDeadLx { static constexpr bool LXD = true; };
// the performed-work counting instances (RenderArgs::perf_counters; measurement only).  The short division
// and the exchange's DPP prefix do the same work as the forms they replace, so they have no instance of
// their own: a build names the set that counts for it (PerfSet below)
struct ClosestFatPerf : ClosestFat { static constexpr bool PC = true; };
struct ShadowFatPerf : ShadowFat { static constexpr bool PC = true; };
struct ClosestFatLcPerf : ClosestFatLc { static constexpr bool PC = true; };
struct ShadowFatLcPerf : ShadowFatLc { static constexpr bool PC = true; };
struct ClosestFatLc5Perf : ClosestFatLc5 { static constexpr bool PC = true; };
struct ShadowFatLc5Perf : ClosestFatLc5Perf { static constexpr bool SHADOW = true; };
struct ClosestFatLc5LxPerf : ClosestFatLc5Lx { static constexpr bool PC = true; };
struct ShadowFatLc5LxPerf : ClosestFatLc5LxPerf { static constexpr bool SHADOW = true; };
// the counting build (SURVEY §8d work counters, diagnostics: RenderArgs::full_counters), 1 wave per SIMD
struct Count : TraceDefaults { static constexpr bool FULL = true; static constexpr int MINW = 1; };
struct CameraCount : Count { static constexpr bool CAM = true; };
struct ClosestCount : Count {};
struct ShadowCount : Count { static constexpr bool SHADOW = true; };
// a build's trace with the options of TraceDefaults::FIX at their defaults, fixed at compile time: the
// same build number, taken by the launchers when wf_fixed_options holds
template <class B> struct Fixed : B { static constexpr bool FIX = true; };

// wf_trace_packet<R, S, PC, FD>: the camera rays of a tile as packets of 64 S per wave (PC: with the
// performed-work counts; FD: the short division).  Its ring is [R][blockDim][S] of uint32_t.
template <int R_, int S_, bool PC_, bool FD_> struct Packet {
    static constexpr int R = R_, S = S_, MINW = 8, CULL = 2; // (the kernel's own launch bounds and cull level)
    static constexpr bool PC = PC_, FD = FD_;
    using Perf = Packet<R_, S_, true, FD_>;
};
template <class T> struct IsPacket : std::false_type {};
template <int R, int S, bool PC, bool FD> struct IsPacket<Packet<R, S, PC, FD>> : std::true_type {};
// wf_tail<FULL, R, MINW, LC, PC>: the rest of a chunk in one launch, on MINW blocks per CU
template <bool FULL_, int MINW_, int LC_, bool PC_> struct Tail {
    static constexpr bool FULL = FULL_, PC = PC_;
    static constexpr int R = 8, MINW = MINW_, LC = LC_;
};
// wf_shade<MINW, CH, BS>: CH appends in chunks (WfArgs::app_chunk), BS threads per block
template <int MINW_, bool CH_, int BS_> struct Shade {
    static constexpr int MINW = MINW_, BS = BS_;
    static constexpr bool CH = CH_;
};
// the closest and shadow instances whose performed-work counts stand for a build's
template <class Cl, class Sh> struct PerfSet {
    using Closest = Cl;
    using Shadow = Sh;
};
using PerfFat = PerfSet<ClosestFatPerf, ShadowFatPerf>;
using PerfFatLc = PerfSet<ClosestFatLcPerf, ShadowFatLcPerf>;
using PerfFatLc5 = PerfSet<ClosestFatLc5Perf, ShadowFatLc5Perf>;
using PerfFatLc5LxShadow = PerfSet<ClosestFatLc5Perf, ShadowFatLc5LxPerf>;
using PerfFatLc5Lx = PerfSet<ClosestFatLc5LxPerf, ShadowFatLc5LxPerf>;
} // namespace tc

// ------------------------------------------------------------ the kernels --
// A list of kernel configurations; a kernel's identifier is its index.
template <class... T> struct KernelList { static constexpr int N = (int)sizeof...(T); };
template <class T, class L> struct KernelIndex;
template <class T, class... U> struct KernelIndex<T, KernelList<T, U...>> { static constexpr int value = 0; };
template <class T, class H, class... U> struct KernelIndex<T, KernelList<H, U...>> {
    static constexpr int value = 1 + KernelIndex<T, KernelList<U...>>::value;
};
template <class L> struct KernelIndex<void, L> { static constexpr int value = -1; }; // "the build has none"
// (a type that is not in the list does not compile: there is no kernel to launch for it)

using TraceKernels = KernelList<
    tc::CameraRef, tc::ClosestRef, tc::ShadowRef, tc::CameraCull, tc::ClosestFat, tc::ShadowFat, tc::ClosestFatLc,
    tc::ShadowFatLc, tc::ShadowFatLcFd, tc::ShadowFatFd, tc::ShadowFatFdDead, tc::ClosestFatLc5, tc::ShadowFatLc5Fd,
    tc::ShadowFatLc5FdDead, tc::ClosestFatLc5Lx, tc::ShadowFatLc5FdLx, tc::ShadowFatLc5FdDeadLx, tc::ClosestFatLc5LxD,
    tc::ShadowFatLc5FdLxD, tc::ShadowFatLc5FdDeadLxD, tc::Fixed<tc::ClosestFat>, tc::Fixed<tc::ShadowFatFd>,
    tc::Fixed<tc::ShadowFatFdDead>, tc::Fixed<tc::ClosestFatLc5LxD>, tc::Fixed<tc::ShadowFatLc5FdLxD>,
    tc::Fixed<tc::ShadowFatLc5FdDeadLxD>, tc::ClosestFatPerf, tc::ShadowFatPerf, tc::ClosestFatLcPerf,
    tc::ShadowFatLcPerf, tc::ClosestFatLc5Perf, tc::ShadowFatLc5Perf, tc::ClosestFatLc5LxPerf, tc::ShadowFatLc5LxPerf,
    tc::CameraCount, tc::ClosestCount, tc::ShadowCount>;
using PacketKernels = KernelList<tc::Packet<8, 2, false, false>, tc::Packet<8, 2, false, true>,
                                 tc::Packet<8, 2, true, false>, tc::Packet<8, 2, true, true>>;
// lean at 4, 5 or 6 waves per SIMD (option "wf_tail_waves"); performed-work and counting at 4 (the path
// bodies need more registers than the trace kernels' 64)
using TailKernels = KernelList<
    tc::Tail<false, 4, 0, false>, tc::Tail<false, 5, 0, false>, tc::Tail<false, 6, 0, false>,
    tc::Tail<false, 4, 4, false>, tc::Tail<false, 5, 4, false>, tc::Tail<false, 6, 4, false>,
    tc::Tail<false, 4, 5, false>, tc::Tail<false, 5, 5, false>, tc::Tail<false, 6, 5, false>,
    tc::Tail<false, 4, 0, true>, tc::Tail<false, 4, 4, true>, tc::Tail<false, 4, 5, true>, tc::Tail<true, 4, 0, false>>;
using ShadeKernels = KernelList<tc::Shade<8, false, 256>, tc::Shade<1, false, 256>, tc::Shade<8, false, 512>,
                                tc::Shade<1, false, 512>, tc::Shade<8, false, 1024>, tc::Shade<1, false, 1024>,
                                tc::Shade<8, true, 256>, tc::Shade<1, true, 256>, tc::Shade<8, true, 1024>>;

template <class C> constexpr int trace_id() { return KernelIndex<C, TraceKernels>::value; }
template <class C> constexpr int packet_id() { return KernelIndex<C, PacketKernels>::value; }

// What the selections match a tail or shade kernel by, one row per list entry (the same order).
struct TailDesc {
    bool full, pc;
    int waves, lc, ring;
};
struct ShadeDesc {
    int minw, bs;
    bool chunked;
};
template <class L> struct KernelDescs;
template <class... K> struct KernelDescs<KernelList<K...>> {
    static constexpr TailDesc tail[] = {{K::FULL, K::PC, K::MINW, K::LC, K::R}...};
};
template <class L> struct ShadeDescs;
template <class... K> struct ShadeDescs<KernelList<K...>> {
    static constexpr ShadeDesc shade[] = {{K::MINW, K::BS, K::CH}...};
};
inline const TailDesc &tail_desc(int id) { return KernelDescs<TailKernels>::tail[id]; }
inline const ShadeDesc &shade_desc(int id) { return ShadeDescs<ShadeKernels>::shade[id]; }

// ------------------------------------------------------------- the builds --
// The kernels of a build in one counting mode: indices into TraceKernels (camera: into PacketKernels when
// `packet`), -1 where the build has none.
struct WfKernels {
    int camera, closest, shadow;
    int shadow_dead;                              // shadow queues wf_shade appended in chunks (dead entries skipped)
    int closest_fix, shadow_fix, shadow_dead_fix; // tc::Fixed of the three
};
struct WfBuild {
    int id;
    WfKernels lean, perf; // perf: RenderArgs::perf_counters (never a dead or fixed flavour)
    bool has_perf;
    int ring;  // LDS ring entries per thread of every trace launch of the build
    int waves; // blocks per CU (= waves per SIMD) of every trace launch
    int cull;  // the camera trace reads the cull boxes (1: references and leaves, 2: also subtrees)
    int packet; // the camera trace is a packet trace (needs a near child common to all camera rays)
    int lc;     // the leaf cull form of the secondary traces and of the tail kernel (0: none)
};

// One build.  Camera: a wf_trace configuration or a tc::Packet; Dead: the shadow trace's DEAD flavour or
// void; FIXED: tc::Fixed instantiations of closest, shadow and dead exist; Perf: the tc::PerfSet that counts
// for it or void; GRID_WAVES: blocks per CU, the launch bounds' waves per SIMD unless stated.
template <class Camera, class Closest, class Shadow, class Dead = void, bool FIXED = false, class Perf = void,
          int GRID_WAVES = Closest::MINW>
constexpr WfBuild wf_declare(int id) {
    constexpr bool packet = tc::IsPacket<Camera>::value, dead = !std::is_void<Dead>::value;
    // one dynamic LDS size and one grid serve the camera, closest and shadow launches of a build
    static_assert(Camera::R == Closest::R && Shadow::R == Closest::R, "a build's traces share the ring depth");
    static_assert(Camera::MINW == Closest::MINW && Shadow::MINW == Closest::MINW, "... and the launch bounds");
    static_assert(!Closest::SHADOW && Shadow::SHADOW && !Closest::CAM && !Shadow::CAM, "closest / shadow swapped");
    static_assert(Closest::LC == Shadow::LC, "one leaf cull form per build (the tail kernel's too)");
    static_assert(!FIXED || dead, "the fixed flavours come in threes");
    int cam = 0, cam_perf = -1;
    if constexpr (packet) {
        // the packet's ring [R][block][S] of uint32_t fills exactly the [R][block] ring entries of the launch
        static_assert(Camera::S * sizeof(uint32_t) == WF_RING_ENTRY, "packet ring bytes");
        static_assert(!Camera::PC, "declare the lean packet; the counting one is derived");
        cam = packet_id<Camera>();
        cam_perf = packet_id<typename Camera::Perf>();
    } else {
        static_assert(Camera::CAM && !Camera::SHADOW, "camera configuration");
        cam = trace_id<Camera>();
    }
    WfKernels lean = {cam, trace_id<Closest>(), trace_id<Shadow>(), -1, -1, -1, -1};
    if constexpr (dead) {
        static_assert(Dead::DEAD && Dead::SHADOW && Dead::R == Shadow::R && Dead::MINW == Shadow::MINW &&
                      Dead::LC == Shadow::LC, "dead flavour of another shadow trace");
        lean.shadow_dead = trace_id<Dead>();
    }
    if constexpr (FIXED) {
        lean.closest_fix = trace_id<tc::Fixed<Closest>>();
        lean.shadow_fix = trace_id<tc::Fixed<Shadow>>();
        lean.shadow_dead_fix = trace_id<tc::Fixed<Dead>>();
    }
    WfKernels perf = {-1, -1, -1, -1, -1, -1, -1};
    if constexpr (!std::is_void<Perf>::value) {
        using PCl = typename Perf::Closest;
        using PSh = typename Perf::Shadow;
        static_assert(packet, "the performed-work camera is the counting packet");
        static_assert(PCl::PC && PSh::PC && !PCl::SHADOW && PSh::SHADOW, "performed-work set");
        static_assert(PCl::R == Closest::R && PSh::R == Closest::R && PCl::MINW == Closest::MINW &&
                      PSh::MINW == Closest::MINW && PCl::LC == Closest::LC && PSh::LC == Closest::LC,
                      "the counting set runs on the build's LDS, grid and tail");
        perf = {cam_perf, trace_id<PCl>(), trace_id<PSh>(), -1, -1, -1, -1};
    }
    return {id, lean, perf, !std::is_void<Perf>::value, Closest::R, GRID_WAVES, Camera::CULL, packet ? 1 : 0, Closest::LC};
}

using PacketCam = tc::Packet<8, 2, false, false>;   // two camera rays per lane (128-ray packets)
using PacketCamFd = tc::Packet<8, 2, false, true>;  // ... dividing by the rays' RN(1/d) kept in VGPRs

// The trace builds by number.  The measured and superseded builds 1-14, 16, 17, 19-25, 27-39, 41, 45-48
// and 51 are gone; DESIGN.md keeps their numbers.  Adding or removing one: DESIGN.md "Adding or removing a
// trace build".
constexpr WfBuild kWfBuilds[] = {
    // 0: the plain reference build
    wf_declare<tc::CameraRef, tc::ClosestRef, tc::ShadowRef>(0),
    // 15: fat records, scalar loads, branch-light steps; the camera trace skips the tests, leaves and
    // subtrees whose screen-space cull box excludes the sample
    wf_declare<tc::CameraCull, tc::ClosestFat, tc::ShadowFat>(15),
    // 18: 15 whose camera rays traverse as one packet of 128 per wave (wf_trace_packet)
    wf_declare<PacketCam, tc::ClosestFat, tc::ShadowFat, void, false, tc::PerfFat>(18),
    // 26: 18 whose secondary closest and shadow traces skip the references a leaf's packed cull record
    // (leafcull.hpp: two normal groups, each a box and a normal cone) excludes for the ray; the tail
    // kernel culls the same way
    wf_declare<PacketCam, tc::ClosestFatLc, tc::ShadowFatLc, void, false, tc::PerfFatLc>(26),
    // 40 / 42: 26 / 18 whose camera packet divides by the rays' RN(1/d) (FD; the packet's spills are
    //     outside its loops): camera trace 41.0 -> 37.7 ms, 363.1 -> 360.0 ms per pass
    wf_declare<PacketCamFd, tc::ClosestFatLc, tc::ShadowFatLc, void, false, tc::PerfFatLc>(40),
    wf_declare<PacketCamFd, tc::ClosestFat, tc::ShadowFat, void, false, tc::PerfFat>(42),
    // 43 / 44: 40 / 42 whose shadow trace divides by the ray's RN(1/d) in VGPRs too (no spills at 8 waves
    //     once the stack-overflow pointer and the query count stopped occupying VGPRs): 357.5 / 355.3 vs
    //     358.4 / 358.1 ms per pass, nanobox 162.4 vs 163.7 ms (shadow 30.7 -> 29.9)
    wf_declare<PacketCamFd, tc::ClosestFatLc, tc::ShadowFatLcFd, void, false, tc::PerfFatLc>(43),
    wf_declare<PacketCamFd, tc::ClosestFat, tc::ShadowFatFd, tc::ShadowFatFdDead, true, tc::PerfFat>(44),
    // 49: 43 whose secondary closest, shadow and tail traces read the compressed leaf cull records
    //     (leafcull.hpp LC_RECC: boxes on the scene's 16-bit grid, octahedral axes, half constants)
    wf_declare<PacketCamFd, tc::ClosestFatLc5, tc::ShadowFatLc5Fd, tc::ShadowFatLc5FdDead, false, tc::PerfFatLc5>(49),
    // 53 / 54: 49 whose shadow trace (53) or shadow and secondary closest traces (54) test a divergent leaf
    //     round's masked references with the whole wave (the leaf exchange, traverse.hpp leaf_exchange,
    //     DESIGN.md §3.16): sponza 2315 -> 2348 (53) / 2362 (54) Mray/s, shadow trace 39.2 -> 38.3 ms, closest
    //     68.9 -> 67.2 ms per launch beside it.  Measured and removed: the shadow exchange at 7 waves per
    //     SIMD (no spills then; 2305 Mray/s) and the lane index recomputed per use instead of held in a
    //     register (no spills at 8 waves; 2300 / 2330 Mray/s)
    wf_declare<PacketCamFd, tc::ClosestFatLc5, tc::ShadowFatLc5FdLx, tc::ShadowFatLc5FdDeadLx, false,
               tc::PerfFatLc5LxShadow>(53),
    wf_declare<PacketCamFd, tc::ClosestFatLc5Lx, tc::ShadowFatLc5FdLx, tc::ShadowFatLc5FdDeadLx, false,
               tc::PerfFatLc5Lx>(54),
    // 59: 54 with the exchange's prefix by a DPP scan (LXD: six row-shift / row-broadcast adds instead of
    //     six bit-sliced ballots with their mbcnt pairs): 2348 -> 2395 Mray/s, shadow trace 38.4 -> 37.6 ms,
    //     closest 67.3 -> 65.5 ms (three interleaved rounds)
    wf_declare<PacketCamFd, tc::ClosestFatLc5LxD, tc::ShadowFatLc5FdLxD, tc::ShadowFatLc5FdDeadLxD, true,
               tc::PerfFatLc5Lx>(59),
};
constexpr int kNumWfBuilds = (int)(sizeof(kWfBuilds) / sizeof(kWfBuilds[0]));
// The counting build (RenderArgs::full_counters), whatever the build number: its launch bounds ask for one
// wave per SIMD (registers for the counters), its grid is the 8 blocks per CU of every other build.
constexpr WfBuild kWfCountBuild = wf_declare<tc::CameraCount, tc::ClosestCount, tc::ShadowCount, void, false, void, 8>(-1);

// The named builds: a scene's default from LEAF_CULL_MIN_TRIS triangles on and below it (the leaf cull
// pays on large scenes only: cabi.cpp fill_args has the history), the camera trace a packet build falls
// back to when the eye lies exactly on a split plane (the packet needs a near child common to all camera
// rays), and the fat kernels without a leaf cull that answer the ray queries the default build cannot
// (queryroute.hpp QR_FAT).
enum : int { WF_BUILD_LEAF_CULL = 59, WF_BUILD_SMALL = 44, WF_BUILD_EYE_ON_SPLIT = 15, WF_BUILD_QUERY_FAT = 44 };
enum : uint32_t { LEAF_CULL_MIN_TRIS = 65536 };
constexpr int wf_default_build(uint32_t n_tris) { return n_tris >= LEAF_CULL_MIN_TRIS ? WF_BUILD_LEAF_CULL : WF_BUILD_SMALL; }

// the build numbered `variant`, or null when there is none
constexpr const WfBuild *wf_build(int variant) {
    for (int i = 0; i < kNumWfBuilds; i++)
        if (kWfBuilds[i].id == variant) return &kWfBuilds[i];
    return nullptr;
}
constexpr bool wf_named_builds_ok() {
    const WfBuild *f = wf_build(WF_BUILD_EYE_ON_SPLIT), *q = wf_build(WF_BUILD_QUERY_FAT);
    if (!f || f->packet || !q || q->lc || !wf_build(WF_BUILD_LEAF_CULL) || !wf_build(WF_BUILD_SMALL)) return false;
    // the fallback camera trace is launched with the packet build's LDS and grid
    for (int i = 0; i < kNumWfBuilds; i++)
        if (kWfBuilds[i].packet && (kWfBuilds[i].ring != f->ring || kWfBuilds[i].waves != f->waves)) return false;
    return true;
}
static_assert(wf_named_builds_ok(), "the named builds exist and fit the launches that borrow them");

constexpr bool wf_variant_available(int variant) { return wf_build(variant) != nullptr; }
// the variant's camera trace skips Moller-Trumbore tests by the cull boxes
constexpr bool wf_variant_culls(int variant) { return wf_build(variant) && wf_build(variant)->cull; }
// the variant's secondary closest and shadow traces read leaf cull records (leafcull.hpp)
constexpr bool wf_variant_leaf_cull(int variant) { return wf_build(variant) && wf_build(variant)->lc != 0; }
// a performed-work set counts for this build
constexpr bool wf_perf_available(int variant) { return wf_build(variant) && wf_build(variant)->has_perf; }
// one past the largest build number (option validation)
constexpr int num_wf_variants() {
    int m = 0;
    for (int i = 0; i < kNumWfBuilds; i++) m = kWfBuilds[i].id + 1 > m ? kWfBuilds[i].id + 1 : m;
    return m;
}
// "18, 26, ... and 59": the builds wf_perf_available accepts, for messages
inline std::string wf_perf_builds_text() {
    int n = 0, k = 0;
    for (int i = 0; i < kNumWfBuilds; i++) n += kWfBuilds[i].has_perf ? 1 : 0;
    std::string s;
    for (int i = 0; i < kNumWfBuilds; i++)
        if (kWfBuilds[i].has_perf) {
            if (k) s += k == n - 1 ? " and " : ", ";
            s += std::to_string(kWfBuilds[i].id);
            k++;
        }
    return s;
}

// ---------------------------------------------------------- the selection --
enum WfMode { WF_LEAN = 0, WF_PERF = 1, WF_COUNT = 2 };
constexpr WfMode wf_mode(bool full_counters, bool perf_counters) {
    return full_counters ? WF_COUNT : perf_counters ? WF_PERF : WF_LEAN;
}
// The build whose kernels a render launches: the counting build whatever the number; null for a number that
// does not exist or, under perf_counters, has no performed-work set (run_render refuses both before any launch).
constexpr const WfBuild *wf_render_build(int variant, WfMode m) {
    if (m == WF_COUNT) return &kWfCountBuild;
    const WfBuild *b = wf_build(variant);
    return b && (m != WF_PERF || b->has_perf) ? b : nullptr;
}
constexpr const WfKernels &wf_kernels(const WfBuild &b, WfMode m) { return m == WF_PERF ? b.perf : b.lean; }
// Block and grid of the build's trace launches (and the stride of the stack-overflow rows, sized from them).
// -1: the counting build; a number that does not exist: the reference build 0's.
constexpr uint32_t wf_trace_blocks(int variant, int num_cus) {
    const WfBuild *b = variant == -1 ? &kWfCountBuild : wf_build(variant);
    return (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)(b ? b : &kWfBuilds[0])->waves;
}
inline void wf_trace_geometry(int variant, int num_cus, uint32_t &block, uint32_t &blocks) {
    block = WF_TRACE_BLOCK;
    blocks = wf_trace_blocks(variant, num_cus);
}
constexpr size_t wf_ring_bytes(int ring) { return (size_t)ring * WF_TRACE_BLOCK * WF_RING_ENTRY; }

// True when every option a tc::Fixed instantiation fixes has its fixed value for a launch
// (TraceDefaults::FIX); any other value selects the build's generic kernels.
constexpr bool wf_fixed_options(int vis_mark, uint32_t ended_only, int lc_debug) {
    return vis_mark == 1 && ended_only == 0u && lc_debug == 0;
}
// True when the split division of a render's secondary and shadow rays stays below its upper range bound by
// the scene alone: the dividend is split - o_a with |split| <= db and |o_a| <= db (DevScene::db: every vertex,
// so every split plane, and every origin the render makes lie in the padded box), the reciprocal is at most
// 2^40 (rcp_for_div), so |q0| <= 2 db 2^40 <= 2^60 once db <= 2^19.  A scene outside it renders with the
// build's generic kernels, whose division tests both bounds.  (A caller's ray queries never take a fixed
// kernel: wf_query_kernel.)
constexpr bool wf_short_division_scene(float db) { return db <= 0x1p19f; }
// A selected camera trace: `id` indexes PacketKernels when `packet`, else TraceKernels.
struct CameraSel {
    int packet, id;
};
// The camera-ray trace: the packet needs a near child common to all camera rays, which an eye lying exactly
// on a split plane breaks -- WF_BUILD_EYE_ON_SPLIT's camera trace then (under perf_counters too).
constexpr CameraSel wf_camera_kernel(const WfBuild &b, WfMode m, bool eye_on_split) {
    if (b.packet && eye_on_split) return {0, wf_build(WF_BUILD_EYE_ON_SPLIT)->lean.camera};
    return {b.packet, wf_kernels(b, m).camera};
}
// The secondary closest and the shadow trace of a launch: the build's tc::Fixed instantiation when it has one
// and the launch's options are the fixed ones, else its generic kernel.  dead: the shadow queue may hold dead
// entries (-1 when the build has no such trace: wf_appends_chunked is false for it, so none is ever asked for).
constexpr int wf_closest_kernel(const WfBuild &b, WfMode m, bool fixed_options) {
    const WfKernels &k = wf_kernels(b, m);
    return k.closest_fix >= 0 && fixed_options ? k.closest_fix : k.closest;
}
constexpr int wf_shadow_kernel(const WfBuild &b, WfMode m, bool fixed_options, bool dead) {
    const WfKernels &k = wf_kernels(b, m);
    if (dead) return k.shadow_dead_fix >= 0 && fixed_options ? k.shadow_dead_fix : k.shadow_dead;
    return k.shadow_fix >= 0 && fixed_options ? k.shadow_fix : k.shadow;
}
// wf_shade may append in chunks (leaving dead entries) only where a shadow trace skips them
constexpr bool wf_appends_chunked(const WfBuild &b, WfMode m) { return wf_kernels(b, m).shadow_dead >= 0; }
// One trace launch over a ray-query queue: the generic closest or shadow kernel of the scene's default build
// (cull: QR_DEFAULT queries) or of WF_BUILD_QUERY_FAT.  Never fixed, never dead.  Null build: no such build.
constexpr const WfBuild *wf_query_build(int default_variant, bool cull) {
    return wf_build(cull ? default_variant : WF_BUILD_QUERY_FAT);
}
constexpr int wf_query_kernel(const WfBuild &b, bool shadow) { return shadow ? b.lean.shadow : b.lean.closest; }

// The tail kernel: counting and performed-work at 4 blocks per CU; lean at lean_waves (5 or 6 when the option
// "wf_tail_waves" says so, else 4), with the build's leaf cull form.  -1: no such kernel.
inline int wf_tail_kernel(const WfBuild &b, WfMode m, int lean_waves) {
    const TailDesc want = {m == WF_COUNT, m == WF_PERF,
                           m == WF_LEAN && (lean_waves == 5 || lean_waves == 6) ? lean_waves : 4, b.lc, 8};
    for (int i = 0; i < TailKernels::N; i++) {
        const TailDesc &d = tail_desc(i);
        if (d.full == want.full && d.pc == want.pc && d.waves == want.waves && d.lc == want.lc) return i;
    }
    return -1;
}
inline uint32_t wf_tail_blocks(int tail_id, int num_cus) {
    return (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)tail_desc(tail_id).waves;
}

// wf_shade of a launch, from WfArgs::app_chunk / shade_block / shade_waves ("wf_shade_waves" 8, or 6: launch
// bounds of 1).  A chunk holds at least one iteration's appends, so chunked 1024-thread blocks need chunks of
// 1024 or more and exist at 8 waves only; any other chunked launch runs 256-thread blocks.  -1: no such kernel.
inline int wf_shade_kernel(uint32_t app_chunk, uint32_t shade_block, int shade_waves) {
    const int minw = shade_waves == 8 ? 8 : 1;
    ShadeDesc want = {minw, 256, app_chunk != 0u};
    if (app_chunk >= 1024u && shade_block == 1024u && shade_waves == 8) want.bs = 1024;
    else if (!app_chunk && (shade_block == 1024u || shade_block == 512u)) want.bs = (int)shade_block;
    for (int i = 0; i < ShadeKernels::N; i++) {
        const ShadeDesc &d = shade_desc(i);
        if (d.minw == want.minw && d.bs == want.bs && d.chunked == want.chunked) return i;
    }
    return -1;
}

} // namespace cr
