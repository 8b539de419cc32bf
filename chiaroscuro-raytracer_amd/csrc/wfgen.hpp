// wfgen.hpp -- the schedule of one wavefront chunk, as pure host functions in the style of wfplan.hpp: the chunk's
// start, the append chunk of a wf_shade launch, and what follows a generation's wf_shade once its two queue lengths
// are on the host.  ChunkLauncher (wavefront.hip) executes it for both chunk drivers; nothing here calls the HIP
// runtime, and tests/native/wfgen_check.cpp holds it to what the drivers' own lines computed.
#pragma once
#include "kernels.hpp"

namespace cr {

// What a chunk driver does: the two drivers differ in these four things and in nothing else of the schedule.
struct WfDriver {
    bool sort_g1;      // consults WfArgs::sort_g1 (else: generation-1 queues are sorted like any other)
    bool app_chunks;   // wf_shade may append in chunks (dead queue entries)
    bool tail_overlap; // may start the tail beside the last shadow trace
    int tail_waves;    // waves per SIMD of its lean tail; 0: WfArgs::tail_waves
};
constexpr WfDriver WF_DRIVER_CHUNK = {true, true, true, 0};    // launch_wavefront_chunk
constexpr WfDriver WF_DRIVER_LANES = {false, false, false, 4}; // run_wavefront_lanes
inline int wf_tail_waves(const WfDriver &d, int option) { return d.tail_waves ? d.tail_waves : option; }

// Generation g's appended rays (shadow queue g, closest queue g + 1) get pixel keys: wf_shade's choice on the
// device, the sort's key width on the host
__host__ __device__ inline bool wf_pixel_keys(int leaf_keys, int world_keys, uint32_t g) {
    return !leaf_keys && !(world_keys && g >= (uint32_t)world_keys);
}
// Path state (wavefront.hip PS).  When generation 1 runs as wavefront launches (the chunk is not handed to wf_tail
// at once), wf_camera writes only the resolve mark: wf_shade derives generation 1's RNG state -- the camera
// sample's stream after its two jitter draws -- from the path's (pixel, sample) instead of reading it.
__host__ __device__ __forceinline__ bool camera_state_lean(const WfArgs &W) { return W.cam_lean && W.P >= W.tail_min; }

// The start of the chunk bound as W.  cam_fused: the camera rays come from the packet trace itself, when the ctx
// asks for it (W.cam_fused on entry), the camera kernel is the packet trace and generation 1 runs as its own lean
// launches; else wf_camera launches.  tail_only: the whole chunk goes to wf_tail(1), which reads wf_camera's rays.
struct WfStart { bool cam_fused, camera, tail_only; };
inline WfStart wf_chunk_start(const WfArgs &W, bool packet, bool eye_on_split) {
    const bool fused = W.cam_fused && packet && !eye_on_split && camera_state_lean(W);
    return {fused, !fused, W.P < W.tail_min};
}

// The append chunk of a wf_shade launch over nin rays (WfArgs::app_chunk): a power of two giving each block about
// 16 chunks per queue, so the dead entries stay a few percent of the queue; 0 (one atomic per block iteration) for
// queues that short, and at most what the queues' spare slots hold for every block's partial last chunk.  Only for
// queues traced in append order (W.sort 0: scenes below SORT_MIN_TRIS): round 5, two interleaved rounds, cornell_box
// 13,002 / 13,000 -> 14,331 / 14,298 Mray/s; on sorted queues (sponza stand-in) wf_shade gains 9 % but the shadow
// trace loses 1.7 % -- the chunks change the order among equal keys -- 2278.5 / 2278.7 -> 2274.8 / 2270.4
// grid: wf_shade_blocks(); build_chunks: wf_appends_chunked of the render's build
inline uint32_t wf_app_chunk(const WfArgs &W, uint32_t nin, uint32_t grid, bool build_chunks, const WfDriver &d) {
    if (!d.app_chunks || !build_chunks || !W.qspare) return 0u;
    const uint32_t want = nin / (grid * 16u), cap = W.qspare / grid;
    if (W.app_force) return W.app_force <= cap ? W.app_force : 0u;
    if (W.sort) return 0u;
    uint32_t c = 256u;
    while (c * 2u <= want && c * 2u <= cap && c < 4096u) c *= 2u;
    return c <= want && c <= cap ? c : 0u;
}

// One generation: what follows wf_shade(g) of a chunk of K bounces, given the two lengths read back.
struct WfQueueSort { bool sorted; int bits; }; // (bits: the significant key bits)
struct WfGenStep {
    uint32_t ns, nc; // shadow queue g; closest queue g + 1 (0 at g = K)
    bool next;       // closest g + 1 is its own launch on the side stream, beside shadow g
    // overlapped tail: the rest of the chunk starts on the side stream beside this generation's shadow trace, tracing
    // its own paths' shadow rays of generation g first; the shadow trace and wf_resolve take the paths that end at g
    // (ended_only).  Only for scenes with lights -- a hit whose NEE query was answered without a trace (nee_skip)
    // has no shadow ray, and the tail reads its NO_SLOT as "nothing to trace"
    bool overlap, ended_only;
    WfQueueSort shadow, closest;
    bool tail_after; // wf_tail(g + 1) on the main stream, after the join
    bool finished;   // no wf_shade(g + 1)
};
inline WfGenStep wf_gen_step(uint32_t g, uint32_t K, uint32_t ns, uint32_t nc_read, uint32_t nlights, const WfArgs &W,
                             const WfDriver &d) {
    WfGenStep s = {ns, g < K ? nc_read : 0u};
    s.next = s.nc >= W.tail_min && s.nc > 0;
    s.overlap = d.tail_overlap && !s.next && s.nc > 0 && W.tail_overlap && nlights > 0;
    s.ended_only = s.overlap;
    // queues shorter than sort_min are traced in append order; pixel keys need fewer bits than world keys
    const bool pixel = wf_pixel_keys(W.leaf_keys, W.world_keys, g);
    auto sorts = [&](uint32_t n, uint32_t g1_bit) {
        return W.sort && n >= W.sort_min && !(W.measure_skip & 2u) && (g > 1 || !d.sort_g1 || (W.sort_g1 & g1_bit));
    };
    s.shadow = {sorts(ns, 1u), pixel ? W.key_bits_pixel : W.key_bits_s};
    s.closest = {s.next && sorts(s.nc, 2u), pixel ? W.key_bits_pixel : W.key_bits};
    s.tail_after = !s.next && s.nc > 0 && !s.overlap;
    s.finished = !s.next;
    return s;
}

} // namespace cr
