// wfopts.hpp -- the options of the wavefront render's host path: what the pass plan (wfplan.hpp) and the
// WfArgs of a chunk are made from.  Plain data, no HIP or RCCL include: cr_ctx (ctx.hpp) derives from it, so
// c->wf_paths and the rest read as ever, and the plan's CPU check (tests/native/wfplan_check.cpp) fills one
// without a device.  Defaults from sweeps on MI355X, sponza stand-in 1080p x 128 spp.
#pragma once
#include <stdint.h>

namespace cr {

// Sample buffer budget: a render is split into sample chunks whose per-sample
// buffer fits in this many bytes (whole 1080p x 128 spp frames fit in one).
enum : uint64_t { SAMPLE_BUF_BYTES = 4ull << 30 };

struct WfOptions {
    uint32_t wf_paths = 256u << 20; // wavefront: paths in flight per chunk (capped by free HBM)
    int wf_sort = -1;               // wavefront: sort large shadow / secondary queues for coherence (-1: scenes
                                    // of at least SORT_MIN_TRIS triangles, wfplan.hpp)
    uint32_t wf_sort_min = 1u << 20; // ... of at least this many rays
    // sweep (1080p x 128 spp, refill 56): no sort 807; (8x8 px, 8x8 dirs) 891; (16x16, 16x16) 912;
    // (16x16, 32x32 Morton) 930; (32x32, 32x32) 914 Mray/s
    uint32_t wf_sort_tile = 4;      // key: log2 pixel sub-tile edge
    // direction bins per octahedral axis: 32 -> 64 575.6 -> 570.2 ms per pass, rank 0 of 8 79.6 -> 78.0
    // (world bits 5 / 7 and 16 bins measured slower; 7 bits x 64 bins: 31-bit keys, 607 ms)
    uint32_t wf_dir_res = 128;      // key: direction bins per octahedral axis (round 3: 128 at leaf shift 1,
                                    // 365.1 vs 367.1 ms per pass; halved for leaf keys until they fit 32 bits)
    int wf_world_keys = 2;          // key: world-space origins for queues starting at hits of gen >= 2
    uint32_t wf_world_bits = 6;     // key: Morton bits per axis of the origin
    // closest queues shorter than this finish in one wf_tail launch (0: never).  Sweep, sponza
    // 1080p x 128 spp: 0 / 256K / 1M / 4M / 16M -> 594.7 / 591.6 / 590.2 / 592.9 / 626.5 ms;
    // rank 0 of an 8-way split: 0 / 64K / 256K / 1M / 4M -> 88.8 / 85.9 / 83.3 / 83.1 / 84.2 ms
    uint32_t wf_tail_min = 1u << 20;
    // the tail starts beside the last shadow trace (WfArgs::tail_overlap); measured neutral (round 3:
    // 366.5 / 367.2 vs 366.9 / 366.8 ms per pass, rank 0 of 8 57.25 vs 57.36 ms -- the tail's chains
    // gain one shadow query each and share the GPU with that trace), so off by default
    int wf_tail_overlap = 0;
    uint32_t wf_sort_g1 = 3;        // generation-1 queues sorted: bit 0 shadow, bit 1 closest (WfArgs::sort_g1)
    int wf_cam_lean = 1;            // WfArgs::cam_lean
    // WfArgs::cam_fused (no wf_camera: the packet trace makes the rays) and WfArgs::ctl_ray (the RNG
    // counter in the closest ray, no control slot for generations >= 2); round 4, two interleaved rounds,
    // ms per layer: sponza 1080p x 128 spp 321.8 / 322.3 -> fused 320.1 / 320.5 -> both 318.8 / 319.4;
    // cornell_box 1024^2 x 500 spp 112.9 / 112.4 -> both 108.5 / 106.0 (C2 moves path state, not rays)
    int wf_cam_fuse = 1;
    int wf_ctl_ray = 1;
    // WfArgs::vis_dw; round 4, two interleaved rounds: sponza 318.1 / 317.9 -> 318.0 / 318.3 ms per layer,
    // cornell_box 105.7 / 106.1 -> 105.1 / 105.1 ms per pass
    int wf_vis_dw = 1;
    // WfArgs::vis_mark (round 5)
    int wf_vis_mark = 1;
    // WfArgs::nee_skip; round 4, two interleaved rounds: sponza 316.6 / 317.0 -> 293.7 / 293.1 ms per
    // layer, cornell_box 103.2 / 102.3 -> 95.1 / 95.3 ms per pass, nanobox 144.6 / 145.0 -> 142.9 / 143.0
    int wf_nee_skip = 1;
    int wf_tail_waves = 4;          // WfArgs::tail_waves
    uint32_t wf_dir_res_shadow = 0; // shadow queues' direction bins per axis with leaf keys (0: wf_dir_res)
    // per-sample buffer budget of one sample chunk (cr_set_option "sample_buf_bytes"); a
    // render whose n_items * 12 B * spp exceeds it runs in sample chunks whose running sum
    // carries over in d_run (sum_samples) -- the 4K x 100 spp batches of C5 do
    uint64_t sample_buf = SAMPLE_BUF_BYTES;
    int wf_lanes = 1;                 // wavefront chunks in flight at once (1 or 2)
    // XCD-partitioned queues (WfArgs::xcd bits: 1 shadow, 2 secondary closest, 4 camera rays);
    // sponza 1080p x 128 spp, 2 interleaved rounds: 0 / 1 / 3 / 7 -> 435.1 / 432.4 / 431.4 / 423.1 ms
    // per pass (build 15); build 17: 429.3 -> 416.5 ms with 7
    uint32_t wf_xcd = 7;
    // queue keys from the starting hit's kd leaf (WfArgs::leaf_keys), sponza 1080p x 128 spp,
    // 2 interleaved rounds: pixel / world keys 409.5 -> leaf keys 396.4 ms per pass; coarser
    // regions (node index >> 3 / 6 / 9) 405.2 / 418.7 / 440.2 vs 401.6 ms, 32 direction bins 409.3
    int wf_leaf_keys = 1;
    uint32_t wf_leaf_shift = 1; // ... its node index >> this (a leaf and its sibling share a key region)
    // sweep (1080p x 128 spp, 2 rounds): 0 / 1 / 2 / 4 / 8 / 16 / 64 -> 399.2 / 394.6 / 394.8 / 394.8 / 393.8 / 393.6 / 394.5 ms
    uint32_t wf_resolve_paths = 16; // wf_resolve in path order for queues of at least P / this rays (0: never)
    uint32_t wf_measure_skip = 0;   // WfArgs::measure_skip (measurement only: wrong images)
    // WfArgs::shade_waves (option "wf_shade_waves": 6 or 8); round 4, two interleaved rounds: sponza
    // 322.5 / 322.9 vs 322.6 / 322.2 ms per layer, cornell_box 108.4 / 108.7 vs 107.6 / 107.3 ms per pass
    int wf_shade_waves = 8;
    // wf_shade's append chunk (WfArgs::app_force): 0 = by the queue's length (launch_wavefront_chunk), else
    // this power of two >= 256 whenever the queue arrays have room (tests: the dead entries at small sizes)
    int wf_app_chunk = 0;
    // WfArgs::shade_block (option "wf_shade_block"): threads per wf_shade block, i.e. rays per queue append on
    // sorted queues (round 5, sponza stand-in, two interleaved rounds: 256 -> 2270.9 / 2276.0, 512 -> 2313.8 /
    // 2314.6, 1024 -> 2318.1 / 2314.2 Mray/s -- the same-address append atomics, scripts/append_bench.hip)
    int wf_shade_block = 1024;
    // WfArgs::packet_unanimous (option "wf_packet_unanimous"): the camera packet decides unanimous kd steps once
    // per packet; 0: every step per lane -- the same image and counters
    int wf_packet_unanimous = 1;
};

} // namespace cr
