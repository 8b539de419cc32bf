// ctxopts.hpp -- every option of a cr_ctx and the one table that names, bounds and stores them (cr_set_option;
// "wf_side_priority", the one option with a side effect, is cabi.cpp's).  Plain data, no HIP runtime call: cr_ctx
// derives from CtxOptions, and tests/native/options_check.cpp walks the table without a device.
#pragma once
#include "kernels.hpp" // (wfbuilds.hpp, wfopts.hpp)

#include <cstring>

namespace cr {

// (the wavefront host path's options -- wf_*, sample_buf -- are the base struct: wfopts.hpp)
// Defaults from sweeps on MI355X, sponza stand-in 1080p x 128 spp: wavefront (kernel 2), the scene's
// default trace build (wfbuilds.hpp wf_default_build), refill 64/56/48, sorted queues, tail below 1M rays
// (the persistent megakernel, kernel 0: 615 Mray/s; one thread per pixel, kernel 1: ~60; both removed: DESIGN.md §3)
struct CtxOptions : WfOptions {
    int kernel = 2;
    int full_counters = 1;
    int lc_debug = 0;                      // measurement only (RenderArgs::lc_debug)
    uint32_t lc_min = 0;                   // RenderArgs::lc_min
    int desc_quorum = -1;                  // RenderArgs::desc_quorum; -1: 8, 0 (off) for SORT_MIN_TRIS <= tris < LEAF_CULL_MIN_TRIS
    uint32_t diag_kinds = 0;               // counting renders: trace kinds of the DIAG_* census (1 << TK_*)
    int perf_counters = 0;                 // RenderArgs::perf_counters (option "perf_counters")
    int variant = -1;       // -1: the kernel's default build
    uint32_t refill = 0;    // 0: the default (48)
    uint32_t refill_shadow = 0; // wavefront shadow trace; 0: refill if set, else 56
    uint32_t refill_camera = 0; // wavefront generation-1 closest trace; 0: refill if set, else 64
    uint32_t sum_lds = 0;           // launch_sum_samples' LDS reservation per block (occupancy cap)
    int sum_staged = 1;             // sum_samples_lds (sample runs staged through LDS) when aligned
    uint32_t node_bfs = NODE_BFS;   // nodes numbered breadth-first at the next cr_upload_scene
    uint32_t comm_timeout_ms = 120000; // cr_comm_init: peers must join within this (option "comm_timeout_ms")
    int query_route = 0;              // 0 automatic, 1 every query by the per-thread kernel, 2 no leaf-cull build
    int query_sort = -1; // -1 automatic (>= SORT_MIN_TRIS triangles, chunks >= QUERY_SORT_MIN = 2^22), 0 append, 1 sort
    uint32_t query_chunk = 1u << 24;  // queries per chunk (2^24 rays in chunks of 2^22: 13-27% slower)
    uint32_t query_trace_min = 1u << 16; // shorter batches: the per-thread kernel (the crossover)
};

// One row per option.  v is stored when lo <= v <= hi (RANGE); and v & (v - 1) == 0 (POW2: 0 passes where lo admits
// it); or v == 0 below such a range (POW2_OR_0); when v is lo or hi (ENDS: a set of two values); when
// lo <= v < num_wf_variants() (VARIANT, hi unused).  store: the cast to the field's own type.
enum OptRule { OPT_RANGE, OPT_POW2, OPT_POW2_OR_0, OPT_ENDS, OPT_VARIANT };
struct OptRow {
    const char *name;
    int64_t lo, hi;
    OptRule rule;
    void (*store)(CtxOptions &, int64_t);
};
#define CR_OPT(name, lo, hi, field, rule)                                                                             \
    OptRow { name, lo, hi, rule, [](CtxOptions &o, int64_t v) { o.field = (decltype(o.field))v; } }
static const OptRow kOptions[] = {
    CR_OPT("kernel", 2, 2, kernel, OPT_RANGE),
    CR_OPT("counters", 0, 1, full_counters, OPT_RANGE),
    CR_OPT("perf_counters", 0, 1, perf_counters, OPT_RANGE),
    CR_OPT("wf_tail_overlap", 0, 1, wf_tail_overlap, OPT_RANGE),
    CR_OPT("wf_sort_g1", 0, 3, wf_sort_g1, OPT_RANGE),
    CR_OPT("wf_cam_lean", 0, 1, wf_cam_lean, OPT_RANGE),
    CR_OPT("wf_cam_fuse", 0, 1, wf_cam_fuse, OPT_RANGE),
    CR_OPT("wf_ctl_ray", 0, 1, wf_ctl_ray, OPT_RANGE),
    CR_OPT("wf_vis_dw", 0, 1, wf_vis_dw, OPT_RANGE),
    CR_OPT("wf_vis_mark", 0, 1, wf_vis_mark, OPT_RANGE),
    CR_OPT("sum_lds", 0, 65536, sum_lds, OPT_RANGE),
    CR_OPT("wf_nee_skip", 0, 1, wf_nee_skip, OPT_RANGE),
    CR_OPT("sum_staged", 0, 1, sum_staged, OPT_RANGE),
    CR_OPT("wf_tail_waves", 4, 6, wf_tail_waves, OPT_RANGE),
    CR_OPT("diag_kinds", 0, 7, diag_kinds, OPT_RANGE),
    CR_OPT("lc_debug", 0, 2, lc_debug, OPT_RANGE),
    CR_OPT("lc_min", 0, 33, lc_min, OPT_RANGE),
    CR_OPT("desc_quorum", -1, 64, desc_quorum, OPT_RANGE),
    CR_OPT("comm_timeout_ms", 1, 3600000, comm_timeout_ms, OPT_RANGE),
    CR_OPT("variant", -1, 0, variant, OPT_VARIANT), // -1 default; clamped per kernel
    CR_OPT("refill", 0, 64, refill, OPT_RANGE), // 0: per-kernel default
    CR_OPT("refill_shadow", 0, 64, refill_shadow, OPT_RANGE),
    CR_OPT("refill_camera", 0, 64, refill_camera, OPT_RANGE),
    CR_OPT("wf_sort", -1, 1, wf_sort, OPT_RANGE),
    CR_OPT("wf_world_keys", 0, 64, wf_world_keys, OPT_RANGE),
    CR_OPT("wf_world_bits", 1, 10, wf_world_bits, OPT_RANGE),
    CR_OPT("wf_sort_min", 0, 1ll << 31, wf_sort_min, OPT_RANGE),
    CR_OPT("wf_tail_min", 0, 0xffffffffll, wf_tail_min, OPT_RANGE),
    CR_OPT("wf_sort_tile", 0, 5, wf_sort_tile, OPT_RANGE),
    CR_OPT("wf_dir_res", 1, 256, wf_dir_res, OPT_POW2),
    CR_OPT("wf_dir_res_shadow", 0, 256, wf_dir_res_shadow, OPT_POW2),
    CR_OPT("wf_paths", 4096, 1ll << 30, wf_paths, OPT_RANGE),
    CR_OPT("wf_lanes", 1, 2, wf_lanes, OPT_RANGE),
    CR_OPT("wf_xcd", 0, 7, wf_xcd, OPT_RANGE),
    CR_OPT("wf_leaf_keys", 0, 1, wf_leaf_keys, OPT_RANGE),
    CR_OPT("wf_resolve_paths", 0, 64, wf_resolve_paths, OPT_RANGE),
    CR_OPT("wf_measure_skip", 0, 3, wf_measure_skip, OPT_RANGE),
    CR_OPT("wf_shade_waves", 6, 8, wf_shade_waves, OPT_ENDS),
    CR_OPT("wf_shade_block", 256, 1024, wf_shade_block, OPT_POW2), // 256 | 512 | 1024
    CR_OPT("wf_app_chunk", 256, 65536, wf_app_chunk, OPT_POW2_OR_0),
    CR_OPT("wf_leaf_shift", 0, 24, wf_leaf_shift, OPT_RANGE),
    CR_OPT("wf_packet_unanimous", 0, 1, wf_packet_unanimous, OPT_RANGE),
    CR_OPT("node_bfs", 1, 1ll << 30, node_bfs, OPT_RANGE),
    CR_OPT("sample_buf_bytes", 1, 1ll << 40, sample_buf, OPT_RANGE),
    CR_OPT("query_route", 0, 2, query_route, OPT_RANGE),
    CR_OPT("query_sort", -1, 1, query_sort, OPT_RANGE),
    CR_OPT("query_chunk", 256, 1ll << 24, query_chunk, OPT_RANGE),
    CR_OPT("query_trace_min", 0, 0xffffffffll, query_trace_min, OPT_RANGE),
};
#undef CR_OPT

// Store v under `key` when the table has the key and its row accepts the value; false otherwise, nothing written.
inline bool set_option(CtxOptions &o, const char *key, int64_t v) {
    for (const OptRow &r : kOptions) {
        if (std::strcmp(key, r.name)) continue;
        const bool in = v >= r.lo && v <= r.hi, pow2 = (v & (v - 1)) == 0;
        const bool ok = r.rule == OPT_RANGE ? in : r.rule == OPT_POW2 ? in && pow2
                        : r.rule == OPT_POW2_OR_0 ? v == 0 || (in && pow2)
                        : r.rule == OPT_ENDS ? v == r.lo || v == r.hi : v >= r.lo && v < (int64_t)num_wf_variants();
        if (ok) r.store(o, v);
        return ok;
    }
    return false;
}

} // namespace cr
