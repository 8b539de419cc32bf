// radiance.hpp -- the host plan of a radiance query (cr_radiance_device / cr_gather_device), as pure functions in
// the style of adaptive.hpp: the argument check, and how the plan of a list render (ad_plan) becomes ray passes.
// Nothing here calls the HIP runtime; tests/native/radiance_check.cpp runs all of it on the CPU.
#pragma once
#include "adaptive.hpp"

namespace cr {

// The argument check of the four entry points, in the order the messages name: null (or the first bad value's text)
// means CR_E_INVALID; nullptr: the arguments are sound.  arrays: both input arrays and the output are given
// (n == 0 needs none of them).
inline const char *rad_check(uint32_t n, bool arrays, bool have_params, uint32_t spp, int32_t k, uint32_t layer,
                             uint32_t id0, uint32_t nlayers) {
    if (!have_params) return "null radiance params";
    if (n && !arrays) return "null ray / output arrays";
    if (spp == 0) return "spp must be > 0";
    if (k < 1 || k > 64) return "k must be in [1, 64]";
    if (layer < 1) return "layer must be >= 1";
    if (nlayers < 1) return "no layers";
    if ((uint64_t)id0 + n > 0xffffffffull) return "id0 + n must not exceed 0xffffffff";
    if ((uint64_t)layer + nlayers - 1 > 0xffffffffull) return "layer + nlayers - 1 must fit 32 bits";
    return nullptr;
}

// ... and what the list forms add (cr_radiance_list_device / cr_gather_list_device), after rad_check: the arrays are
// the n x 1 frame of a list pass, so n is bounded as a frame's pixels are
inline const char *rad_check_list(uint32_t n, uint32_t n_list, bool have_list) {
    if (n_list && !have_list) return "null list";
    if (n_list > (1u << 31)) return "list too long";
    if (n > (1u << 31)) return "a list call's arrays hold at most 2^31 entries";
    return nullptr;
}

// A ray pass: entries [first, first + count) of the call's arrays as an n x 1 "frame" of `count` pixels whose work
// items are `items` (the entries padded to whole tiles); entry e of the pass draws from stream id0 + e and its
// arrays start `first` rays into the caller's (3 * first floats).
struct RadPass {
    uint32_t first, count, items;
    uint32_t id0;   // stream id of the pass's entry 0
    uint32_t layer; // the pass's first layer
    uint32_t nl;    // ... and its layers
};
inline RadPass rad_pass(const AdPass &p, uint32_t tile, uint32_t id0, uint32_t layer) {
    return {p.first, p.count, (uint32_t)ad_padded(p.count, tile), id0 + p.first, layer + p.layer0, p.nl};
}
// the plan's input: n rays, nlayers layers, one tile edge for the padding (32: the render's default)
enum : uint32_t { RAD_TILE = 32 };
inline AdPlanIn rad_plan_in(uint32_t n, uint32_t nlayers, uint32_t spp, uint32_t max_nl, uint64_t paths_cap,
                            uint64_t sample_buf) {
    AdPlanIn in;
    in.m = n, in.n = nlayers, in.spp = spp, in.tile = RAD_TILE, in.max_nl = max_nl;
    in.paths_cap = paths_cap, in.sample_buf = sample_buf;
    return in;
}

} // namespace cr
