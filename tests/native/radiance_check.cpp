// radiance_check.cpp -- csrc/radiance.hpp on the CPU (tests/test_radiance_host.py):
//   * rad_check: every CR_E_INVALID case of the radiance entries and their order, the id and layer ranges at their
//     last sound value and one past it;
//   * the ray passes of a call (ad_plan through rad_plan_in / rad_pass) for ray counts 1, 63, 64, 65, 257, 1025,
//     4097 and 70000 under caps that force splits by batch, by layers and by both: every (ray, layer) exactly once
//     with a ray's layers ascending, every pass's stream ids id0 + first .. and its array offset `first`, its work
//     items whole tiles that hold its rays, id0 + n never wrapping.
// With -DMUTATE every pass's first stream id is one too high: the id check must fail.
#include "radiance.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace cr;

static int fails = 0;
#define CHECK(cond, ...)                                                                                              \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (fails++ < 10) std::printf("FAIL %s: ", #cond), std::printf(__VA_ARGS__), std::printf("\n");          \
        }                                                                                                            \
    } while (0)

static bool says(const char *msg, const char *part) { return msg && std::strstr(msg, part); }

static void check_arguments() {
    // sound: n rays, arrays, params, spp 4, k 6, layer 1, id0 0, 3 layers
    CHECK(!rad_check(257, true, true, 4, 6, 1, 0, 3), "sound arguments");
    CHECK(!rad_check(0, false, true, 4, 6, 1, 0, 3), "n == 0 needs no arrays");
    CHECK(says(rad_check(257, true, false, 4, 6, 1, 0, 3), "params"), "null params");
    CHECK(says(rad_check(1, false, true, 4, 6, 1, 0, 3), "arrays"), "null arrays");
    CHECK(says(rad_check(1, true, true, 0, 6, 1, 0, 3), "spp"), "spp 0");
    CHECK(says(rad_check(1, true, true, 4, 0, 1, 0, 3), "k"), "k 0");
    CHECK(says(rad_check(1, true, true, 4, 65, 1, 0, 3), "k"), "k 65");
    CHECK(says(rad_check(1, true, true, 4, -1, 1, 0, 3), "k"), "k -1");
    CHECK(!rad_check(1, true, true, 4, 1, 1, 0, 3) && !rad_check(1, true, true, 4, 64, 1, 0, 3), "k 1 and 64");
    CHECK(says(rad_check(1, true, true, 4, 6, 0, 0, 3), "layer"), "layer 0");
    CHECK(says(rad_check(1, true, true, 4, 6, 1, 0, 0), "layers"), "nlayers 0");
    // id0 + n <= 0xffffffff
    CHECK(!rad_check(1, true, true, 4, 6, 1, 0xfffffffeu, 1), "the last id");
    CHECK(says(rad_check(2, true, true, 4, 6, 1, 0xfffffffeu, 1), "id0"), "one id too many");
    CHECK(says(rad_check(0xffffffffu, true, true, 4, 6, 1, 1, 1), "id0"), "n at its largest, id0 1");
    CHECK(!rad_check(0xffffffffu, true, true, 4, 6, 1, 0, 1), "n at its largest, id0 0");
    CHECK(!rad_check(0, false, true, 4, 6, 1, 0xffffffffu, 1), "no rays at the last id");
    // the last layer fits 32 bits
    CHECK(!rad_check(1, true, true, 4, 6, 0xffffffffu, 0, 1), "the last layer");
    CHECK(says(rad_check(1, true, true, 4, 6, 0xffffffffu, 0, 2), "nlayers"), "one layer too many");
    // the order: params, arrays, spp, k, layer, nlayers, ids
    CHECK(says(rad_check(1, false, false, 0, 0, 0, 0, 0), "params"), "params first");
    CHECK(says(rad_check(1, false, true, 0, 0, 0, 0, 0), "arrays"), "then the arrays");
    CHECK(says(rad_check(1, true, true, 0, 0, 0, 0, 0), "spp"), "then spp");
    CHECK(says(rad_check(1, true, true, 1, 0, 0, 0, 0), "k"), "then k");
    CHECK(says(rad_check(2, true, true, 1, 1, 0, 0xffffffffu, 0), "layer must"), "then the layer");
    CHECK(says(rad_check(2, true, true, 1, 1, 1, 0xffffffffu, 0), "no layers"), "then the layer count");
}

int main() {
    check_arguments();
    const uint32_t counts[] = {1, 63, 64, 65, 257, 1025, 4097, 70000};
    int plans = 0, whole = 0, split_batch = 0, split_layers = 0, split_both = 0;
    for (uint32_t n : counts)
        for (uint32_t spp : {1u, 4u, 5u})
            for (uint32_t nlayers : {1u, 3u, 40u})
                for (uint32_t max_nl : {1u, 32u})
                    for (uint32_t id0 : {0u, 100u, 0xffffffffu - n}) {
                        const uint64_t TT = (uint64_t)RAD_TILE * RAD_TILE;
                        const uint64_t caps[][2] = {{~0ull, 4ull << 30},
                                                    {2 * TT * spp, 4ull << 30},
                                                    {~0ull, 12 * TT * spp * 3},
                                                    {3 * TT * spp * 2, 12 * TT * spp * 2 * 2},
                                                    {TT * spp / 2 + 1, 4ull << 30}};
                        for (const auto &cap : caps) {
                            const uint32_t layer = 1 + (id0 & 3u);
                            const AdPlanIn in = rad_plan_in(n, nlayers, spp, max_nl, cap[0], cap[1]);
                            CHECK(in.m == n && in.n == nlayers && in.spp == spp && in.tile == RAD_TILE, "plan input");
                            std::vector<uint32_t> next((size_t)n, layer);
                            bool batches = false, layers = false;
                            for (const AdPass &ap : ad_plan(in)) {
                                RadPass ps = rad_pass(ap, in.tile, id0, layer);
#ifdef MUTATE
                                ps.id0++;
#endif
                                CHECK(ps.count >= 1 && (uint64_t)ps.first + ps.count <= n, "range of pass at %u", ps.first);
                                CHECK(ps.items >= ps.count && ps.items % TT == 0 && ps.items - ps.count < TT,
                                      "items %u of %u rays", ps.items, ps.count);
                                CHECK((uint64_t)ps.id0 == (uint64_t)id0 + ps.first, "stream id %u of ray %u, id0 %u", ps.id0,
                                      ps.first, id0);
                                CHECK((uint64_t)ps.id0 + ps.count - 1 <= 0xffffffffull, "ids wrap at ray %u", ps.first);
                                CHECK(ps.nl >= 1 && ps.nl <= (max_nl > 1 ? max_nl : 1u), "layers of a pass");
                                const bool smallest = ps.nl == 1 && ps.count <= TT;
                                CHECK(smallest || wf_layers_fit(ps.items, spp, ps.nl, cap[0], cap[1]), "pass at %u fits",
                                      ps.first);
                                for (uint32_t i = ps.first; i < ps.first + ps.count && i < n; i++) {
                                    CHECK(next[i] == ps.layer, "ray %u: layer %u, expected %u", i, ps.layer, next[i]);
                                    next[i] = ps.layer + ps.nl;
                                }
                                batches |= ps.count < n, layers |= ps.nl < nlayers;
                            }
                            for (uint32_t i = 0; i < n; i++)
                                CHECK(next[i] == layer + nlayers, "ray %u ends at layer %u", i, next[i]);
                            plans++;
                            whole += !batches && !layers, split_batch += batches && !layers;
                            split_layers += layers && !batches, split_both += batches && layers;
                        }
                    }
    std::printf("plans %d whole %d split_batch %d split_layers %d split_both %d\n", plans, whole, split_batch, split_layers,
                split_both);
    CHECK(whole > 0 && split_batch > 0 && split_layers > 0 && split_both > 0, "every kind of plan occurs");
    std::printf(fails ? "radiance_check: %d failures\n" : "radiance_check: ok\n", fails);
    return fails ? 1 : 0;
}
