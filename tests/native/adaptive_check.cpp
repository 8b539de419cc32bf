// adaptive_check.cpp -- csrc/adaptive.hpp on the CPU (tests/test_adaptive_host.py):
//   * the check schedule of cr_render_adaptive over small ranges of min_layers / check_every / max_layers, against
//     the rule restated here: checks at the multiples of check_every that are >= min_layers, and at max_layers;
//   * the pass plan of a list render for list lengths 0, 1, 1023, 1024, 1025 (and more) under caps that force splits
//     by list range, by layers and by both: every (entry, layer) covered exactly once with a pixel's layers
//     ascending, every pass one path chunk and one sample buffer (wf_layers_fit) unless it is the smallest pass there
//     is -- one layer of at most one tile of entries.
// With -DMUTATE the plan under check has its first pass's range shortened by one entry: the cover check must fail.
#include "adaptive.hpp"

#include <cstdio>
#include <vector>

using namespace cr;

static int fails = 0;
#define CHECK(cond, ...)                                                                                              \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (fails++ < 10) std::printf("FAIL %s: ", #cond), std::printf(__VA_ARGS__), std::printf("\n");          \
        }                                                                                                            \
    } while (0)

static void check_schedule() {
    int cases = 0;
    for (uint32_t maxl = 1; maxl <= 9; maxl++)
        for (uint32_t minl = 0; minl <= maxl; minl++)
            for (uint32_t every = 1; every <= maxl + 2; every++) { // (check_every > max_layers included)
                std::vector<uint32_t> want;
                for (uint32_t L = 1; L <= maxl; L++)
                    if ((L % every == 0 && L >= minl) || L == maxl) want.push_back(L);
                const std::vector<uint32_t> got = ad_checks(minl, maxl, every);
                CHECK(got == want, "schedule min %u max %u every %u", minl, maxl, every);
                // the steps themselves: never past max_layers, never more than check_every layers
                for (uint32_t L = 0; L < maxl;) {
                    const AdStep s = ad_step(L, minl, maxl, every);
                    CHECK(s.n >= 1 && s.n <= every && L + s.n <= maxl, "step at %u", L);
                    L += s.n;
                }
                cases++;
            }
    std::printf("schedule cases %d\n", cases);
}

// true: the plan covers every (entry, layer) of in exactly once, layers ascending per entry, every pass sound
static bool plan_ok(const AdPlanIn &in, const std::vector<AdPass> &plan, bool say) {
    std::vector<uint32_t> next((size_t)in.m, 0u); // the next layer each entry expects
    bool ok = true;
    auto bad = [&](const char *what, const AdPass &p) {
        if (say && ok) std::printf("  plan m %u n %u: %s at pass {%u, %u, %u, %u}\n", in.m, in.n, what, p.first, p.count, p.layer0, p.nl);
        ok = false;
    };
    for (const AdPass &p : plan) {
        if (!p.count || !p.nl || (uint64_t)p.first + p.count > in.m || p.layer0 + p.nl > in.n) {
            bad("range", p);
            continue;
        }
        if (p.nl > std::max(in.max_nl, 1u)) bad("more layers than a pass may hold", p);
        const bool smallest = p.nl == 1 && p.count <= in.tile * in.tile;
        if (!ad_pass_fits(in, p) && !smallest) bad("does not fit", p);
        if (ad_padded(p.count, in.tile) % ((uint64_t)in.tile * in.tile) || ad_padded(p.count, in.tile) < p.count) bad("padding", p);
        for (uint32_t i = p.first; i < p.first + p.count; i++) {
            if (next[i] != p.layer0) bad("layer order", p);
            next[i] = p.layer0 + p.nl;
        }
    }
    for (uint32_t i = 0; i < in.m; i++)
        if (next[i] != in.n) {
            if (say && ok) std::printf("  plan m %u n %u: entry %u ends at layer %u\n", in.m, in.n, i, next[i]);
            ok = false;
        }
    if (!in.m || !in.n) ok = ok && plan.empty();
    return ok;
}

int main() {
    check_schedule();
    const uint32_t lens[] = {0, 1, 1023, 1024, 1025, 4097, 70000};
    const uint32_t tiles[] = {32, 8};
    struct Caps { uint64_t paths, sbuf; const char *what; };
    int plans = 0, split_range = 0, split_layers = 0, split_both = 0, whole = 0;
    for (uint32_t m : lens)
        for (uint32_t tile : tiles)
            for (uint32_t spp : {1u, 4u, 5u})
                for (uint32_t n : {0u, 1u, 2u, 6u, 40u})
                    for (uint32_t max_nl : {1u, 32u}) {
                        const uint64_t TT = (uint64_t)tile * tile;
                        const Caps caps[] = {
                            {~0ull, 4ull << 30, "roomy"},
                            {2 * TT * spp, 4ull << 30, "paths: two tiles of one layer"},
                            {~0ull, 12 * TT * spp * 3, "samples: one tile of three layers"},
                            {ad_padded(m, tile) * spp * 2, 4ull << 30, "paths: the list of two layers"},
                            {3 * TT * spp * 2, 12 * TT * spp * 2 * 2, "both"},
                            {TT * spp / 2 + 1, 4ull << 30, "less than one tile of one layer"},
                        };
                        for (const Caps &c : caps) {
                            AdPlanIn in;
                            in.m = m, in.n = n, in.spp = spp, in.tile = tile, in.max_nl = max_nl;
                            in.paths_cap = c.paths, in.sample_buf = c.sbuf;
                            std::vector<AdPass> plan = ad_plan(in);
#ifdef MUTATE
                            if (!plan.empty() && plan[0].count > 0) plan[0].count--; // an off-by-one range
#endif
                            if (!plan_ok(in, plan, fails < 10)) {
                                if (fails++ < 10) std::printf("FAIL plan m %u tile %u spp %u n %u max_nl %u (%s)\n", m, tile, spp, n, max_nl, c.what);
                            }
                            plans++;
                            bool ranges = false, layers = false;
                            for (const AdPass &p : plan) ranges |= p.count < m, layers |= p.nl < n;
                            split_range += ranges && !layers, split_layers += layers && !ranges;
                            split_both += ranges && layers, whole += !plan.empty() && !ranges && !layers;
                        }
                    }
    std::printf("plans %d whole %d split_range %d split_layers %d split_both %d\n", plans, whole, split_range, split_layers,
                split_both);
    CHECK(whole > 0 && split_range > 0 && split_layers > 0 && split_both > 0, "every kind of plan occurs");
    std::printf(fails ? "adaptive_check: %d failures\n" : "adaptive_check: ok\n", fails);
    return fails ? 1 : 0;
}
