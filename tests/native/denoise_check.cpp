// denoise_check.cpp -- csrc/denoise.hpp on the CPU (tests/test_denoise_abi.py): prints the defaults, the verdict of
// the validation on a list of cases, the level schedule for every level count and the scratch layout for a few
// frame sizes, one record per line; the test compares them with its own restatement.
#include "denoise.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

int main() {
    cr_denoise_params d{};
    cr::dn_defaults(d);
    std::printf("defaults %u %g %g %g %u\n", d.levels, d.sigma_l, d.sigma_z, d.sigma_a, d.normal_squarings);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    struct {
        const char *name;
        cr_denoise_params p;
    } cases[] = {
        {"default", d},
        {"levels0", {0, 4.f, .1f, .1f, 5}},
        {"levels8", {8, 4.f, .1f, .1f, 8}},
        {"levels9", {9, 4.f, .1f, .1f, 5}},
        {"squarings9", {4, 4.f, .1f, .1f, 9}},
        {"sigma_l0", {4, 0.f, .1f, .1f, 5}},
        {"sigma_z_neg", {4, 4.f, -.1f, .1f, 5}},
        {"sigma_a_nan", {4, 4.f, .1f, nan, 5}},
        {"sigma_l_inf", {4, inf, .1f, .1f, 5}},
        {"sigma_a_tiny", {4, 4.f, .1f, 1e-30f, 5}},
    };
    for (const auto &c : cases) std::printf("params %s %d\n", c.name, cr::dn_check_params(&c.p) ? 1 : 0);
    std::printf("params null %d\n", cr::dn_check_params(nullptr) ? 1 : 0);
    const uint32_t shapes[][4] = {{4, 4, 1, 1},      {0, 4, 1, 1},          {4, 0, 1, 1},     {4, 4, 0, 1},
                                  {4, 4, 1, 0},      {4, 4, 1u << 16, 1u << 16}, {4, 4, 65535, 65537}, {65536, 32768, 1, 1},
                                  {65536, 32769, 1, 1}};
    for (const auto &s : shapes)
        std::printf("shape %u %u %u %u %d\n", s[0], s[1], s[2], s[3], cr::dn_check_shape(s[0], s[1], s[2], s[3]) ? 1 : 0);
    for (uint32_t levels = 0; levels <= cr::DN_MAX_LEVELS; levels++) {
        std::printf("schedule %u", levels);
        for (const cr::DnLevel &L : cr::dn_levels(levels)) std::printf(" %u:%d:%d:%d", L.step, L.src, L.dst, L.lds ? 1 : 0);
        std::printf("\n");
    }
    const uint64_t sizes[] = {1, 7, 16, 17, 70 * 45, 1920 * 1080, 1ull << 31};
    for (uint64_t n : sizes)
        for (uint32_t levels : {0u, 1u, 2u, 5u}) {
            const cr::DnScratch s = cr::dn_scratch(n, levels);
            std::printf("scratch %llu %u %zu %zu %zu %zu\n", (unsigned long long)n, levels, s.guide, s.frame[0], s.frame[1],
                        s.bytes);
        }
    for (uint64_t n : sizes) {
        const cr::GuideScratch g = cr::guide_scratch(n);
        std::printf("guide %llu %zu %zu %zu %zu %zu %zu %zu\n", (unsigned long long)n, g.orig, g.dir, g.hit, g.tri, g.bary,
                    g.dist, g.bytes);
    }
    std::printf("denoise_check: ok\n");
    return 0;
}
