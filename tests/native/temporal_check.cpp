// temporal_check.cpp -- csrc/temporal.hpp on the CPU (tests/test_temporal_abi.py): prints the defaults, the verdict of
// the validation on a list of cases, the history layout for a few frame sizes and -- for each camera read from the
// standard input as 12 hexadecimal float bit patterns (eye, left_upper, dx, dy) -- the projector's bits, one record
// per line; the test compares them with its own restatement and with tests/temporal_model.py.
#include "temporal.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

int main() {
    cr_temporal_params d{};
    cr::tp_defaults(d);
    std::printf("defaults %.9g %.9g %u\n", d.depth_tol, d.normal_min, d.max_history);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    struct {
        const char *name;
        cr_temporal_params p;
    } cases[] = {
        {"default", d},
        {"tol_tiny", {1e-30f, .9f, 1}},
        {"tol0", {0.f, .9f, 65536}},
        {"tol_neg", {-.05f, .9f, 65536}},
        {"tol_nan", {nan, .9f, 65536}},
        {"tol_inf", {inf, .9f, 65536}},
        {"nmin_neg", {.05f, -2.f, 65536}},
        {"nmin_nan", {.05f, nan, 65536}},
        {"nmin_inf", {.05f, inf, 65536}},
        {"nmin_ninf", {.05f, -inf, 65536}},
        {"hist0", {.05f, .9f, 0}},
        {"hist_max", {.05f, .9f, 0xFFFFFFFFu}},
    };
    for (const auto &c : cases) std::printf("params %s %d\n", c.name, cr::tp_check_params(&c.p) ? 1 : 0);
    std::printf("params null %d\n", cr::tp_check_params(nullptr) ? 1 : 0);
    const uint32_t shapes[][2] = {{4, 4}, {0, 4}, {4, 0}, {1, 1}, {65536, 32768}, {65536, 32769}};
    for (const auto &s : shapes) std::printf("shape %u %u %d\n", s[0], s[1], cr::tp_check_shape(s[0], s[1]) ? 1 : 0);
    const uint64_t sizes[] = {1, 7, 16, 17, 70 * 45, 1920 * 1080, 1ull << 31};
    for (uint64_t n : sizes)
        for (int packed = 0; packed < 2; packed++) {
            const cr::TpScratch s = cr::tp_scratch(n, packed != 0);
            std::printf("scratch %llu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", (unsigned long long)n, packed,
                        s.frame, s.m2, s.count, s.normal, s.depth, s.rec, s.side, s.cur_frame, s.cur_m2, s.cur_albedo,
                        s.bytes);
        }
    unsigned w[12];
    while (std::scanf("%x %x %x %x %x %x %x %x %x %x %x %x", w, w + 1, w + 2, w + 3, w + 4, w + 5, w + 6, w + 7, w + 8,
                      w + 9, w + 10, w + 11) == 12) {
        cr_camera cam{};
        float f[12];
        static_assert(sizeof(unsigned) == sizeof(float), "bit patterns");
        std::memcpy(f, w, sizeof(f));
        std::memcpy(cam.eye, f, 12);
        std::memcpy(cam.left_upper, f + 3, 12);
        std::memcpy(cam.dx, f + 6, 12);
        std::memcpy(cam.dy, f + 9, 12);
        cr::TpProjector p;
        const bool ok = cr::tp_projector(cam, p);
        float o[10];
        std::memcpy(o, p.ra, 12), std::memcpy(o + 3, p.rb, 12), std::memcpy(o + 6, p.rc, 12), o[9] = p.det;
        unsigned b[10];
        std::memcpy(b, o, sizeof(o));
        std::printf("projector %d", ok ? 1 : 0);
        for (unsigned v : b) std::printf(" %08x", v);
        std::printf("\n");
    }
    std::printf("temporal_check: ok\n");
    return 0;
}
