// probe_check.cpp -- csrc/probe.hpp on the CPU (tests/test_probe_model.py):
//   probe_check args                 the argument checks of the probe entries
//   probe_check dirs <in> <out>      probe_dir and probe_basis over raw draw pairs: d [n][3], then Y [n][9]
//   probe_check fold <in> <out>      probe_fold_host per probe: sh [n][27], then m2 [n][27]
//   probe_check eval <in> <out>      probe_eval: out [m][3]
//   probe_check sample <in> <out>    probe_grid_positions, then probe_sample: positions [count][3], out [m][3]
// The case files are raw little-endian arrays written and read by the test, which compares the outputs with
// tests/probe_model.py bit for bit.  The sine and cosine are libm's, which the kernels restate.  Built with
// -DPROBE_NO_CLAMP the grid coordinate is not clamped: the test's comparison must then fail.
#include "probe.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

template <class T> static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return !n || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static void put(FILE *f, const T *v, size_t n) {
    if (n && std::fwrite(v, sizeof(T), n, f) != n) std::exit(3);
}

static int check_arguments() {
    const float inf = INFINITY, nan = NAN;
    // cr_probe_sh: the size of the coefficients (the other rules are rad_check's, tests/native/radiance_check.cpp)
    CHECK(!probe_check_size(0) && !probe_check_size(4) && !probe_check_size(0xffffffffu), "sound sizes");
    CHECK(says(probe_check_size(5, 134), "overflow") && !probe_check_size(4, 134) && !probe_check_size(5, 135),
          "27 n floats against the most an array holds");
    CHECK(says(probe_check_size(0xffffffffu, 0xffffffffu), "overflow"), "a 32-bit size");
    // the grid
    ProbeGrid g = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, {4, 3, 2}};
    CHECK(!probe_check_grid(&g) && probe_grid_count(g) == 24, "a sound grid");
    CHECK(says(probe_check_grid(nullptr), "null"), "null grid");
    for (int a = 0; a < 3; a++) {
        ProbeGrid b = g;
        b.dims[a] = 0;
        CHECK(says(probe_check_grid(&b), "dims"), "dims[%d] == 0", a);
        b = g, b.origin[a] = nan;
        CHECK(says(probe_check_grid(&b), "origin"), "origin[%d] NaN", a);
        b = g, b.origin[a] = -inf;
        CHECK(says(probe_check_grid(&b), "origin"), "origin[%d] inf", a);
        const float bad[4] = {0.f, -1.f, inf, nan};
        for (float s : bad) {
            b = g, b.step[a] = s;
            CHECK(says(probe_check_grid(&b), "step"), "step[%d] = %g", a, s);
            b.dims[a] = 1; // (an axis of one probe does not read its step)
            CHECK(!probe_check_grid(&b), "step[%d] = %g on an axis of one probe", a, s);
        }
    }
    ProbeGrid big = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, {65536, 65536, 1}};
    CHECK(says(probe_check_grid(&big), "too large"), "2^32 probes");
    big.dims[1] = 65535;
    CHECK(!probe_check_grid(&big), "2^32 - 65536 probes");
    ProbeGrid both = g;
    both.dims[0] = 0, both.origin[0] = nan, both.step[1] = 0.f;
    CHECK(says(probe_check_grid(&both), "dims"), "dims first");
    both.dims[0] = 4;
    CHECK(says(probe_check_grid(&both), "origin"), "then the origin");
    // the lookups
    float sh[24 * 27], out[3 * 8];
    CHECK(!probe_check_eval(8, true, sh, 24, out) && !probe_check_eval(0, false, nullptr, 0, nullptr), "sound eval");
    CHECK(says(probe_check_eval(8, false, sh, 24, out), "null"), "null arrays");
    CHECK(says(probe_check_eval(8, true, sh, 24, sh), "alias") && says(probe_check_eval(8, true, sh, 0, sh), "alias") &&
              says(probe_check_eval(8, true, sh, 24, sh + 23 * 27), "alias") && !probe_check_eval(8, true, sh, 1, sh + 27),
          "the output inside the coefficients");
    CHECK(!probe_check_sample(&g, 8, true, sh, out) && !probe_check_sample(&g, 0, false, nullptr, nullptr), "sound sample");
    CHECK(says(probe_check_sample(nullptr, 8, true, sh, out), "grid"), "null grid");
    CHECK(says(probe_check_sample(&both, 8, false, sh, sh), "origin"), "the grid first");
    CHECK(says(probe_check_sample(&g, 8, false, sh, sh), "null"), "then the arrays");
    CHECK(says(probe_check_sample(&g, 8, true, sh, sh + 24 * 27 - 1), "alias") && !probe_check_sample(&g, 8, true, sh, sh + 24 * 27),
          "the output against the grid's coefficients");
    if (!fails) std::printf("args ok\n");
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "args") return check_arguments();
    if (argc != 4) return 2;
    FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> hdr;
    if (mode == "dirs") {
        std::vector<uint32_t> raw;
        if (!get(in, hdr, 1) || !get(in, raw, 2 * (size_t)hdr[0])) return 2;
        const size_t n = hdr[0];
        std::vector<float> d(3 * n), Y(9 * n);
        for (size_t i = 0; i < n; i++) {
            probe_dir(raw[2 * i], raw[2 * i + 1], &d[3 * i]);
            probe_basis(d[3 * i], d[3 * i + 1], d[3 * i + 2], &Y[9 * i]);
        }
        put(out, d.data(), d.size());
        put(out, Y.data(), Y.size());
    } else if (mode == "fold") { // n, layers, spp, first layer; raw [n][layers][spp][2]; rad [n][layers][spp][3]
        std::vector<uint32_t> raw;
        std::vector<float> rad;
        if (!get(in, hdr, 4)) return 2;
        const size_t n = hdr[0], per = (size_t)hdr[1] * hdr[2];
        if (!get(in, raw, 2 * n * per) || !get(in, rad, 3 * n * per)) return 2;
        std::vector<float> sh(27 * n, 0.f), m2(27 * n, 0.f);
        for (size_t i = 0; i < n; i++)
            probe_fold_host(hdr[3], hdr[1], hdr[2], &raw[2 * i * per], &rad[3 * i * per], &sh[27 * i], &m2[27 * i]);
        put(out, sh.data(), sh.size());
        put(out, m2.data(), m2.size());
        // (without a moment array the coefficients are the same)
        std::vector<float> alone(27 * n, 0.f);
        for (size_t i = 0; i < n; i++)
            probe_fold_host(hdr[3], hdr[1], hdr[2], &raw[2 * i * per], &rad[3 * i * per], &alone[27 * i], nullptr);
        if (std::memcmp(alone.data(), sh.data(), sh.size() * sizeof(float))) return 4;
    } else if (mode == "eval") {
        std::vector<float> sh, nrm;
        if (!get(in, hdr, 1) || !get(in, sh, 27 * (size_t)hdr[0]) || !get(in, nrm, 3 * (size_t)hdr[0])) return 2;
        std::vector<float> o(3 * (size_t)hdr[0]);
        for (size_t j = 0; j < hdr[0]; j++) probe_eval(&sh[27 * j], &nrm[3 * j], &o[3 * j]);
        put(out, o.data(), o.size());
    } else if (mode == "sample") { // the grid (9 words), m; sh [count][27]; pos, nrm [m][3]
        ProbeGrid g;
        std::vector<float> sh, pos, nrm;
        if (std::fread(&g, sizeof g, 1, in) != 1 || probe_check_grid(&g) || !get(in, hdr, 1)) return 2;
        const size_t count = (size_t)probe_grid_count(g), m = hdr[0];
        if (!get(in, sh, 27 * count) || !get(in, pos, 3 * m) || !get(in, nrm, 3 * m)) return 2;
        std::vector<float> where(3 * count), o(3 * m);
        probe_grid_positions(g, where.data());
        for (size_t j = 0; j < m; j++) probe_sample(g, sh.data(), &pos[3 * j], &nrm[3 * j], &o[3 * j]);
        put(out, where.data(), where.size());
        put(out, o.data(), o.size());
    } else {
        return 2;
    }
    std::fclose(in);
    return std::fclose(out) ? 3 : 0;
}
