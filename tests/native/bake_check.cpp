// bake_check.cpp -- csrc/bake.hpp on the CPU (tests/test_bake_model.py):
//   bake_check args                   the argument checks of the bake entries and of the grid atlas
//   bake_check surface <in> <out>     bake_surface_host over a case file: owner, pos, nrm, count, list
//   bake_check dilate <in> <out>      bake_dilate_host over a case file
//   bake_check atlas <n> <cell> <gutter> <out>   bake_atlas_grid: W, H, the UVs
// The case files are raw little-endian arrays written and read by the test, which compares the outputs with
// tests/bake_model.py bit for bit.  Built with -D'BAKE_EDGE_IN(w)=((w)>0.f)' the coverage rule is the exclusive one:
// the test's comparison must then fail.
#include "bake.hpp"

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
    CHECK(!bake_check_map(1, 1) && !bake_check_map(1u << 31, 1) && !bake_check_map(65536, 32768), "sound maps");
    CHECK(says(bake_check_map(0, 4), "> 0") && says(bake_check_map(4, 0), "> 0"), "an empty map");
    CHECK(says(bake_check_map(65536, 32769), "2^31") && says(bake_check_map(0xffffffffu, 0xffffffffu), "2^31"),
          "a map above 2^31 texels");
    CHECK(!bake_check_surface(true, 7, 5, 0.001f, true) && !bake_check_surface(true, 7, 5, 0.f, true) &&
              !bake_check_surface(true, 7, 5, -1.f, true),
          "sound surface arguments");
    CHECK(says(bake_check_surface(false, 7, 5, 0.001f, true), "params"), "null params");
    CHECK(says(bake_check_surface(true, 0, 5, 0.001f, true), "> 0"), "W == 0");
    CHECK(says(bake_check_surface(true, 7, 5, inf, true), "offset") && says(bake_check_surface(true, 7, 5, nan, true), "offset"),
          "an offset that is not finite");
    CHECK(says(bake_check_surface(true, 7, 5, 0.001f, false), "null"), "null outputs");
    // the order: params, the map, the offset, the pointers
    CHECK(says(bake_check_surface(false, 0, 0, nan, false), "params"), "params first");
    CHECK(says(bake_check_surface(true, 0, 0, nan, false), "> 0"), "then the map");
    CHECK(says(bake_check_surface(true, 1, 1, nan, false), "offset"), "then the offset");
    CHECK(!bake_check_sampling(1, 1, 1) && !bake_check_sampling(4, 64, 1000), "sound sampling");
    CHECK(says(bake_check_sampling(0, 6, 1), "spp") && says(bake_check_sampling(1, 0, 1), "k") &&
              says(bake_check_sampling(1, 65, 1), "k") && says(bake_check_sampling(1, 6, 0), "layers") &&
              says(bake_check_sampling(65536, 6, 65536), "32 bits"),
          "bad sampling");
    CHECK(!bake_check_dilate(65, 63, true, false), "sound dilation");
    CHECK(says(bake_check_dilate(0, 63, true, false), "> 0") && says(bake_check_dilate(65, 63, false, false), "null") &&
              says(bake_check_dilate(65, 63, true, true), "alias"),
          "bad dilation");
    CHECK(bake_dilate_passes(65, 63, 3) == 3 && bake_dilate_passes(65, 63, 0) == 0 &&
              bake_dilate_passes(65, 63, 0xffffffffu) == 65,
          "the passes that can change anything");
    CHECK(!bake_atlas_check(36, 4, 0.25f) && !bake_atlas_check(1, 1, 0.f), "sound atlas");
    CHECK(says(bake_atlas_check(0, 4, 0.25f), "no triangles") && says(bake_atlas_check(36, 0, 0.25f), "cell") &&
              says(bake_atlas_check(36, 4, 2.f), "gutter") && says(bake_atlas_check(36, 4, -0.1f), "gutter") &&
              says(bake_atlas_check(36, 4, nan), "gutter") && says(bake_atlas_check(1u << 20, 1u << 10, 0.25f), "2^31"),
          "bad atlas");
    uint32_t W = 0, H = 0;
    bake_atlas_grid(36, 4, 0.25f, &W, &H, nullptr);
    CHECK(W == 24 && H == 24, "36 triangles at cell 4: %u x %u", W, H);
    bake_atlas_grid(37, 4, 0.25f, &W, &H, nullptr);
    CHECK(W == 28 && H == 24, "37 triangles at cell 4: %u x %u", W, H);
    bake_atlas_grid(1, 5, 0.25f, &W, &H, nullptr);
    CHECK(W == 5 && H == 5, "one triangle at cell 5: %u x %u", W, H);
    std::printf(fails ? "bake_check: %d failures\n" : "bake_check: ok\n", fails);
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "args") return check_arguments();
    if (mode == "atlas" && argc == 6) {
        const uint32_t n = (uint32_t)std::atoi(argv[2]), cell = (uint32_t)std::atoi(argv[3]);
        const float g = (float)std::atof(argv[4]);
        if (bake_atlas_check(n, cell, g)) return 2;
        uint32_t wh[2];
        std::vector<float> uv(6 * (size_t)n);
        bake_atlas_grid(n, cell, g, &wh[0], &wh[1], uv.data());
        FILE *o = std::fopen(argv[5], "wb");
        if (!o) return 2;
        put(o, wh, 2), put(o, uv.data(), uv.size());
        return std::fclose(o) ? 3 : 0;
    }
    if ((mode != "surface" && mode != "dilate") || argc != 4) return std::printf("usage: see the file's head\n"), 2;
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    uint32_t h[3];
    if (std::fread(h, 4, 3, f) != 3) return 2;
    if (mode == "surface") {
        const uint32_t nt = h[0], W = h[1], H = h[2];
        const size_t n = (size_t)W * H;
        float offset;
        std::vector<float> uv, tp, tn;
        if (bake_check_map(W, H) || std::fread(&offset, 4, 1, f) != 1 || !get(f, uv, 6 * (size_t)nt) ||
            !get(f, tp, 9 * (size_t)nt) || !get(f, tn, 3 * (size_t)nt))
            return 2;
        std::vector<uint32_t> owner(n), list(n);
        std::vector<float> pos(3 * n), nrm(3 * n);
        const uint32_t count = bake_surface_host(nt, uv.data(), tp.data(), tn.data(), W, H, offset, owner.data(), pos.data(),
                                                 nrm.data(), list.data());
        put(o, owner.data(), n), put(o, pos.data(), 3 * n), put(o, nrm.data(), 3 * n), put(o, &count, 1);
        put(o, list.data(), count);
    } else {
        const uint32_t W = h[0], H = h[1], passes = h[2];
        const size_t n = (size_t)W * H;
        std::vector<uint32_t> owner;
        std::vector<float> in;
        if (bake_check_map(W, H) || !get(f, owner, n) || !get(f, in, 3 * n)) return 2;
        std::vector<float> out(3 * n);
        bake_dilate_host(W, H, owner.data(), passes, in.data(), out.data());
        put(o, out.data(), 3 * n);
    }
    std::fclose(f);
    return std::fclose(o) ? 3 : 0;
}
