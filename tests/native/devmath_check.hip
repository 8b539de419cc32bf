// GPU known-answer harness for the per-function helpers of csrc/device_math.hpp and csrc/render_common.hpp:
// the RNG and its two distributions, the min / max ternaries, the BRDF sampling, the wave-uniform forms of the
// exact divisions and of the triangle test, the root-box slab test and the texture lookup.
// Built once and run by tests/test_gpu_devmath.py:
//   devmath_check <stage> <in.bin> <out.bin>
// in.bin is a flat file of little-endian 32-bit words the test writes from numpy, one record per case; the stage's
// kernel runs one case per lane and out.bin receives the raw output words.  One JSON line with counts goes to
// stdout.  Nothing is compared here: every expected value is computed on the host by the test.
//
// Records (32-bit words; floats as their bit patterns):
//   rng     in  8: kind (0: seed, layer, pixel, sample -> rng_make; 1: raw key, ctr), w0..w3, ops (bit 0:
//                  rng_uniform, bit 1: rng_index), a bits | n, b bits
//           out 14: key, 8 rng_u32 draws, ctr; rng_uniform(a, b), ctr; rng_index(n), ctr -- each of the three from a
//                  fresh copy of the stream; an op not asked for leaves zeros
//   minmax  in  2: a, b                      out 3: std_min, std_max, glm_max
//   brdf    in  5: n.xyz, sx, sy             out 9: perpendicular(n).xyz, concentric dx dy, sample_wi wi.xyz pdf
//   wave    in  groups of 64 lane records of 32 words (one wave per group), then 2 words per group: the active mask
//                  lane record: a; da, db; o.xyz, d.xyz, A.xyz, e1.xyz, e2.xyz, tmax, live; box ray o.xyz, d.xyz,
//                  box min.xyz, max.xyz
//           out [run][group][lane][16]: rcp_rn_wave, rcp_rn; div_by_rcp_wave, div_by_rcp; tri_test_wave accept, ux,
//                  uy, t; tri_test accept, ux, uy, t; ray_box first, second; ray_box_inv first, second.
//                  run 0: the whole wave active.  run 1: inside a divergent branch taken by the lanes of the
//                  group's mask (the ballots see only those); the other lanes write WAVE_SENTINEL.
//   tex     in  ntex, ncases; per texture w, h, nc and its w*h*nc bytes padded to a word; cases of 3: ti, u, v
//           out 3 per case: tex_lookup rgb; then 4 per texture: DevScene::texs; then the atlas bytes
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "render_common.hpp"
#include "scenelayout.hpp"

using namespace cr;

enum { RNG_IN = 8, RNG_OUT = 14, MM_IN = 2, MM_OUT = 3, BRDF_IN = 5, BRDF_OUT = 9, WAVE_IN = 32, WAVE_OUT = 16 };
static const uint32_t WAVE_SENTINEL = 0xDEADBEEFu;

__device__ __forceinline__ uint32_t fb(float x) { return __float_as_uint(x); }
__device__ __forceinline__ float bf(uint32_t u) { return __uint_as_float(u); }

__global__ void k_rng(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *c = in + (size_t)RNG_IN * i;
    uint32_t *o = out + (size_t)RNG_OUT * i;
    const Rng r0 = c[0] == 0 ? rng_make(c[1], c[2], c[3], c[4]) : Rng{c[1], c[2]};
    Rng r = r0;
    o[0] = r.key;
    for (int j = 0; j < 8; j++) o[1 + j] = rng_u32(r);
    o[9] = r.ctr;
    o[10] = o[11] = o[12] = o[13] = 0u;
    if (c[5] & 1u) {
        r = r0;
        o[10] = fb(rng_uniform(r, bf(c[6]), bf(c[7])));
        o[11] = r.ctr;
    }
    if (c[5] & 2u) {
        r = r0;
        o[12] = rng_index(r, c[6]);
        o[13] = r.ctr;
    }
}

__global__ void k_minmax(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = bf(in[2 * (size_t)i]), b = bf(in[2 * (size_t)i + 1]);
    uint32_t *o = out + (size_t)MM_OUT * i;
    o[0] = fb(std_min(a, b));
    o[1] = fb(std_max(a, b));
    o[2] = fb(glm_max(a, b));
}

__global__ void k_brdf(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *c = in + (size_t)BRDF_IN * i;
    uint32_t *o = out + (size_t)BRDF_OUT * i;
    const f3 nn = mk(bf(c[0]), bf(c[1]), bf(c[2]));
    const float sx = bf(c[3]), sy = bf(c[4]);
    const f3 p = perpendicular(nn);
    o[0] = fb(p.x), o[1] = fb(p.y), o[2] = fb(p.z);
    float dx, dy;
    concentric(sx, sy, dx, dy);
    o[3] = fb(dx), o[4] = fb(dy);
    f3 wi;
    float pdf;
    sample_wi(nn, sx, sy, wi, pdf);
    o[5] = fb(wi.x), o[6] = fb(wi.y), o[7] = fb(wi.z), o[8] = fb(pdf);
}

// One lane's record through every wave-uniform helper and its scalar form.  Called with the wave converged
// (run 0) or from inside the mask's branch (run 1): the helpers' ballots see the lanes that are here.
__device__ __forceinline__ void wave_lane(const uint32_t *c, uint32_t *o) {
    const float a = bf(c[0]);
    o[0] = fb(rcp_rn_wave(a));
    o[1] = fb(rcp_rn(a));
    const float da = bf(c[1]), db = bf(c[2]);
    const float y = rcp_for_div(db);
    o[2] = fb(div_by_rcp_wave(da, db, y));
    o[3] = fb(div_by_rcp(da, db, y));
    const f3 ro = mk(bf(c[3]), bf(c[4]), bf(c[5])), rd = mk(bf(c[6]), bf(c[7]), bf(c[8]));
    const TriRec rec{make_float4(bf(c[9]), bf(c[10]), bf(c[11]), 0.f), make_float4(bf(c[12]), bf(c[13]), bf(c[14]), 0.f),
                     make_float4(bf(c[15]), bf(c[16]), bf(c[17]), 0.f)};
    const float tmax = bf(c[18]);
    const bool live = c[19] != 0u;
    float ux = 0.f, uy = 0.f, t = 0.f;
    const bool aw = tri_test_wave(ro, rd, rec, tmax, ux, uy, t, live);
    o[4] = aw ? 1u : 0u, o[5] = fb(ux), o[6] = fb(uy), o[7] = fb(t);
    ux = uy = t = 0.f;
    const bool as = tri_test(ro, rd, rec, tmax, ux, uy, t);
    o[8] = as ? 1u : 0u, o[9] = fb(ux), o[10] = fb(uy), o[11] = fb(t);
    const f3 bo = mk(bf(c[20]), bf(c[21]), bf(c[22])), bd = mk(bf(c[23]), bf(c[24]), bf(c[25]));
    DevScene S{};
    S.bmin = make_float3(bf(c[26]), bf(c[27]), bf(c[28]));
    S.bmax = make_float3(bf(c[29]), bf(c[30]), bf(c[31]));
    float first, second;
    ray_box(S, bo, bd, first, second);
    o[12] = fb(first), o[13] = fb(second);
    const f3 inv = mk(rcp_rn_wave(bd.x), rcp_rn_wave(bd.y), rcp_rn_wave(bd.z)); // the packet trace's root slab
    ray_box_inv(S, bo, inv, first, second);
    o[14] = fb(first), o[15] = fb(second);
}

// one block of 64 lanes = one wave = one group
template <bool MASKED>
__global__ __launch_bounds__(64) void k_wave(const uint32_t *in, const uint32_t *masks, uint32_t *out) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t *c = in + ((size_t)g * 64 + lane) * WAVE_IN;
    uint32_t *o = out + ((size_t)g * 64 + lane) * WAVE_OUT;
    if (!MASKED) {
        wave_lane(c, o);
    } else {
        const uint64_t m = (uint64_t)masks[2 * g] | ((uint64_t)masks[2 * g + 1] << 32);
        if ((m >> lane) & 1ull) {
            wave_lane(c, o);
        } else {
            for (int j = 0; j < WAVE_OUT; j++) o[j] = WAVE_SENTINEL;
        }
    }
}

__global__ void k_tex(DevScene S, const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 c = tex_lookup(S, (int)in[3 * (size_t)i], bf(in[3 * (size_t)i + 1]), bf(in[3 * (size_t)i + 2]));
    out[3 * (size_t)i] = fb(c.x), out[3 * (size_t)i + 1] = fb(c.y), out[3 * (size_t)i + 2] = fb(c.z);
}

static bool read_words(const char *path, std::vector<uint32_t> &w) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    bool ok = bytes >= 0 && bytes % 4 == 0;
    if (ok) {
        w.resize((size_t)bytes / 4);
        ok = fread(w.data(), 4, w.size(), f) == w.size();
    }
    fclose(f);
    return ok;
}
static bool write_words(const char *path, const std::vector<uint32_t> &w, const std::vector<uint8_t> &tail = {}) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    bool ok = fwrite(w.data(), 4, w.size(), f) == w.size();
    ok = ok && fwrite(tail.data(), 1, tail.size(), f) == tail.size();
    return fclose(f) == 0 && ok;
}
static int fail(const char *msg) {
    fprintf(stderr, "devmath_check: %s\n", msg);
    return 2;
}
#define HIP_OK(x)                                                                                                      \
    do {                                                                                                               \
        const hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "devmath_check: %s: %s\n", #x, hipGetErrorString(e_));                                     \
            return 2;                                                                                                  \
        }                                                                                                              \
    } while (0)

// in -> device, run(d_in, d_out), device -> out
template <class F>
static int round_trip(const std::vector<uint32_t> &in, std::vector<uint32_t> &out, F run) {
    uint32_t *di = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc(&di, std::max<size_t>(in.size(), 1) * 4));
    HIP_OK(hipMalloc(&dout, std::max<size_t>(out.size(), 1) * 4));
    HIP_OK(hipMemcpy(di, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, out.size() * 4));
    run(di, dout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    (void)hipFree(di);
    (void)hipFree(dout);
    return 0;
}

template <class K>
static int per_lane(K kernel, int win, int wout, const std::vector<uint32_t> &in, std::vector<uint32_t> &out,
                    uint32_t &n) {
    if (in.size() % win) return fail("input is not a whole number of records");
    n = (uint32_t)(in.size() / win);
    out.assign((size_t)n * wout, 0u);
    return round_trip(in, out, [&](uint32_t *di, uint32_t *dout) {
        if (n) hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, 0, di, dout, n);
    });
}

static int stage_wave(const std::vector<uint32_t> &in, std::vector<uint32_t> &out, uint32_t &groups) {
    const size_t per_group = (size_t)64 * WAVE_IN + 2;
    if (in.size() % per_group) return fail("input is not a whole number of groups");
    groups = (uint32_t)(in.size() / per_group);
    const size_t run_words = (size_t)groups * 64 * WAVE_OUT;
    out.assign(2 * run_words, 0u);
    return round_trip(in, out, [&](uint32_t *di, uint32_t *dout) {
        if (!groups) return;
        const uint32_t *masks = di + (size_t)groups * 64 * WAVE_IN;
        hipLaunchKernelGGL(k_wave<false>, dim3(groups), dim3(64), 0, 0, di, masks, dout);
        hipLaunchKernelGGL(k_wave<true>, dim3(groups), dim3(64), 0, 0, di, masks, dout + run_words);
    });
}

// The atlas is laid out by the product's own scene_layout from a description with nothing but the textures
// (and the one empty leaf a description must have).
static int stage_tex(const std::vector<uint32_t> &in, std::vector<uint32_t> &out, std::vector<uint8_t> &atlas,
                     uint32_t &ncases, uint32_t &ntex) {
    if (in.size() < 2) return fail("short texture input");
    ntex = in[0], ncases = in[1];
    size_t at = 2;
    std::vector<cr_texture> tex(ntex);
    for (uint32_t i = 0; i < ntex; i++) {
        if (at + 3 > in.size()) return fail("short texture header");
        const int w = (int)in[at], h = (int)in[at + 1], nc = (int)in[at + 2];
        if (w <= 0 || h <= 0 || nc <= 0 || w > 4096 || h > 4096 || nc > 4) return fail("bad texture header");
        const size_t words = ((size_t)w * h * nc + 3) / 4;
        at += 3;
        if (at + words > in.size()) return fail("short texture data");
        tex[i] = cr_texture{w, h, nc, (const uint8_t *)(in.data() + at)};
        at += words;
    }
    if (at + (size_t)3 * ncases != in.size()) return fail("texture cases do not fill the input");
    for (uint32_t i = 0; i < ncases; i++)
        if (in[at + 3 * (size_t)i] >= ntex) return fail("texture index out of range");
    cr_kdnode leaf{};
    leaf.axis = 3;
    cr_scene_desc d{};
    d.n_nodes = 1, d.nodes = &leaf, d.max_depth = 1;
    d.n_textures = ntex, d.textures = tex.data();
    SceneLayout L;
    std::string err;
    if (scene_layout(&d, 1, L, err) != CR_OK) return fail(err.c_str());
    atlas = L.texels;
    uint4 *dtexs = nullptr;
    uint8_t *dtexels = nullptr;
    HIP_OK(hipMalloc(&dtexs, std::max<size_t>(L.texs.size(), 1) * sizeof(uint4)));
    HIP_OK(hipMalloc(&dtexels, std::max<size_t>(L.texels.size(), 1)));
    HIP_OK(hipMemcpy(dtexs, L.texs.data(), L.texs.size() * sizeof(uint4), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dtexels, L.texels.data(), L.texels.size(), hipMemcpyHostToDevice));
    DevScene S = L.S;
    S.texs = dtexs, S.texels = dtexels;
    const std::vector<uint32_t> cases(in.begin() + (long)at, in.end());
    out.assign((size_t)3 * ncases, 0u);
    const uint32_t n = ncases;
    const int rc = round_trip(cases, out, [&](uint32_t *di, uint32_t *dout) {
        if (n) hipLaunchKernelGGL(k_tex, dim3((n + 255) / 256), dim3(256), 0, 0, S, di, dout, n);
    });
    (void)hipFree(dtexs);
    (void)hipFree(dtexels);
    for (const uint4 &t : L.texs) out.insert(out.end(), {t.x, t.y, t.z, t.w});
    return rc;
}

int main(int argc, char **argv) {
    if (argc != 4) return fail("usage: devmath_check <rng|minmax|brdf|wave|tex> <in.bin> <out.bin>");
    const std::string stage = argv[1];
    std::vector<uint32_t> in, out;
    std::vector<uint8_t> tail;
    if (!read_words(argv[2], in)) return fail("cannot read the input");
    uint32_t n = 0, extra = 0;
    int rc;
    if (stage == "rng") rc = per_lane(k_rng, RNG_IN, RNG_OUT, in, out, n);
    else if (stage == "minmax") rc = per_lane(k_minmax, MM_IN, MM_OUT, in, out, n);
    else if (stage == "brdf") rc = per_lane(k_brdf, BRDF_IN, BRDF_OUT, in, out, n);
    else if (stage == "wave") rc = stage_wave(in, out, n);
    else if (stage == "tex") rc = stage_tex(in, out, tail, n, extra);
    else return fail("unknown stage");
    if (rc) return rc;
    if (!write_words(argv[3], out, tail)) return fail("cannot write the output");
    if (stage == "wave")
        printf("{\"stage\": \"wave\", \"groups\": %u, \"lanes\": %u, \"out_words\": %zu}\n", n, n * 64, out.size());
    else if (stage == "tex")
        printf("{\"stage\": \"tex\", \"cases\": %u, \"textures\": %u, \"atlas_bytes\": %zu, \"out_words\": %zu}\n", n,
               extra, tail.size(), out.size());
    else
        printf("{\"stage\": \"%s\", \"cases\": %u, \"out_words\": %zu}\n", stage.c_str(), n, out.size());
    return 0;
}
