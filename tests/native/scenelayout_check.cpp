// CPU check of the scene layout (csrc/scenelayout.hpp); tests/test_scenelayout.py builds and runs it.
// argv[1]: a manifest.  Per case a line "case NAME FILE", then "KEY VALUE" lines -- what the parent commit's
// cr_upload_scene computed for that description (tests/golden/scenelayout_parent.json) -- and "end".
// FILE is one scene description as a flat little-endian file:
//   u32 magic "CRSL", node_bfs, n_nodes, n_refs, max_depth, n_tris, n_lights, n_textures, flags; f32 box_min[3],
//   box_max[3]; nodes, refs, tri_pos, tri_normal, tri_kd, tri_ke, tri_uv, tri_tex (flags & 1), tri_emissive
//   (flags & 2), light_id, light_surface; per texture i32 width, height, components, u32 bytes (0xffffffff: null
//   data) and the bytes.
// Per case the program runs scene_layout and compares, key by key: the code and message; per output array the
// element count and a 64-bit FNV-1a hash of its bytes; every scalar.
#include "scenelayout.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

typedef std::vector<std::pair<std::string, std::string>> Pairs;

struct Desc {
    cr_scene_desc d{};
    uint32_t node_bfs = 0;
    std::vector<cr_kdnode> nodes;
    std::vector<uint32_t> refs, light_id;
    std::vector<float> pos, nrm, kd, ke, uv, light_surface;
    std::vector<int32_t> tex;
    std::vector<uint8_t> emissive;
    std::vector<cr_texture> textures;
    std::vector<std::vector<uint8_t>> texdata;
};

static bool read_desc(const std::string &path, Desc &D) {
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    bool ok = (bool)f || f.eof();
    auto take = [&](void *dst, size_t bytes) {
        if (at + bytes > buf.size()) {
            ok = false;
            return;
        }
        if (bytes) std::memcpy(dst, buf.data() + at, bytes);
        at += bytes;
    };
    auto vec = [&](auto &v, size_t n) {
        if ((buf.size() - at) / sizeof(v[0]) < n) {
            ok = false;
            return;
        }
        v.resize(n);
        take(v.data(), n * sizeof(v[0]));
    };
    uint32_t h[9] = {};
    take(h, sizeof(h));
    if (!ok || h[0] != 0x4C535243u) return false;
    cr_scene_desc &d = D.d;
    D.node_bfs = h[1], d.n_nodes = h[2], d.n_refs = h[3], d.max_depth = h[4], d.n_tris = h[5], d.n_lights = h[6];
    d.n_textures = h[7];
    take(d.box_min, 12);
    take(d.box_max, 12);
    const size_t nt = d.n_tris;
    vec(D.nodes, d.n_nodes), vec(D.refs, d.n_refs);
    vec(D.pos, 9 * nt), vec(D.nrm, 3 * nt), vec(D.kd, 3 * nt), vec(D.ke, 3 * nt), vec(D.uv, 6 * nt);
    if (h[8] & 1u) vec(D.tex, nt);
    if (h[8] & 2u) vec(D.emissive, nt);
    vec(D.light_id, d.n_lights), vec(D.light_surface, d.n_lights);
    D.textures.resize(d.n_textures);
    D.texdata.resize(d.n_textures);
    for (uint32_t i = 0; i < d.n_textures && ok; i++) {
        int32_t whc[3] = {};
        uint32_t bytes = 0;
        take(whc, 12), take(&bytes, 4);
        if (bytes != 0xffffffffu) vec(D.texdata[i], bytes);
        D.textures[i] = cr_texture{whc[0], whc[1], whc[2], bytes != 0xffffffffu ? D.texdata[i].data() : nullptr};
    }
    d.nodes = D.nodes.data(), d.refs = D.refs.data();
    d.tri_pos = D.pos.data(), d.tri_normal = D.nrm.data(), d.tri_kd = D.kd.data(), d.tri_ke = D.ke.data();
    d.tri_uv = D.uv.data();
    d.tri_tex = (h[8] & 1u) ? D.tex.data() : nullptr;
    d.tri_emissive = (h[8] & 2u) ? D.emissive.data() : nullptr;
    d.light_id = D.light_id.data(), d.light_surface = D.light_surface.data();
    d.textures = D.textures.data();
    return ok && at == buf.size();
}

static std::string hex64(uint64_t v) {
    char s[20];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)v);
    return s;
}
static uint64_t fnv(const void *p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
    return h;
}
template <class T> static void put_array(Pairs &r, const char *name, const std::vector<T> &v) {
    r.emplace_back(std::string(name) + ".n", std::to_string(v.size()));
    r.emplace_back(std::string(name) + ".hash", hex64(fnv(v.data(), v.size() * sizeof(T))));
}
static void put_bits(Pairs &r, const char *name, const float *f, int n) {
    std::string s;
    for (int i = 0; i < n; i++) {
        uint32_t b;
        std::memcpy(&b, f + i, 4);
        char t[12];
        std::snprintf(t, sizeof(t), "%s%08x", i ? "," : "", b);
        s += t;
    }
    r.emplace_back(name, s);
}

// what a call computed, as (key, value) pairs: a refusal is its code and message alone
static Pairs result_of(int code, const std::string &msg, const cr::SceneLayout &L) {
    Pairs r;
    r.emplace_back("code", std::to_string(code));
    r.emplace_back("msg", msg);
    if (code != CR_OK) return r;
    put_array(r, "levels", L.levels), put_array(r, "nodes", L.nodes), put_array(r, "fat", L.fat);
    put_array(r, "recs", L.recs), put_array(r, "lcullp", L.lcullp), put_array(r, "lcullc", L.lcullc);
    put_array(r, "tri", L.tri), put_array(r, "mat_n", L.mat_n), put_array(r, "mat_kd", L.mat_kd);
    put_array(r, "mat_ke", L.mat_ke), put_array(r, "mat_uv", L.mat_uv), put_array(r, "lights", L.lights);
    put_array(r, "texs", L.texs), put_array(r, "texels", L.texels), put_array(r, "level_off", L.level_off);
    for (int a = 0; a < 3; a++) put_array(r, a == 0 ? "splits0" : a == 1 ? "splits1" : "splits2", L.splits[a]);
    static_assert(sizeof(cr::LcGrid) == 9 * sizeof(float), "LcGrid is nine floats");
    put_bits(r, "lcg", (const float *)&L.S.lcg, 9);
    put_bits(r, "db", &L.S.db, 1);
    const float box[6] = {L.S.bmin.x, L.S.bmin.y, L.S.bmin.z, L.S.bmax.x, L.S.bmax.y, L.S.bmax.z};
    put_bits(r, "box", box, 6);
    r.emplace_back("tree_depth", std::to_string(L.tree_depth));
    r.emplace_back("stack_depth", std::to_string(L.stack_depth));
    r.emplace_back("n_refs", std::to_string(L.n_refs));
    r.emplace_back("n_tris", std::to_string(L.n_tris));
    r.emplace_back("n_nodes", std::to_string(L.S.n_nodes));
    r.emplace_back("n_lights", std::to_string(L.S.nlights));
    return r;
}

static Pairs run_case(const Desc &D) {
    cr::SceneLayout L;
    std::string err;
    const int code = cr::scene_layout(&D.d, D.node_bfs, L, err);
    return result_of(code, err, L);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream man(argv[1]);
    std::string line, name;
    Pairs want, got;
    int cases = 0, checks = 0, failures = 0;
    auto fail = [&](const std::string &what) {
        failures++;
        std::printf("FAIL case %s %s\n", name.c_str(), what.c_str());
    };
    while (std::getline(man, line)) {
        std::istringstream ss(line);
        std::string key, value;
        ss >> key;
        std::getline(ss, value);
        if (!value.empty()) value.erase(0, 1);
        if (key == "case") {
            std::istringstream cs(value);
            std::string file;
            cs >> name >> file;
            Desc D;
            if (!read_desc(file, D)) {
                std::printf("cannot read %s\n", file.c_str());
                return 2;
            }
            got = run_case(D);
            want.clear();
            cases++;
        } else if (key == "end") {
            checks++;
            if (want.size() != got.size())
                fail("keys: " + std::to_string(got.size()) + " != " + std::to_string(want.size()));
            for (size_t i = 0; i < want.size(); i++) {
                checks++;
                if (i >= got.size() || got[i].first != want[i].first) fail("parent: " + want[i].first + " missing");
                else if (got[i].second != want[i].second)
                    fail("parent: " + want[i].first + " " + got[i].second + " != " + want[i].second);
            }
        } else if (!key.empty()) {
            want.emplace_back(key, value);
        }
    }
    std::printf("cases %d checks %d failures %d\n", cases, checks, failures);
    return failures ? 1 : 0;
}
