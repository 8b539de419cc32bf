// CPU check of the wavefront pass plan and the path-chunk layout (csrc/wfplan.hpp); tests/test_wfplan.py builds
// and runs it.  argv[1]: the cases of tests/golden/wfplan_parent.json, one per line as "name value" pairs, the
// expected refusal's text after a '|'.
//
// Per case: (parent) the plan, the WfArgs it binds and every array's offset equal what the parent commit's
// run_render computed for the same inputs; (sound) the arrays lie in wf_arrays' order on multiples of 256 bytes,
// none overlaps the next, each has room for the elements its WfArgs comment promises, and the last ends inside
// `need` <= `need_alloc`; (layers) whatever cr_layers_per_pass's rule accepts, the plan takes as one sample
// chunk and one path chunk.
#include "wfplan.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

static int g_checks = 0, g_failures = 0;
static int g_case = 0;
static std::string g_label;
static void check(bool ok, const char *kind, const std::string &what) {
    g_checks++;
    if (ok) return;
    g_failures++;
    std::printf("FAIL case %d [%s] %s: %s\n", g_case, g_label.c_str(), kind, what.c_str());
}
template <class A, class B> static void equal(const char *kind, const std::string &what, A got, B want) {
    check((unsigned long long)got == (unsigned long long)want, kind,
          what + " " + std::to_string((unsigned long long)got) + " != " + std::to_string((unsigned long long)want));
}

typedef std::map<std::string, unsigned long long> Case;

static cr::WfPlanIn input_of(const Case &c) {
    cr::WfPlanIn in;
    in.n_items = (uint32_t)c.at("in.n_items");
    in.spp = (uint32_t)c.at("in.spp");
    in.nl = (uint32_t)c.at("in.nl");
    in.K = (int)c.at("in.K");
    in.tile = (uint32_t)c.at("in.tile");
    in.n_tris = (uint32_t)c.at("in.n_tris");
    in.n_nodes = (uint32_t)c.at("in.n_nodes");
    in.stack_depth = (uint32_t)c.at("in.stack_depth");
    in.gstride = (uint32_t)c.at("in.gstride");
    in.shade_blocks = (uint32_t)c.at("in.shade_blocks");
    in.path_cap = c.at("in.path_cap");
    in.opt.wf_paths = (uint32_t)c.at("in.wf_paths");
    in.opt.sample_buf = c.at("in.sample_buf");
    in.opt.wf_lanes = (int)c.at("in.wf_lanes");
    in.opt.wf_sort = (int)(long long)c.at("in.wf_sort");
    in.opt.wf_leaf_keys = (int)c.at("in.wf_leaf_keys");
    in.opt.wf_world_keys = (int)c.at("in.wf_world_keys");
    in.opt.wf_dir_res_shadow = (uint32_t)c.at("in.wf_dir_res_shadow");
    in.opt.wf_app_chunk = (int)c.at("in.wf_app_chunk");
    return in;
}

// the check's own statement of which WfArgs field each array is, and of the elements its comment promises
struct Promise {
    const char *name;
    const void *field;
    size_t bytes;
};

static void check_plan(const Case &c, const cr::WfPlanIn &in, const cr::WfPlan &pl) {
    const cr::WfDims &d = pl.dims;
    char *const base = (char *)(1ull << 32); // (never dereferenced)
    uint2 *const gbase = (uint2 *)(1ull << 40);
    cr::WfArgs W{}, W2{};
    cr::wf_bind(in, pl, base, gbase, 0, W);
    cr::wf_bind(in, pl, base, gbase, 1, W2);
    // ---- equal to the parent ----
    equal("parent", "chunk", pl.chunk, c.at("out.chunk"));
    equal("parent", "P", d.P, c.at("out.P"));
    equal("parent", "W.P", W.P, c.at("out.P"));
    equal("parent", "Q", d.Q, c.at("out.Q"));
    equal("parent", "sort", W.sort, c.at("out.sort"));
    equal("parent", "key_bits", W.key_bits, c.at("out.key_bits"));
    equal("parent", "key_bits_pixel", W.key_bits_pixel, c.at("out.key_bits_pixel"));
    equal("parent", "key_bits_s", W.key_bits_s, c.at("out.key_bits_s"));
    equal("parent", "dir_res", W.dir_res, c.at("out.dir_res"));
    equal("parent", "dir_res_s", W.dir_res_s, c.at("out.dir_res_s"));
    equal("parent", "leaf_keys", W.leaf_keys, c.at("out.leaf_keys"));
    equal("parent", "world_keys", W.world_keys, c.at("out.world_keys"));
    equal("parent", "sort_tmp", W.sort_tmp_bytes, c.at("out.sort_tmp"));
    equal("parent", "need", pl.need, c.at("out.need"));
    equal("parent", "need_alloc", pl.need_alloc, c.at("out.need_alloc"));
    equal("parent", "gstack_bytes", pl.gstack_bytes, c.at("out.gstack_bytes"));
    equal("parent", "samples_bytes", pl.samples_bytes, c.at("out.samples_bytes"));
    equal("parent", "run_bytes", pl.run_bytes, c.at("out.run_bytes"));
    equal("parent", "qspare", W.qspare, c.at("out.qspare"));
    equal("parent", "vis_mark", W.vis_mark, c.at("out.vis_mark"));
    equal("parent", "gstack", W.gstack - gbase, c.at("gstack.0"));
    equal("parent", "gstack2", W.gstack2 - gbase, c.at("gstack.1"));
    equal("parent", "gstride", W.gstride, in.gstride);
    if (in.opt.wf_lanes == 2) {
        equal("parent", "lane 1 gstack", W2.gstack - gbase, c.at("gstack.2"));
        equal("parent", "lane 1 gstack2", W2.gstack2 - gbase, c.at("gstack.3"));
    }
    const size_t q4 = 16 * (size_t)d.Q, p4 = 16 * (size_t)d.P;
    const Promise promised[] = {
        {"ray0", W.ray[0], 2 * q4}, {"ray1", W.ray[1], 2 * q4},
        {"hit0", W.hit[0], q4}, {"hit1", W.hit[1], q4},
        {"sray", W.sray, 2 * q4},
        {"ps", W.ps, cr::WF_STATE * p4},
        {"dw", W.dw, 2 * (size_t)in.K * p4},
        {"sexcl", W.sexcl, 4 * (size_t)d.Q}, {"occ", W.occ, 4 * (size_t)d.Q},
        {"cnt", W.cnt, cr::WF_CNT * sizeof(uint32_t)},
        {"cxy", W.cxy, sizeof(float2) * (size_t)d.P},
        {"mark", W.mark, (size_t)d.P},
        {"key00", W.key[0][0], 4 * (size_t)d.Q}, {"perm00", W.perm[0][0], 4 * (size_t)d.Q},
        {"key01", W.key[0][1], 4 * (size_t)d.Q}, {"perm01", W.perm[0][1], 4 * (size_t)d.Q},
        {"key10", W.key[1][0], 4 * (size_t)d.Q}, {"perm10", W.perm[1][0], 4 * (size_t)d.Q},
        {"key11", W.key[1][1], 4 * (size_t)d.Q}, {"perm11", W.perm[1][1], 4 * (size_t)d.Q},
        {"sort_tmp", W.sort_tmp, cr::rs_tmp_bytes((uint32_t)d.Q)},
    };
    const int n = (int)(sizeof(promised) / sizeof(promised[0]));
    // what wf_arrays lists for this chunk, in its order, and where wf_layout put each (W's fields above)
    std::vector<std::pair<std::string, size_t>> rows;
    cr::WfArgs Wn{};
    cr::wf_arrays(d, Wn, [&](const char *name, size_t bytes) {
        rows.push_back({name, bytes});
        return (char *)nullptr;
    });
    cr::WfArgs Wl{};
    const size_t end = cr::wf_layout(d, base, Wl);
    check(std::memcmp(&Wl.ray, &W.ray, sizeof(W.ray)) == 0 && Wl.sort_tmp == W.sort_tmp, "sound",
          "wf_bind carves by wf_layout");
    check((int)rows.size() == (d.sort ? n : n - 9), "sound", "the check knows every array of the walk");
    size_t last_end = 0;
    for (int i = 0; i < n; i++) {
        const std::string name = promised[i].name;
        const auto want = c.find("off." + name);
        const bool have = i < (int)rows.size();
        check(have == (want != c.end()), "parent", name + " present");
        check(have == (promised[i].field != nullptr), "parent", name + " bound");
        if (!have || want == c.end() || !promised[i].field) continue;
        check(name == rows[i].first, "sound", name + " is array " + std::to_string(i));
        const size_t off = (size_t)((const char *)promised[i].field - base);
        equal("parent", name + " offset", off, want->second);
        // ---- sound ----
        check(off % 256 == 0, "sound", name + " on a multiple of 256");
        check(off >= last_end, "sound", name + " in order, past the array before it");
        const size_t next = i + 1 < (int)rows.size() ? (size_t)((const char *)promised[i + 1].field - base) : end;
        check(next >= off && next - off >= promised[i].bytes, "room", name + " holds its elements");
        check(rows[i].second >= promised[i].bytes, "room", name + " is sized for its elements");
        last_end = off + promised[i].bytes;
    }
    check(end <= pl.need, "room", "the last array ends inside need");
    check(pl.need <= pl.need_alloc, "sound", "need <= need_alloc");
    if (!in.opt.wf_app_chunk)
        check(pl.need - d.sort_tmp - cr::WF_CNT * 4 - 8192 <=
                  d.P * cr::wf_bytes_per_path(in.K, cr::wf_chunked(in.opt, in.n_tris)),
              "sound", "wf_bytes_per_path bounds a path's bytes");
}

// whatever the layers rule accepts is one sample chunk and one path chunk of the plan
static void check_layers(const cr::WfPlanIn &in0) {
    if (in0.opt.wf_lanes != 1) return;
    // (a stack-overflow area above 4 GiB is refused whatever the layers: not the rule's business)
    if (cr::gstack_bytes(in0.stack_depth, in0.gstride) >= (1ull << 32)) return;
    const uint64_t paths_cap = std::min<uint64_t>(in0.opt.wf_paths, in0.path_cap);
    for (uint32_t nl = 1; nl <= 4; nl++) {
        if (!cr::wf_layers_fit(in0.n_items, in0.spp, nl, paths_cap, in0.opt.sample_buf)) continue;
        cr::WfPlanIn in = in0;
        in.nl = nl;
        const cr::WfPlan pl = cr::wf_plan(in);
        const std::string what = "nl " + std::to_string(nl);
        check(pl.code == CR_OK, "layers", what + " not refused");
        check(!pl.chunked, "layers", what + " one sample chunk");
        equal("layers", what + " P", pl.dims.P, (uint64_t)in.n_items * in.spp * nl);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        const size_t bar = line.find('|');
        if (bar == std::string::npos) continue;
        const std::string refusal = line.substr(bar + 1);
        std::istringstream ss(line.substr(0, bar));
        Case c;
        std::string name, value;
        while (ss >> name >> value)
            c[name] = value[0] == '-' ? (unsigned long long)std::stoll(value) : std::stoull(value);
        const cr::WfPlanIn in = input_of(c);
        const bool chunked = cr::wf_chunked(in.opt, in.n_tris);
        g_label = "nodes=" + std::to_string(in.n_nodes) + " items=" + std::to_string(in.n_items) +
                  (chunked ? " spare" : " nospare") + " lanes=" + std::to_string(in.opt.wf_lanes);
        const cr::WfPlan pl = cr::wf_plan(in);
        if (!refusal.empty()) {
            check(pl.code == (int)(long long)c.at("code"), "parent", "refused with the parent's code");
            check(pl.msg && refusal == pl.msg, "parent", "refused with \"" + refusal + "\"");
        } else {
            check(pl.code == CR_OK && !pl.msg, "parent", "not refused");
            if (pl.code == CR_OK) check_plan(c, in, pl);
        }
        check_layers(in);
        g_case++;
    }
    std::printf("cases %d\nchecks %d failures %d\n", g_case, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
