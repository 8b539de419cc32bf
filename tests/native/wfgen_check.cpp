// CPU check of the wavefront chunk schedule (csrc/wfgen.hpp); tests/test_wfgen.py builds and runs it.
// argv[1]: tests/golden/wfgen_parent.json as lines of "name value ..." (its layout note says what each holds).
//
// Per case: (parent) every field the schedule returns equals what the parent commit's two chunk drivers computed
// with their own lines for the same inputs; (sound) the step's invariants: overlap implies not next, ended_only
// equals overlap, a sorted queue is non-empty and at least sort_min long.  Once: the two driver constants differ
// in exactly their four fields.
#include "wfgen.hpp"

#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

static long long g_checks = 0, g_failures = 0, g_cases = 0;
static std::string g_label;
static void check(bool ok, const char *kind, const char *what) {
    g_checks++;
    if (ok) return;
    if (g_failures++ < 40) std::printf("FAIL case %lld [%s] %s: %s\n", g_cases, g_label.c_str(), kind, what);
}
typedef std::vector<unsigned long long> Row;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::map<std::string, Row> in;
    std::vector<Row> rows, lengths;
    std::string line, name;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        Row r;
        unsigned long long v;
        ss >> name;
        while (ss >> v) r.push_back(v);
        if (name == "step_row") rows.push_back(r);
        else if (name == "lengths") lengths.push_back(r);
        else in[name] = r;
    }
    const cr::WfDriver drivers[2] = {cr::WF_DRIVER_CHUNK, cr::WF_DRIVER_LANES};
    const char *const driver_name[2] = {"chunk", "lanes"};
    const Row &gk = in.at("gk"), &fixed = in.at("fixed"), &row_of = in.at("step_row_of");
    // ---- the two drivers ----
    g_label = "drivers";
    const cr::WfDriver &c = cr::WF_DRIVER_CHUNK, &l = cr::WF_DRIVER_LANES;
    check(sizeof(cr::WfDriver) == 2 * sizeof(int), "sound", "a driver is its four fields");
    check(c.sort_g1 && !l.sort_g1, "sound", "the lanes driver ignores sort_g1");
    check(c.app_chunks && !l.app_chunks, "sound", "the lanes driver never appends in chunks");
    check(c.tail_overlap && !l.tail_overlap, "sound", "the lanes driver never overlaps the tail");
    check(cr::wf_tail_waves(c, (int)fixed[4]) == (int)fixed[4] && cr::wf_tail_waves(l, (int)fixed[4]) == 4, "sound",
          "the lanes driver's tail runs at 4 waves per SIMD");
    // ---- the generation step ----
    size_t combo = 0;
    for (int drv = 0; drv < 2; drv++)
    for (size_t i = 0; i + 1 < gk.size(); i += 2)
    for (size_t t = 0; t < in.at("tail_min").size(); t++)
    for (auto sort : in.at("sort")) for (auto g1 : in.at("sort_g1")) for (auto leaf : in.at("leaf_keys"))
    for (auto world : in.at("world_keys")) for (auto ovl : in.at("tail_overlap")) for (auto nlights : in.at("nlights"))
    for (auto ms : in.at("measure_skip")) {
        if (combo >= row_of.size() || row_of[combo] >= rows.size() || lengths.at(t).size() != 7 ||
            rows[row_of[combo]].size() != 49)
            return 2;
        const Row &want = rows[row_of[combo++]], &len = lengths[t];
        cr::WfArgs W{};
        W.tail_min = (uint32_t)in.at("tail_min")[t], W.sort = (int)sort, W.sort_g1 = (uint32_t)g1;
        W.leaf_keys = (int)leaf, W.world_keys = (int)world, W.tail_overlap = (int)ovl, W.measure_skip = (uint32_t)ms;
        W.sort_min = (uint32_t)fixed[0], W.key_bits = (int)fixed[1], W.key_bits_s = (int)fixed[2];
        W.key_bits_pixel = (int)fixed[3], W.tail_waves = (int)fixed[4];
        const uint32_t g = (uint32_t)gk[i], K = (uint32_t)gk[i + 1];
        for (int a = 0; a < 7; a++)
        for (int b = 0; b < 7; b++, g_cases++) {
            const uint32_t ns = (uint32_t)len[a], nc = (uint32_t)len[b], w = (uint32_t)want[7 * a + b];
            g_label = std::string(driver_name[drv]) + " g=" + std::to_string(g) + " K=" + std::to_string(K) + " tail_min=" +
                      std::to_string(W.tail_min) + " sort=" + std::to_string(sort) + " sort_g1=" + std::to_string(g1) +
                      " leaf=" + std::to_string(leaf) + " world=" + std::to_string(world) + " overlap=" +
                      std::to_string(ovl) + " nlights=" + std::to_string(nlights) + " skip=" + std::to_string(ms) +
                      " ns=" + std::to_string(ns) + " nc=" + std::to_string(nc);
            const cr::WfGenStep s = cr::wf_gen_step(g, K, ns, nc, (uint32_t)nlights, W, drivers[drv]);
            check(s.ns == ns, "parent", "ns");
            check(s.nc == ((w & 1u) ? 0u : nc), "parent", "nc");
            check(s.next == ((w >> 1) & 1u), "parent", "next");
            check(s.overlap == ((w >> 2) & 1u), "parent", "overlap");
            check(s.ended_only == ((w >> 3) & 1u), "parent", "ended_only");
            check(s.tail_after == ((w >> 4) & 1u), "parent", "tail_after");
            check(s.finished == ((w >> 5) & 1u), "parent", "finished");
            check(s.shadow.sorted == ((w >> 6) & 1u), "parent", "shadow sorted");
            check(s.closest.sorted == ((w >> 7) & 1u), "parent", "closest sorted");
            check(!s.shadow.sorted || s.shadow.bits == (int)((w >> 8) & 255u), "parent", "shadow key bits");
            check(!s.closest.sorted || s.closest.bits == (int)((w >> 16) & 255u), "parent", "closest key bits");
            check(!s.overlap || !s.next, "sound", "overlap implies not next");
            check(s.ended_only == s.overlap, "sound", "ended_only equals overlap");
            check(!s.shadow.sorted || (s.ns > 0 && s.ns >= W.sort_min), "sound", "a sorted shadow queue is long");
            check(!s.closest.sorted || (s.nc > 0 && s.nc >= W.sort_min), "sound", "a sorted closest queue is long");
        }
    }
    if (combo != row_of.size()) return 2;
    // ---- the append chunk ----
    const Row &app = in.at("app_cases");
    for (size_t i = 0; i + 7 < app.size(); i += 8, g_cases++) {
        cr::WfArgs W{};
        W.qspare = (uint32_t)app[i + 3], W.app_force = (uint32_t)app[i + 4], W.sort = (int)app[i + 5];
        g_label = std::string(driver_name[app[i]]) + " append build=" + std::to_string(app[i + 1]) + " grid=" +
                  std::to_string(app[i + 2]) + " qspare=" + std::to_string(W.qspare) + " force=" +
                  std::to_string(W.app_force) + " sort=" + std::to_string(W.sort) + " nin=" + std::to_string(app[i + 6]);
        check(cr::wf_app_chunk(W, (uint32_t)app[i + 6], (uint32_t)app[i + 2], app[i + 1] != 0, drivers[app[i]]) == app[i + 7],
              "parent", "app_chunk");
    }
    // ---- the chunk's start ----
    const Row &st = in.at("start_cases");
    for (size_t i = 0; i + 8 < st.size(); i += 9, g_cases++) {
        g_label = "start P=" + std::to_string(st[i]) + " tail_min=" + std::to_string(st[i + 1]);
        cr::WfArgs W{};
        W.P = (uint32_t)st[i], W.tail_min = (uint32_t)st[i + 1], W.cam_fused = (int)st[i + 2], W.cam_lean = (int)st[i + 5];
        const cr::WfStart s = cr::wf_chunk_start(W, st[i + 3] != 0, st[i + 4] != 0);
        check(s.cam_fused == (st[i + 6] != 0), "parent", "cam_fused");
        check(s.camera == (st[i + 7] != 0), "parent", "camera");
        check(s.tail_only == (st[i + 8] != 0), "parent", "tail_only");
    }
    std::printf("cases %lld\nchecks %lld failures %lld\n", g_cases, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
