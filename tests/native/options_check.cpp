// CPU check of the option table (csrc/ctxopts.hpp); tests/test_options.py builds and runs it.
// argv[1]: what the parent commit's cr_set_option did (tests/golden/options_parent.json), as lines
//   probes V V V ...                 every probe value
//   key NAME FIELD V:S V:S ...       the probes the parent accepted for the key, each with what it stored in FIELD
// Per (key, probe) every option field is filled with a sentinel, set_option is called, and two things are checked:
// the same acceptance as the parent's; and an accepted pair changed exactly FIELD, to the same value, a rejected
// pair changed nothing.  The program prints the table's names for the test to compare with the parent's keys.
#include "ctxopts.hpp"

#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

// the check's own statement of the option fields (WfOptions' and CtxOptions')
#define OPTION_FIELDS(X)                                                                                              \
    X(wf_paths) X(wf_sort) X(wf_sort_min) X(wf_sort_tile) X(wf_dir_res) X(wf_world_keys) X(wf_world_bits)             \
    X(wf_tail_min) X(wf_tail_overlap) X(wf_sort_g1) X(wf_cam_lean) X(wf_cam_fuse) X(wf_ctl_ray) X(wf_vis_dw)          \
    X(wf_vis_mark) X(wf_nee_skip) X(wf_tail_waves) X(wf_dir_res_shadow) X(sample_buf) X(wf_lanes) X(wf_xcd)           \
    X(wf_leaf_keys) X(wf_leaf_shift) X(wf_resolve_paths) X(wf_measure_skip) X(wf_shade_waves) X(wf_app_chunk)         \
    X(wf_shade_block) X(wf_packet_unanimous) X(kernel) X(full_counters) X(lc_debug) X(lc_min) X(desc_quorum)          \
    X(diag_kinds) X(perf_counters) X(variant) X(refill) X(refill_shadow) X(refill_camera) X(sum_lds) X(sum_staged)    \
    X(node_bfs) X(comm_timeout_ms) X(query_route) X(query_sort) X(query_chunk) X(query_trace_min)

// every option field of o as (name, value); the sentinel: each field's bytes all 0x5a
template <class O> static std::vector<std::pair<std::string, long long>> fields_of(const O &o) {
    std::vector<std::pair<std::string, long long>> r;
#define X(f) r.emplace_back(#f, (long long)o.f);
    OPTION_FIELDS(X)
#undef X
    return r;
}
template <class O> static void fill_sentinel(O &o) {
#define X(f) std::memset(&o.f, 0x5a, sizeof(o.f));
    OPTION_FIELDS(X)
#undef X
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    std::vector<long long> probes;
    int keys = 0, checks = 0, failures = 0;
    cr::CtxOptions sentinel;
    fill_sentinel(sentinel);
    const auto blank = fields_of(sentinel);
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string what, key, field, tok;
        ss >> what;
        if (what == "probes") {
            long long v;
            while (ss >> v) probes.push_back(v);
            continue;
        }
        if (what != "key") continue;
        ss >> key >> field;
        std::map<long long, long long> accepted;
        while (ss >> tok) accepted[std::stoll(tok)] = std::stoll(tok.substr(tok.find(':') + 1));
        keys++;
        for (long long v : probes) {
            cr::CtxOptions o;
            fill_sentinel(o);
            const bool ok = cr::set_option(o, key.c_str(), v);
            const bool want = accepted.count(v) != 0;
            checks++;
            if (ok != want) {
                failures++;
                std::printf("FAIL %s %lld accepted: %d != %d\n", key.c_str(), v, (int)ok, (int)want);
            }
            const auto after = fields_of(o);
            std::string diff;
            for (size_t i = 0; i < after.size(); i++) {
                const bool written = ok && want && after[i].first == field;
                const long long expect = written ? accepted[v] : blank[i].second;
                if (after[i].second != expect)
                    diff += " " + after[i].first + " " + std::to_string(after[i].second) + " != " + std::to_string(expect);
            }
            checks++;
            if (!diff.empty()) {
                failures++;
                std::printf("FAIL %s %lld fields:%s\n", key.c_str(), v, diff.c_str());
            }
        }
    }
    std::printf("names");
    for (const cr::OptRow &r : cr::kOptions) std::printf(" %s", r.name);
    std::printf("\nvariants %d\n", cr::num_wf_variants());
    std::printf("keys %d probes %zu checks %d failures %d\n", keys, probes.size(), checks, failures);
    return failures ? 1 : 0;
}
