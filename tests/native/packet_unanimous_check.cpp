// packet_unanimous_check.cpp -- CPU model check of the camera packet's unanimous kd steps
// (csrc/wavefront.hip wf_trace_packet): the packet walk of packet_check.cpp
// WITH the hull proofs, against the per-ray recursion of kdtree.cpp:248-281.
//
// The proofs.  All rays of a packet share the eye, so a node's numerator n = split - eye[a] is one
// number.  Every ray's split distance is RN(n / d_a), and correctly rounded division by divisors of
// one sign is monotone in the divisor, so with [d_lo, d_hi] the hull of the LIVE rays' d_a every ray's
// tsp lies in [tsp_lo, tsp_hi] = [min, max] of RN(n / d_lo), RN(n / d_hi).  With two bounds over the
// active rays, Tub >= max tmax and Mlb <= min tmin:
//     near-only for all   tsp_lo >= Tub  or  tsp_hi < 0
//     far-only  for all   tsp_lo >= 0   and  tsp_hi < Mlb      (strict: tsp == tmin == tmax is near-only)
// A proven step sets the node and nothing else.  An axis hull is usable only if d_lo, d_hi have one
// sign, lie in 2^-40 <= |d| <= 2^40 (the range of the kernel's short division) and within a factor 2 of
// each other; a hull quotient outside 2^-59 <= |q| <= 2^59 proves nothing (inside it the short division's
// own test 2^-60 <= |n * RN(1/d)| <= 2^60 holds, so q is RN(n / d)).  The bounds: a per-ray step on a usable axis
// leaves the near side with Tub' = min(Tub, tsp_hi) when no active ray stayed near-only; the pushed
// entry's rays come back with tmax <= Tub(push) and tmin >= tsp_lo(push) -- or min(Mlb(push), tsp_lo(push))
// where far-only rays are parked in it with their own tmin --, kept per
// stack entry for the first `store` entries (the kernel: 24); a deeper entry's rays come back with
// Tub = +inf, Mlb = -inf, which prove nothing until a later step or pop refreshes them.  (store 0: the
// bounds recomputed at every pop by a min / max over the re-activated rays, the other valid choice.)
//
// Inputs: random trees, eyes and direction fans as in packet_check.cpp, plus the adversarial ones:
// fans whose component hull contains 0 or changes sign, components at the 2^-40 / 2^40 guard,
// intervals with tsp == tmax / tsp == tmin at the root, quotients that underflow to +-0, an eye one
// ulp from a split plane, dead slots (direction (0, 0, 1)) and box-missed rays mixed into the
// packets, and stacks deeper than the bound storage.
//   packet_unanimous_check <seed> <cases> [mutant]
//   prints "violations N rays M leaf_tests L steps S proven P near Q far F loose H"
// (loose: usable hull ends that no live ray attains.)  Mutants, all of which must be caught:
// 1: `<=` in the far-only proof; 2: the hull taken over every slot, dead rays' (0, 0, 1) included;
// 3: the bounds not refreshed at a pop.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

uint64_t rs = 88172645463325252ull;
uint64_t next() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
}
double rnd() { return (double)(next() >> 11) * 0x1p-53; }

struct Node {
    int axis = -1; // -1: leaf
    float split = 0;
    int child = -1; // children at child, child + 1
    std::vector<float> hits;
};
std::vector<Node> tree;
float scale = 1.f; // the case's scene scale (tiny: quotients that underflow)

int build(int depth, float lo[3], float hi[3]) {
    const int id = (int)tree.size();
    tree.push_back(Node());
    if (depth == 0 || rnd() < 0.06) {
        const int nh = rnd() < 0.7 ? 0 : 1 + (int)(rnd() * 3);
        for (int i = 0; i < nh; i++) tree[id].hits.push_back((float)(rnd() * 40.0 - 5.0) * scale);
        return id;
    }
    const int a = (int)(rnd() * 3);
    const float s = lo[a] + (float)rnd() * (hi[a] - lo[a]);
    tree[id].axis = a;
    tree[id].split = s;
    const int c = (int)tree.size();
    tree.push_back(Node());
    tree.push_back(Node());
    tree[id].child = c;
    float h0[3] = {hi[0], hi[1], hi[2]}, l1[3] = {lo[0], lo[1], lo[2]};
    h0[a] = s;
    l1[a] = s;
    const int s0 = build(depth - 1, lo, h0), s1 = build(depth - 1, l1, hi);
    tree[c] = tree[s0];
    tree[c + 1] = tree[s1];
    tree[s0] = Node();
    tree[s1] = Node();
    return id;
}

uint32_t cull_seed;
int mutant = 0;
bool culled(int node, int ray) {
    uint32_t x = (uint32_t)node * 0x9E3779B1u ^ (uint32_t)ray * 0x85EBCA77u ^ cull_seed;
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    return (x & 1023u) < 24u;
}

struct Rec {
    int leaf;
    float t0, t1;
};
float eye[3];

bool ref(int ray, int node, const float d[3], float tmin, float tmax, std::vector<Rec> &log, float &best) {
    if (culled(node, ray)) return false;
    const Node &n = tree[node];
    if (n.axis < 0) {
        log.push_back({node, tmin, tmax});
        bool f = false;
        for (float h : n.hits)
            if (h >= 0.f && h < tmax) {
                tmax = h;
                best = h;
                f = true;
            }
        return f;
    }
    const float oa = eye[n.axis], da = d[n.axis];
    const float tsplit = (n.split - oa) / da;
    const int below = oa < n.split ? 1 : 0;
    const int nearc = n.child + (1 - below), farc = n.child + below;
    if (tsplit >= tmax || tsplit < 0) return ref(ray, nearc, d, tmin, tmax, log, best);
    if (tsplit <= tmin) return ref(ray, farc, d, tmin, tmax, log, best);
    if (ref(ray, nearc, d, tmin, tsplit, log, best)) return true;
    return ref(ray, farc, d, tsplit, tmax, log, best);
}

long long n_steps = 0, n_proven = 0, n_near = 0, n_far = 0, n_loose = 0;
const float INF = INFINITY;

// the hull end's quotient, or NaN where the kernel's range test on the quotient fails.  The test implies the
// short division's own range (bad_range counts the cases where it would not): the quotient is then RN(n / d),
// the value the lanes compute.
long long bad_range = 0;
float hull_quot(float n, float d) {
    const float q = n / d;
    if (!(fabsf(q) >= 0x1p-59f && fabsf(q) <= 0x1p59f)) return NAN;
    const float y = 1.f / d, q0 = n * y;
    if (!(fabsf(d) >= 0x1p-40f && fabsf(d) <= 0x1p40f && fabsf(q0) >= 0x1p-60f && fabsf(q0) <= 0x1p60f)) bad_range++;
    return q;
}

// The packet traversal of wf_trace_packet with the unanimous steps.  live: the ray has a query.
void packet(int nr, const std::vector<std::vector<float>> &dir, const std::vector<char> &live, std::vector<float> tmin,
            std::vector<float> tmax, std::vector<std::vector<Rec>> &log, std::vector<int> &found,
            std::vector<float> &best, size_t store) {
    const uint32_t INACTIVE = 0xffffffffu;
    std::vector<char> active(live);
    struct Entry {
        int node;
        std::vector<uint32_t> t;
        float eT, eM;
    };
    std::vector<Entry> stack;
    auto bits = [](float f) {
        uint32_t u;
        memcpy(&u, &f, 4);
        return u;
    };
    auto flt = [](uint32_t u) {
        float f;
        memcpy(&f, &u, 4);
        return f;
    };
    auto any = [&]() {
        for (int r = 0; r < nr; r++)
            if (active[r]) return true;
        return false;
    };
    // packet setup: the hull of the live rays' components, per axis (NaN ends: unusable)
    float dlo[3], dhi[3];
    for (int a = 0; a < 3; a++) {
        float lo = INF, hi = -INF;
        for (int r = 0; r < nr; r++)
            if (live[r] || mutant == 2) {
                lo = dir[r][a] < lo ? dir[r][a] : lo;
                hi = dir[r][a] > hi ? dir[r][a] : hi;
            }
        const bool ok = lo <= hi && ((lo > 0.f && hi > 0.f) || (lo < 0.f && hi < 0.f)) && fabsf(lo) >= 0x1p-40f &&
                        fabsf(lo) <= 0x1p40f && fabsf(hi) >= 0x1p-40f && fabsf(hi) <= 0x1p40f &&
                        fmaxf(fabsf(lo), fabsf(hi)) <= 2.f * fminf(fabsf(lo), fabsf(hi));
        dlo[a] = ok ? lo : NAN;
        dhi[a] = ok ? hi : NAN;
        if (ok) { // tight: both ends are some live ray's component
            bool al = false, ah = false;
            for (int r = 0; r < nr; r++)
                if (live[r]) al = al || dir[r][a] == lo, ah = ah || dir[r][a] == hi;
            if (!al || !ah) n_loose++;
        }
    }
    float Tub = -INF, Mlb = INF;
    for (int r = 0; r < nr; r++)
        if (live[r]) {
            Tub = tmax[r] > Tub ? tmax[r] : Tub;
            Mlb = tmin[r] < Mlb ? tmin[r] : Mlb;
        }
    int cn = 0;
    bool go = any();
    while (go) {
        bool popit = true;
        for (;;) {
            for (int r = 0; r < nr; r++) active[r] = active[r] && !culled(cn, r);
            if (!any()) break;
            const Node &n = tree[cn];
            if (n.axis < 0) {
                for (int r = 0; r < nr; r++) {
                    if (!active[r]) continue;
                    log[r].push_back({cn, tmin[r], tmax[r]});
                    for (float h : n.hits)
                        if (h >= 0.f && h < tmax[r]) {
                            tmax[r] = h;
                            best[r] = h;
                            found[r] = 1;
                        }
                }
                break;
            }
            const float oa = eye[n.axis];
            const int below = oa < n.split ? 1 : 0;
            const int nearc = n.child + (1 - below), farc = n.child + below;
            for (int r = 0; r < nr; r++) n_steps += active[r] ? 1 : 0;
            // the hull's two quotients; any NaN fails every compare below
            const float num = n.split - oa;
            const float q0 = hull_quot(num, dlo[n.axis]), q1 = hull_quot(num, dhi[n.axis]);
            const bool hv = q0 == q0 && q1 == q1;
            const float tl = hv ? (q0 < q1 ? q0 : q1) : NAN, th = hv ? (q0 < q1 ? q1 : q0) : NAN;
            const bool pnear = tl >= Tub || th < 0.f;
            const bool pfar = tl >= 0.f && (mutant == 1 ? th <= Mlb : th < Mlb);
            if (pnear || pfar) {
                for (int r = 0; r < nr; r++) n_proven += active[r] ? 1 : 0;
                (pnear ? n_near : n_far)++;
                cn = pnear ? nearc : farc;
                popit = false;
                break;
            }
            std::vector<float> tsp(nr);
            std::vector<char> crosses(nr), after(nr), to_near(nr), to_far(nr);
            bool anyn = false, anyf = false, stay = false;
            for (int r = 0; r < nr; r++) {
                tsp[r] = num / dir[r][n.axis];
                crosses[r] = !(tsp[r] >= tmax[r]) && !(tsp[r] < 0.f);
                after[r] = !(tsp[r] <= tmin[r]);
                to_near[r] = active[r] && (!crosses[r] || after[r]);
                to_far[r] = active[r] && crosses[r];
                anyn = anyn || to_near[r];
                anyf = anyf || to_far[r];
                stay = stay || (active[r] && !crosses[r]); // a near-only ray keeps its tmax
            }
            if (!anyn) {
                cn = farc;
            } else {
                if (anyf) {
                    bool parked = false; // far-only rays keep their own tmin
                    for (int r = 0; r < nr; r++) parked = parked || (to_far[r] && !after[r]);
                    Entry e{farc, std::vector<uint32_t>(nr), Tub, hv ? (parked && Mlb < tl ? Mlb : tl) : -INF};
                    for (int r = 0; r < nr; r++) e.t[r] = to_far[r] ? bits(tmax[r]) : INACTIVE;
                    stack.push_back(e);
                }
                for (int r = 0; r < nr; r++) {
                    const float nt = after[r] ? tsp[r] : tmin[r];
                    tmax[r] = to_far[r] ? nt : tmax[r];
                    active[r] = to_near[r];
                }
                if (hv && !stay) Tub = th < Tub ? th : Tub;
                cn = nearc;
            }
            popit = false;
            break;
        }
        if (!popit) continue;
        go = false;
        while (!stack.empty()) {
            Entry e = stack.back();
            stack.pop_back();
            cn = e.node;
            bool a = false;
            float rT = -INF, rM = INF; // the bounds by reduction over the re-activated rays
            for (int r = 0; r < nr; r++) {
                const bool act = live[r] && !found[r] && e.t[r] != INACTIVE;
                if (act) {
                    tmin[r] = tmax[r]; // the stack invariant
                    tmax[r] = flt(e.t[r]);
                    rT = tmax[r] > rT ? tmax[r] : rT;
                    rM = tmin[r] < rM ? tmin[r] : rM;
                }
                active[r] = act;
                a = a || act;
            }
            if (a) {
                if (mutant != 3) {
                    const bool kept = stack.size() < store; // this entry's slot held its bounds
                    // deeper than the storage: no bounds until refreshed (store 0: the min / max instead)
                    Tub = kept ? e.eT : (store ? INF : rT);
                    Mlb = kept ? e.eM : (store ? -INF : rM);
                }
                go = true;
                break;
            }
        }
    }
}

} // namespace

int main(int argc, char **argv) {
    rs ^= (uint64_t)strtoull(argc > 1 ? argv[1] : "1", nullptr, 10) * 0x9E3779B97F4A7C15ull;
    const int cases = argc > 2 ? atoi(argv[2]) : 200;
    mutant = argc > 3 ? atoi(argv[3]) : 0;
    long long viol = 0, rays = 0, tests = 0;
    for (int cs = 0; cs < cases; cs++) {
        tree.clear();
        scale = rnd() < 0.1 ? 0x1p-110f : 1.f;
        float lo[3] = {-10 * scale, -10 * scale, -10 * scale}, hi[3] = {10 * scale, 10 * scale, 10 * scale};
        build(6 + (int)(rnd() * 11), lo, hi);
        cull_seed = (uint32_t)next();
        for (int i = 0; i < 3; i++) eye[i] = (float)(rnd() * 16.0 - 8.0) * scale;
        if (rnd() < 0.3) { // an eye one ulp from a split plane
            std::vector<int> inner;
            for (size_t i = 0; i < tree.size(); i++)
                if (tree[i].axis >= 0) inner.push_back((int)i);
            if (!inner.empty()) {
                const Node &n = tree[inner[(size_t)(rnd() * inner.size())]];
                eye[n.axis] = nextafterf(n.split, rnd() < 0.5 ? -INF : INF);
            }
        }
        bool on_split = false; // (the host gives such an eye to the per-lane camera trace)
        for (const Node &n : tree)
            if (n.axis >= 0 && n.split == eye[n.axis]) on_split = true;
        if (on_split) continue;
        const int nr = 128;
        std::vector<std::vector<float>> dir(nr, std::vector<float>(3));
        std::vector<float> t0(nr), t1(nr);
        std::vector<char> live(nr, 1);
        float base[3] = {(float)(rnd() * 2 - 1), (float)(rnd() * 2 - 1), (float)(rnd() * 2 - 1)};
        // fan widths from a pixel's (1e-3) to one that straddles 0; per axis, a fan centred on 0 at times
        const float spread = (float)pow(10.0, rnd() * 3.5 - 3.5);
        for (int i = 0; i < 3; i++)
            if (rnd() < 0.1) base[i] = 0.f;
        // components at the short division's guard, 2^-40 / 2^40, on one axis
        const int gax = rnd() < 0.15 ? (int)(rnd() * 3) : -1;
        const float gmag = rnd() < 0.5 ? 0x1p-40f : 0x1p40f;
        const bool dead_mix = rnd() < 0.4;
        // root intervals: 0 random, 1 tsp == tmax, 2 tsp == tmin, 3 both equal, 4 one root-axis component for
        // the whole packet, every tmin == tsp and half the rays' tmax too (tsp_hi == Mlb with near-only rays)
        const int kind = (int)(rnd() * 5);
        for (int r = 0; r < nr; r++) {
            for (int i = 0; i < 3; i++) {
                dir[r][i] = base[i] + spread * (float)(rnd() * 2 - 1);
                if (rnd() < 0.01) dir[r][i] = 0.f;
            }
            if (kind == 4 && tree[0].axis >= 0) dir[r][tree[0].axis] = base[tree[0].axis];
            if (gax >= 0 && !(kind == 4 && tree[0].axis == gax)) { // a few ulps either side of the guard, both signs at times
                float g = gmag;
                for (int k = (int)(rnd() * 5); k > 0; k--) g = nextafterf(g, rnd() < 0.5 ? 0.f : INF);
                dir[r][gax] = (base[gax] < 0.f || (spread > 0.5f && rnd() < 0.1)) ? -g : g;
            }
            t0[r] = (rnd() < 0.5 ? 0.f : (float)(rnd() * 5)) * scale;
            t1[r] = t0[r] + (float)(rnd() * 40) * scale;
            if (tree[0].axis >= 0 && kind && rnd() < 0.5) { // ties at the root split
                const float ts = (tree[0].split - eye[tree[0].axis]) / dir[r][tree[0].axis];
                if (ts == ts && ts >= 0.f && fabsf(ts) < INF) {
                    if (kind == 1 && ts >= t0[r]) t1[r] = ts;
                    if (kind == 2 && ts <= t1[r]) t0[r] = ts;
                    if (kind == 3) t0[r] = t1[r] = ts;
                }
            }
            if (tree[0].axis >= 0 && kind == 4) {
                const float ts = (tree[0].split - eye[tree[0].axis]) / dir[r][tree[0].axis];
                if (ts == ts && ts >= 0.f && fabsf(ts) < INF) {
                    t0[r] = ts;
                    t1[r] = (r & 1) ? ts : ts + (float)(rnd() * 40) * scale;
                }
            }
            if (dead_mix && rnd() < 0.2) { // a dead slot (placeholder direction) or a ray that missed the root box
                live[r] = 0;
                if (rnd() < 0.5) dir[r][0] = 0.f, dir[r][1] = 0.f, dir[r][2] = 1.f;
            }
        }
        const size_t store = cs % 3 == 0 ? 0 : (cs % 3 == 1 ? 3 : 24);
        std::vector<std::vector<Rec>> lr(nr), lp(nr);
        std::vector<int> fr(nr, 0), fp(nr, 0);
        std::vector<float> br(nr, -1.f), bp(nr, -1.f);
        for (int r = 0; r < nr; r++)
            if (live[r]) fr[r] = ref(r, 0, dir[r].data(), t0[r], t1[r], lr[r], br[r]) ? 1 : 0;
        packet(nr, dir, live, t0, t1, lp, fp, bp, store);
        for (int r = 0; r < nr; r++) {
            rays += live[r] ? 1 : 0;
            tests += (long long)lr[r].size();
            bool same = fr[r] == fp[r] && br[r] == bp[r] && lr[r].size() == lp[r].size();
            for (size_t i = 0; same && i < lr[r].size(); i++)
                same = lr[r][i].leaf == lp[r][i].leaf && lr[r][i].t0 == lp[r][i].t0 && lr[r][i].t1 == lp[r][i].t1;
            if (!same) {
                if (viol < 5)
                    fprintf(stderr, "VIOLATION case %d ray %d: ref %zu leaves found %d, packet %zu leaves found %d\n", cs,
                            r, lr[r].size(), fr[r], lp[r].size(), fp[r]);
                viol++;
            }
        }
    }
    printf("violations %lld rays %lld leaf_tests %lld steps %lld proven %lld near %lld far %lld loose %lld\n", viol, rays,
           tests, n_steps, n_proven, n_near, n_far, n_loose);
    if (bad_range) fprintf(stderr, "hull quotients in range whose short division is not: %lld\n", bad_range);
    return viol || n_loose || bad_range ? 1 : 0;
}
