// CPU check of the restated libstdc++ distributions (oracle.c rng_uniform / rng_index, device_math.hpp the same):
// a scripted URBG (min() = 0, max() = 2^32 - 1, values from a list) through this machine's real
// std::uniform_real_distribution<float>(a, b) and std::uniform_int_distribution<int>(0, n - 1), the two the
// reference draws through (rayTracer.cpp, scene.cpp:79-82).  Built and run by tests/test_rng_distributions.py.
//   rngdist_check <cases.txt>
// Per input line one output line:
//   R <a bits> <b bits> <draws...>   ->  <value bits> <draws consumed>
//   I <n> <draws...>                 ->  <value> <draws consumed>     uniform_int_distribution<int>, n <= 2^31
//   U <n> <draws...>                 ->  <value> <draws consumed>     uniform_int_distribution<unsigned>: the same
//                                                                     code path for the n an int cannot hold
// "exhausted" instead when the distribution asks for more draws than the line holds.  The first line of the
// output names the library: "libstdc++ <_GLIBCXX_RELEASE> <__GLIBCXX__>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

struct Scripted {
    typedef uint32_t result_type;
    static constexpr result_type min() { return 0u; }
    static constexpr result_type max() { return 0xFFFFFFFFu; }
    const std::vector<uint32_t> &v;
    size_t at = 0;
    explicit Scripted(const std::vector<uint32_t> &values) : v(values) {}
    result_type operator()() {
        if (at >= v.size()) throw std::out_of_range("script exhausted");
        return v[at++];
    }
};

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
#ifdef _GLIBCXX_RELEASE
    printf("libstdc++ %d %d\n", (int)_GLIBCXX_RELEASE, (int)__GLIBCXX__);
#else
    printf("libstdc++ 0 0\n");
#endif
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        char kind = 0;
        uint64_t p0 = 0, p1 = 0, d;
        ls >> kind >> p0;
        if (kind == 'R') ls >> p1;
        std::vector<uint32_t> draws;
        while (ls >> d) draws.push_back((uint32_t)d);
        Scripted g(draws);
        try {
            if (kind == 'R') {
                const uint32_t ab = (uint32_t)p0, bb = (uint32_t)p1;
                float a, b;
                std::memcpy(&a, &ab, 4);
                std::memcpy(&b, &bb, 4);
                std::uniform_real_distribution<float> dist(a, b);
                const float x = dist(g);
                uint32_t xb;
                std::memcpy(&xb, &x, 4);
                printf("%u %zu\n", xb, g.at);
            } else if (kind == 'I') {
                if (p0 == 0 || p0 > 0x80000000ull) return 2;
                std::uniform_int_distribution<int> dist(0, (int)(p0 - 1));
                const int x = dist(g);
                printf("%d %zu\n", x, g.at);
            } else if (kind == 'U') {
                if (p0 == 0 || p0 > 0xFFFFFFFFull) return 2;
                std::uniform_int_distribution<unsigned> dist(0u, (unsigned)(p0 - 1));
                const unsigned x = dist(g);
                printf("%u %zu\n", x, g.at);
            } else {
                return 2;
            }
        } catch (const std::out_of_range &) {
            printf("exhausted\n");
        }
    }
    return 0;
}
