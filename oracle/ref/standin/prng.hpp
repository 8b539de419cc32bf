// Stand-in for the reference's missing include/prng.hpp -- TEST INFRASTRUCTURE
// ONLY (oracle/_ref).  It declares the three names the reference's call sites
// use (PRNG::rng[thread], PRNG::setSeed, PRNG::uniformFloat).
//
// The generator is SCRIPTED: a 32-bit URBG that pops the next word of an array
// the harness was handed (oracle/ref/ref_hot.cpp), counts the words consumed and
// raises a flag when asked for more than it was given.  The words themselves
// come from the project's counter stream (pyoracle.rng_draws), so the stream has
// one definition; what the reference's objects add is libstdc++'s own
// std::uniform_int_distribution (Scene::randomLight, src/scene.cpp) and
// std::uniform_real_distribution<float> (uniformFloat, defined in ref_hot.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <random>

namespace PRNG {

struct ScriptedURBG {
    typedef std::uint32_t result_type;
    static constexpr result_type min() { return 0u; }
    static constexpr result_type max() { return 0xffffffffu; }
    result_type operator()();
};

struct Script {
    const std::uint32_t *words;
    std::size_t count;
    std::size_t used;
    bool overrun;
};
extern Script script;

extern ScriptedURBG rng[1];
void setSeed();
float uniformFloat(float a, float b);

} // namespace PRNG
