// raysort.hpp -- the tile geometry of the queue sort (raysort.hip) and the workspace it needs: host
// arithmetic only, so the pass plan (wfplan.hpp) sizes a chunk's sort workspace without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cr {

constexpr uint32_t RS_BITS = 8, RS_BINS = 1u << RS_BITS;
constexpr uint32_t RS_THREADS = 256, RS_WAVES = RS_THREADS / 64, RS_ROUNDS = 16;
constexpr uint32_t RS_TILE = RS_THREADS * RS_ROUNDS; // 4096 pairs
constexpr uint32_t RS_SEG = RS_THREADS * 16;         // scan segment: 4096 histogram entries

// Workspace: H [256][ntiles] + segment sums.
inline size_t rs_tmp_bytes(uint32_t n) {
    const size_t ntiles = (n + RS_TILE - 1) / RS_TILE;
    const size_t m = RS_BINS * ntiles, nseg = (m + RS_SEG - 1) / RS_SEG;
    return (m + nseg) * sizeof(uint32_t) + 256;
}

} // namespace cr
