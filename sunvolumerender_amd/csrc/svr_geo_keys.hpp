// svr_geo_keys.hpp -- what the two relaxations on packed (cost << 32) | zone keys share (svr_geodesic.hip, svr_growcut.hip): the classes
// of a move and their weights, and the whole-pair accesses to a key that another thread may write (ONE WRITER, WHOLE PAIRS at the head
// of svr_geodesic.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

// w[c]: the weight of move class c (x, y, z, xy, xz, yz, xyz); reach bit c: a tile in a direction of class c can see this tile's keys
struct GeoWeights { uint32_t w[7]; uint32_t reach; };

// the class of a move or direction from the coordinates it changes
__host__ __device__ constexpr int move_class(int dx, int dy, int dz)
{
    const int m = (dx != 0 ? 1 : 0) | (dy != 0 ? 2 : 0) | (dz != 0 ? 4 : 0);
    return m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 3 ? 3 : m == 5 ? 4 : m == 6 ? 5 : 6;
}

// a tile in a direction that changes the coordinates S sees this tile through the moves that change at least S
inline uint32_t geo_reach(const uint32_t w[7])
{
    static const int bits[7] = {1, 2, 4, 3, 5, 6, 7};
    uint32_t reach = 0u;
    for (int dir = 0; dir < 7; ++dir)
        for (int c = 0; c < 7; ++c)
            if (w[c] && (bits[c] & bits[dir]) == bits[dir]) reach |= 1u << dir;
    return reach;
}

__device__ inline uint64_t lds_get(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void lds_put(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline uint64_t key_get(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void key_put(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

} // namespace
