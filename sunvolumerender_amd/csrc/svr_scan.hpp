// svr_scan.hpp -- the exclusive scan of per-word counts that gives items their ranks: SCAN_BLOCK words per block, one launch per level
// up (k_scan_block: the block totals of a level are the next level's input) and one per level down (k_scan_add).  Included by
// svr_label.hip (the numbers of the components) and svr_mesh.hip (the numbers of the vertices and of the quads).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "svr_mask.hpp"             // MASK_THREADS, word_grid

namespace {

constexpr int SCAN_BLOCK = MASK_THREADS;                 // words of a scan level that one block covers (= its threads)

// exclusive scan of SCAN_BLOCK words per block, in place; the block's total goes to sums[block]
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_block(uint32_t* __restrict__ data, size_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t s[2][SCAN_BLOCK];
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + tid;
    const uint32_t v = i < n ? data[i] : 0u;
    s[0][tid] = v;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
        s[cur ^ 1][tid] = s[cur][tid] + (tid >= off ? s[cur][tid - off] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    if (i < n) data[i] = s[cur][tid] - v;
    if (tid == SCAN_BLOCK - 1) sums[blockIdx.x] = s[cur][tid];
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_add(uint32_t* __restrict__ data, size_t n, const uint32_t* __restrict__ sums)
{
    const size_t i = (size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i < n) data[i] += sums[blockIdx.x];
}

// The levels of a scan over n words: n, blocks of words, blocks of blocks, ..., 1 (the total).  place() lays them out back to back from
// `base` (words() uint32); run() scans level 0 in place and leaves the total in *total().
struct ScanLevels {
    std::vector<size_t> level;
    std::vector<uint32_t*> at;
    explicit ScanLevels(size_t n)
    {
        level.push_back(n);
        do level.push_back((level.back() + SCAN_BLOCK - 1) / SCAN_BLOCK); while (level.back() > 1);
    }
    size_t words() const { size_t w = 0; for (size_t n : level) w += n; return w; }
    void place(uint32_t* base)
    {
        at.resize(level.size());
        at[0] = base;
        for (size_t j = 1; j < level.size(); ++j) at[j] = at[j - 1] + level[j - 1];
    }
    uint32_t* total() const { return at.back(); }
    hipError_t run(hipStream_t st) const
    {
        const dim3 b(SCAN_BLOCK);
        for (size_t j = 0; j + 1 < level.size(); ++j) hipLaunchKernelGGL(k_scan_block, word_grid(level[j]), b, 0, st, at[j], level[j], at[j + 1]);
        for (size_t j = level.size() - 2; j-- > 0;)       // (the top level that was scanned is one block: nothing to add to it)
            hipLaunchKernelGGL(k_scan_add, word_grid(level[j]), b, 0, st, at[j], level[j], at[j + 1]);
        return hipGetLastError();
    }
};

} // namespace
