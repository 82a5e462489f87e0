// svr_label.hip -- the "islands" operations on region masks: the window's mask without a seed, connected-component labelling, the
// component table, selection by label and by size (svr_region_threshold, _label, _label_table, _select, _select_by_size; the contract
// is in include/svr_abi.h, the design in DESIGN.md 8j).  Integers only, on the mask layout and padding rule of svr_mask.hpp.
//
// LABEL: union-find by smallest index, in place in the label array L (uint32 [nz][ny][nx]).
//   NODES: a run of set bits inside one mask word is one node, named by the linear voxel index of its first voxel -- the smallest
//   index in it.  Only L[first voxel of a run] is ever read or written before the last pass; the other entries of L are written once,
//   by that pass.
//   k_label_init    one thread per mask word: L[start] = start for every run of the word.
//   k_label_union<CONN>  one thread per mask word.  For each run of the word: the run that ends the previous word of the row (bit 31
//     next to bit 0), and in each of the rows BEHIND it that the connectivity admits (dy = -1 in the same slice, dy = -1, 0, 1 in the
//     slice below) every run that touches it -- found on the words: the run itself (dx = 0) and, where the connectivity admits the
//     diagonal, the run moved one bit each way with the carry bits of the two neighbouring words.  One union per pair of runs, not per
//     pair of voxels.  (With SVR_LABEL_GLOBAL_ONLY the nodes are single voxels and the unions run over every voxel's 3 / 9 / 13
//     backward neighbours: the A/B build of tools/label_time.py.)
//     unite(a, b): find both roots (walk L[x] while L[x] < x), link the higher root under the lower with atomicMin, and if the value
//     displaced shows that the higher one was no longer a root, go on with (that value, the lower root).
//   k_label_flatten one thread per mask word: L[start] = root(start) for every run; a start that is its own root sets its bit in the
//     root mask (mask layout), and the word's popcount goes to the scan array.
//   k_scan_block / k_scan_add (svr_scan.hpp): exclusive scan of the popcounts, SVR_LABEL_SCAN_BLOCK words per block, one launch per level up and one
//     per level down; the block totals of a level are the next level's input, the top level is one word: K.
//   k_label_renumber one lane per voxel, 32 lanes per mask word: the lane of a run's start reads the root r and computes the label =
//     scan[word of r] + popcount(root bits of that word below r's bit) + 1; the other lanes of the run take it by a wave shuffle;
//     every lane writes its own L entry (0 for background).  No lane reads an entry another lane writes.
// TERMINATION and ORDER-INDEPENDENCE: a link always stores a smaller index into a larger one's entry (atomicMin never raises), so
//   L[x] <= x throughout and every walk strictly decreases x; a retry of unite replaces the higher of (a, b) by a smaller index.  No
//   lane or block waits for another.  Every walk and every retry loop also counts its iterations against the voxel count -- no legitimate
//   chain is longer -- and at the cap sets an error word and leaves: the host returns SVR_REGION_ERR_LABEL.  A tree's root is the smallest
//   index in it (induction over the links), two nodes share a root exactly when a chain of unions joins them, so after flatten L[start]
//   is the component's smallest voxel index whatever order the unions landed in, and the numbering by ascending root is unique.
// TABLE (k_label_table): one lane per voxel, 32 per mask word; a run is a row of adjacent lanes with the same non-zero label (any label array
//   will do, not only components).  The first lane of a run collects the run (count
//   from the ballot, sum of the raw values by a segmented shuffle sum) and issues one set of integer atomics on the run's table entry;
//   when every run a wave holds has the same label the wave reduces them first and one lane issues the atomics, so that a single large
//   component does not serialise the pass on its entry.
// SELECT (k_label_select): the same lane mapping; bit = keep[label] != 0, words assembled by ballot.
// THRESHOLD (k_label_threshold): the same lane mapping over the volume; bit = lo <= v <= hi inside the box.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_mask.hpp"             // RegionDims, valid_bits, half_ballot, the grids
#include "svr_scan.hpp"             // k_scan_block, k_scan_add
#include "svr_volume_host.hpp"

using svr::failf;

#define SVR_LABEL_SCAN_BLOCK 256    // words of a scan level that one block covers (= its threads); sunvolumerender_amd/host.py mirrors it

namespace {

constexpr int THREADS = MASK_THREADS;
static_assert(SVR_LABEL_SCAN_BLOCK == SCAN_BLOCK, "k_scan_block scans one word per thread");
static_assert(sizeof(svr_region_component) == 40, "svr_region_component is 40 bytes");

struct LabelBox { int x0, y0, z0, x1, y1, z1; };          // inclusive

// the lowest bit of the run of m that holds bit k
__device__ inline int run_start(uint32_t m, int k)
{
    const uint32_t z = ~m & ((1u << k) - 1u);
    return z ? 32 - __clz(z) : 0;
}

// one past the highest bit of the run of m that holds bit k
__device__ inline int run_end(uint32_t m, int k)
{
    const uint32_t z = ~m & ~((2u << k) - 1u);            // (k = 31: 2u << 31 = 0, so the mask is ~0xffffffff = 0)
    return z ? __ffs(z) - 1 : 32;
}

__device__ inline uint32_t load_entry(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr uint32_t NO_ROOT = 0xffffffffu;

// the root of x: x falls with every step, so every index read lies below the first; NO_ROOT (and *err set) after `cap` steps
__device__ inline uint32_t find_root(const uint32_t* L, uint32_t x, uint32_t cap, uint32_t* err)
{
    for (uint32_t i = 0; i <= cap; ++i) {
        const uint32_t p = load_entry(L + x);
        if (p >= x) return x;
        x = p;
    }
    atomicOr(err, 1u);
    return NO_ROOT;
}

__device__ inline void unite(uint32_t* L, uint32_t a, uint32_t b, uint32_t cap, uint32_t* err)
{
    for (uint32_t i = 0; i <= cap; ++i) {
        a = find_root(L, a, cap, err);
        b = find_root(L, b, cap, err);
        if (a == NO_ROOT || b == NO_ROOT || a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(L + a, b);        // a > b
        if (old == a) return;                             // a was still a root: linked under b
        a = old;                                          // a had been linked under `old` (< a) meanwhile: (old, b) remain to be joined
    }
    atomicOr(err, 2u);
}

struct WordAt { size_t i; int gw, gy, gz; size_t row; };
__device__ inline WordAt word_at(size_t i, const RegionDims& d)
{
    WordAt w;
    w.i = i;
    w.gw = (int)(i % (unsigned)d.wx);
    w.row = i / (unsigned)d.wx;
    w.gy = (int)(w.row % (unsigned)d.ny);
    w.gz = (int)(w.row / (unsigned)d.ny);
    return w;
}

// the mask word (gw, gy, gz) without padding; 0 outside the volume
__device__ inline uint32_t mask_word(const uint32_t* __restrict__ mask, int gw, int gy, int gz, const RegionDims& d)
{
    if (gw < 0 || gw >= d.wx || gy < 0 || gy >= d.ny || gz < 0 || gz >= d.nz) return 0u;
    return mask[((size_t)gz * d.ny + gy) * d.wx + gw] & valid_bits(gw, d);
}

#ifndef SVR_LABEL_GLOBAL_ONLY
__global__ __launch_bounds__(THREADS) void k_label_init(const uint32_t* __restrict__ mask, uint32_t* __restrict__ L, RegionDims d, size_t words)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const uint32_t m = mask[i] & valid_bits(w.gw, d);
    const uint32_t base = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)w.gw * 32u;
    for (uint32_t s = m & ~(m << 1); s; s &= s - 1u) {   // the first bits of the runs
        const uint32_t at = base + (uint32_t)(__ffs(s) - 1);
        L[at] = at;
    }
}

template <int CONN>
__global__ __launch_bounds__(THREADS) void k_label_union(const uint32_t* __restrict__ mask, uint32_t* L, RegionDims d, size_t words, uint32_t cap,
                                                         uint32_t* err)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const uint32_t m = mask[i] & valid_bits(w.gw, d);
    if (!m) return;
    const uint32_t base = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)w.gw * 32u;
    if ((m & 1u) && w.gw > 0) {                          // the run goes on from the previous word of the row
        const uint32_t pm = mask[i - 1];
        if (pm >> 31) unite(L, base, base - 32u + (uint32_t)run_start(pm, 31), cap, err);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {                        // the rows behind: (dy, dz) = (-1, 0), (-1, -1), (0, -1), (1, -1)
        const int dy = j == 0 ? -1 : j - 2, dz = j == 0 ? 0 : -1;
        const int k = (dz != 0) + (dy != 0);              // steps of the move besides the one in x
        const bool plain = k == 1 || CONN >= 18;          // dx = 0
        const bool shifted = k == 1 ? CONN >= 18 : CONN == 26;   // dx = +-1
        if (!plain) continue;
        const int y = w.gy + dy, z = w.gz + dz;
        if (y < 0 || y >= d.ny || z < 0) continue;
        const uint32_t nm = mask_word(mask, w.gw, y, z, d);
        const uint32_t pm = shifted ? mask_word(mask, w.gw - 1, y, z, d) : 0u, qm = shifted ? mask_word(mask, w.gw + 1, y, z, d) : 0u;
        if (!(nm | (pm >> 31) | (qm & 1u))) continue;
        const uint32_t nbase = (uint32_t)(((size_t)z * d.ny + y) * (size_t)d.nx) + (uint32_t)w.gw * 32u;
        for (uint32_t rest = m; rest;) {                  // the runs of this word
            const uint32_t low = rest & (0u - rest), t = rest + low, run = rest & ~t;
            rest &= t;
            const uint32_t me = base + (uint32_t)(__ffs(run) - 1);
            const uint32_t reach = shifted ? run | (run << 1) | (run >> 1) : run;
            for (uint32_t hit = nm & reach; hit;) {       // the runs of the neighbour word that the run touches: one union each
                const int b = __ffs(hit) - 1;
                unite(L, me, nbase + (uint32_t)run_start(nm, b), cap, err);
                const int e = run_end(nm, b);
                hit = e >= 32 ? 0u : hit & (0xffffffffu << e);
            }
            if (shifted) {
                if ((run & 1u) && (pm >> 31)) unite(L, me, nbase - 32u + (uint32_t)run_start(pm, 31), cap, err);
                if ((run >> 31) && (qm & 1u)) unite(L, me, nbase + 32u, cap, err);
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_label_flatten(const uint32_t* __restrict__ mask, uint32_t* L, RegionDims d, size_t words, uint32_t cap,
                                                           uint32_t* err, uint32_t* __restrict__ roots, uint32_t* __restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const uint32_t m = mask[i] & valid_bits(w.gw, d);
    const uint32_t base = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)w.gw * 32u;
    uint32_t rb = 0u;
    for (uint32_t s = m & ~(m << 1); s; s &= s - 1u) {
        const int b = __ffs(s) - 1;
        const uint32_t at = base + (uint32_t)b;
        const uint32_t r = find_root(L, at, cap, err);
        if (r == NO_ROOT) continue;
        if (r == at) rb |= 1u << b;
        else L[at] = r;                                   // (an ancestor: a walk of another thread that passes here stays in the tree)
    }
    roots[i] = rb;
    counts[i] = (uint32_t)__popc(rb);
}
#else
// ---- the A/B form: every voxel a node, every backward neighbour a union, no runs ----
__global__ __launch_bounds__(THREADS) void k_label_init(const uint32_t* __restrict__ mask, uint32_t* __restrict__ L, RegionDims d, size_t words)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const uint32_t base = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)w.gw * 32u;
    for (uint32_t s = mask[i] & valid_bits(w.gw, d); s; s &= s - 1u) {
        const uint32_t at = base + (uint32_t)(__ffs(s) - 1);
        L[at] = at;
    }
}

template <int CONN>
__global__ __launch_bounds__(THREADS) void k_label_union(const uint32_t* __restrict__ mask, uint32_t* L, RegionDims d, size_t words, uint32_t cap,
                                                         uint32_t* err)
{
    const size_t t = lane_thread();
    const size_t i = t >> 5;
    const int bit = (int)(t & 31u);
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const int x = w.gw * 32 + bit;
    if (x >= d.nx || !((mask[i] >> bit) & 1u)) return;
    const uint32_t me = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)x;
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;           // the 13 neighbours behind
                const int k = (dx != 0) + (dy != 0) + (dz != 0);
                if (k > (CONN == 6 ? 1 : CONN == 18 ? 2 : 3)) continue;
                const int ax = x + dx, ay = w.gy + dy, az = w.gz + dz;
                if (ax < 0 || ax >= d.nx || ay < 0 || ay >= d.ny || az < 0) continue;
                const size_t arow = (size_t)az * d.ny + ay;
                if ((mask[arow * d.wx + (ax >> 5)] >> (ax & 31)) & 1u) unite(L, me, (uint32_t)(arow * (size_t)d.nx) + (uint32_t)ax, cap, err);
            }
}

__global__ __launch_bounds__(THREADS) void k_label_flatten(const uint32_t* __restrict__ mask, uint32_t* L, RegionDims d, size_t words, uint32_t cap,
                                                           uint32_t* err, uint32_t* __restrict__ roots, uint32_t* __restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const WordAt w = word_at(i, d);
    const uint32_t base = (uint32_t)(w.row * (size_t)d.nx) + (uint32_t)w.gw * 32u;
    uint32_t rb = 0u;
    for (uint32_t s = mask[i] & valid_bits(w.gw, d); s; s &= s - 1u) {
        const int b = __ffs(s) - 1;
        const uint32_t at = base + (uint32_t)b;
        const uint32_t r = find_root(L, at, cap, err);
        if (r == NO_ROOT) continue;
        if (r == at) rb |= 1u << b;
        else L[at] = r;
    }
    roots[i] = rb;
    counts[i] = (uint32_t)__popc(rb);
}
#endif

// A lane of the kernels below: bit `bit` of mask word i.  This file keeps its own form of svr_mask.hpp's lane_at: with the shared one
// k_label_threshold and k_label_table<> came out with another instruction order (the same instructions and register counts), and the
// device code of these files is pinned (tools/kernel_asm_digest.py).
struct LabelLane { size_t i; int bit, x; bool inside; WordAt w; size_t v; };
__device__ inline LabelLane label_lane(const RegionDims& d, size_t words)
{
    LabelLane a;
    const size_t t = lane_thread();
    a.i = t >> 5;
    a.bit = (int)(t & 31u);
    const bool word_ok = a.i < words;
    a.w = word_at(word_ok ? a.i : 0, d);
    a.x = a.w.gw * 32 + a.bit;
    a.inside = word_ok && a.x < d.nx;
    a.v = a.w.row * (size_t)d.nx + (size_t)a.x;
    return a;
}

__global__ __launch_bounds__(THREADS) void k_label_renumber(const uint32_t* __restrict__ mask, uint32_t* L, RegionDims d, size_t words,
                                                            const uint32_t* __restrict__ roots, const uint32_t* __restrict__ scan)
{
    const LabelLane a = label_lane(d, words);
    const uint32_t m = a.i < words ? mask[a.i] & valid_bits(a.w.gw, d) : 0u;
    const bool set = (m >> a.bit) & 1u;
    const int s = run_start(m, a.bit);
#ifdef SVR_LABEL_GLOBAL_ONLY
    const bool reads = set;
#else
    const bool reads = set && s == a.bit;
#endif
    uint32_t lab = 0u;
    if (reads) {
        const uint32_t r = L[a.v];                        // the root: this lane's own entry
        const uint32_t rrow = r / (uint32_t)d.nx, rx = r % (uint32_t)d.nx;
        const size_t rw = (size_t)rrow * d.wx + (rx >> 5);
        if (rw < words) lab = scan[rw] + (uint32_t)__popc(roots[rw] & ((1u << (rx & 31u)) - 1u)) + 1u;
    }
#ifndef SVR_LABEL_GLOBAL_ONLY
    lab = (uint32_t)__shfl((int)lab, (int)(threadIdx.x & 32) + s);
#endif
    if (a.inside) L[a.v] = set ? lab : 0u;
}

__device__ inline uint32_t shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src); }

__global__ void k_table_init(svr_region_component* t, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    svr_region_component c;
    c.voxels = 0u; c.first = 0xffffffffu; c.sum = 0u;
    for (int a = 0; a < 3; ++a) { c.bbox_min[a] = INT_MAX; c.bbox_max[a] = -1; }
    t[i] = c;
}

template <bool COMBINE>
__global__ __launch_bounds__(THREADS) void k_label_table(const uint32_t* __restrict__ labels, const uint16_t* __restrict__ vox, RegionDims d, size_t words,
                                                         uint32_t count, svr_region_component* table)
{
    const LabelLane a = label_lane(d, words);
    const int lane = threadIdx.x & 63;
    uint32_t lab = a.inside ? labels[a.v] : 0u;
    if (lab > count) lab = 0u;                            // (a label the table has no entry for is ignored)
    const uint32_t m = half_ballot(lab != 0u);
    const bool set = lab != 0u;
    // a run: adjacent set lanes of a word with ONE label (component labels have one per run of set lanes; the zones of svr_region_split need not)
    const uint32_t before = shfl_u32(lab, lane > 0 ? lane - 1 : lane);
    const bool head = set && (a.bit == 0 || before != lab);
    const uint32_t later = half_ballot(head) & ~((2u << a.bit) - 1u);        // the heads after this lane (bit 31: 2u << 31 = 0, so none)
    const int end = min(run_end(m, a.bit), later ? __ffs(later) - 1 : 32);  // (of the run of this lane, if it is set)
    uint32_t sum32 = set && vox ? vox[a.v] : 0u;          // the sum over this lane and those after it in the run: at most 32 * 65535
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const uint32_t t = shfl_u32(sum32, lane + off < 64 ? lane + off : lane);
        if (set && a.bit + off < end) sum32 += t;
    }
    uint32_t n = head ? (uint32_t)(end - a.bit) : 0u;
    unsigned long long sum = head ? sum32 : 0ull;
    uint32_t first = head ? (uint32_t)a.v : 0xffffffffu;
    int x0 = head ? a.x : INT_MAX, x1 = head ? a.x + (end - a.bit) - 1 : -1;
    int y0 = head ? a.w.gy : INT_MAX, y1 = head ? a.w.gy : -1, z0 = head ? a.w.gz : INT_MAX, z1 = head ? a.w.gz : -1;
    bool issue = head;
    if (COMBINE) {
        const unsigned long long heads = __ballot(head);
        if (!heads) return;
        const int src = __ffsll((long long)heads) - 1;
        const uint32_t ref = shfl_u32(lab, src);
        if (__all(!head || lab == ref)) {                 // one label in the whole wave: reduce, and one lane issues the atomics
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int p = lane ^ off;
                n += shfl_u32(n, p);
                const uint32_t lo = shfl_u32((uint32_t)sum, p), hi = shfl_u32((uint32_t)(sum >> 32), p);
                sum += ((unsigned long long)hi << 32) | lo;
                first = min(first, shfl_u32(first, p));
                x0 = min(x0, __shfl(x0, p)); x1 = max(x1, __shfl(x1, p));
                y0 = min(y0, __shfl(y0, p)); y1 = max(y1, __shfl(y1, p));
                z0 = min(z0, __shfl(z0, p)); z1 = max(z1, __shfl(z1, p));
            }
            lab = ref;
            issue = lane == 0;
        }
    }
    if (!issue) return;
    svr_region_component* e = table + (lab - 1u);
    atomicAdd(&e->voxels, n);
    atomicMin(&e->first, first);
    atomicMin(&e->bbox_min[0], x0); atomicMax(&e->bbox_max[0], x1);
    atomicMin(&e->bbox_min[1], y0); atomicMax(&e->bbox_max[1], y1);
    atomicMin(&e->bbox_min[2], z0); atomicMax(&e->bbox_max[2], z1);
    if (vox) atomicAdd((unsigned long long*)&e->sum, sum);
}

__global__ __launch_bounds__(THREADS) void k_label_select(const uint32_t* __restrict__ labels, RegionDims d, size_t words, uint32_t count,
                                                          const uint8_t* __restrict__ keep, uint32_t* __restrict__ out)
{
    const LabelLane a = label_lane(d, words);
    const uint32_t lab = a.inside ? labels[a.v] : 0u;
    const bool on = lab != 0u && lab <= count && keep[lab] != 0;
    const uint32_t wv = half_ballot(on);
    if (a.bit == 0 && a.i < words) out[a.i] = wv;
}

__global__ __launch_bounds__(THREADS) void k_label_threshold(const uint16_t* __restrict__ vox, RegionDims d, size_t words, uint32_t lo, uint32_t hi, LabelBox b,
                                                             uint32_t* __restrict__ out)
{
    const LabelLane a = label_lane(d, words);
    bool on = false;
    if (a.inside && a.x >= b.x0 && a.x <= b.x1 && a.w.gy >= b.y0 && a.w.gy <= b.y1 && a.w.gz >= b.z0 && a.w.gz <= b.z1) {   // (voxels outside the box are not read)
        const uint32_t v = vox[a.v];
        on = v >= lo && v <= hi;
    }
    const uint32_t wv = half_ballot(on);
    if (a.bit == 0 && a.i < words) out[a.i] = wv;
}

// ---------------- host side ----------------
CallEvents g_events;                                      // around the device work of the last call of this file (svr_region_label_last_ms)

hipError_t launch_select(hipStream_t st, const uint32_t* labels, const RegionDims& d, uint32_t count, const uint8_t* keep, uint32_t* out)
{
    const size_t words = mask_words(d);
    hipLaunchKernelGGL(k_label_select, lane_grid(words), dim3(THREADS), 0, st, labels, d, words, count, keep, out);
    return hipGetLastError();
}

} // namespace

extern "C" {

int svr_region_threshold(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, uint32_t lo, uint32_t hi, const int32_t* box_min,
                         const int32_t* box_max, uint32_t* out_mask_device)
{
    const char* who = "svr_region_threshold";
    if (!voxels || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (lo > hi || hi > 65535u) return failf(-3, "%s: the window must satisfy lo <= hi <= 65535 (got %u .. %u)", who, lo, hi);
    if ((box_min == nullptr) != (box_max == nullptr)) return failf(-3, "%s: the box needs both box_min and box_max, or neither", who);
    int b0[3] = {0, 0, 0}, b1[3] = {nx - 1, ny - 1, nz - 1};
    if (box_min)
        if (int e = clamp_box(who, box_min, box_max, nx, ny, nz, b0, b1)) return e;
    const LabelBox box = {b0[0], b0[1], b0[2], b1[0], b1[1], b1[2]};
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    DeviceVoxels dv;
    SVR_HIP_TRY(dv.get(voxels, (size_t)nx * ny * nz, src_is_device, st));
    hipLaunchKernelGGL(k_label_threshold, lane_grid(words), dim3(THREADS), 0, st, dv.p, d, words, lo, hi, box, out_mask_device);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    if (dv.owned()) SVR_HIP_TRY(hipStreamSynchronize(st));   // the upload is freed on return
    return 0;
}

int svr_region_label(const uint32_t* in_mask_device, int nx, int ny, int nz, int connectivity, uint32_t* labels_device, uint32_t* count_out)
{
    const char* who = "svr_region_label";
    if (!in_mask_device || !labels_device || !count_out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    const uint32_t cap = (uint32_t)((size_t)nx * ny * nz);   // no chain is longer than the voxel count (<= 2^31)
    // the scan's levels: words, blocks of words, blocks of blocks, ... , 1 (the total)
    ScanLevels scan(words);
    DeviceBuffer buf;                                    // the root mask, the scan levels, the error word
    SVR_HIP_TRY(buf.alloc((words + scan.words() + 1) * sizeof(uint32_t)));
    CallTimer timer(g_events, st);                        // (the launches, not the allocation)
    uint32_t* roots = buf.as<uint32_t>();
    scan.place(roots + words);
    uint32_t* d_err = scan.total() + 1;
    SVR_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(uint32_t), st));
    const dim3 wg = word_grid(words), b(THREADS);
    hipLaunchKernelGGL(k_label_init, wg, b, 0, st, in_mask_device, labels_device, d, words);
#ifdef SVR_LABEL_GLOBAL_ONLY
    const dim3 ug = lane_grid(words);
#else
    const dim3 ug = wg;
#endif
    if (connectivity == 6) hipLaunchKernelGGL((k_label_union<6>), ug, b, 0, st, in_mask_device, labels_device, d, words, cap, d_err);
    else if (connectivity == 18) hipLaunchKernelGGL((k_label_union<18>), ug, b, 0, st, in_mask_device, labels_device, d, words, cap, d_err);
    else hipLaunchKernelGGL((k_label_union<26>), ug, b, 0, st, in_mask_device, labels_device, d, words, cap, d_err);
    hipLaunchKernelGGL(k_label_flatten, wg, b, 0, st, in_mask_device, labels_device, d, words, cap, d_err, roots, scan.at[0]);
    SVR_HIP_TRY(hipGetLastError());
    SVR_HIP_TRY(scan.run(st));
    hipLaunchKernelGGL(k_label_renumber, lane_grid(words), b, 0, st, in_mask_device, labels_device, d, words, roots, scan.at[0]);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    uint32_t back[2] = {0u, 0u};                          // the total, the error word (adjacent)
    SVR_HIP_TRY(hipMemcpyAsync(back, scan.total(), sizeof back, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (buf is freed on return)
    if (back[1]) return failf(SVR_REGION_ERR_LABEL, "%s: a union-find walk reached its iteration cap (%u; flags %u); the labels are not valid", who, cap, back[1]);
    *count_out = back[0];
    return 0;
}

int svr_region_label_table(const uint32_t* labels_device, const uint16_t* voxels_or_null, int nx, int ny, int nz, int src_is_device, uint32_t count,
                           svr_region_component* table_device)
{
    const char* who = "svr_region_label_table";
    if (!labels_device || !table_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (count == 0u) return failf(-3, "%s: count must be at least 1 (a caller with no component has no table)", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    DeviceVoxels dv;
    if (voxels_or_null) SVR_HIP_TRY(dv.get(voxels_or_null, (size_t)nx * ny * nz, src_is_device, st));
    hipLaunchKernelGGL(k_table_init, dim3((count + THREADS - 1) / THREADS), dim3(THREADS), 0, st, table_device, count);
#ifdef SVR_LABEL_TABLE_PLAIN                               // (the A/B build of tools/label_time.py: every run issues its own atomics)
    hipLaunchKernelGGL((k_label_table<false>), lane_grid(words), dim3(THREADS), 0, st, labels_device, dv.p, d, words, count, table_device);
#else
    hipLaunchKernelGGL((k_label_table<true>), lane_grid(words), dim3(THREADS), 0, st, labels_device, dv.p, d, words, count, table_device);
#endif
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    if (dv.owned()) SVR_HIP_TRY(hipStreamSynchronize(st));   // the upload is freed on return
    return 0;
}

int svr_region_select(const uint32_t* labels_device, int nx, int ny, int nz, uint32_t count, const uint8_t* keep_device, uint32_t* out_mask_device)
{
    const char* who = "svr_region_select";
    if (!labels_device || !keep_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (count == 0u) return failf(-3, "%s: count must be at least 1 (a caller with no component has nothing to select)", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_select(st, labels_device, make_dims(nx, ny, nz), count, keep_device, out_mask_device));
    return 0;
}

int svr_region_select_by_size(const uint32_t* labels_device, int nx, int ny, int nz, uint32_t count, const svr_region_component* table_device,
                              uint32_t min_voxels, uint32_t largest_k, uint32_t* out_mask_device, uint32_t* kept_out)
{
    const char* who = "svr_region_select_by_size";
    if (!labels_device || !table_device || !out_mask_device || !kept_out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (count == 0u) return failf(-3, "%s: count must be at least 1 (a caller with no component has nothing to select)", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    DeviceBuffer d_keep;
    std::vector<svr_region_component> table(count);
    SVR_HIP_TRY(hipMemcpyAsync(table.data(), table_device, (size_t)count * sizeof(svr_region_component), hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    std::vector<std::pair<uint32_t, uint32_t>> cand;      // (size, label) of the components that are large enough
    for (uint32_t i = 0; i < count; ++i)
        if (table[i].voxels >= min_voxels && table[i].voxels > 0u) cand.emplace_back(table[i].voxels, i + 1u);
    if (largest_k != 0u && cand.size() > largest_k) {     // size descending, label ascending: ties go to the lower label
        std::partial_sort(cand.begin(), cand.begin() + largest_k, cand.end(),
                          [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        cand.resize(largest_k);
    }
    std::vector<uint8_t> keep((size_t)count + 1u, 0);
    for (const auto& c : cand) keep[c.second] = 1;
    SVR_HIP_TRY(d_keep.alloc(keep.size()));
    SVR_HIP_TRY(hipMemcpyAsync(d_keep.p, keep.data(), keep.size(), hipMemcpyHostToDevice, st));
    SVR_HIP_TRY(launch_select(st, labels_device, make_dims(nx, ny, nz), count, d_keep.as<uint8_t>(), out_mask_device));
    timer.stop();
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (d_keep is freed on return)
    *kept_out = (uint32_t)cand.size();
    return 0;
}

int svr_region_label_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_label_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
