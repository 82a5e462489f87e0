// svr_morph.hip -- what operates on a region mask once it exists: dilate / erode / open / close, set operations, regrowth from a mask
// inside a mask, hole filling and the cutting of thin leaks (svr_region_morph, _combine, _reconstruct, _fill_holes, _detach; the
// contract is in include/svr_abi.h, the design in DESIGN.md 8i).  Integers only, on the mask layout and padding rule of svr_mask.hpp:
// every kernel here ANDs what it loads and what it stores with the word's valid bits.
//
// MORPH: radius r = r unit steps (open / close: r of one polarity, then r of the other).  Steps of one polarity are made four at a
//   time (k_morph_fused<ELEMENT, ERODE, 4>), then two (<.., 2>), then one (k_morph_step<ELEMENT, ERODE>) -- the fused forms measured
//   faster than single steps at radius 2, 4 and 8 -- and the launches ping-pong between `out` and one temporary so that
//   the last lands in `out`.
//   k_morph_step: one thread per mask word.  The thread ORs the words of the 3 x 3 rows around its own that the element admits, by the
//   plain / shifted table of k_region_grow: `plain` takes the word as it is (dx = 0), `shifted` takes it moved one bit each way with
//   the carry bit of the neighbouring word (dx = +-1).  Words outside the volume read as 0, so nothing enters from outside.  Erode is
//   the dual on complemented loads, erode(M) = NOT dilate(NOT M): the complement of a word outside the volume and of the padding is
//   0, i.e. they read as SET, and a region that touches a face is not eroded from it.
//   k_morph_fused: one block per grow tile (4 words x 8 rows x 8 slices) loads the tile with a halo of S rows / slices and one word in
//   x into LDS (S = 4: 16 x 16 x 6 words, twice: 12 KB) and makes the S steps there, by the same table.
// COMBINE (k_mask_combine): one streaming pass, a thread reads and writes its own word (so `out` may alias an input).
// RECONSTRUCT: k_recon_seed -- one block per grow tile, one thread per word -- writes the cleaned candidates (the source mask or its
//   complement, padding cleared: k_region_grow treats every bit of a candidate word as a voxel, so set padding would carry the region
//   from row to row through voxels that do not exist, and into the output's padding) and region = marker &
//   candidates, where the marker is a mask or, for hole filling, the six faces of the volume; a tile that got a bit marks itself and
//   its 26 neighbours dirty for the first sweep.  Then the sweep loop of svr_region_grow.hpp runs k_region_grow<CONN> to the fixpoint:
//   the same kernel, the same worklist, the same cap.  The termination argument of svr_region.hip holds as it stands: a tile that is
//   not marked holds no bit and sees none.
// FILL HOLES = NOT reconstruct(faces, NOT in); DETACH = dilate(reconstruct(dilate(seeds), erode(in))) & in: host compositions of the
//   above (k_mask_points sets the seed voxels in a zeroed mask).
//
// No block waits for another: there is no flag to spin on and no barrier wider than a block.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_region_grow.hpp"      // the grow kernel and its sweep loop; svr_mask.hpp
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int THREADS = MASK_THREADS;

struct MorphSeeds { int n; int xyz[SVR_REGION_MAX_SEEDS][3]; };

template <int ELEMENT, bool ERODE>
__global__ __launch_bounds__(THREADS) void k_morph_step(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims d, unsigned long long words)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const int gw = (int)(i % (unsigned)d.wx);
    const unsigned long long row = i / (unsigned)d.wx;
    const int gy = (int)(row % (unsigned)d.ny), gz = (int)(row / (unsigned)d.ny);
    // a word of the (complemented, for erode) input; 0 outside the volume and in the padding
    auto word = [&](int w, int y, int z) -> uint32_t {
        if (w < 0 || w >= d.wx || y < 0 || y >= d.ny || z < 0 || z >= d.nz) return 0u;
        const uint32_t m = in[((size_t)z * d.ny + y) * d.wx + w];
        return (ERODE ? ~m : m) & valid_bits(w, d);
    };
    uint32_t n = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int k = (dz != 0) + (dy != 0);                                         // steps of the move besides the one in x
            const bool plain = k <= 1 ? true : ELEMENT >= 18;                            // dx = 0 (the centre word included)
            const bool shifted = k == 0 ? true : k == 1 ? ELEMENT >= 18 : ELEMENT == 26; // dx = +-1
            if (!plain && !shifted) continue;
            const uint32_t m = word(gw, gy + dy, gz + dz);
            if (plain) n |= m;
            if (shifted) n |= (m << 1) | (m >> 1) | (word(gw - 1, gy + dy, gz + dz) >> 31) | (word(gw + 1, gy + dy, gz + dz) << 31);
        }
    out[i] = (ERODE ? ~n : n) & valid_bits(gw, d);
}

// S unit steps in one launch: a block takes a grow tile (4 words x 8 rows x 8 slices) with a halo of S rows / slices and one word in x
// into LDS and iterates there; after step s the cells nearer than s to the edge of the buffer are stale, so the centre is exact after S
// steps (one word of x halo carries up to 32 steps).  Words outside the volume and padding bits are forced to 0 after every step, as
// the one-step kernel reads them.
template <int ELEMENT, bool ERODE, int S>
__global__ __launch_bounds__(GROW_THREADS) void k_morph_fused(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims d, int ntx, int nty)
{
    constexpr int BX = TWX + 2, BY = TY + 2 * S, BZ = TZ + 2 * S, CELLS = BX * BY * BZ, PER = (CELLS + GROW_THREADS - 1) / GROW_THREADS;
    __shared__ uint32_t buf[2][BZ][BY][BX];
    const size_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    uint32_t keep[PER];                                  // the valid bits of each of this thread's cells; 0 outside the volume
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * GROW_THREADS;
        keep[j] = 0u;
        if (i >= CELLS) continue;
        const int hx = i % BX, hy = (i / BX) % BY, hz = i / (BX * BY);
        const int gw = tx * TWX + hx - 1, gy = ty * TY + hy - S, gz = tz * TZ + hz - S;
        uint32_t m = 0u;
        if (gw >= 0 && gw < d.wx && gy >= 0 && gy < d.ny && gz >= 0 && gz < d.nz) {
            keep[j] = valid_bits(gw, d);
            m = in[((size_t)gz * d.ny + gy) * d.wx + gw];
            m = (ERODE ? ~m : m) & keep[j];
        }
        buf[0][hz][hy][hx] = m;
    }
    __syncthreads();
#pragma unroll
    for (int s = 1; s <= S; ++s) {
        const int from = (s - 1) & 1, to = s & 1;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * GROW_THREADS;
            if (i >= CELLS) continue;
            const int hx = i % BX, hy = (i / BX) % BY, hz = i / (BX * BY);
            if (hy < s || hy >= BY - s || hz < s || hz >= BZ - s) continue;              // stale from here on: never read by a cell that counts
            uint32_t n = 0u;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const int k = (dz != 0) + (dy != 0);
                    const bool plain = k <= 1 ? true : ELEMENT >= 18;
                    const bool shifted = k == 0 ? true : k == 1 ? ELEMENT >= 18 : ELEMENT == 26;
                    if (!plain && !shifted) continue;
                    const uint32_t* row = buf[from][hz + dz][hy + dy];
                    const uint32_t m = row[hx];
                    if (plain) n |= m;
                    if (shifted) n |= (m << 1) | (m >> 1) | (hx > 0 ? row[hx - 1] >> 31 : 0u) | (hx < BX - 1 ? row[hx + 1] << 31 : 0u);
                }
            buf[to][hz][hy][hx] = n & keep[j];
        }
        __syncthreads();
    }
    const int lx = tid % TWX, ly = (tid / TWX) % TY, lz = tid / (TWX * TY);
    const int gw = tx * TWX + lx, gy = ty * TY + ly, gz = tz * TZ + lz;
    if (gw < d.wx && gy < d.ny && gz < d.nz) {
        const uint32_t n = buf[S & 1][lz + S][ly + S][lx + 1];
        out[((size_t)gz * d.ny + gy) * d.wx + gw] = (ERODE ? ~n : n) & valid_bits(gw, d);
    }
}

__global__ __launch_bounds__(THREADS) void k_mask_combine(const uint32_t* a, const uint32_t* b, uint32_t* out, int op, RegionDims d, unsigned long long words)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const uint32_t va = a[i], vb = b ? b[i] : 0u;        // (read before the store: out may alias either)
    uint32_t r;
    switch (op) {
    case SVR_MASK_AND: r = va & vb; break;
    case SVR_MASK_OR: r = va | vb; break;
    case SVR_MASK_ANDNOT: r = va & ~vb; break;
    case SVR_MASK_XOR: r = va ^ vb; break;
    default: r = ~va; break;                             // SVR_MASK_NOT
    }
    out[i] = r & valid_bits((int)(i % (unsigned)d.wx), d);
}

// candidates = (the source mask, or its complement) without padding; region = marker & candidates, the marker being a mask or (marker ==
// nullptr) every voxel on the six faces of the volume.  A tile that got a bit marks the 27 tiles around it dirty and sets *seeded.
__global__ __launch_bounds__(GROW_THREADS) void k_recon_seed(const uint32_t* __restrict__ marker, const uint32_t* __restrict__ src, int complement,
                                                             RegionDims d, int ntx, int nty, int ntz, uint32_t* __restrict__ cand,
                                                             uint32_t* __restrict__ region, uint32_t* dirty, uint32_t* seeded)
{
    const size_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    const int lx = tid % TWX, ly = (tid / TWX) % TY, lz = tid / (TWX * TY);
    const int gw = tx * TWX + lx, gy = ty * TY + ly, gz = tz * TZ + lz;
    const bool valid = gw < d.wx && gy < d.ny && gz < d.nz;
    uint32_t r = 0u;
    if (valid) {
        const size_t at = ((size_t)gz * d.ny + gy) * d.wx + gw;
        const uint32_t vb = valid_bits(gw, d);
        const uint32_t s = src[at];
        const uint32_t c = (complement ? ~s : s) & vb;
        uint32_t m;
        if (marker) {
            m = marker[at];
        } else if (gy == 0 || gy == d.ny - 1 || gz == 0 || gz == d.nz - 1) {
            m = 0xffffffffu;
        } else {
            m = (gw == 0 ? 1u : 0u) | (gw == d.wx - 1 ? 1u << ((d.nx - 1) & 31) : 0u);
        }
        r = m & c;
        cand[at] = c;
        region[at] = r;
    }
    const int any = __syncthreads_or(r != 0u);
    if (!any) return;
    if (tid == 0) *seeded = 1u;
    if (tid < 27) {
        const int ax = tx + tid % 3 - 1, ay = ty + (tid / 3) % 3 - 1, az = tz + tid / 9 - 1;
        if (ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz) dirty[((size_t)az * nty + ay) * ntx + ax] = 1u;
    }
}

// sets the seed voxels in a zeroed mask
__global__ void k_mask_points(MorphSeeds s, RegionDims d, uint32_t* mask)
{
    const int i = threadIdx.x;
    if (i >= s.n) return;
    const int x = s.xyz[i][0], y = s.xyz[i][1], z = s.xyz[i][2];
    atomicOr(&mask[((size_t)z * d.ny + y) * d.wx + (x >> 5)], 1u << (x & 31));
}

// ---------------- host side ----------------
int check_radius(const char* who, uint32_t radius)
{
    if (radius == 0u || radius > SVR_MORPH_MAX_RADIUS) return failf(-3, "%s: the radius must lie in 1 .. %d (got %u)", who, SVR_MORPH_MAX_RADIUS, radius);
    return 0;
}

hipError_t launch_step(hipStream_t st, int element, bool erode, const uint32_t* in, uint32_t* out, const RegionDims& d)
{
    const unsigned long long words = mask_words(d);
    const dim3 g = word_grid(words), b(THREADS);
    if (element == 6) {
        if (erode) hipLaunchKernelGGL((k_morph_step<6, true>), g, b, 0, st, in, out, d, words);
        else hipLaunchKernelGGL((k_morph_step<6, false>), g, b, 0, st, in, out, d, words);
    } else if (element == 18) {
        if (erode) hipLaunchKernelGGL((k_morph_step<18, true>), g, b, 0, st, in, out, d, words);
        else hipLaunchKernelGGL((k_morph_step<18, false>), g, b, 0, st, in, out, d, words);
    } else {
        if (erode) hipLaunchKernelGGL((k_morph_step<26, true>), g, b, 0, st, in, out, d, words);
        else hipLaunchKernelGGL((k_morph_step<26, false>), g, b, 0, st, in, out, d, words);
    }
    return hipGetLastError();
}

template <int S>
hipError_t launch_fused(hipStream_t st, int element, bool erode, const uint32_t* in, uint32_t* out, const RegionDims& d)
{
    const RegionSweep t(d);
    const dim3 g((uint32_t)t.tiles), b(GROW_THREADS);
    if (element == 6) {
        if (erode) hipLaunchKernelGGL((k_morph_fused<6, true, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
        else hipLaunchKernelGGL((k_morph_fused<6, false, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
    } else if (element == 18) {
        if (erode) hipLaunchKernelGGL((k_morph_fused<18, true, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
        else hipLaunchKernelGGL((k_morph_fused<18, false, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
    } else {
        if (erode) hipLaunchKernelGGL((k_morph_fused<26, true, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
        else hipLaunchKernelGGL((k_morph_fused<26, false, S>), g, b, 0, st, in, out, d, t.ntx, t.nty);
    }
    return hipGetLastError();
}

// the launches (kind: the unit steps it makes) that take `n` unit steps of one polarity: fours, a two, a one
int plan_steps(int n, int kinds[SVR_MORPH_MAX_RADIUS])
{
    int c = 0;
#ifndef SVR_MORPH_ONE_STEP                                // (the A/B build of tools/morph_time.py makes every unit step a launch)
    for (; n >= 4; n -= 4) kinds[c++] = 4;
    if (n >= 2) { kinds[c++] = 2; n -= 2; }
#endif
    for (; n > 0; --n) kinds[c++] = 1;
    return c;
}

int morph_launches(int op, uint32_t radius)
{
    int kinds[SVR_MORPH_MAX_RADIUS];
    return (op == SVR_MORPH_OPEN || op == SVR_MORPH_CLOSE ? 2 : 1) * plan_steps((int)radius, kinds);
}

// `op` as launches from `in` to `out`; tmp (needed when there is more than one launch) and out take turns so that the last lands in out
hipError_t run_morph(hipStream_t st, int op, int element, uint32_t radius, const uint32_t* in, uint32_t* out, uint32_t* tmp, const RegionDims& d)
{
    int kinds[2 * SVR_MORPH_MAX_RADIUS];
    bool erodes[2 * SVR_MORPH_MAX_RADIUS];
    int n = 0;
    const int halves = op == SVR_MORPH_OPEN || op == SVR_MORPH_CLOSE ? 2 : 1;
    for (int h = 0; h < halves; ++h) {
        const int c = plan_steps((int)radius, kinds + n);
        const bool erode = op == SVR_MORPH_ERODE || (op == SVR_MORPH_OPEN && h == 0) || (op == SVR_MORPH_CLOSE && h == 1);
        for (int i = 0; i < c; ++i) erodes[n + i] = erode;
        n += c;
    }
    const uint32_t* src = in;
    for (int i = 0; i < n; ++i) {
        uint32_t* dst = (n - 1 - i) % 2 == 0 ? out : tmp;
        hipError_t e;
        if (kinds[i] == 4) e = launch_fused<4>(st, element, erodes[i], src, dst, d);
        else if (kinds[i] == 2) e = launch_fused<2>(st, element, erodes[i], src, dst, d);
        else e = launch_step(st, element, erodes[i], src, dst, d);
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}

hipError_t launch_combine(hipStream_t st, const uint32_t* a, const uint32_t* b, int op, uint32_t* out, const RegionDims& d)
{
    const unsigned long long words = mask_words(d);
    hipLaunchKernelGGL(k_mask_combine, word_grid(words), dim3(THREADS), 0, st, a, b, out, op, d, words);
    return hipGetLastError();
}

// out = the components of the candidates (src, or NOT src) that the marker (a mask, or the faces of the volume for nullptr) touches.
// `cand` is scratch of the mask's size.  Synchronises the stream.
struct Recon { uint32_t sweeps = 0u; bool done = false; bool seeded = false; };
hipError_t run_reconstruct(hipStream_t st, const uint32_t* marker, const uint32_t* src, bool complement, const RegionDims& d, int connectivity,
                           uint32_t cap, uint32_t* cand, uint32_t* out, Recon* res)
{
    RegionSweep sw(d);
    DeviceBuffer small_buf;                              // the two dirty maps, the batch's counters, the `seeded` flag
    const size_t small = 2 * sw.tiles + SVR_REGION_BATCH + 1;
    hipError_t e = small_buf.alloc(small * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    uint32_t* const d_small = small_buf.as<uint32_t>();
    sw.dirty = d_small; sw.added = d_small + 2 * sw.tiles;
    uint32_t* d_seeded = sw.added + SVR_REGION_BATCH;
    e = hipMemsetAsync(d_small, 0, small * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_recon_seed, dim3((uint32_t)sw.tiles), dim3(GROW_THREADS), 0, st, marker, src, complement ? 1 : 0, d, sw.ntx, sw.nty, sw.ntz,
                           cand, out, sw.dirty, d_seeded);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = region_sweep_to_fixpoint(st, connectivity, cand, out, d, sw, cap, &res->sweeps, &res->done);
    uint32_t seeded = 0u;
    if (e == hipSuccess) e = hipMemcpyAsync(&seeded, d_seeded, sizeof seeded, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    res->seeded = seeded != 0u;
    return e;
}

// Around the device work of the last mask call (svr_region_mask_last_ms).  No entry point here stops its timer: it ends when it is
// destroyed, so every temporary is declared AFTER the timer and its hipFree lies inside the time (tools/morph_time.py relies on it).
CallEvents g_events;

} // namespace

extern "C" {

int svr_region_morph(const uint32_t* in_mask_device, int nx, int ny, int nz, int op, int element, uint32_t radius, uint32_t* out_mask_device)
{
    const char* who = "svr_region_morph";
    if (!in_mask_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (op != SVR_MORPH_DILATE && op != SVR_MORPH_ERODE && op != SVR_MORPH_OPEN && op != SVR_MORPH_CLOSE) return failf(-3, "%s: unknown op %d", who, op);
    if (int e = check_connectivity(who, "element", element)) return e;
    if (int e = check_radius(who, radius)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t bytes = mask_words(d) * sizeof(uint32_t);
    if (overlap(in_mask_device, bytes, out_mask_device, bytes)) return failf(-3, "%s: out must not overlap in", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    DeviceBuffer tmp;                                    // (after the timer: see g_events)
    if (morph_launches(op, radius) > 1) SVR_HIP_TRY(tmp.alloc(bytes));
    SVR_HIP_TRY(run_morph(st, op, element, radius, in_mask_device, out_mask_device, tmp.as<uint32_t>(), d));
    if (tmp) SVR_HIP_TRY(hipStreamSynchronize(st));      // the temporary is freed on return
    return 0;
}

int svr_region_combine(const uint32_t* a_device, const uint32_t* b_device, int nx, int ny, int nz, int op, uint32_t* out_device)
{
    const char* who = "svr_region_combine";
    if (!a_device || !out_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (op != SVR_MASK_AND && op != SVR_MASK_OR && op != SVR_MASK_ANDNOT && op != SVR_MASK_XOR && op != SVR_MASK_NOT) return failf(-3, "%s: unknown op %d", who, op);
    if (op != SVR_MASK_NOT && !b_device) return failf(-4, "%s: null argument (b)", who);
    if (op == SVR_MASK_NOT && b_device) return failf(-3, "%s: b must be NULL for SVR_MASK_NOT", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_combine(st, a_device, b_device, op, out_device, make_dims(nx, ny, nz)));
    return 0;
}

int svr_region_reconstruct(const uint32_t* marker_device, const uint32_t* cand_device, int nx, int ny, int nz, int connectivity, uint32_t max_sweeps,
                           uint32_t* out_device, uint32_t* sweeps_out)
{
    const char* who = "svr_region_reconstruct";
    if (!marker_device || !cand_device || !out_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t bytes = mask_words(d) * sizeof(uint32_t);
    if (overlap(marker_device, bytes, out_device, bytes) || overlap(cand_device, bytes, out_device, bytes))
        return failf(-3, "%s: out must not overlap marker or cand", who);
    const uint32_t cap = max_sweeps ? max_sweeps : svr_region_default_max_sweeps(nx, ny, nz);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    DeviceBuffer cand;
    SVR_HIP_TRY(cand.alloc(bytes));
    Recon res;
    SVR_HIP_TRY(run_reconstruct(st, marker_device, cand_device, false, d, connectivity, cap, cand.as<uint32_t>(), out_device, &res));
    if (sweeps_out) *sweeps_out = res.sweeps;
    if (!res.done) return failf(SVR_REGION_ERR_SWEEPS, "%s: the region was still growing after %u sweeps (max_sweeps); the mask is incomplete", who, res.sweeps);
    return 0;
}

int svr_region_fill_holes(const uint32_t* in_device, int nx, int ny, int nz, int background_connectivity, uint32_t max_sweeps, uint32_t* out_device)
{
    const char* who = "svr_region_fill_holes";
    if (!in_device || !out_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "background connectivity", background_connectivity)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t bytes = mask_words(d) * sizeof(uint32_t);
    if (overlap(in_device, bytes, out_device, bytes)) return failf(-3, "%s: out must not overlap in", who);
    const uint32_t cap = max_sweeps ? max_sweeps : svr_region_default_max_sweeps(nx, ny, nz);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    DeviceBuffer cand;
    SVR_HIP_TRY(cand.alloc(bytes));
    Recon res;
    SVR_HIP_TRY(run_reconstruct(st, nullptr, in_device, true, d, background_connectivity, cap, cand.as<uint32_t>(), out_device, &res));
    SVR_HIP_TRY(launch_combine(st, out_device, nullptr, SVR_MASK_NOT, out_device, d));     // the background reached -> everything else
    if (!res.done)
        return failf(SVR_REGION_ERR_SWEEPS, "%s: the background was still growing after %u sweeps (max_sweeps); out holds more than the filled mask", who, res.sweeps);
    return 0;
}

int svr_region_detach(const uint32_t* in_device, int nx, int ny, int nz, const int32_t* seeds_xyz, uint32_t nseeds, int element, uint32_t radius,
                      int connectivity, uint32_t max_sweeps, uint32_t* out_device, int32_t* status)
{
    const char* who = "svr_region_detach";
    if (!in_device || !seeds_xyz || !out_device || !status) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    MorphSeeds seeds;
    memset(&seeds, 0, sizeof seeds);
    seeds.n = (int)nseeds;
    for (uint32_t i = 0; i < nseeds; ++i)
        for (int a = 0; a < 3; ++a) seeds.xyz[i][a] = seeds_xyz[3u * i + a];
    if (int e = check_connectivity(who, "element", element)) return e;
    if (int e = check_radius(who, radius)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d), bytes = words * sizeof(uint32_t);
    if (overlap(in_device, bytes, out_device, bytes)) return failf(-3, "%s: out must not overlap in", who);
    const uint32_t cap = max_sweeps ? max_sweeps : svr_region_default_max_sweeps(nx, ny, nz);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    DeviceBuffer buf;                                    // four masks: the eroded core, two work masks, the temporary of the morph steps
    SVR_HIP_TRY(buf.alloc(4 * bytes));
    uint32_t *core = buf.as<uint32_t>(), *a = core + words, *b = core + 2 * words, *tmp = core + 3 * words;
    SVR_HIP_TRY(run_morph(st, SVR_MORPH_ERODE, element, radius, in_device, core, tmp, d));
    SVR_HIP_TRY(hipMemsetAsync(a, 0, bytes, st));
    hipLaunchKernelGGL(k_mask_points, dim3(1), dim3(64), 0, st, seeds, d, a);
    SVR_HIP_TRY(hipGetLastError());
    SVR_HIP_TRY(run_morph(st, SVR_MORPH_DILATE, element, radius, a, b, tmp, d));           // b = the dilated seeds: the marker
    Recon res;
    SVR_HIP_TRY(run_reconstruct(st, b, core, false, d, connectivity, cap, tmp, a, &res));  // a = the core's components under the marker
    SVR_HIP_TRY(run_morph(st, SVR_MORPH_DILATE, element, radius, a, b, tmp, d));
    SVR_HIP_TRY(launch_combine(st, b, in_device, SVR_MASK_AND, out_device, d));
    SVR_HIP_TRY(hipStreamSynchronize(st));               // (the masks are freed on return)
    *status = res.seeded ? SVR_REGION_STATUS_OK : SVR_REGION_STATUS_EMPTY;
    if (!res.done) return failf(SVR_REGION_ERR_SWEEPS, "%s: the core was still growing after %u sweeps (max_sweeps); the mask is incomplete", who, res.sweeps);
    return 0;
}

int svr_region_mask_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_mask_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
