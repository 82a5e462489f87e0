// svr_mesh.hip -- surface meshes of region masks and of isosurfaces by surface nets (svr_mesh_isosurface, _region, _measure, _positions;
// the contract is in include/svr_abi.h, the design in DESIGN.md 8o).  Integers only; the mesh is defined index for index, whatever order
// the GPU works in: every vertex and every quad is written at its rank, and nothing but the bounding box goes through an atomic
// (minima and maxima of integers: the same in any order).
//
// THE GRID: the padded samples (x', y', z'), 0 .. n + 1 per axis, x' = x + 1; a sample outside the volume is 0.  Point p stands for the
//   padded sample p AND for the cell whose lowest corner it is, so the three edges p -> p + e_a are edges of that cell (a cell at
//   n + 1 has no inside corner and is never active).  A WAVE holds 64 consecutive points of one row (y', z'); a row has spr =
//   ceil((nx + 2) / 64) waves, wave w = (z' py + y') spr + (x' >> 6).  Ascending (w, lane) is ascending (z', y', x'): the order of the
//   vertex numbers and -- with the axis as the last digit -- of the quad keys.
// k_mesh_classify  one lane per point: the 8 corners of the cell, active = mixed corners, crossing_a = the sample and its +a neighbour
//   differ.  Per wave: the ballot of the active lanes (one uint64), its popcount and the popcount of the three crossing ballots.
// ScanLevels (svr_scan.hpp)  exclusive scans of the two count arrays: the number of the first vertex and of the first quad of every wave.
// k_mesh_emit      the same lanes; a wave with an active cell (a crossing edge makes its cell active, so the others have nothing to
//   emit) reads the corners of its active cells again: the vertex at rank[w] + popcount(active ballot below the lane), the quads of
//   the lane's crossing edges at rank[w] + popcount(the three crossing ballots below the lane) + (crossing edges of the lane on lower
//   axes); the four vertices of a quad are looked up the same way in the active words of the neighbouring cells -- there is no dense
//   cell-to-vertex array.  With relax > 0 also the cell and the six linked neighbours of every vertex.
// k_mesh_relax     one thread per vertex, ping-pong between two vertex arrays.
// k_mesh_bbox, k_mesh_measure  reductions over the vertices / the triangles.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_mask.hpp"             // the mask layout, MASK_THREADS, word_grid
#include "svr_scan.hpp"
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int THREADS = MASK_THREADS;
constexpr int WAVES_PER_BLOCK = THREADS / 64;
constexpr uint32_t NO_VERTEX = 0xffffffffu;
constexpr uint32_t BBOX_BLOCKS = 256;                    // the blocks of k_mesh_bbox: one per compute unit
static_assert(sizeof(svr_mesh_params) == 8 && sizeof(svr_mesh_info) == 56, "svr_mesh_params is 8 bytes, svr_mesh_info 56");

struct MeshDims { int nx, ny, nz, px, py, pz; uint32_t spr, waves; };   // the volume, the padded grid, waves per row and in all

// the field of a u16 volume: sample (x', y', z') in padded coordinates; 0 outside the volume
struct VoxelField {
    const uint16_t* v;
    uint32_t level;
    __device__ uint32_t at(int x, int y, int z, const MeshDims& d) const
    {
        x -= 1; y -= 1; z -= 1;
        if ((unsigned)x >= (unsigned)d.nx || (unsigned)y >= (unsigned)d.ny || (unsigned)z >= (unsigned)d.nz) return 0u;
        return v[((size_t)z * d.ny + y) * d.nx + x];
    }
};

// the field of a region mask: 2 inside, 0 outside, level 1 (the padding bits of a row's last word are never looked at)
struct MaskField {
    const uint32_t* m;
    int wx;
    uint32_t level;
    __device__ uint32_t at(int x, int y, int z, const MeshDims& d) const
    {
        x -= 1; y -= 1; z -= 1;
        if ((unsigned)x >= (unsigned)d.nx || (unsigned)y >= (unsigned)d.ny || (unsigned)z >= (unsigned)d.nz) return 0u;
        return ((m[((size_t)z * d.ny + y) * wx + (x >> 5)] >> (x & 31)) & 1u) << 1;
    }
};

// a lane: point (x, y, z) of wave w; ok: the point exists
struct PointAt { uint32_t w; int lane, x, y, z; bool ok; };
__device__ inline PointAt point_at(const MeshDims& d)
{
    PointAt a;
    a.w = blockIdx.x * (uint32_t)WAVES_PER_BLOCK + (threadIdx.x >> 6);
    a.lane = (int)(threadIdx.x & 63u);
    const bool wave_ok = a.w < d.waves;
    const uint32_t w = wave_ok ? a.w : 0u;
    const uint32_t row = w / d.spr;
    a.x = (int)(w - row * d.spr) * 64 + a.lane;
    a.y = (int)(row % (uint32_t)d.py);
    a.z = (int)(row / (uint32_t)d.py);
    a.ok = wave_ok && a.x < d.px;
    return a;
}

// the values of the 8 corners of the cell at point a (corner o: bit 0 = +x, bit 1 = +y, bit 2 = +z) and their inside bits
template <class F>
__device__ inline uint32_t load_corners(const F& f, const PointAt& a, const MeshDims& d, uint32_t c[8])
{
    uint32_t bits = 0u;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        c[o] = f.at(a.x + (o & 1), a.y + ((o >> 1) & 1), a.z + (o >> 2), d);
        bits |= (c[o] >= f.level ? 1u : 0u) << o;
    }
    return bits;
}

__device__ inline bool is_active(uint32_t bits) { return bits != 0u && bits != 0xffu; }
// the edge from corner 0 along axis a crosses the surface
__device__ inline bool crosses(uint32_t bits, int a) { return ((bits ^ (bits >> (1 << a))) & 1u) != 0u; }

template <class F>
__global__ __launch_bounds__(THREADS) void k_mesh_classify(F f, MeshDims d, unsigned long long* __restrict__ active, uint32_t* __restrict__ vcount,
                                                           uint32_t* __restrict__ qcount)
{
    const PointAt a = point_at(d);
    uint32_t c[8];
    const uint32_t bits = a.ok ? load_corners(f, a, d, c) : 0u;
    const unsigned long long act = __ballot(is_active(bits));
    const uint32_t nq = (uint32_t)(__popcll(__ballot(crosses(bits, 0))) + __popcll(__ballot(crosses(bits, 1))) + __popcll(__ballot(crosses(bits, 2))));
    if (a.lane == 0 && a.w < d.waves) {
        active[a.w] = act;
        vcount[a.w] = (uint32_t)__popcll(act);
        qcount[a.w] = nq;
    }
}

// the number of the vertex of cell (x, y, z): the rank of its wave plus the active cells below it in the wave
__device__ inline uint32_t vertex_of(int x, int y, int z, const MeshDims& d, const unsigned long long* __restrict__ active, const uint32_t* __restrict__ vrank)
{
    uint32_t w = ((uint32_t)z * (uint32_t)d.py + (uint32_t)y) * d.spr + ((uint32_t)x >> 6);
    if (w >= d.waves) w = 0u;                             // (never: the cells asked for exist)
    return vrank[w] + (uint32_t)__popcll(active[w] & ((1ull << (x & 63)) - 1ull));
}

// The vertex of an active cell: per axis 256 i + (2 S + m) / (2 m), S = the sum of the cell-relative coordinates of the m crossing points.
// A crossing point lies q = 256 (level - vo) / (vi - vo) from the outside end of its edge.
__device__ inline void cell_vertex(const uint32_t c[8], uint32_t bits, uint32_t level, const PointAt& a, int32_t out[3])
{
    uint32_t S[3] = {0u, 0u, 0u}, m = 0u;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int b = (ax + 1) % 3, cc = (ax + 2) % 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ob = k & 1, oc = k >> 1;
            const int lo = (ob << b) | (oc << cc), hi = lo | (1 << ax);
            const bool lo_in = (bits >> lo) & 1u, hi_in = (bits >> hi) & 1u;
            if (lo_in == hi_in) continue;
            const uint32_t vi = lo_in ? c[lo] : c[hi], vo = lo_in ? c[hi] : c[lo];   // vo < level <= vi
            const uint32_t q = (256u * (level - vo)) / (vi - vo);
            S[ax] += lo_in ? 256u - q : q;
            S[b] += 256u * (uint32_t)ob;
            S[cc] += 256u * (uint32_t)oc;
            ++m;
        }
    }
    const int base[3] = {a.x, a.y, a.z};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) out[ax] = 256 * base[ax] + (int32_t)((2u * S[ax] + m) / (2u * m));
}

template <class F, bool RELAX>
__global__ __launch_bounds__(THREADS) void k_mesh_emit(F f, MeshDims d, const unsigned long long* __restrict__ active, const uint32_t* __restrict__ vrank,
                                                       const uint32_t* __restrict__ qrank, uint32_t nv, uint32_t nq, int32_t* __restrict__ verts,
                                                       uint32_t* __restrict__ tris, uint32_t* __restrict__ cell_of, uint32_t* __restrict__ links)
{
    const PointAt a = point_at(d);
    if (a.w >= d.waves) return;
    // A crossing edge from corner 0 makes its cell active, so a wave without an active cell (most waves) has nothing to emit, and only the
    // active lanes of the others read their corners
    const unsigned long long actw = active[a.w];
    if (!actw) return;
    const bool act = (actw >> a.lane) & 1ull;
    uint32_t c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t bits = act ? load_corners(f, a, d, c) : 0u;
    const unsigned long long below = (1ull << a.lane) - 1ull;
    const bool cr[3] = {crosses(bits, 0), crosses(bits, 1), crosses(bits, 2)};
    const unsigned long long cw0 = __ballot(cr[0]), cw1 = __ballot(cr[1]), cw2 = __ballot(cr[2]);
    if (act && is_active(bits)) {                         // (is_active: always, unless the source changed since the classify pass; so is id < nv)
        const uint32_t id = vrank[a.w] + (uint32_t)__popcll(actw & below);
        if (id < nv) {
            int32_t p[3];
            cell_vertex(c, bits, f.level, a, p);
            verts[3 * (size_t)id] = p[0]; verts[3 * (size_t)id + 1] = p[1]; verts[3 * (size_t)id + 2] = p[2];
            if (RELAX) {
                cell_of[id] = ((uint32_t)a.z * (uint32_t)(d.ny + 1) + (uint32_t)a.y) * (uint32_t)(d.nx + 1) + (uint32_t)a.x;
#pragma unroll
                for (int face = 0; face < 6; ++face) {    // -x, +x, -y, +y, -z, +z: linked iff the face's corners are mixed
                    const int ax = face >> 1, side = face & 1;
                    const uint32_t sel = ax == 0 ? 0x55u : ax == 1 ? 0x33u : 0x0fu;
                    const uint32_t fb = (bits >> (side << ax)) & sel;
                    uint32_t n = NO_VERTEX;
                    if (fb != 0u && fb != sel) {
                        const int step = side ? 1 : -1;
                        n = vertex_of(a.x + (ax == 0 ? step : 0), a.y + (ax == 1 ? step : 0), a.z + (ax == 2 ? step : 0), d, active, vrank);
                    }
                    links[6 * (size_t)id + face] = n;
                }
            }
        }
    }
    if (!tris || !(cr[0] || cr[1] || cr[2])) return;
    uint32_t q = qrank[a.w] + (uint32_t)(__popcll(cw0 & below) + __popcll(cw1 & below) + __popcll(cw2 & below));
    const bool s_in = bits & 1u;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!cr[ax]) continue;
        const int b = (ax + 1) % 3, cc = (ax + 2) % 3;
        uint32_t corner[4];                               // C(-1,-1), C(0,-1), C(0,0), C(-1,0) in (b, c) offsets
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int t[3] = {a.x, a.y, a.z};
            t[b] += (k == 0 || k == 3) ? -1 : 0;
            t[cc] += (k == 0 || k == 1) ? -1 : 0;
            corner[k] = vertex_of(t[0], t[1], t[2], d, active, vrank);
        }
        if (q < nq) {
            uint32_t* o = tris + 6 * (size_t)q;
            const uint32_t q1 = s_in ? corner[1] : corner[3], q3 = s_in ? corner[3] : corner[1];
            o[0] = corner[0]; o[1] = q1; o[2] = corner[2];
            o[3] = corner[0]; o[4] = corner[2]; o[5] = q3;
        }
        ++q;
    }
}

// one Jacobi step: per axis (2 sum + m) / (2 m) over the m linked neighbours, clamped to the vertex's own cell
__global__ __launch_bounds__(THREADS) void k_mesh_relax(const int32_t* __restrict__ in, int32_t* __restrict__ out, const uint32_t* __restrict__ cell_of,
                                                        const uint32_t* __restrict__ links, uint32_t nv, uint32_t cx, uint32_t cy)
{
    const uint32_t v = blockIdx.x * (uint32_t)THREADS + threadIdx.x;
    if (v >= nv) return;
    long long sum[3] = {0, 0, 0}, m = 0;                  // (six coordinates below 2^31)
#pragma unroll
    for (int face = 0; face < 6; ++face) {
        const uint32_t n = links[6 * (size_t)v + face];
        if (n >= nv) continue;                            // NO_VERTEX
        sum[0] += in[3 * (size_t)n]; sum[1] += in[3 * (size_t)n + 1]; sum[2] += in[3 * (size_t)n + 2];
        ++m;
    }
    const uint32_t cell = cell_of[v], row = cell / cx;
    const int lo[3] = {(int)(256u * (cell - row * cx)), (int)(256u * (row % cy)), (int)(256u * (row / cy))};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        int p = m ? (int)((2 * sum[ax] + m) / (2 * m)) : in[3 * (size_t)v + ax];   // (m >= 3 for every vertex of a mesh of this file)
        p = p < lo[ax] ? lo[ax] : p > lo[ax] + 256 ? lo[ax] + 256 : p;
        out[3 * (size_t)v + ax] = p;
    }
}

// box[0..2] = min, box[3..5] = max of the vertex coordinates.  A fixed number of blocks strides over the vertices and every wave ends
// with one set of atomics: atomics on one address take some 7 ns each, and one set per 64 vertices cost more than the emit pass
__global__ __launch_bounds__(THREADS) void k_mesh_bbox(const int32_t* __restrict__ verts, uint32_t nv, int* box)
{
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    for (size_t v = (size_t)blockIdx.x * THREADS + threadIdx.x; v < nv; v += (size_t)gridDim.x * THREADS)
        for (int ax = 0; ax < 3; ++ax) {
            const int p = verts[3 * v + ax];
            lo[ax] = min(lo[ax], p);
            hi[ax] = max(hi[ax], p);
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            lo[ax] = min(lo[ax], __shfl_xor(lo[ax], off));
            hi[ax] = max(hi[ax], __shfl_xor(hi[ax], off));
        }
    if ((threadIdx.x & 63u) == 0u && hi[0] >= 0)
        for (int ax = 0; ax < 3; ++ax) { atomicMin(box + ax, lo[ax]); atomicMax(box + 3 + ax, hi[ax]); }
}

struct Scale3 { double x, y, z; };

// per block: the wrap-around 64-bit sum of a . (b x c) and the double sum of the triangle areas, reduced in a fixed tree; a triangle
// with an index >= nv counts nothing and raises *bad
__global__ __launch_bounds__(THREADS) void k_mesh_measure(const int32_t* __restrict__ verts, uint32_t nv, const uint32_t* __restrict__ tris, size_t nt, Scale3 s,
                                                          unsigned long long* __restrict__ vol_part, double* __restrict__ area_part, uint32_t* bad)
{
    __shared__ unsigned long long sv[THREADS];
    __shared__ double sa[THREADS];
    const size_t t = (size_t)blockIdx.x * THREADS + threadIdx.x;
    unsigned long long vol = 0ull;
    double area = 0.0;
    if (t < nt) {
        const uint32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        if (i0 >= nv || i1 >= nv || i2 >= nv) atomicOr(bad, 1u);
        else {
            long long a[3], b[3], c[3];
            for (int k = 0; k < 3; ++k) { a[k] = verts[3 * (size_t)i0 + k]; b[k] = verts[3 * (size_t)i1 + k]; c[k] = verts[3 * (size_t)i2 + k]; }
            const unsigned long long cx = (unsigned long long)(b[1] * c[2] - b[2] * c[1]), cy = (unsigned long long)(b[2] * c[0] - b[0] * c[2]),
                                     cz = (unsigned long long)(b[0] * c[1] - b[1] * c[0]);
            vol = (unsigned long long)a[0] * cx + (unsigned long long)a[1] * cy + (unsigned long long)a[2] * cz;
            const double ux = (double)(b[0] - a[0]) * s.x, uy = (double)(b[1] - a[1]) * s.y, uz = (double)(b[2] - a[2]) * s.z;
            const double wx = (double)(c[0] - a[0]) * s.x, wy = (double)(c[1] - a[1]) * s.y, wz = (double)(c[2] - a[2]) * s.z;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        }
    }
    sv[threadIdx.x] = vol;
    sa[threadIdx.x] = area;
    __syncthreads();
    for (int off = THREADS / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) { sv[threadIdx.x] += sv[threadIdx.x + off]; sa[threadIdx.x] += sa[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { vol_part[blockIdx.x] = sv[0]; area_part[blockIdx.x] = sa[0]; }
}

// ---------------- host side ----------------
hipEvent_t g_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // classify, emit, relax of the last call: start, end
bool g_ran[3] = {false, false, false};

struct Phase {                                            // records the pair of one phase on the stream
    int k; hipStream_t st; bool on;
    Phase(int k_, hipStream_t s) : k(k_), st(s), on(events_ready(g_ev, 6) && hipEventRecord(g_ev[2 * k_], s) == hipSuccess) {}
    Phase(const Phase&) = delete;
    Phase& operator=(const Phase&) = delete;
    void stop() { if (on) g_ran[k] = hipEventRecord(g_ev[2 * k + 1], st) == hipSuccess; on = false; }
    ~Phase() { stop(); }
};

int check_mesh_dims(const char* who, int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return failf(-6, "%s: bad dimensions %d x %d x %d", who, nx, ny, nz);
    if (((unsigned long long)nx + 1ull) * ((unsigned long long)ny + 1ull) * ((unsigned long long)nz + 1ull) > (1ull << 31))
        return failf(-6, "%s: %d x %d x %d is more than 2^31 cells", who, nx, ny, nz);
    if (nx > SVR_MESH_MAX_DIM || ny > SVR_MESH_MAX_DIM || nz > SVR_MESH_MAX_DIM)
        return failf(-6, "%s: a dimension of %d x %d x %d is above %d: its coordinates in 1/256 voxel leave int32", who, nx, ny, nz, SVR_MESH_MAX_DIM);
    return 0;
}

int check_mesh_args(const char* who, const void* src, int nx, int ny, int nz, const svr_mesh_params* p, bool level_counts, const void* verts, const void* tris,
                    const svr_mesh_info* info)
{
    if (!src || !p || !info) return failf(-4, "%s: null argument", who);
    if (int e = check_mesh_dims(who, nx, ny, nz)) return e;
    if (level_counts && (p->level == 0u || p->level > 65535u)) return failf(-3, "%s: the level must lie in 1 .. 65535 (got %u)", who, p->level);
    if (p->relax > SVR_MESH_MAX_RELAX) return failf(-3, "%s: relax must lie in 0 .. %d (got %u)", who, SVR_MESH_MAX_RELAX, p->relax);
    if ((verts == nullptr) != (tris == nullptr)) return failf(-3, "%s: the vertex and triangle outputs must both be given, or both be NULL", who);
    return 0;
}

MeshDims make_mesh_dims(int nx, int ny, int nz)
{
    MeshDims d{nx, ny, nz, nx + 2, ny + 2, nz + 2, 0u, 0u};
    d.spr = (uint32_t)((d.px + 63) / 64);
    d.waves = (uint32_t)((unsigned long long)d.py * d.pz * d.spr);   // < 2^32: (ny + 1)(nz + 1) <= 2^31 / (nx + 1), see DESIGN.md 8o
    return d;
}

template <class F>
int mesh_run(const char* who, const F& f, const MeshDims& d, uint32_t relax, int32_t* verts_out, uint64_t vcap, uint32_t* tris_out, uint64_t tcap,
             svr_mesh_info* info, hipStream_t st)
{
    g_ran[0] = g_ran[1] = g_ran[2] = false;
    const dim3 grid((d.waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), b(THREADS);
    ScanLevels vscan(d.waves), qscan(d.waves);
    // the active words, the two scans, the box
    DeviceBuffer buf;
    SVR_HIP_TRY(buf.alloc((size_t)d.waves * 8 + (vscan.words() + qscan.words() + 6) * 4));
    unsigned long long* active = buf.as<unsigned long long>();
    vscan.place(reinterpret_cast<uint32_t*>(active + d.waves));
    qscan.place(vscan.total() + 1);
    int* box = reinterpret_cast<int*>(qscan.total() + 1);
    const int box_init[6] = {INT_MAX, INT_MAX, INT_MAX, -1, -1, -1};
    uint32_t nv = 0u, nq = 0u;
    {
        Phase phase(0, st);
        SVR_HIP_TRY(hipMemcpyAsync(box, box_init, sizeof box_init, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((k_mesh_classify<F>), grid, b, 0, st, f, d, active, vscan.at[0], qscan.at[0]);
        SVR_HIP_TRY(hipGetLastError());
        SVR_HIP_TRY(vscan.run(st));
        SVR_HIP_TRY(qscan.run(st));
        phase.stop();
        SVR_HIP_TRY(hipMemcpyAsync(&nv, vscan.total(), 4, hipMemcpyDeviceToHost, st));
        SVR_HIP_TRY(hipMemcpyAsync(&nq, qscan.total(), 4, hipMemcpyDeviceToHost, st));
        SVR_HIP_TRY(hipStreamSynchronize(st));
    }
    // A crossing edge lies in four active cells and a cell has at most 12: quads <= 3 vertices.  Up to 2^32 / 3 vertices the 32-bit
    // total of the quads is therefore exact; beyond, and beyond 2^31 quads, the triangles cannot be numbered in 32 bits
    if (nv > 0x55555555u || nq > (1u << 31))
        return failf(-6, "%s: a mesh of %u vertices and (modulo 2^32) %u quads is too large: its triangles cannot be numbered in 32 bits", who, nv, nq);
    memset(info, 0, sizeof *info);
    info->vertices = nv;
    info->quads = nq;
    info->triangles = 2ull * nq;
    info->bbox_min[0] = 256 * d.px; info->bbox_min[1] = 256 * d.py; info->bbox_min[2] = 256 * d.pz;
    info->bbox_max[0] = info->bbox_max[1] = info->bbox_max[2] = -1;
    info->status = nv ? SVR_REGION_STATUS_OK : SVR_REGION_STATUS_EMPTY;
    if (nv == 0u) return 0;
    const bool write = verts_out && vcap >= info->vertices && tcap >= info->triangles;
    // the vertex arrays: `last` receives the final coordinates (the caller's array when it is written), `other` is the second of the pair
    DeviceBuffer tmp_last, tmp_other, relax_buf;
    int32_t* last = verts_out;
    if (!write) { SVR_HIP_TRY(tmp_last.alloc((size_t)nv * 12)); last = tmp_last.as<int32_t>(); }
    int32_t* other = nullptr;
    uint32_t *cell_of = nullptr, *links = nullptr;
    if (relax) {
        SVR_HIP_TRY(tmp_other.alloc((size_t)nv * 12));
        other = tmp_other.as<int32_t>();
        SVR_HIP_TRY(relax_buf.alloc((size_t)nv * 28));
        links = relax_buf.as<uint32_t>();
        cell_of = links + 6 * (size_t)nv;
    }
    int32_t* cur = (relax & 1u) ? other : last;           // so that the last step lands in `last`
    {
        Phase phase(1, st);
        uint32_t* tris = write ? tris_out : nullptr;
        if (relax) hipLaunchKernelGGL((k_mesh_emit<F, true>), grid, b, 0, st, f, d, active, vscan.at[0], qscan.at[0], nv, nq, cur, tris, cell_of, links);
        else hipLaunchKernelGGL((k_mesh_emit<F, false>), grid, b, 0, st, f, d, active, vscan.at[0], qscan.at[0], nv, nq, cur, tris, cell_of, links);
        SVR_HIP_TRY(hipGetLastError());
    }
    if (relax) {
        Phase phase(2, st);
        for (uint32_t it = 0; it < relax; ++it) {
            int32_t* next = cur == last ? other : last;
            hipLaunchKernelGGL(k_mesh_relax, word_grid(nv), b, 0, st, cur, next, cell_of, links, nv, (uint32_t)(d.nx + 1), (uint32_t)(d.ny + 1));
            cur = next;
        }
        SVR_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mesh_bbox, dim3(std::min<uint32_t>(word_grid(nv).x, BBOX_BLOCKS)), b, 0, st, last, nv, box);
    SVR_HIP_TRY(hipGetLastError());
    int box_host[6];
    SVR_HIP_TRY(hipMemcpyAsync(box_host, box, sizeof box_host, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (the buffers are freed on return)
    for (int a = 0; a < 3; ++a) { info->bbox_min[a] = box_host[a]; info->bbox_max[a] = box_host[3 + a]; }
    if (verts_out && !write)
        return failf(SVR_MESH_ERR_CAPACITY, "%s: the mesh has %llu vertices and %llu triangles; the capacities are %llu and %llu", who,
                     (unsigned long long)info->vertices, (unsigned long long)info->triangles, (unsigned long long)vcap, (unsigned long long)tcap);
    return 0;
}

} // namespace

extern "C" {

int svr_mesh_params_default(svr_mesh_params* p)
{
    if (!p) return failf(-4, "svr_mesh_params_default: null argument");
    p->level = 32768u;
    p->relax = 0u;
    return 0;
}

int svr_mesh_isosurface(const uint16_t* voxels,
                        int nx, int ny, int nz, int src_is_device, const svr_mesh_params* params, int32_t* vertices_xyz_device, uint64_t vertex_capacity,
                        uint32_t* triangles_device, uint64_t triangle_capacity, svr_mesh_info* info_host)
{
    const char* who = "svr_mesh_isosurface";
    if (int e = check_mesh_args(who, voxels, nx, ny, nz, params, true, vertices_xyz_device, triangles_device, info_host)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceVoxels dv;
    SVR_HIP_TRY(dv.get(voxels, (size_t)nx * ny * nz, src_is_device, st));
    const VoxelField f{dv.p, params->level};
    return mesh_run(who, f, make_mesh_dims(nx, ny, nz), params->relax, vertices_xyz_device, vertex_capacity, triangles_device, triangle_capacity, info_host, st);
}

int svr_mesh_region(const uint32_t* mask_device,
                    int nx, int ny, int nz, const svr_mesh_params* params, int32_t* vertices_xyz_device, uint64_t vertex_capacity,
                    uint32_t* triangles_device, uint64_t triangle_capacity, svr_mesh_info* info_host)
{
    const char* who = "svr_mesh_region";
    if (int e = check_mesh_args(who, mask_device, nx, ny, nz, params, false, vertices_xyz_device, triangles_device, info_host)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    const MaskField f{mask_device, (nx + 31) / 32, 1u};
    return mesh_run(who, f, make_mesh_dims(nx, ny, nz), params->relax, vertices_xyz_device, vertex_capacity, triangles_device, triangle_capacity, info_host,
                    svr::current_stream());
}

int svr_mesh_measure(const int32_t* vertices_device, uint64_t nv, const uint32_t* triangles_device, uint64_t nt, const double scale[3], int64_t* volume6_units,
                     double* area)
{
    const char* who = "svr_mesh_measure";
    if (!scale || !volume6_units || !area || (nt && (!vertices_device || !triangles_device))) return failf(-4, "%s: null argument", who);
    if (nv > 0xffffffffull || nt > 0xffffffffull) return failf(-6, "%s: more than 2^32 vertices or triangles", who);
    for (int a = 0; a < 3; ++a)
        if (!(scale[a] > 0.0) || !std::isfinite(scale[a])) return failf(-3, "%s: the scale must be positive and finite", who);
    if (nt == 0u) { *volume6_units = 0; *area = 0.0; return 0; }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const size_t blocks = (size_t)((nt + THREADS - 1) / THREADS);
    DeviceBuffer buf;
    SVR_HIP_TRY(buf.alloc(blocks * 16 + 8));
    unsigned long long* vol_part = buf.as<unsigned long long>();
    double* area_part = reinterpret_cast<double*>(vol_part + blocks);
    uint32_t* bad = reinterpret_cast<uint32_t*>(area_part + blocks);
    SVR_HIP_TRY(hipMemsetAsync(bad, 0, 4, st));
    const Scale3 s{scale[0], scale[1], scale[2]};
    hipLaunchKernelGGL(k_mesh_measure, dim3((uint32_t)blocks), dim3(THREADS), 0, st, vertices_device, (uint32_t)nv, triangles_device, (size_t)nt, s, vol_part,
                       area_part, bad);
    SVR_HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> part(2 * blocks + 1);
    SVR_HIP_TRY(hipMemcpyAsync(part.data(), buf.p, blocks * 16 + 4, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    if ((uint32_t)part[2 * blocks]) return failf(-3, "%s: a triangle names a vertex >= %llu", who, (unsigned long long)nv);
    unsigned long long vol = 0ull;
    double sum = 0.0;
    for (size_t i = 0; i < blocks; ++i) {                 // in block order: the same sum every time
        vol += part[i];
        double t;
        memcpy(&t, &part[blocks + i], 8);
        sum += t;
    }
    *volume6_units = (int64_t)vol;
    *area = sum;
    return 0;
}

int svr_mesh_positions(const int32_t* vertices_host, uint64_t nv, const double spacing[3], const svr_volume* volume_or_null, float* xyz_host)
{
    const char* who = "svr_mesh_positions";
    if ((nv && (!vertices_host || !xyz_host)) || (!volume_or_null && !spacing)) return failf(-4, "%s: null argument", who);
    double pitch[3], origin[3] = {0.0, 0.0, 0.0};
    if (volume_or_null) {                                 // world: sample x sits at texture coordinate (x + 0.5) / nx of the unclipped box = vmin + (x + 0.5) pitch
        const svr_vec3 &s = volume_or_null->spacing, &o = volume_or_null->bbox.vmin;
        pitch[0] = s.x; pitch[1] = s.y; pitch[2] = s.z;
        origin[0] = o.x; origin[1] = o.y; origin[2] = o.z;
    } else {
        for (int a = 0; a < 3; ++a) pitch[a] = spacing[a];
    }
    for (int a = 0; a < 3; ++a)
        if (!(pitch[a] > 0.0) || !std::isfinite(pitch[a]) || !std::isfinite(origin[a])) return failf(-3, "%s: the spacing must be positive and finite", who);
    for (uint64_t i = 0; i < 3 * nv; ++i) {
        const int a = (int)(i % 3u);
        xyz_host[i] = (float)(origin[a] + ((double)vertices_host[i] / 256.0 - 0.5) * pitch[a]);
    }
    return 0;
}

int svr_mesh_last_ms(float* classify_ms, float* emit_ms, float* relax_ms)
{
    float* out[3] = {classify_ms, emit_ms, relax_ms};
    for (int k = 0; k < 3; ++k)
        if (out[k]) *out[k] = g_ran[k] ? elapsed_ms(g_ev[2 * k], g_ev[2 * k + 1]) : 0.f;
    return 0;
}

} // extern "C"
