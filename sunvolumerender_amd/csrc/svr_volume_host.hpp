// svr_volume_host.hpp -- the host scaffolding of the volume-op entry points (svr_region.hip, svr_morph.hip, svr_label.hip,
// svr_distance.hip, svr_filter.hip, svr_resample.hip, and through svr_geo_relax.hpp svr_geodesic.hip and svr_growcut.hip): the argument checks they share,
// device memory that frees itself, and the event
// pair behind each family's svr_*_last_ms.  Host only.  An entry point checks in the order null (-4), dimensions (-6), the rest (-3),
// then svr::ensure_ready(); after that it owns what it allocates through DeviceBuffer / DeviceVoxels and leaves through SVR_HIP_TRY.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

// returns from the entry point with the HIP error as the code; needs `const char* who` in scope.  What the function owns is freed by
// its destructors, WITHOUT a synchronisation: a path on which the stream may still use a buffer synchronises explicitly first.
#define SVR_HIP_TRY(call)                                                                                                             \
    do {                                                                                                                              \
        hipError_t _e = (call);                                                                                                       \
        if (_e != hipSuccess) return svr::failf((int)_e, "%s: HIP error %s at line %d", who, hipGetErrorName(_e), __LINE__);           \
    } while (0)

namespace {

inline int check_dims(const char* who, int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return svr::failf(-6, "%s: bad dimensions %d x %d x %d", who, nx, ny, nz);
    if ((unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz > (1ull << 31))
        return svr::failf(-6, "%s: %d x %d x %d is more than 2^31 voxels", who, nx, ny, nz);
    return 0;
}

// `what`: the noun of the message ("connectivity", "element", "background connectivity")
inline int check_connectivity(const char* who, const char* what, int value)
{
    if (value != 6 && value != 18 && value != 26) return svr::failf(-3, "%s: the %s must be 6, 18 or 26 (got %d)", who, what, value);
    return 0;
}

inline bool overlap(const void* a, size_t abytes, const void* b, size_t bbytes)
{
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bbytes && q < p + abytes;
}

// a seed list: 1 .. SVR_REGION_MAX_SEEDS points (x, y, z) inside the volume
inline int check_seeds(const char* who, const int32_t* seeds_xyz, uint32_t nseeds, int nx, int ny, int nz)
{
    if (nseeds == 0u || nseeds > SVR_REGION_MAX_SEEDS) return svr::failf(-3, "%s: nseeds must lie in 1 .. %d (got %u)", who, SVR_REGION_MAX_SEEDS, nseeds);
    for (uint32_t i = 0; i < nseeds; ++i) {
        const int32_t x = seeds_xyz[3u * i], y = seeds_xyz[3u * i + 1u], z = seeds_xyz[3u * i + 2u];
        if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz)
            return svr::failf(-3, "%s: seed %u (%d, %d, %d) lies outside the %d x %d x %d volume", who, i, x, y, z, nx, ny, nz);
    }
    return 0;
}

// the caller's inclusive box cut to the volume: b0 .. b1 per axis; refuses a box that leaves nothing
inline int clamp_box(const char* who, const int32_t* box_min, const int32_t* box_max, int nx, int ny, int nz, int b0[3], int b1[3])
{
    const int dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        if (box_min[a] > box_max[a] || box_max[a] < 0 || box_min[a] >= dims[a])
            return svr::failf(-3, "%s: the box %d .. %d on axis %d is empty, inverted or outside the volume", who, (int)box_min[a], (int)box_max[a], a);
        b0[a] = box_min[a] < 0 ? 0 : box_min[a];
        b1[a] = box_max[a] >= dims[a] ? dims[a] - 1 : box_max[a];
    }
    return 0;
}

// device memory that is freed when its owner goes out of scope (hipFree alone: see SVR_HIP_TRY)
struct DeviceBuffer {
    void* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p) { o.p = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(p, o.p); return *this; }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    explicit operator bool() const { return p != nullptr; }
};

// an event that is destroyed with its owner (the events of one call; the per-family pairs below live as long as the library)
struct DeviceEvent {
    hipEvent_t e = nullptr;
    DeviceEvent() = default;
    DeviceEvent(const DeviceEvent&) = delete;
    DeviceEvent& operator=(const DeviceEvent&) = delete;
    ~DeviceEvent() { if (e) hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
};

// the volume on the device: the caller's pointer, or an upload of the host array on the library's stream
struct DeviceVoxels {
    const uint16_t* p = nullptr;
    DeviceBuffer upload;
    hipError_t get(const uint16_t* voxels, size_t n, int src_is_device, hipStream_t st)
    {
        if (src_is_device) { p = voxels; return hipSuccess; }
        hipError_t e = upload.alloc(n * sizeof(uint16_t));
        if (e != hipSuccess) return e;
        p = upload.as<uint16_t>();
        return hipMemcpyAsync(upload.p, voxels, n * sizeof(uint16_t), hipMemcpyHostToDevice, st);
    }
    bool owned() const { return (bool)upload; }
};

// creates the n events of `ev` on first use
inline bool events_ready(hipEvent_t* ev, int n)
{
    if (ev[0]) return true;
    for (int i = 0; i < n; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) { ev[0] = nullptr; return false; }
    return true;
}

// the milliseconds from a to b once b has happened; 0 (and no pending HIP error) if they cannot be had
inline float elapsed_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    return ms;
}

// The events around the device work of the last call of one family (one instance per translation unit, behind its svr_*_last_ms),
// created on first use, and the timer of one call: it records the start when it is made and the end at stop() or, failing that, when
// it is destroyed -- AFTER the objects declared after it, so a file that wants their hipFree inside the time declares them after it.
struct CallEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms() { return ev[0] ? elapsed_ms(ev[0], ev[1]) : 0.f; }
};
struct CallTimer {
    CallEvents& ce;
    hipStream_t st;
    bool on;
    CallTimer(CallEvents& c, hipStream_t s) : ce(c), st(s), on(events_ready(c.ev, 2) && hipEventRecord(c.ev[0], s) == hipSuccess) {}
    CallTimer(const CallTimer&) = delete;
    CallTimer& operator=(const CallTimer&) = delete;
    void stop() { if (on) hipEventRecord(ce.ev[1], st); on = false; }
    ~CallTimer() { stop(); }
};

} // namespace
