// svr_api_dist.hip -- frame assembly across processes in the C-ABI layer (svr_api.hip): strip packing and the RCCL gather, the native
// counterpart of sunvolumerender_amd/dist.py.
#include "svr_api_state.hpp"

#include <dlfcn.h>
#include <vector>

using namespace svr_host;

namespace {

float* g_stage = nullptr;          // svr_assemble_frame: packed rows -- this rank's, and on root every rank's
size_t g_stage_floats = 0;

// the four RCCL entry points of the exchange, resolved from the RCCL the process has loaded (rccl.h: ncclResult_t is an int, 0 = success)
struct Rccl {
    int (*group_start)() = nullptr;
    int (*group_end)() = nullptr;
    int (*send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    bool tried = false;
} g_rccl;
constexpr int RCCL_FLOAT32 = 7;                          // ncclFloat32
bool rccl_resolve()
{
    if (!g_rccl.tried) {
        g_rccl.tried = true;
        void* h = nullptr;
        for (const char* name : {"librccl.so", "librccl.so.1", "libnccl.so", "libnccl.so.2"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
        if (h) {
            g_rccl.group_start = (int (*)())dlsym(h, "ncclGroupStart");
            g_rccl.group_end = (int (*)())dlsym(h, "ncclGroupEnd");
            g_rccl.send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
            g_rccl.recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
        }
    }
    return g_rccl.group_start && g_rccl.group_end && g_rccl.send && g_rccl.recv;
}

} // namespace

namespace svr_host {

// the staging buffer (svr_shutdown)
void free_stage()
{
    if (g_stage) { hipFree(g_stage); g_stage = nullptr; g_stage_floats = 0; }
}

} // namespace svr_host

extern "C" {

// ---------------- frame assembly (native counterpart of sunvolumerender_amd/dist.py) ----------------
uint32_t svr_strip_rows_owned(uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world)
{
    if (world <= 1 || strip_rows == 0) return rank == 0 || world <= 1 ? H : 0;
    if (rank >= world) return 0;
    uint32_t rows = 0;
    const uint32_t nstrips = (H + strip_rows - 1) / strip_rows;
    for (uint32_t sidx = rank; sidx < nstrips; sidx += world) {
        const uint32_t ys = sidx * strip_rows, ye = ys + strip_rows < H ? ys + strip_rows : H;
        rows += ye - ys;
    }
    return rows;
}

uint32_t svr_strip_row_to_y(uint32_t p, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world)
{
    if (p >= svr_strip_rows_owned(H, strip_rows, rank, world)) return 0xffffffffu;
    if (world <= 1 || strip_rows == 0) return p;
    const uint32_t q = p / strip_rows;
    return (q * world + rank) * strip_rows + (p - q * strip_rows);
}

static int strips_call(void* packed, void* frame, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world, int to_packed, const char* who)
{
    if (ensure_init()) return g.err_code;
    if (!packed || !frame || W == 0 || H == 0) return fail(-4, "%s: bad argument", who);
    if (world > 1 && (rank >= world || strip_rows == 0)) return fail(-6, "%s: rank %u of %u, strip_rows %u", who, rank, world, strip_rows);
    HIP_TRY(svr::launch_strips((float*)packed, (float*)frame, 3u * W, svr_strip_rows_owned(H, strip_rows, rank, world), strip_rows, rank, world, to_packed, g.stream));
    return 0;
}
int svr_pack_strips(void* packed, const void* hdr, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world)
{
    return strips_call(packed, const_cast<void*>(hdr), W, H, strip_rows, rank, world, 1, "svr_pack_strips");
}
int svr_unpack_strips(void* frame, const void* packed, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world)
{
    return strips_call(const_cast<void*>(packed), frame, W, H, strip_rows, rank, world, 0, "svr_unpack_strips");
}

int svr_assemble_frame(void* nccl_comm, void* frame_on_root, const void* hdr_local, uint32_t W, uint32_t H,
                       uint32_t strip_rows, uint32_t rank, uint32_t world, uint32_t root)
{
    if (ensure_init()) return g.err_code;
    if (!hdr_local || W == 0 || H == 0 || world == 0 || rank >= world || root >= world) return fail(-4, "svr_assemble_frame: bad argument");
    if (rank == root && !frame_on_root) return fail(-4, "svr_assemble_frame: frame_on_root is null on the root rank");
    const size_t row = (size_t)3 * W;
    if (world == 1) {
        HIP_TRY(hipMemcpyAsync(frame_on_root, hdr_local, row * H * sizeof(float), hipMemcpyDeviceToDevice, g.stream));
        return 0;
    }
    if (!nccl_comm) return fail(-4, "svr_assemble_frame: nccl_comm is null");
    if (strip_rows == 0) return fail(-6, "svr_assemble_frame: strip_rows is 0");
    if (!rccl_resolve()) return fail(-7, "svr_assemble_frame: no RCCL in this process (dlopen(\"librccl.so\") / ncclSend / ncclRecv not found)");
    // staging: on root the packed rows of every rank back to back (= one frame), elsewhere this rank's rows
    const size_t need = rank == root ? row * H : row * svr_strip_rows_owned(H, strip_rows, rank, world);
    if (need > g_stage_floats) {
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (g_stage) HIP_TRY(hipFree(g_stage));
        g_stage = nullptr; g_stage_floats = 0;
        HIP_TRY(hipMalloc((void**)&g_stage, need * sizeof(float)));
        g_stage_floats = need;
    }
    if (rank != root) {
        const uint32_t mine = svr_strip_rows_owned(H, strip_rows, rank, world);
        if (svr_pack_strips(g_stage, hdr_local, W, H, strip_rows, rank, world)) return g.err_code;
        if (mine) {
            const int rc = g_rccl.send(g_stage, row * mine, RCCL_FLOAT32, (int)root, nccl_comm, g.stream);
            if (rc != 0) return fail(-7, "svr_assemble_frame: ncclSend failed (%d)", rc);
        }
        return 0;
    }
    // root: its own rows straight into the frame, the peers' rows through the staging buffer
    if (frame_on_root != hdr_local) {
        if (svr_pack_strips(g_stage, hdr_local, W, H, strip_rows, rank, world)) return g.err_code;
        if (svr_unpack_strips(frame_on_root, g_stage, W, H, strip_rows, rank, world)) return g.err_code;
    }
    int rc = g_rccl.group_start();
    size_t off = 0;
    std::vector<size_t> offs(world, 0);
    for (uint32_t r = 0; r < world && rc == 0; ++r) {
        const uint32_t n = svr_strip_rows_owned(H, strip_rows, r, world);
        offs[r] = off;
        if (r != root && n) rc = g_rccl.recv(g_stage + off, row * n, RCCL_FLOAT32, (int)r, nccl_comm, g.stream);
        off += row * n;
    }
    const int rc2 = g_rccl.group_end();
    if (rc != 0 || rc2 != 0) return fail(-7, "svr_assemble_frame: ncclRecv failed (%d, %d)", rc, rc2);
    for (uint32_t r = 0; r < world; ++r)
        if (r != root && svr_unpack_strips(frame_on_root, g_stage + offs[r], W, H, strip_rows, r, world)) return g.err_code;
    return 0;
}

} // extern "C"
