// svr_internal.hpp -- what svr_api.hip offers the other translation units of libsvr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

namespace svr {
int report_error(int code, const char* msg);   // records (or, in fatal mode, prints and exits); returns code
int ensure_ready();                            // device selected, context created; 0 on success
hipStream_t current_stream();                  // the caller's stream (svr_set_stream)
struct DevWork;                                // svr_kernels.hpp
// the pixels of a W x H image that an image call works on, with the shared tickets: the owned ones (svr_set_row_shard,
// svr_set_render_window), or with `whole` all of them.  After ensure_ready()
void image_work(DevWork& work, uint32_t W, uint32_t H, bool whole);
int device_cus();                              // compute units of the device, after ensure_ready()
// svr_distance.hip: w = the three weights of a distance call (NULL = 1, 1, 1); refuses a weight of 0 and the overflow bound (-3)
int check_distance_weights(const char* who, const unsigned* weights_or_null, int nx, int ny, int nz, unsigned w[3]);

inline int failf(int code, const char* fmt, ...)
{
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return report_error(code, buf);
}
}
