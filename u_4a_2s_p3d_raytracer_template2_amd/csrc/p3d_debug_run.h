// p3d_debug_run.h -- how a p3d_debug_* entry (p3d_capi_misc.cpp, p3d_debug_planes.cpp) runs one device function on host
// arguments.  Internal: not installed with include/.
#ifndef P3D_DEBUG_RUN_H
#define P3D_DEBUG_RUN_H

#include "p3d_scene_state.h"

#pragma GCC visibility push(hidden)
namespace p3d {

// One argument of a debug entry on the device: `bytes` of scratch, filled from `in` before the launch (if any) and copied
// to `out` after it (if any).
struct DebugArg {
    const void* in; void* out; size_t bytes;
    void* d = nullptr;
    template <typename T> T* as() const { return (T*)d; }
};

// Runs one debug launch on `device`: scratch for the arguments (an array or a vector of DebugArg), inputs up, launch, wait,
// outputs back.  The scratch is freed on every path; a HIP error is reported as "<entry>: <error>".
template <typename Args, typename Launch>
int debug_run(const char* entry, int device, Args& args, Launch launch) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(P3D_ERR_NO_DEVICE, "no HIP device visible");
    hipError_t e = hipSetDevice(device);
    for (DebugArg& a : args) if (e == hipSuccess) e = hipMalloc(&a.d, a.bytes);
    for (DebugArg& a : args) if (e == hipSuccess && a.in) e = hipMemcpy(a.d, a.in, a.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (DebugArg& a : args) if (e == hipSuccess && a.out) e = hipMemcpy(a.out, a.d, a.bytes, hipMemcpyDeviceToHost);
    for (DebugArg& a : args) (void)hipFree(a.d);
    if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
    return P3D_OK;
}

}  // namespace p3d
#pragma GCC visibility pop

#endif
