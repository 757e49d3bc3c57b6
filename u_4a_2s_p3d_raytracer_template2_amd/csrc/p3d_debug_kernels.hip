// p3d_debug_kernels.hip -- unit probes of the device arithmetic (p3d_debug_* of include/p3d_hip.h) and their launchers.
// No frame launches them: they live apart from p3d_kernels.hip so that they do not rebuild with the ray kernels.  Same
// compiler flags as those, so a probe runs the arithmetic a frame runs.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_launch.h"
#include "p3d_rand.h"
#include "sample_stream.h"
#include "p3d_shade.h"

namespace p3d {

// ------------------------------------------------------------------ one intersection test per thread
__global__ void debug_intersect_kernel(uint32_t n, const uint32_t* type, const float* prim12,
                                       const float* origin, const float* dir, int32_t* hit, float* t,
                                       float* normal) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* d = prim12 + 12 * (size_t)i;
    Ray r; r.o = mk(origin[3 * i], origin[3 * i + 1], origin[3 * i + 2]);
    r.d = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    float tt = 0.0f; bool h = false; V3 nn = mk(0.0f, 0.0f, 0.0f);
    switch (type[i]) {
    case 0: {
        V3 c = mk(d[0], d[1], d[2]);
        h = hit_sphere(r, c, d[3], tt);
        if (h) { V3 hp = add(r.o, mul(r.d, tt)); nn = normalized(normalized(sub(hp, c))); }
        break;
    }
    case 1:
    case 4: {    // 4: the same triangle through hit_triangle<true>, the frcp() form every scene read from HBM tests with
        V3 p0 = mk(d[0], d[1], d[2]), p1 = mk(d[3], d[4], d[5]), p2 = mk(d[6], d[7], d[8]);
        V3 e1 = sub(p1, p0), e2 = sub(p2, p0);
        h = type[i] == 4 ? hit_triangle<true>(r, p0, e1, e2, tt) : hit_triangle<false>(r, p0, e1, e2, tt);
        if (h) {     // the host-side statement of this lives in scene_flatten.cpp; the probe keeps the device arithmetic
            V3 m = mk((e1.y * e2.z) - (e1.z * e2.y), (e1.z * e2.x) - (e1.x * e2.z), (e1.x * e2.y) - (e1.y * e2.x));
            nn = normalized(normalized(m));
        }
        break;
    }
    case 2: {
        V3 f;
        h = hit_aabox(r, mk(d[0], d[1], d[2]), mk(d[3], d[4], d[5]), tt, f);
        if (h) nn = normalized(f);
        break;
    }
    default: {
        V3 pn = mk(d[0], d[1], d[2]);
        h = hit_plane(r, pn, d[3], tt);
        if (h) nn = normalized(pn);
        break;
    }
    }
    hit[i] = h ? 1 : 0;
    t[i] = tt;
    normal[3 * i] = nn.x; normal[3 * i + 1] = nn.y; normal[3 * i + 2] = nn.z;
}

// every bit pattern in [first, first + count): frcp(x) against the division it replaces (NaNs compare equal to NaNs)
__global__ void debug_check_rcp_kernel(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        const float a = frcp(x), b = 1.0f / x;
        const bool same = __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
        if (!same) { atomicAdd(n_bad, 1ull); atomicMin(first_bad, bits); }
    }
}
// the same for rcp_len(x), the reciprocal of a square root's output
__global__ void debug_check_rcp_len_kernel(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        const float a = rcp_len(x), b = 1.0f / x;
        const bool same = __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
        if (!same) { atomicAdd(n_bad, 1ull); atomicMin(first_bad, bits); }
    }
}
hipError_t launch_debug_check_rcp(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad, hipStream_t stream) {
    hipLaunchKernelGGL(debug_check_rcp_kernel, dim3(256 * 16), dim3(256), 0, stream, first, count, n_bad, first_bad);
    return hipGetLastError();
}
hipError_t launch_debug_check_rcp_len(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad, hipStream_t stream) {
    hipLaunchKernelGGL(debug_check_rcp_len_kernel, dim3(256 * 16), dim3(256), 0, stream, first, count, n_bad, first_bad);
    return hipGetLastError();
}

__global__ void debug_powf_kernel(uint32_t n, const float* x, const float* y, float* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = p3d_powf(x[i], y[i]);
}
hipError_t launch_debug_powf(uint32_t n, const float* x, const float* y, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(debug_powf_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, x, y, out);
    return hipGetLastError();
}

__global__ void debug_pow_kernel(uint32_t n, const double* x, const double* y, double* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = p3d_pow(x[i], y[i]);
}
hipError_t launch_debug_pow(uint32_t n, const double* x, const double* y, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(debug_pow_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, x, y, out);
    return hipGetLastError();
}
// the KR expression of shade_hit<..., SCHLICK = true> on (ior_1, newIor, cos_theta_i) triples
__global__ void debug_schlick_kr_kernel(uint32_t n, const float* ior_1, const float* new_ior, const float* cos_theta_i, float* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = p3d_schlick_kr(ior_1[i], new_ior[i], cos_theta_i[i], PowTab());
}
hipError_t launch_debug_schlick_kr(uint32_t n, const float* ior_1, const float* new_ior, const float* cos_theta_i, float* out,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(debug_schlick_kr_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, ior_1, new_ior, cos_theta_i, out);
    return hipGetLastError();
}

hipError_t launch_debug_intersect(uint32_t n, const uint32_t* type, const float* prim12, const float* origin,
                                  const float* dir, int32_t* hit, float* t, float* normal, hipStream_t stream) {
    hipLaunchKernelGGL(debug_intersect_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, type, prim12,
                       origin, dir, hit, t, normal);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the restated rand(), 31 values per thread (p3d_rand.h)
struct RandWindow { uint32_t w[2 * kRandDeg - 1]; };               // s[0 .. 60]: the seed state and the 30 words after it

__global__ void __launch_bounds__(256) debug_rand_kernel(RandWindow seed_window, uint64_t first, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t at = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)kRandDeg;
    if (at >= n) return;
    uint32_t c[kRandDeg], st[kRandDeg];
    rand_poly_pow((uint64_t)kRandFirstDraw + first + at, c);
    rand_poly_apply(c, seed_window.w, kRandDeg, st);
    for (uint32_t i = 0; i < (uint32_t)kRandDeg && at + i < n; i++) out[at + i] = st[i] >> 1;
}

hipError_t launch_debug_rand(uint32_t seed, uint64_t first, uint32_t n, uint32_t* out, hipStream_t stream) {
    RandWindow w;
    rand_seed_state(seed, w.w);
    rand_extend(w.w, kRandDeg, 2 * kRandDeg - 1);
    const uint32_t threads = (n + (uint32_t)kRandDeg - 1) / (uint32_t)kRandDeg;
    hipLaunchKernelGGL(debug_rand_kernel, dim3((threads + 255) / 256), dim3(256), 0, stream, w, first, n, out);
    return hipGetLastError();
}

}  // namespace p3d
