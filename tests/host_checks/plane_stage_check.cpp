// plane_stage_check.cpp -- csrc/p3d_plane_stage.h on its own, for a sanitizer build on the CPU (tests/test_plane_stage.py):
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iinclude -I<package>/csrc tests/host_checks/plane_stage_check.cpp
// p3d_scene_state.h is replaced by the stubs below: "device" memory is the heap, a copy is a memcpy, and the stream's
// capture state is a flag.  Exit status 0 and "plane_stage_check ok" when every check holds.
#define P3D_SCENE_STATE_H           // the helper includes nothing else of the project
#include "p3d_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
typedef struct StubStream* hipStream_t;
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost };
static const char* hipGetErrorString(hipError_t) { return "stub"; }

static int g_allocations = 0, g_copies[2] = {0, 0}, g_waits = 0;
static bool g_capturing = false;
static std::string g_error;

static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    memcpy(dst, src, bytes);
    g_copies[kind]++;
    return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t) { g_waits++; return hipSuccess; }

namespace p3d {
static int fail(int code, const std::string& msg) { g_error = msg; return code; }
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
struct RawBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~RawBuf() { free(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        free(p);
        p = malloc(bytes); cap = bytes; g_allocations++;
        return hipSuccess;
    }
};
static bool stream_capturing(hipStream_t) { return g_capturing; }
}  // namespace p3d
struct p3d_scene { hipStream_t stream = nullptr; p3d_scene_stats stats{}; };

#include "p3d_plane_stage.h"

using namespace p3d;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold (last error: %s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); return 1; } } while (0)

namespace {

struct Buffers { RawBuf in, out, scratch; };

// An entry in the helper's three steps: out = in + 1 through `scratch`, n floats.  checks_between fails: the entry's own
// refusal between the two halves of "prepare".
int entry(p3d_scene* s, Buffers& B, const float* in, bool host_in, float* out, bool host_out, size_t n, bool checks_between_fail = false) {
    PlaneStage st(s, "p3d_check", "its scratch");
    const PlaneStage::Plane scratch = st.scratch(B.scratch, n * 4);
    const PlaneStage::Plane i = st.in(B.in, in, n * 4, host_in), o = st.out(B.out, out, n * 4, host_out);
    if (const int rc = st.refuse_in_capture()) return rc;
    if (checks_between_fail) return fail(P3D_ERR_LIMIT, "the entry's own check");
    if (const int rc = st.allocate()) return rc;
    if (const int rc = st.upload()) return rc;
    const float* src = i;
    float *mid = scratch, *dst = o;
    if (out) {
        for (size_t k = 0; k < n; k++) mid[k] = src[k] + 1.0f;       // the "launch"
        for (size_t k = 0; k < n; k++) dst[k] = mid[k];
    } else if (dst) {
        return fail(P3D_ERR_ARG, "a plane that is not there has a pointer");
    }
    return st.finish();
}

}  // namespace

int main() {
    p3d_scene s;
    Buffers B;
    const size_t n = 70 * 5;
    std::vector<float> in(n), out(n, 0.0f), dev_in(n), dev_out(n, 0.0f);
    for (size_t k = 0; k < n; k++) in[k] = dev_in[k] = (float)k;

    // host in, host out: staged both ways, one wait, three buffers counted
    CHECK(entry(&s, B, in.data(), true, out.data(), true, n) == P3D_OK);
    for (size_t k = 0; k < n; k++) CHECK(out[k] == (float)k + 1.0f);
    CHECK(g_allocations == 3 && g_copies[hipMemcpyHostToDevice] == 1 && g_copies[hipMemcpyDeviceToHost] == 1 && g_waits == 1);
    CHECK(s.stats.device_bytes == 3 * n * 4);
    // a second call of the shape allocates nothing
    CHECK(entry(&s, B, in.data(), true, out.data(), true, n) == P3D_OK);
    CHECK(g_allocations == 3 && s.stats.device_bytes == 3 * n * 4 && g_waits == 2);
    // host in, device out: the upload, no copy back, and the wait all the same
    CHECK(entry(&s, B, in.data(), true, dev_out.data(), false, n) == P3D_OK);
    CHECK(g_copies[hipMemcpyHostToDevice] == 3 && g_copies[hipMemcpyDeviceToHost] == 2 && g_waits == 3);
    for (size_t k = 0; k < n; k++) CHECK(dev_out[k] == (float)k + 1.0f);
    // device in, device out: the caller's pointers are handed out; no copy, no wait
    std::fill(dev_out.begin(), dev_out.end(), 0.0f);
    CHECK(entry(&s, B, dev_in.data(), false, dev_out.data(), false, n) == P3D_OK);
    CHECK(g_copies[hipMemcpyHostToDevice] == 3 && g_copies[hipMemcpyDeviceToHost] == 2 && g_waits == 3 && g_allocations == 3);
    for (size_t k = 0; k < n; k++) CHECK(dev_out[k] == (float)k + 1.0f);
    // a plane that is not there: nullptr for the kernels, and its memory field still counts (host: the wait)
    CHECK(entry(&s, B, dev_in.data(), false, nullptr, true, n) == P3D_OK);
    CHECK(g_waits == 4 && g_copies[hipMemcpyDeviceToHost] == 2);

    // while the stream is captured: host planes are refused, and so is a shape that has to allocate; neither grows the handle
    g_capturing = true;
    CHECK(entry(&s, B, in.data(), true, dev_out.data(), false, n) == P3D_ERR_STATE);
    CHECK(g_error == "p3d_check copies host planes and waits for them: not while the stream is being captured");
    CHECK(entry(&s, B, dev_in.data(), false, dev_out.data(), false, n) == P3D_OK);            // the scratch is there
    std::vector<float> big_in(2 * n, 1.0f), big_out(2 * n);
    CHECK(entry(&s, B, big_in.data(), false, big_out.data(), false, 2 * n) == P3D_ERR_STATE);
    CHECK(g_error == "p3d_check has to allocate its scratch: make a call of this shape before the capture");
    CHECK(g_allocations == 3 && s.stats.device_bytes == 3 * n * 4 && g_waits == 4);
    g_capturing = false;
    // the entry's own refusal between refuse_in_capture() and allocate() leaves the handle alone, too
    CHECK(entry(&s, B, big_in.data(), false, big_out.data(), false, 2 * n, true) == P3D_ERR_LIMIT);
    CHECK(g_allocations == 3 && s.stats.device_bytes == 3 * n * 4);
    CHECK(entry(&s, B, big_in.data(), false, big_out.data(), false, 2 * n) == P3D_OK);
    CHECK(g_allocations == 4 && s.stats.device_bytes == 2 * n * 4 + 2 * n * 4);               // the scratch grew, counted at its new size
    g_capturing = true;
    CHECK(entry(&s, B, big_in.data(), false, big_out.data(), false, 2 * n) == P3D_OK);
    g_capturing = false;

    // more declarations than the helper holds: refused before anything is allocated, nothing written past the table
    {
        std::vector<RawBuf> many(PlaneStage::kMaxPlanes + 1);
        PlaneStage st(&s, "p3d_check", "its scratch");
        for (RawBuf& b : many) st.scratch(b, 16);
        CHECK(st.refuse_in_capture() == P3D_ERR_LIMIT);
        CHECK(g_allocations == 4);
    }
    printf("plane_stage_check ok\n");
    return 0;
}
