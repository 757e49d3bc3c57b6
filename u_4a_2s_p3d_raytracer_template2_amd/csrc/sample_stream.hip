// sample_stream.hip -- the reference's pixel-sample stream (set_rand_seed + the jitter and sampleUnitDisk() draws of
// renderScene(), RT/main.cpp:747,776-801) produced on the device in the bits the host C library's rand() gives.
// p3d_rand.h has the arithmetic; this file lays it out over the machine.  One pass over `pairs` pairs of draws:
//   1. summary   a thread owns a chunk of kSampleChunkPairs pairs.  It reaches the chunk's 31 words of generator state by a
//                jump, reads its pairs and stores the chunk's map {A, B} -> (exit state, samples completed); the workgroup
//                stores the composition of its chunks' maps.
//   2. scan      one workgroup composes the workgroups' maps in order, from the state and sample index the pass starts
//                with: every workgroup's entry, and the pass's exit state and completed-sample count.
//   3. emit      a workgroup scans its chunks' maps from its entry; every thread jumps again, replays its chunk from its
//                own entry and writes.  Workgroups (and threads) that begin past the last sample do nothing.
// How a thread reaches its state -- 32-bit multiply-adds only:
//   - the host hands every pass a window of 91 stream words at the pass's first draw (one jump there, p3d_rand.h);
//   - workgroup g multiplies the table polynomials x^(2 P T v 16^d) of the hex digits v of g (P pairs per chunk, T chunks per
//     workgroup): at most 8 cooperative products of 31 x 31 words, reduced with the table of x^31 .. x^60; applied to the
//     window this gives 61 words at the workgroup's first draw, in LDS;
//   - thread t applies x^(2 P t), read from the third table, to those: 31 x 31 multiply-adds for its 31 words.
// Jumping twice costs those 961 multiply-adds a second time against about 1000 draws and their float work; keeping the
// state between the passes would cost 124 bytes per chunk against the 8 of its map.  Built with the ray kernels' flags
// (-ffp-contract=off, correctly rounded division).  Nothing crosses workgroups inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "p3d_rand.h"
#include "sample_stream.h"

namespace p3d {

namespace {

constexpr uint32_t P = kSampleChunkPairs, T = kSampleChunkThreads;
constexpr int kDigits = 8;                                   // hex digits of a workgroup index
// the tables, in words: x^(2 P t) as [coefficient][t]; x^(2 P T v 16^d) as [d][v - 1][coefficient]; x^(31 + m) as [m][coefficient]
constexpr uint32_t kTabThread = 0, kTabGroup = kTabThread + kRandDeg * T, kTabReduce = kTabGroup + kDigits * 15 * kRandDeg,
                   kTabWords = kTabReduce + (kRandDeg - 1) * kRandDeg;
constexpr uint32_t kWindowWords = 3 * kRandDeg - 2;          // 91: 31 coefficients reach 61 words, which 31 more reach 31
constexpr uint32_t kPassResult = 96, kPassWords = 128;       // the pass buffer: window, then completed samples and exit state
constexpr uint32_t kMaxPassPairs = 0xFFFF0000u;              // a pass completes at most pairs / 2 + 1 samples: fits a map's 31 bits
static_assert(T >= 2 * kRandDeg - 1 && T % 64 == 0, "the cooperative products use 61 threads");

// Inclusive scan of the workgroup's maps under composition (thread order = stream order); buf[tid] holds the result too.
template <uint32_t N>
__device__ __forceinline__ SampleMap block_scan_maps(SampleMap v, SampleMap* buf) {
    const uint32_t tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < N; off <<= 1) {
        SampleMap left = sample_map_identity();
        if (tid >= off) left = buf[tid - off];
        __syncthreads();
        v = sample_map_compose(left, v);
        buf[tid] = v;
        __syncthreads();
    }
    return v;
}

// st = the 31 stream words at the first draw of chunk (workgroup * T + thread) of the pass whose window is `window`.
// Every thread of the workgroup must call it (barriers).
__device__ __forceinline__ void chunk_start_state(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ window, uint32_t group,
                                                  uint32_t st[kRandDeg]) {
    __shared__ uint32_t acc[kRandDeg], fac[kRandDeg], prod[2 * kRandDeg - 1], win[2 * kRandDeg - 1];
    const uint32_t tid = threadIdx.x;
    if (tid < kRandDeg) acc[tid] = tid == 0;                 // the polynomial 1
    __syncthreads();
    uint32_t g = group;
    for (int d = 0; d < kDigits && g; d++, g >>= 4) {        // uniform over the workgroup
        const uint32_t v = g & 15u;
        if (!v) continue;
        if (tid < kRandDeg) fac[tid] = tab[kTabGroup + ((uint32_t)d * 15 + v - 1) * kRandDeg + tid];
        __syncthreads();
        if (tid < 2 * kRandDeg - 1) {
            const int k = (int)tid, lo = k > kRandDeg - 1 ? k - (kRandDeg - 1) : 0, hi = k < kRandDeg - 1 ? k : kRandDeg - 1;
            uint32_t sum = 0;
            for (int i = lo; i <= hi; i++) sum += acc[i] * fac[k - i];
            prod[k] = sum;
        }
        __syncthreads();
        if (tid < kRandDeg) {
            uint32_t r = prod[tid];
            for (int m = 0; m < kRandDeg - 1; m++) r += prod[kRandDeg + m] * tab[kTabReduce + (uint32_t)m * kRandDeg + tid];
            acc[tid] = r;
        }
        __syncthreads();
    }
    if (tid < 2 * kRandDeg - 1) {
        uint32_t sum = 0;
        for (int j = 0; j < kRandDeg; j++) sum += acc[j] * window[j + tid];
        win[tid] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRandDeg; k++) st[k] = 0;
#pragma unroll
    for (int j = 0; j < kRandDeg; j++) {
        const uint32_t c = tab[kTabThread + (uint32_t)j * T + tid];
#pragma unroll
        for (int k = 0; k < kRandDeg; k++) st[k] += c * win[j + k];
    }
}

__device__ __forceinline__ uint32_t chunk_pairs(uint32_t chunk, uint32_t pass_pairs) {
    const uint64_t first = (uint64_t)chunk * P;
    if (first >= pass_pairs) return 0;
    const uint64_t left = pass_pairs - first;
    return left < P ? (uint32_t)left : P;
}

__global__ void __launch_bounds__(T) sample_summary_kernel(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ window,
                                                           uint32_t pass_pairs, SampleMap* __restrict__ chunk_maps,
                                                           SampleMap* __restrict__ group_maps) {
    __shared__ SampleMap buf[T];
    const uint32_t chunk = blockIdx.x * T + threadIdx.x;
    uint32_t st[kRandDeg];
    chunk_start_state(tab, window, blockIdx.x, st);
    SampleSummarySink sum;
    rand_read_pairs(st, chunk_pairs(chunk, pass_pairs), sum);      // no pairs: the identity
    const SampleMap m = sum.map();
    chunk_maps[chunk] = m;
    const SampleMap all = block_scan_maps<T>(m, buf);
    if (threadIdx.x == T - 1) group_maps[blockIdx.x] = all;
}

// entry[g] = {first sample, state} workgroup g starts with; result = {samples completed so far, exit state} after the pass
__global__ void __launch_bounds__(256) sample_scan_kernel(const SampleMap* __restrict__ group_maps, uint32_t n_groups, uint32_t first_sample,
                                                          uint32_t state, uint2* __restrict__ entry, uint32_t* __restrict__ result) {
    __shared__ SampleMap buf[256];
    const uint32_t tid = threadIdx.x, per = (n_groups + 255u) / 256u;
    const uint32_t lo = tid * per < n_groups ? tid * per : n_groups, hi = lo + per < n_groups ? lo + per : n_groups;
    SampleMap m = sample_map_identity();
    for (uint32_t i = lo; i < hi; i++) m = sample_map_compose(m, group_maps[i]);
    block_scan_maps<256>(m, buf);
    const SampleMap before = tid ? buf[tid - 1] : sample_map_identity();
    uint32_t r = state ? before.b : before.a;
    uint32_t s = first_sample + (r >> 1), st = r & 1u;
    for (uint32_t i = lo; i < hi; i++) {
        entry[i] = make_uint2(s, st);
        const SampleMap g = group_maps[i];
        r = st ? g.b : g.a;
        s += r >> 1; st = r & 1u;
    }
    if (tid == 255) { result[0] = s; result[1] = st; }
}

__global__ void __launch_bounds__(T) sample_emit_kernel(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ window,
                                                        uint32_t pass_pairs, const SampleMap* __restrict__ chunk_maps,
                                                        const uint2* __restrict__ entry, uint32_t n_samples, int32_t res_x, int32_t spp,
                                                        float aperture, float* __restrict__ out) {
    __shared__ SampleMap buf[T];
    const uint2 e = entry[blockIdx.x];
    if (e.x >= n_samples) return;                                  // the whole workgroup lies past the last sample
    const uint32_t tid = threadIdx.x, chunk = blockIdx.x * T + tid;
    uint32_t st[kRandDeg];
    chunk_start_state(tab, window, blockIdx.x, st);
    block_scan_maps<T>(chunk_maps[chunk], buf);
    const SampleMap before = tid ? buf[tid - 1] : sample_map_identity();
    const uint32_t r = e.y ? before.b : before.a;
    const uint32_t s = e.x + (r >> 1);
    if (s >= n_samples) return;
    SampleEmitSink emit;
    emit.init(out, n_samples, s, r & 1u, res_x, spp, aperture);
    rand_read_pairs(st, chunk_pairs(chunk, pass_pairs), emit);
}

// the three tables, made once per process
const std::vector<uint32_t>& jump_tables() {
    static const std::vector<uint32_t> tables = [] {
        std::vector<uint32_t> t(kTabWords);
        uint32_t step[kRandDeg], cur[kRandDeg];
        rand_poly_pow(2ull * P, step);
        rand_poly_one(cur);
        for (uint32_t i = 0; i < T; i++) {
            for (int j = 0; j < kRandDeg; j++) t[kTabThread + (uint32_t)j * T + i] = cur[j];
            rand_poly_mul(cur, step, cur);
        }
        rand_poly_pow(2ull * P * T, step);                          // x^(2 P T 16^d), d = 0
        for (int d = 0; d < kDigits; d++) {
            rand_poly_one(cur);
            for (uint32_t v = 1; v <= 15; v++) {
                rand_poly_mul(cur, step, cur);
                for (int j = 0; j < kRandDeg; j++) t[kTabGroup + ((uint32_t)d * 15 + v - 1) * kRandDeg + j] = cur[j];
            }
            rand_poly_mul(cur, step, step);                         // ^16
        }
        rand_poly_pow(kRandDeg, cur);
        for (int m = 0; m < kRandDeg - 1; m++) {
            for (int j = 0; j < kRandDeg; j++) t[kTabReduce + (uint32_t)m * kRandDeg + j] = cur[j];
            rand_poly_mul_x(cur);
        }
        return t;
    }();
    return tables;
}

// pairs to provision for `samples` more samples: a sample reads 1 + 4 / pi pairs on average (one jitter, then candidates
// accepted with probability pi / 4: variance 0.35 pairs^2), so 8 sqrt(samples) on top is 13 standard deviations
uint64_t provision_pairs(uint32_t samples) {
    return (uint64_t)std::ceil(2.2733 * (double)samples + 8.0 * std::sqrt((double)samples)) + 64;
}

}  // namespace

#define SS_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t generate_sample_stream(SampleStreamScratch& S, uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp, float aperture,
                                  float* d_out, uint64_t pairs_per_pass, int32_t* passes, hipStream_t stream) {
    const uint32_t n_samples = (uint32_t)((uint64_t)res_x * res_y * spp * spp);
    if (!S.tables) {
        const std::vector<uint32_t>& t = jump_tables();
        SS_TRY(hipMalloc((void**)&S.tables, kTabWords * sizeof(uint32_t)));
        S.bytes += kTabWords * sizeof(uint32_t);
        SS_TRY(hipMemcpy(S.tables, t.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice));
        SS_TRY(hipMalloc((void**)&S.pass, kPassWords * sizeof(uint32_t)));
        S.bytes += kPassWords * sizeof(uint32_t);
    }
    uint32_t seed_window[kWindowWords], window[kPassWords], at[kRandDeg], step[kRandDeg];
    rand_seed_state(seed, seed_window);
    rand_extend(seed_window, kRandDeg, (int)kWindowWords);
    rand_poly_pow(kRandFirstDraw, at);                              // x^(the pass's first draw)
    uint64_t step_pairs = 0;
    uint32_t completed = 0, state = 0;
    int32_t n_passes = 0;
    while (completed < n_samples) {
        uint64_t want = pairs_per_pass ? pairs_per_pass : provision_pairs(n_samples - completed);
        const uint32_t pairs = (uint32_t)(want < kMaxPassPairs ? want : kMaxPassPairs);
        const uint32_t n_groups = (uint32_t)(((uint64_t)pairs + (uint64_t)P * T - 1) / ((uint64_t)P * T));
        const size_t chunks = (size_t)n_groups * T;
        if (chunks > S.map_chunks) {
            if (S.maps) { (void)hipFree(S.maps); S.maps = nullptr; S.bytes -= (S.map_chunks + 2 * (S.map_chunks / T)) * sizeof(SampleMap); S.map_chunks = 0; }
            SS_TRY(hipMalloc(&S.maps, (chunks + 2 * (size_t)n_groups) * sizeof(SampleMap)));
            S.map_chunks = chunks;
            S.bytes += (chunks + 2 * (size_t)n_groups) * sizeof(SampleMap);
        }
        SampleMap* chunk_maps = (SampleMap*)S.maps;
        SampleMap* group_maps = chunk_maps + S.map_chunks;
        uint2* entry = (uint2*)(group_maps + S.map_chunks / T);
        rand_poly_apply(at, seed_window, kRandDeg, window);
        rand_extend(window, kRandDeg, (int)kWindowWords);
        SS_TRY(hipMemcpyAsync(S.pass, window, kWindowWords * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(sample_summary_kernel, dim3(n_groups), dim3(T), 0, stream, S.tables, S.pass, pairs, chunk_maps, group_maps);
        hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(256), 0, stream, group_maps, n_groups, completed, state, entry, S.pass + kPassResult);
        hipLaunchKernelGGL(sample_emit_kernel, dim3(n_groups), dim3(T), 0, stream, S.tables, S.pass, pairs, chunk_maps, entry, n_samples, res_x, spp,
                           aperture, d_out);
        SS_TRY(hipGetLastError());
        uint32_t result[2] = {0, 0};
        SS_TRY(hipMemcpyAsync(result, S.pass + kPassResult, sizeof result, hipMemcpyDeviceToHost, stream));
        SS_TRY(hipStreamSynchronize(stream));
        n_passes++;
        if (result[0] < completed || result[1] > 1u) return hipErrorUnknown;       // (a pass never loses samples)
        completed = result[0]; state = result[1];
        if (completed < n_samples) {                                // the stream continues where this pass stopped
            if (step_pairs != pairs) { rand_poly_pow(2ull * pairs, step); step_pairs = pairs; }
            rand_poly_mul(at, step, at);
        }
    }
    if (passes) *passes = n_passes;
    return hipSuccess;
}

}  // namespace p3d
