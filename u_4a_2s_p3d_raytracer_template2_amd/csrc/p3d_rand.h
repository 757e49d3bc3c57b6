// p3d_rand.h -- the host C library's srand() / rand(), restated so that any position of the stream can be reached
// directly, and the reference's pixel-sample loop (RT/main.cpp:776-801) restated as a two-state machine over that
// stream.  Plain C++ for host and device, like p3d_powf.h.
//
// glibc's rand() (stdlib/random_r.c, TYPE_3) is an additive feedback generator over 32-bit words:
//   srand(seed):  r[0] = seed (0 becomes 1) as int32_t;  r[i] = 16807 * (r[i-1] % 127773) - 2836 * (r[i-1] / 127773),
//                 plus 2147483647 when negative, for i = 1..30 (C's truncating / and %);  r[31..33] = r[0..2];
//   from i = 34:  r[i] = r[i-31] + r[i-3]  mod 2^32;  the k-th rand() is r[344 + k] >> 1  (310 values are discarded).
// Here s[n] = r[3 + n]: s[n] = s[n-31] + s[n-3] holds for every n >= 31, s[0..30] is the seed state and the k-th rand() is
// s[341 + k] >> 1.  The recurrence is linear over Z / 2^32, so with c = x^n mod (x^31 - x^28 - 1)
//   s[n + k] = sum_j c[j] * s[j + k]      (j = 0..30, any k >= 0):
// a polynomial of 31 words is a jump by n, products of polynomials add jumps.  tests/test_rand_port.py pins all of it to
// this image's libc on the CPU; tests/test_gpu_sample_stream.py shows the device computes the same bits.
//
// The sample loop draws two values for the pixel jitter, then pairs until one lies in the unit disk: every sample consumes
// an even number of draws, so the stream is a sequence of PAIRS read by a machine of two states -- A: the pair is a
// jitter, go to B; B: the pair is a lens candidate, accepted: the sample is complete, go to A; rejected: stay.  A run of
// pairs is then a map {A, B} -> (exit state, samples completed); such maps compose (SampleMap), which is what lets
// csrc/sample_stream.hip parse the stream in parallel.
#ifndef P3D_RAND_H
#define P3D_RAND_H

#include <stddef.h>
#include <stdint.h>
#if defined(P3D_RAND_HOST_CHECK)
// tests/test_rand_port.py compiles this header with g++ to run the same expressions against libc on the CPU
#define P3D_RAND_FN static inline
#define P3D_RAND_MEMBER inline
#elif defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P3D_RAND_FN __host__ __device__ static inline
#define P3D_RAND_MEMBER __host__ __device__ inline
#else
#define P3D_RAND_FN static inline
#define P3D_RAND_MEMBER inline
#endif
#if defined(__clang__)
#define P3D_RAND_UNROLL _Pragma("unroll")
#else
#define P3D_RAND_UNROLL
#endif

namespace p3d {

constexpr int kRandDeg = 31;               // words of state: s[n] = s[n-31] + s[n-3]
constexpr uint32_t kRandFirstDraw = 341;   // the k-th rand() is s[341 + k] >> 1

// srand(seed): s[0..30].  The products fit 32 bits in value (Schrage's split), so unsigned wrap-around computes them.
P3D_RAND_FN void rand_seed_state(uint32_t seed, uint32_t s[kRandDeg]) {
    int32_t r[34];
    r[0] = seed ? (int32_t)seed : 1;
    for (int i = 1; i < 31; i++) {
        const int32_t hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
        int32_t w = (int32_t)(16807u * (uint32_t)lo - 2836u * (uint32_t)hi);
        if (w < 0) w = (int32_t)((uint32_t)w + 2147483647u);
        r[i] = w;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int k = 0; k < kRandDeg; k++) s[k] = (uint32_t)r[3 + k];
}

// s[from .. to-1] from the 31 values in front of them
P3D_RAND_FN void rand_extend(uint32_t* s, int from, int to) {
    for (int i = from; i < to; i++) s[i] = s[i - 31] + s[i - 3];
}

// st = s[n .. n+30] becomes s[n+31 .. n+61], in place: constant indices, so an unrolled caller keeps st in registers
P3D_RAND_FN void rand_advance31(uint32_t st[kRandDeg]) {
    P3D_RAND_UNROLL
    for (int i = 0; i < kRandDeg; i++) st[i] += st[(i + 28) % kRandDeg];
}

// ---- the jump polynomial: multiply, reduce, power.  x^31 = x^28 + 1, so x^k = x^(k-3) + x^(k-31) for k >= 31.
P3D_RAND_FN void rand_poly_reduce(uint32_t p[2 * kRandDeg - 1]) {
    for (int k = 2 * kRandDeg - 2; k >= kRandDeg; k--) { p[k - 3] += p[k]; p[k - 31] += p[k]; }
}
P3D_RAND_FN void rand_poly_mul(const uint32_t a[kRandDeg], const uint32_t b[kRandDeg], uint32_t c[kRandDeg]) {   // c may be a or b
    uint32_t p[2 * kRandDeg - 1];
    for (int k = 0; k < 2 * kRandDeg - 1; k++) p[k] = 0;
    for (int i = 0; i < kRandDeg; i++)
        for (int j = 0; j < kRandDeg; j++) p[i + j] += a[i] * b[j];
    rand_poly_reduce(p);
    for (int k = 0; k < kRandDeg; k++) c[k] = p[k];
}
P3D_RAND_FN void rand_poly_mul_x(uint32_t c[kRandDeg]) {
    const uint32_t top = c[kRandDeg - 1];
    for (int j = kRandDeg - 1; j >= 1; j--) c[j] = c[j - 1];
    c[0] = top; c[28] += top;
}
P3D_RAND_FN void rand_poly_one(uint32_t c[kRandDeg]) {
    for (int j = 0; j < kRandDeg; j++) c[j] = j == 0;
}
// c = x^n, square and multiply from the top bit down
P3D_RAND_FN void rand_poly_pow(uint64_t n, uint32_t c[kRandDeg]) {
    rand_poly_one(c);
    int top = 63;
    while (top >= 0 && !((n >> top) & 1)) top--;
    for (int b = top; b >= 0; b--) {
        rand_poly_mul(c, c, c);
        if ((n >> b) & 1) rand_poly_mul_x(c);
    }
}
// out[k] = s[m + n + k], k = 0..count-1, from c = x^n and w = s[m .. m + 30 + count - 1]
P3D_RAND_FN void rand_poly_apply(const uint32_t c[kRandDeg], const uint32_t* w, int count, uint32_t* out) {
    for (int k = 0; k < count; k++) {
        uint32_t v = 0;
        for (int j = 0; j < kRandDeg; j++) v += c[j] * w[j + k];
        out[k] = v;
    }
}

// rand_float() as g++ compiles RT/maths.h:67-70, ((float)rand() / ((float)RAND_MAX + 1.0)) returned as float: (float) of the
// 31-bit draw rounds to nearest even (and reaches 2^31, so the result can be 1.0f), the division by 2147483648.0 runs in
// double, where it is exact, and its result -- a 24-bit significand scaled by 2^-31, never subnormal -- is a float, so the
// final rounding changes nothing: one float multiplication by 2^-31 gives the same bits.
P3D_RAND_FN float rand_float_of(uint32_t draw) { return (float)(int32_t)draw * 0x1p-31f; }

// sampleUnitDisk()'s candidate (RT/main.cpp:723-730) from a pair of draws: the first draw lands in y (the two draws are
// constructor arguments, evaluated right to left).  True when the candidate is accepted.
P3D_RAND_FN bool rand_lens_candidate(uint32_t d0, uint32_t d1, float& dx, float& dy) {
    const float ry = rand_float_of(d0);
    const float rx = rand_float_of(d1);
    dx = rx * 2 - 1.0f; dy = ry * 2 - 1.0f;
    return !(dx * dx + dy * dy + 0.0f * 0.0f >= 1.0f);
}

// ---- runs of pairs as maps.  a / b: the run entered in state A / B -> samples completed << 1 | exit state (0 = A, 1 = B)
struct SampleMap { uint32_t a, b; };
P3D_RAND_FN SampleMap sample_map_identity() { SampleMap m; m.a = 0u; m.b = 1u; return m; }
P3D_RAND_FN uint32_t sample_map_apply(const SampleMap& g, uint32_t entry) {          // entry and result: count << 1 | state
    return (entry & ~1u) + ((entry & 1u) ? g.b : g.a);
}
P3D_RAND_FN SampleMap sample_map_compose(const SampleMap& f, const SampleMap& g) {    // the run of f, then the run of g
    SampleMap h; h.a = sample_map_apply(g, f.a); h.b = sample_map_apply(g, f.b); return h;
}

// Reads n_pairs pairs of draws, the first of them s[n], s[n+1] with st = s[n .. n+30], and hands each to sink.pair(d0, d1)
// (the rand() values, already shifted); stops early once sink.done().  62 draws = 31 pairs per round, every index constant.
template <typename Sink>
P3D_RAND_FN void rand_read_pairs(uint32_t st[kRandDeg], uint32_t n_pairs, Sink& sink) {
    for (uint32_t at = 0; at < n_pairs; at += kRandDeg) {
        if (sink.done()) break;
        uint32_t nx[kRandDeg];
        P3D_RAND_UNROLL
        for (int i = 0; i < kRandDeg; i++) nx[i] = st[i];
        rand_advance31(nx);
        P3D_RAND_UNROLL
        for (int m = 0; m < kRandDeg; m++) {
            if (at + (uint32_t)m < n_pairs) {
                const uint32_t w0 = 2 * m < kRandDeg ? st[(2 * m) % kRandDeg] : nx[(2 * m) % kRandDeg];
                const uint32_t w1 = 2 * m + 1 < kRandDeg ? st[(2 * m + 1) % kRandDeg] : nx[(2 * m + 1) % kRandDeg];
                sink.pair(w0 >> 1, w1 >> 1);
            }
        }
        P3D_RAND_UNROLL
        for (int i = 0; i < kRandDeg; i++) st[i] = nx[i];
        rand_advance31(st);
    }
}

// The map of a run: both entries are followed at once (they share every acceptance test).
struct SampleSummarySink {
    uint32_t state_a = 0, state_b = 1, count_a = 0, count_b = 0;
    P3D_RAND_MEMBER void pair(uint32_t d0, uint32_t d1) {
        float dx, dy;
        const uint32_t accepted = rand_lens_candidate(d0, d1, dx, dy) ? 1u : 0u;
        const uint32_t done_a = state_a & accepted, done_b = state_b & accepted;    // only state B completes a sample
        count_a += done_a; count_b += done_b;
        state_a = done_a ^ 1u; state_b = done_b ^ 1u;                              // A -> B; B -> A when accepted
    }
    P3D_RAND_MEMBER bool done() const { return false; }
    P3D_RAND_MEMBER SampleMap map() const { SampleMap m; m.a = count_a << 1 | state_a; m.b = count_b << 1 | state_b; return m; }
};

// The writes of generate_samples() (csrc/host/p3d_scene.cpp) for a run entered in `state` at sample `s`: out[s].xy in
// state A, out[s].zw on acceptance -- two separate stores, so a sample that straddles runs needs no special case.  The float
// expressions are the host's, operand for operand (int operands convert first; IEEE division; no contraction).  Samples
// from n_samples on are not written.
struct SampleEmitSink {
    float* out; uint32_t n_samples, s, state;
    int32_t x, y, i, j, res_x, spp; float aperture;
    P3D_RAND_MEMBER void init(float* out_, uint32_t n_samples_, uint32_t s_, uint32_t state_, int32_t res_x_, int32_t spp_, float aperture_) {
        out = out_; n_samples = n_samples_; s = s_; state = state_; res_x = res_x_; spp = spp_; aperture = aperture_;
        const uint32_t per = (uint32_t)spp * (uint32_t)spp, pixel = s / per, sub = s % per;
        i = (int32_t)(sub / (uint32_t)spp); j = (int32_t)(sub % (uint32_t)spp);
        x = (int32_t)(pixel % (uint32_t)res_x); y = (int32_t)(pixel / (uint32_t)res_x);
    }
    P3D_RAND_MEMBER void pair(uint32_t d0, uint32_t d1) {
        if (state == 0u) {
            if (s < n_samples) {
                float* o = out + 4 * (size_t)s;
                o[0] = x + (i + rand_float_of(d0)) / spp;                 // RT/main.cpp:781-782
                o[1] = y + (j + rand_float_of(d1)) / spp;
            }
            state = 1u;
        } else {
            float dx, dy;
            if (rand_lens_candidate(d0, d1, dx, dy)) {
                if (s < n_samples) {
                    float* o = out + 4 * (size_t)s;
                    o[2] = dx * aperture; o[3] = dy * aperture;           // cameralens = disk * aperture, RT/main.cpp:790
                }
                s++;
                if (++j == spp) { j = 0; if (++i == spp) { i = 0; if (++x == res_x) { x = 0; y++; } } }
                state = 0u;
            }
        }
    }
    P3D_RAND_MEMBER bool done() const { return s >= n_samples; }
};

}  // namespace p3d
#endif
