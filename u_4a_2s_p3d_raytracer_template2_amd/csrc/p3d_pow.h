// p3d_pow.h -- the host C library's pow(double, double), restated for the device.
//
// With SCHLICK_APPROX (P3D_FEATURE_SCHLICK) the reference's Fresnel weight is KR = rI + (1 - rI) * pow(1 - cos_theta_i, 5)
// (RT/main.cpp:699-702): a float base widened to double, glibc's pow, and the double result multiplied and added BEFORE
// the one rounding to float.  glibc's pow is not correctly rounded (on the 2^24 + 1 reachable bases k * 2^-24 it is one
// ulp off the exact x^5 about once in 10^3), so a correctly rounded x^5 would not give the reference's KR in every bit.
// This header is therefore the algorithm itself, as p3d_powf.h is for powf: glibc 2.35 sysdeps/ieee754/dbl-64/e_pow.c
// (Szabolcs Nagy's table-driven pow of ARM optimized-routines) in the variant x86-64 selects at load time on a host with
// FMA and AVX2 (__pow_fma): log(x) from a 128-entry {1/c, log(c), tail} table and a degree-8 polynomial carried in
// double-double, y * log(x) split into a head and a tail with one FMA, exp from a 128-entry 2^(k/128) table and a
// degree-5 polynomial, one final rounding.  The constants below are that routine's tables (__pow_log_data with
// POW_LOG_TABLE_BITS 7, __exp_data with EXP_TABLE_BITS 7), read out of the image's libm.so.6 and checked value by value;
// which multiply-adds are fused was read from the same object code (glibc is built with GCC's default -ffp-contract=fast,
// so besides the two explicit __builtin_fma of the source, kd*Ln2hi + logc, z*InvLn2N + Shift, the Horner steps and the
// final scale + scale*tmp are fused -- and the subnormal branch of specialcase() is not).
// tests/test_schlick_port.py compiles this header for the host and compares it with libm; tests/test_gpu_schlick.py
// compares the device with the same libm.
//
// The tables (6 KiB) are NOT part of the scene blob: they live in their own __device__ array, read through the vector
// memory path (L1/L2), and only the kernels instantiated with Schlick touch them -- the LDS budget and the blob layout
// of every scene stay as they are.
#ifndef P3D_POW_H
#define P3D_POW_H

#include <stdint.h>
#if defined(P3D_POW_HOST_CHECK)
// tests/test_schlick_port.py compiles this header with g++ -mfma -ffp-contract=off to run the same expressions on the CPU
#define __device__
#define __forceinline__ inline
#else
#include <hip/hip_runtime.h>
#endif

namespace p3d {

// Ln2hi Ln2lo | A[0..6] of the log polynomial | InvLn2N Shift NegLn2hiN NegLn2loN | C2 C3 C4 C5 of the exp polynomial | pad
#define P3D_DPOW_COEF_INIT { \
    0x1.62e42fefa3800p-1, 0x1.ef35793c76730p-45,                      /* Ln2hi Ln2lo */ \
    -0x1.0000000000000p-1, -0x1.5555555555560p-1, 0x1.0000000000006p-1, 0x1.999999959554ep-1, -0x1.555555529a47ap-1, -0x1.2495b9b4845e9p+0, 0x1.0002b8b263fc3p+0, \
    0x1.71547652b82fep+7, 0x1.8000000000000p+52, -0x1.62e42fefa0000p-8, -0x1.cf79abc9e3b3ap-47, \
    0x1.ffffffffffdbdp-2, 0x1.555555555543cp-3, 0x1.55555cf172b91p-5, 0x1.1111167a4d017p-7, 0.0 \
}
// __pow_log_data.tab without its pad word: {invc, logc, logctail, 0} for the 128 sub-intervals of [OFF, 2 OFF)
#define P3D_DPOW_LOG_TAB_INIT { \
    {0x1.6a00000000000p+0, -0x1.62c82f2b9c800p-2, 0x1.ab42428375680p-48, 0.0}, {0x1.6800000000000p+0, -0x1.5d1bdbf580800p-2, -0x1.ca508d8e0f720p-46, 0.0}, \
    {0x1.6600000000000p+0, -0x1.5767717455800p-2, -0x1.362a4d5b6506dp-45, 0.0}, {0x1.6400000000000p+0, -0x1.51aad872df800p-2, -0x1.684e49eb067d5p-49, 0.0}, \
    {0x1.6200000000000p+0, -0x1.4be5f95777800p-2, -0x1.41b6993293ee0p-47, 0.0}, {0x1.6000000000000p+0, -0x1.4618bc21c6000p-2, 0x1.3d82f484c84ccp-46, 0.0}, \
    {0x1.5e00000000000p+0, -0x1.404308686a800p-2, 0x1.c42f3ed820b3ap-50, 0.0}, {0x1.5c00000000000p+0, -0x1.3a64c55694800p-2, 0x1.0b1c686519460p-45, 0.0}, \
    {0x1.5a00000000000p+0, -0x1.347dd9a988000p-2, 0x1.5594dd4c58092p-45, 0.0}, {0x1.5800000000000p+0, -0x1.2e8e2bae12000p-2, 0x1.67b1e99b72bd8p-45, 0.0}, \
    {0x1.5600000000000p+0, -0x1.2895a13de8800p-2, 0x1.5ca14b6cfb03fp-46, 0.0}, {0x1.5600000000000p+0, -0x1.2895a13de8800p-2, 0x1.5ca14b6cfb03fp-46, 0.0}, \
    {0x1.5400000000000p+0, -0x1.22941fbcf7800p-2, -0x1.65a242853da76p-46, 0.0}, {0x1.5200000000000p+0, -0x1.1c898c1699800p-2, -0x1.fafbc68e75404p-46, 0.0}, \
    {0x1.5000000000000p+0, -0x1.1675cababa800p-2, 0x1.f1fc63382a8f0p-46, 0.0}, {0x1.4e00000000000p+0, -0x1.1058bf9ae4800p-2, -0x1.6a8c4fd055a66p-45, 0.0}, \
    {0x1.4c00000000000p+0, -0x1.0a324e2739000p-2, -0x1.c6bee7ef4030ep-47, 0.0}, {0x1.4a00000000000p+0, -0x1.0402594b4d000p-2, -0x1.036b89ef42d7fp-48, 0.0}, \
    {0x1.4a00000000000p+0, -0x1.0402594b4d000p-2, -0x1.036b89ef42d7fp-48, 0.0}, {0x1.4800000000000p+0, -0x1.fb9186d5e4000p-3, 0x1.d572aab993c87p-47, 0.0}, \
    {0x1.4600000000000p+0, -0x1.ef0adcbdc6000p-3, 0x1.b26b79c86af24p-45, 0.0}, {0x1.4400000000000p+0, -0x1.e27076e2af000p-3, -0x1.72f4f543fff10p-46, 0.0}, \
    {0x1.4200000000000p+0, -0x1.d5c216b4fc000p-3, 0x1.1ba91bbca681bp-45, 0.0}, {0x1.4000000000000p+0, -0x1.c8ff7c79aa000p-3, 0x1.7794f689f8434p-45, 0.0}, \
    {0x1.4000000000000p+0, -0x1.c8ff7c79aa000p-3, 0x1.7794f689f8434p-45, 0.0}, {0x1.3e00000000000p+0, -0x1.bc286742d9000p-3, 0x1.94eb0318bb78fp-46, 0.0}, \
    {0x1.3c00000000000p+0, -0x1.af3c94e80c000p-3, 0x1.a4e633fcd9066p-52, 0.0}, {0x1.3a00000000000p+0, -0x1.a23bc1fe2b000p-3, -0x1.58c64dc46c1eap-45, 0.0}, \
    {0x1.3a00000000000p+0, -0x1.a23bc1fe2b000p-3, -0x1.58c64dc46c1eap-45, 0.0}, {0x1.3800000000000p+0, -0x1.9525a9cf45000p-3, -0x1.ad1d904c1d4e3p-45, 0.0}, \
    {0x1.3600000000000p+0, -0x1.87fa06520d000p-3, 0x1.bbdbf7fdbfa09p-45, 0.0}, {0x1.3400000000000p+0, -0x1.7ab890210e000p-3, 0x1.bdb9072534a58p-45, 0.0}, \
    {0x1.3400000000000p+0, -0x1.7ab890210e000p-3, 0x1.bdb9072534a58p-45, 0.0}, {0x1.3200000000000p+0, -0x1.6d60fe719d000p-3, -0x1.0e46aa3b2e266p-46, 0.0}, \
    {0x1.3000000000000p+0, -0x1.5ff3070a79000p-3, -0x1.e9e439f105039p-46, 0.0}, {0x1.3000000000000p+0, -0x1.5ff3070a79000p-3, -0x1.e9e439f105039p-46, 0.0}, \
    {0x1.2e00000000000p+0, -0x1.526e5e3a1b000p-3, -0x1.0de8b90075b8fp-45, 0.0}, {0x1.2c00000000000p+0, -0x1.44d2b6ccb8000p-3, 0x1.70cc16135783cp-46, 0.0}, \
    {0x1.2c00000000000p+0, -0x1.44d2b6ccb8000p-3, 0x1.70cc16135783cp-46, 0.0}, {0x1.2a00000000000p+0, -0x1.371fc201e9000p-3, 0x1.178864d27543ap-48, 0.0}, \
    {0x1.2800000000000p+0, -0x1.29552f81ff000p-3, -0x1.48d301771c408p-45, 0.0}, {0x1.2600000000000p+0, -0x1.1b72ad52f6000p-3, -0x1.e80a41811a396p-45, 0.0}, \
    {0x1.2600000000000p+0, -0x1.1b72ad52f6000p-3, -0x1.e80a41811a396p-45, 0.0}, {0x1.2400000000000p+0, -0x1.0d77e7cd09000p-3, 0x1.a699688e85bf4p-47, 0.0}, \
    {0x1.2400000000000p+0, -0x1.0d77e7cd09000p-3, 0x1.a699688e85bf4p-47, 0.0}, {0x1.2200000000000p+0, -0x1.fec9131dbe000p-4, -0x1.575545ca333f2p-45, 0.0}, \
    {0x1.2000000000000p+0, -0x1.e27076e2b0000p-4, 0x1.a342c2af0003cp-45, 0.0}, {0x1.2000000000000p+0, -0x1.e27076e2b0000p-4, 0x1.a342c2af0003cp-45, 0.0}, \
    {0x1.1e00000000000p+0, -0x1.c5e548f5bc000p-4, -0x1.d0c57585fbe06p-46, 0.0}, {0x1.1c00000000000p+0, -0x1.a926d3a4ae000p-4, 0x1.53935e85baac8p-45, 0.0}, \
    {0x1.1c00000000000p+0, -0x1.a926d3a4ae000p-4, 0x1.53935e85baac8p-45, 0.0}, {0x1.1a00000000000p+0, -0x1.8c345d631a000p-4, 0x1.37c294d2f5668p-46, 0.0}, \
    {0x1.1a00000000000p+0, -0x1.8c345d631a000p-4, 0x1.37c294d2f5668p-46, 0.0}, {0x1.1800000000000p+0, -0x1.6f0d28ae56000p-4, -0x1.69737c93373dap-45, 0.0}, \
    {0x1.1600000000000p+0, -0x1.51b073f062000p-4, 0x1.f025b61c65e57p-46, 0.0}, {0x1.1600000000000p+0, -0x1.51b073f062000p-4, 0x1.f025b61c65e57p-46, 0.0}, \
    {0x1.1400000000000p+0, -0x1.341d7961be000p-4, 0x1.c5edaccf913dfp-45, 0.0}, {0x1.1400000000000p+0, -0x1.341d7961be000p-4, 0x1.c5edaccf913dfp-45, 0.0}, \
    {0x1.1200000000000p+0, -0x1.16536eea38000p-4, 0x1.47c5e768fa309p-46, 0.0}, {0x1.1000000000000p+0, -0x1.f0a30c0118000p-5, 0x1.d599e83368e91p-45, 0.0}, \
    {0x1.1000000000000p+0, -0x1.f0a30c0118000p-5, 0x1.d599e83368e91p-45, 0.0}, {0x1.0e00000000000p+0, -0x1.b42dd71198000p-5, 0x1.c827ae5d6704cp-46, 0.0}, \
    {0x1.0e00000000000p+0, -0x1.b42dd71198000p-5, 0x1.c827ae5d6704cp-46, 0.0}, {0x1.0c00000000000p+0, -0x1.77458f632c000p-5, -0x1.cfc4634f2a1eep-45, 0.0}, \
    {0x1.0c00000000000p+0, -0x1.77458f632c000p-5, -0x1.cfc4634f2a1eep-45, 0.0}, {0x1.0a00000000000p+0, -0x1.39e87b9fec000p-5, 0x1.502b7f526feaap-48, 0.0}, \
    {0x1.0a00000000000p+0, -0x1.39e87b9fec000p-5, 0x1.502b7f526feaap-48, 0.0}, {0x1.0800000000000p+0, -0x1.f829b0e780000p-6, -0x1.980267c7e09e4p-45, 0.0}, \
    {0x1.0800000000000p+0, -0x1.f829b0e780000p-6, -0x1.980267c7e09e4p-45, 0.0}, {0x1.0600000000000p+0, -0x1.7b91b07d58000p-6, -0x1.88d5493faa639p-45, 0.0}, \
    {0x1.0400000000000p+0, -0x1.fc0a8b0fc0000p-7, -0x1.f1e7cf6d3a69cp-50, 0.0}, {0x1.0400000000000p+0, -0x1.fc0a8b0fc0000p-7, -0x1.f1e7cf6d3a69cp-50, 0.0}, \
    {0x1.0200000000000p+0, -0x1.fe02a6b100000p-8, -0x1.9e23f0dda40e4p-46, 0.0}, {0x1.0200000000000p+0, -0x1.fe02a6b100000p-8, -0x1.9e23f0dda40e4p-46, 0.0}, \
    {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0.0}, {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0.0}, \
    {0x1.fc00000000000p-1, 0x1.0101575890000p-7, -0x1.0c76b999d2be8p-46, 0.0}, {0x1.f800000000000p-1, 0x1.0205658938000p-6, -0x1.3dc5b06e2f7d2p-45, 0.0}, \
    {0x1.f400000000000p-1, 0x1.8492528c90000p-6, -0x1.aa0ba325a0c34p-45, 0.0}, {0x1.f000000000000p-1, 0x1.0415d89e74000p-5, 0x1.111c05cf1d753p-47, 0.0}, \
    {0x1.ec00000000000p-1, 0x1.466aed42e0000p-5, -0x1.c167375bdfd28p-45, 0.0}, {0x1.e800000000000p-1, 0x1.894aa149fc000p-5, -0x1.97995d05a267dp-46, 0.0}, \
    {0x1.e400000000000p-1, 0x1.ccb73cdddc000p-5, -0x1.a68f247d82807p-46, 0.0}, {0x1.e200000000000p-1, 0x1.eea31c006c000p-5, -0x1.e113e4fc93b7bp-47, 0.0}, \
    {0x1.de00000000000p-1, 0x1.1973bd1466000p-4, -0x1.5325d560d9e9bp-45, 0.0}, {0x1.da00000000000p-1, 0x1.3bdf5a7d1e000p-4, 0x1.cc85ea5db4ed7p-45, 0.0}, \
    {0x1.d600000000000p-1, 0x1.5e95a4d97a000p-4, -0x1.c69063c5d1d1ep-45, 0.0}, {0x1.d400000000000p-1, 0x1.700d30aeac000p-4, 0x1.c1e8da99ded32p-49, 0.0}, \
    {0x1.d000000000000p-1, 0x1.9335e5d594000p-4, 0x1.3115c3abd47dap-45, 0.0}, {0x1.cc00000000000p-1, 0x1.b6ac88dad6000p-4, -0x1.390802bf768e5p-46, 0.0}, \
    {0x1.ca00000000000p-1, 0x1.c885801bc4000p-4, 0x1.646d1c65aacd3p-45, 0.0}, {0x1.c600000000000p-1, 0x1.ec739830a2000p-4, -0x1.dc068afe645e0p-45, 0.0}, \
    {0x1.c400000000000p-1, 0x1.fe89139dbe000p-4, -0x1.534d64fa10afdp-45, 0.0}, {0x1.c000000000000p-1, 0x1.1178e8227e000p-3, 0x1.1ef78ce2d07f2p-45, 0.0}, \
    {0x1.be00000000000p-1, 0x1.1aa2b7e23f000p-3, 0x1.ca78e44389934p-45, 0.0}, {0x1.ba00000000000p-1, 0x1.2d1610c868000p-3, 0x1.39d6ccb81b4a1p-47, 0.0}, \
    {0x1.b800000000000p-1, 0x1.365fcb0159000p-3, 0x1.62fa8234b7289p-51, 0.0}, {0x1.b400000000000p-1, 0x1.4913d8333b000p-3, 0x1.5837954fdb678p-45, 0.0}, \
    {0x1.b200000000000p-1, 0x1.527e5e4a1b000p-3, 0x1.633e8e5697dc7p-45, 0.0}, {0x1.ae00000000000p-1, 0x1.6574ebe8c1000p-3, 0x1.9cf8b2c3c2e78p-46, 0.0}, \
    {0x1.ac00000000000p-1, 0x1.6f0128b757000p-3, -0x1.5118de59c21e1p-45, 0.0}, {0x1.aa00000000000p-1, 0x1.7898d85445000p-3, -0x1.c661070914305p-46, 0.0}, \
    {0x1.a600000000000p-1, 0x1.8beafeb390000p-3, -0x1.73d54aae92cd1p-47, 0.0}, {0x1.a400000000000p-1, 0x1.95a5adcf70000p-3, 0x1.7f22858a0ff6fp-47, 0.0}, \
    {0x1.a000000000000p-1, 0x1.a93ed3c8ae000p-3, -0x1.8724350562169p-45, 0.0}, {0x1.9e00000000000p-1, 0x1.b31d8575bd000p-3, -0x1.c358d4eace1aap-47, 0.0}, \
    {0x1.9c00000000000p-1, 0x1.bd087383be000p-3, -0x1.d4bc4595412b6p-45, 0.0}, {0x1.9a00000000000p-1, 0x1.c6ffbc6f01000p-3, -0x1.1ec72c5962bd2p-48, 0.0}, \
    {0x1.9600000000000p-1, 0x1.db13db0d49000p-3, -0x1.aff2af715b035p-45, 0.0}, {0x1.9400000000000p-1, 0x1.e530effe71000p-3, 0x1.212276041f430p-51, 0.0}, \
    {0x1.9200000000000p-1, 0x1.ef5ade4dd0000p-3, -0x1.a211565bb8e11p-51, 0.0}, {0x1.9000000000000p-1, 0x1.f991c6cb3b000p-3, 0x1.bcbecca0cdf30p-46, 0.0}, \
    {0x1.8c00000000000p-1, 0x1.07138604d5800p-2, 0x1.89cdb16ed4e91p-48, 0.0}, {0x1.8a00000000000p-1, 0x1.0c42d67616000p-2, 0x1.7188b163ceae9p-45, 0.0}, \
    {0x1.8800000000000p-1, 0x1.1178e8227e800p-2, -0x1.c210e63a5f01cp-45, 0.0}, {0x1.8600000000000p-1, 0x1.16b5ccbacf800p-2, 0x1.b9acdf7a51681p-45, 0.0}, \
    {0x1.8400000000000p-1, 0x1.1bf99635a6800p-2, 0x1.ca6ed5147bdb7p-45, 0.0}, {0x1.8200000000000p-1, 0x1.214456d0eb800p-2, 0x1.a87deba46baeap-47, 0.0}, \
    {0x1.7e00000000000p-1, 0x1.2bef07cdc9000p-2, 0x1.a9cfa4a5004f4p-45, 0.0}, {0x1.7c00000000000p-1, 0x1.314f1e1d36000p-2, -0x1.8e27ad3213cb8p-45, 0.0}, \
    {0x1.7a00000000000p-1, 0x1.36b6776be1000p-2, 0x1.16ecdb0f177c8p-46, 0.0}, {0x1.7800000000000p-1, 0x1.3c25277333000p-2, 0x1.83b54b606bd5cp-46, 0.0}, \
    {0x1.7600000000000p-1, 0x1.419b423d5e800p-2, 0x1.8e436ec90e09dp-47, 0.0}, {0x1.7400000000000p-1, 0x1.4718dc271c800p-2, -0x1.f27ce0967d675p-45, 0.0}, \
    {0x1.7200000000000p-1, 0x1.4c9e09e173000p-2, -0x1.e20891b0ad8a4p-45, 0.0}, {0x1.7000000000000p-1, 0x1.522ae0738a000p-2, 0x1.ebe708164c759p-45, 0.0}, \
    {0x1.6e00000000000p-1, 0x1.57bf753c8d000p-2, 0x1.fadedee5d40efp-46, 0.0}, {0x1.6c00000000000p-1, 0x1.5d5bddf596000p-2, -0x1.a0b2a08a465dcp-47, 0.0} }
// __exp_data.tab: {tail, bits of 2^(k/128) with k << 45 subtracted} for k = 0..127
#define P3D_DPOW_EXP_TAB_INIT { \
    0x0000000000000000ull, 0x3ff0000000000000ull, 0x3c9b3b4f1a88bf6eull, 0x3feff63da9fb3335ull, \
    0xbc7160139cd8dc5dull, 0x3fefec9a3e778061ull, 0xbc905e7a108766d1ull, 0x3fefe315e86e7f85ull, \
    0x3c8cd2523567f613ull, 0x3fefd9b0d3158574ull, 0xbc8bce8023f98efaull, 0x3fefd06b29ddf6deull, \
    0x3c60f74e61e6c861ull, 0x3fefc74518759bc8ull, 0x3c90a3e45b33d399ull, 0x3fefbe3ecac6f383ull, \
    0x3c979aa65d837b6dull, 0x3fefb5586cf9890full, 0x3c8eb51a92fdeffcull, 0x3fefac922b7247f7ull, \
    0x3c3ebe3d702f9cd1ull, 0x3fefa3ec32d3d1a2ull, 0xbc6a033489906e0bull, 0x3fef9b66affed31bull, \
    0xbc9556522a2fbd0eull, 0x3fef9301d0125b51ull, 0xbc5080ef8c4eea55ull, 0x3fef8abdc06c31ccull, \
    0xbc91c923b9d5f416ull, 0x3fef829aaea92de0ull, 0x3c80d3e3e95c55afull, 0x3fef7a98c8a58e51ull, \
    0xbc801b15eaa59348ull, 0x3fef72b83c7d517bull, 0xbc8f1ff055de323dull, 0x3fef6af9388c8deaull, \
    0x3c8b898c3f1353bfull, 0x3fef635beb6fcb75ull, 0xbc96d99c7611eb26ull, 0x3fef5be084045cd4ull, \
    0x3c9aecf73e3a2f60ull, 0x3fef54873168b9aaull, 0xbc8fe782cb86389dull, 0x3fef4d5022fcd91dull, \
    0x3c8a6f4144a6c38dull, 0x3fef463b88628cd6ull, 0x3c807a05b0e4047dull, 0x3fef3f49917ddc96ull, \
    0x3c968efde3a8a894ull, 0x3fef387a6e756238ull, 0x3c875e18f274487dull, 0x3fef31ce4fb2a63full, \
    0x3c80472b981fe7f2ull, 0x3fef2b4565e27cddull, 0xbc96b87b3f71085eull, 0x3fef24dfe1f56381ull, \
    0x3c82f7e16d09ab31ull, 0x3fef1e9df51fdee1ull, 0xbc3d219b1a6fbffaull, 0x3fef187fd0dad990ull, \
    0x3c8b3782720c0ab4ull, 0x3fef1285a6e4030bull, 0x3c6e149289cecb8full, 0x3fef0cafa93e2f56ull, \
    0x3c834d754db0abb6ull, 0x3fef06fe0a31b715ull, 0x3c864201e2ac744cull, 0x3fef0170fc4cd831ull, \
    0x3c8fdd395dd3f84aull, 0x3feefc08b26416ffull, 0xbc86a3803b8e5b04ull, 0x3feef6c55f929ff1ull, \
    0xbc924aedcc4b5068ull, 0x3feef1a7373aa9cbull, 0xbc9907f81b512d8eull, 0x3feeecae6d05d866ull, \
    0xbc71d1e83e9436d2ull, 0x3feee7db34e59ff7ull, 0xbc991919b3ce1b15ull, 0x3feee32dc313a8e5ull, \
    0x3c859f48a72a4c6dull, 0x3feedea64c123422ull, 0xbc9312607a28698aull, 0x3feeda4504ac801cull, \
    0xbc58a78f4817895bull, 0x3feed60a21f72e2aull, 0xbc7c2c9b67499a1bull, 0x3feed1f5d950a897ull, \
    0x3c4363ed60c2ac11ull, 0x3feece086061892dull, 0x3c9666093b0664efull, 0x3feeca41ed1d0057ull, \
    0x3c6ecce1daa10379ull, 0x3feec6a2b5c13cd0ull, 0x3c93ff8e3f0f1230ull, 0x3feec32af0d7d3deull, \
    0x3c7690cebb7aafb0ull, 0x3feebfdad5362a27ull, 0x3c931dbdeb54e077ull, 0x3feebcb299fddd0dull, \
    0xbc8f94340071a38eull, 0x3feeb9b2769d2ca7ull, 0xbc87deccdc93a349ull, 0x3feeb6daa2cf6642ull, \
    0xbc78dec6bd0f385full, 0x3feeb42b569d4f82ull, 0xbc861246ec7b5cf6ull, 0x3feeb1a4ca5d920full, \
    0x3c93350518fdd78eull, 0x3feeaf4736b527daull, 0x3c7b98b72f8a9b05ull, 0x3feead12d497c7fdull, \
    0x3c9063e1e21c5409ull, 0x3feeab07dd485429ull, 0x3c34c7855019c6eaull, 0x3feea9268a5946b7ull, \
    0x3c9432e62b64c035ull, 0x3feea76f15ad2148ull, 0xbc8ce44a6199769full, 0x3feea5e1b976dc09ull, \
    0xbc8c33c53bef4da8ull, 0x3feea47eb03a5585ull, 0xbc845378892be9aeull, 0x3feea34634ccc320ull, \
    0xbc93cedd78565858ull, 0x3feea23882552225ull, 0x3c5710aa807e1964ull, 0x3feea155d44ca973ull, \
    0xbc93b3efbf5e2228ull, 0x3feea09e667f3bcdull, 0xbc6a12ad8734b982ull, 0x3feea012750bdabfull, \
    0xbc6367efb86da9eeull, 0x3fee9fb23c651a2full, 0xbc80dc3d54e08851ull, 0x3fee9f7df9519484ull, \
    0xbc781f647e5a3ecfull, 0x3fee9f75e8ec5f74ull, 0xbc86ee4ac08b7db0ull, 0x3fee9f9a48a58174ull, \
    0xbc8619321e55e68aull, 0x3fee9feb564267c9ull, 0x3c909ccb5e09d4d3ull, 0x3feea0694fde5d3full, \
    0xbc7b32dcb94da51dull, 0x3feea11473eb0187ull, 0x3c94ecfd5467c06bull, 0x3feea1ed0130c132ull, \
    0x3c65ebe1abd66c55ull, 0x3feea2f336cf4e62ull, 0xbc88a1c52fb3cf42ull, 0x3feea427543e1a12ull, \
    0xbc9369b6f13b3734ull, 0x3feea589994cce13ull, 0xbc805e843a19ff1eull, 0x3feea71a4623c7adull, \
    0xbc94d450d872576eull, 0x3feea8d99b4492edull, 0x3c90ad675b0e8a00ull, 0x3feeaac7d98a6699ull, \
    0x3c8db72fc1f0eab4ull, 0x3feeace5422aa0dbull, 0xbc65b6609cc5e7ffull, 0x3feeaf3216b5448cull, \
    0x3c7bf68359f35f44ull, 0x3feeb1ae99157736ull, 0xbc93091fa71e3d83ull, 0x3feeb45b0b91ffc6ull, \
    0xbc5da9b88b6c1e29ull, 0x3feeb737b0cdc5e5ull, 0xbc6c23f97c90b959ull, 0x3feeba44cbc8520full, \
    0xbc92434322f4f9aaull, 0x3feebd829fde4e50ull, 0xbc85ca6cd7668e4bull, 0x3feec0f170ca07baull, \
    0x3c71affc2b91ce27ull, 0x3feec49182a3f090ull, 0x3c6dd235e10a73bbull, 0x3feec86319e32323ull, \
    0xbc87c50422622263ull, 0x3feecc667b5de565ull, 0x3c8b1c86e3e231d5ull, 0x3feed09bec4a2d33ull, \
    0xbc91bbd1d3bcbb15ull, 0x3feed503b23e255dull, 0x3c90cc319cee31d2ull, 0x3feed99e1330b358ull, \
    0x3c8469846e735ab3ull, 0x3feede6b5579fdbfull, 0xbc82dfcd978e9db4ull, 0x3feee36bbfd3f37aull, \
    0x3c8c1a7792cb3387ull, 0x3feee89f995ad3adull, 0xbc907b8f4ad1d9faull, 0x3feeee07298db666ull, \
    0xbc55c3d956dcaebaull, 0x3feef3a2b84f15fbull, 0xbc90a40e3da6f640ull, 0x3feef9728de5593aull, \
    0xbc68d6f438ad9334ull, 0x3feeff76f2fb5e47ull, 0xbc91eee26b588a35ull, 0x3fef05b030a1064aull, \
    0x3c74ffd70a5fddcdull, 0x3fef0c1e904bc1d2ull, 0xbc91bdfbfa9298acull, 0x3fef12c25bd71e09ull, \
    0x3c736eae30af0cb3ull, 0x3fef199bdd85529cull, 0x3c8ee3325c9ffd94ull, 0x3fef20ab5fffd07aull, \
    0x3c84e08fd10959acull, 0x3fef27f12e57d14bull, 0x3c63cdaf384e1a67ull, 0x3fef2f6d9406e7b5ull, \
    0x3c676b2c6c921968ull, 0x3fef3720dcef9069ull, 0xbc808a1883ccb5d2ull, 0x3fef3f0b555dc3faull, \
    0xbc8fad5d3ffffa6full, 0x3fef472d4a07897cull, 0xbc900dae3875a949ull, 0x3fef4f87080d89f2ull, \
    0x3c74a385a63d07a7ull, 0x3fef5818dcfba487ull, 0xbc82919e2040220full, 0x3fef60e316c98398ull, \
    0x3c8e5a50d5c192acull, 0x3fef69e603db3285ull, 0x3c843a59ac016b4bull, 0x3fef7321f301b460ull, \
    0xbc82d52107b43e1full, 0x3fef7c97337b9b5full, 0xbc892ab93b470dc9ull, 0x3fef864614f5a129ull, \
    0x3c74b604603a88d3ull, 0x3fef902ee78b3ff6ull, 0x3c83c5ec519d7271ull, 0x3fef9a51fbc74c83ull, \
    0xbc8ff7128fd391f0ull, 0x3fefa4afa2a490daull, 0xbc8dae98e223747dull, 0x3fefaf482d8e67f1ull, \
    0x3c8ec3bc41aa2008ull, 0x3fefba1bee615a27ull, 0x3c842b94c3a9eb32ull, 0x3fefc52b376bba97ull, \
    0x3c8a64a931d185eeull, 0x3fefd0765b6e4540ull, 0xbc8e37bae43be3edull, 0x3fefdbfdad9cbe14ull, \
    0x3c77893b4d91cd9dull, 0x3fefe7c1819e90d8ull, 0x3c5305c14160cc89ull, 0x3feff3c22b8f71f1ull }
struct alignas(16) PowTables { double coef[18]; double log[128][4]; uint64_t exp[256]; };
__device__ static const PowTables kPowTables = {P3D_DPOW_COEF_INIT, P3D_DPOW_LOG_TAB_INIT, P3D_DPOW_EXP_TAB_INIT};
enum { kPowLogAt = 18, kPowExpAt = 18 + 512 };           // where the two tables start, in doubles

struct alignas(16) PowPair { double a, b; };
__device__ __forceinline__ uint64_t pow_bits(double d) { return __builtin_bit_cast(uint64_t, d); }
__device__ __forceinline__ double pow_double(uint64_t u) { return __builtin_bit_cast(double, u); }

// The tables through the vector memory path.  `zero` is a VGPR holding 0 that the compiler cannot see through: with a
// provably uniform address it would use scalar loads and keep the coefficients in SGPR pairs (constants
// in scalar registers spilled SGPRs into the traversal loops).
struct PowTab {
    const double* base; uint32_t zero;
    __device__ __forceinline__ PowTab() : base(kPowTables.coef) {
        zero = 0u;
#ifndef P3D_POW_HOST_CHECK
        asm volatile("" : "+v"(zero));
#endif
    }
    __device__ __forceinline__ PowPair pair(uint32_t i) const { return *reinterpret_cast<const PowPair*>(base + (i + zero)); }   // i even
    __device__ __forceinline__ double at(uint32_t i) const { return base[i + zero]; }
};

// log(x) = hi + tail for the bits ix of a positive normal double (glibc: log_inline)
template <class TAB>
__device__ __forceinline__ double pow_log_inline(uint64_t ix, double& tail, const TAB& T) {
    const uint64_t tmp = ix - 0x3fe6955500000000ull;                 // OFF
    const uint32_t i = (uint32_t)(tmp >> 45) & 127u;
    const int k = (int)((int64_t)tmp >> 52);
    const uint64_t iz = ix - (tmp & (0xfffull << 52));
    const double z = pow_double(iz);
    const double kd = (double)k;
    const PowPair e = T.pair(kPowLogAt + 4u * i);
    const double invc = e.a, logc = e.b, logctail = T.at(kPowLogAt + 4u * i + 2u);
    const PowPair ln2 = T.pair(0), a01 = T.pair(2), a23 = T.pair(4), a45 = T.pair(6), a6 = T.pair(8);
    const double r = __builtin_fma(z, invc, -1.0);
    const double t1 = __builtin_fma(kd, ln2.a, logc);
    const double t2 = t1 + r;
    const double lo1 = __builtin_fma(kd, ln2.b, logctail);
    const double lo2 = t1 - t2 + r;
    const double ar = a01.a * r;                                      // A[0] = -0.5
    const double ar2 = r * ar;
    const double ar3 = r * ar2;
    const double hi = t2 + ar2;
    const double lo3 = __builtin_fma(ar, r, -ar2);
    const double lo4 = t2 - hi + ar2;
    // ar3 * (A1 + r A2 + ar2 (A3 + r A4 + ar2 (A5 + r A6))), its last multiply fused with the sum of the low parts
    const double q = __builtin_fma(ar2, __builtin_fma(r, a6.a, a45.b), __builtin_fma(r, a45.a, a23.b));
    const double p = __builtin_fma(ar2, q, __builtin_fma(r, a23.a, a01.b));
    const double lo = __builtin_fma(ar3, p, lo1 + lo2 + lo3 + lo4);
    const double y = hi + lo;
    tail = hi - y + lo;
    return y;
}

// glibc's exp_inline(x, xtail, sign_bias) on its common path (2^-54 <= |x| < 512): 2^(k/128) from the table, the
// polynomial, scale + scale * tmp.  `special` is set where the routine would leave that path (the caller re-runs those
// lanes through pow_any()); table indices stay in range for every input.
template <class TAB>
__device__ __forceinline__ double pow_exp_common(double x, double xtail, uint64_t sign_bias, const TAB& T, bool& special) {
    const uint32_t abstop = (uint32_t)(pow_bits(x) >> 52) & 0x7ffu;
    special = abstop - 0x3c9u >= 0x408u - 0x3c9u;
    const PowPair c89 = T.pair(8), c1011 = T.pair(10), c1213 = T.pair(12), c1415 = T.pair(14), c16 = T.pair(16);
    const double InvLn2N = c89.b, Shift = c1011.a, NegLn2hiN = c1011.b, NegLn2loN = c1213.a;
    const double C2 = c1213.b, C3 = c1415.a, C4 = c1415.b, C5 = c16.a;
    double kd = __builtin_fma(x, InvLn2N, Shift);                     // InvLn2N * x + Shift, fused
    const uint64_t ki = pow_bits(kd);
    kd -= Shift;
    double r = __builtin_fma(kd, NegLn2loN, __builtin_fma(kd, NegLn2hiN, x));
    r = r + xtail;
    const uint32_t idx = 2u * ((uint32_t)ki & 127u);
    const uint64_t top = (ki + sign_bias) << 45;
    const PowPair e = T.pair(kPowExpAt + idx);
    const double tail = e.a;
    const uint64_t sbits = pow_bits(e.b) + top;
    const double r2 = r * r;
    const double tmp = __builtin_fma(__builtin_fma(r, C5, C4), r2 * r2, __builtin_fma(__builtin_fma(r, C3, C2), r2, tail + r));
    const double scale = pow_double(sbits);
    return __builtin_fma(scale, tmp, scale);
}

// the whole of exp_inline (specialcase() included)
template <class TAB>
__device__ inline double pow_exp_any(double x, double xtail, uint64_t sign_bias, const TAB& T) {
    uint32_t abstop = (uint32_t)(pow_bits(x) >> 52) & 0x7ffu;
    if (abstop - 0x3c9u >= 0x408u - 0x3c9u) {
        if (abstop - 0x3c9u >= 0x80000000u) {                           // |x| < 2^-54 (0 included)
            const double one = 1.0 + x;
            return sign_bias ? -one : one;
        }
        if (abstop >= 0x409u) {                                         // |x| >= 1024: __math_uflow / __math_oflow
            if (pow_bits(x) >> 63) return sign_bias ? -0.0 : 0.0;
            return sign_bias ? -__builtin_inf() : __builtin_inf();
        }
        abstop = 0;                                                     // large |x|: specialcase() below
    }
    const PowPair c89 = T.pair(8), c1011 = T.pair(10), c1213 = T.pair(12), c1415 = T.pair(14), c16 = T.pair(16);
    const double InvLn2N = c89.b, Shift = c1011.a, NegLn2hiN = c1011.b, NegLn2loN = c1213.a;
    const double C2 = c1213.b, C3 = c1415.a, C4 = c1415.b, C5 = c16.a;
    double kd = __builtin_fma(x, InvLn2N, Shift);
    const uint64_t ki = pow_bits(kd);
    kd -= Shift;
    double r = __builtin_fma(kd, NegLn2loN, __builtin_fma(kd, NegLn2hiN, x));
    r = r + xtail;
    const uint32_t idx = 2u * ((uint32_t)ki & 127u);
    const uint64_t top = (ki + sign_bias) << 45;
    const PowPair e = T.pair(kPowExpAt + idx);
    const double tail = e.a;
    uint64_t sbits = pow_bits(e.b) + top;
    const double r2 = r * r;
    const double tmp = __builtin_fma(__builtin_fma(r, C5, C4), r2 * r2, __builtin_fma(__builtin_fma(r, C3, C2), r2, tail + r));
    if (abstop == 0) {                                                  // specialcase(tmp, sbits, ki)
        if ((ki & 0x80000000u) == 0) {                                  // k > 0: the exponent of scale may have overflowed
            sbits -= 1009ull << 52;
            const double scale = pow_double(sbits);
            return 0x1p1009 * __builtin_fma(scale, tmp, scale);
        }
        sbits += 1022ull << 52;                                         // k < 0: the subnormal range, rounded once
        const double scale = pow_double(sbits);
        const double st = scale * tmp;                                  // (not fused in __pow_fma)
        double y = scale + st;
        if (__builtin_fabs(y) < 1.0) {
            const double one = y < 0.0 ? -1.0 : 1.0;
            double lo = scale - y + st;
            const double hi = one + y;
            lo = one - hi + y + lo;
            y = (hi + lo) - one;
            if (y == 0.0) y = pow_double(sbits & 0x8000000000000000ull);
        }
        return 0x1p-1022 * y;
    }
    const double scale = pow_double(sbits);
    return __builtin_fma(scale, tmp, scale);
}

// 0: y is not an integer, 1: odd integer, 2: even integer (iy: a non-zero finite double)
__device__ __forceinline__ int pow_checkint(uint64_t iy) {
    const int e = (int)(iy >> 52 & 0x7ff);
    if (e < 0x3ff) return 0;
    if (e > 0x3ff + 52) return 2;
    if (iy & ((1ull << (0x3ff + 52 - e)) - 1)) return 0;
    if (iy & (1ull << (0x3ff + 52 - e))) return 1;
    return 2;
}
__device__ __forceinline__ bool pow_zeroinfnan(uint64_t i) { return 2 * i - 1 >= 2 * 0x7ff0000000000000ull - 1; }
__device__ __forceinline__ bool pow_signaling(uint64_t i) { return 2 * (i ^ 0x0008000000000000ull) > 2 * 0x7ff8000000000000ull; }

// Every case of glibc's __pow, written with its branches (the debug probe's full sweep and the lanes p3d_pow_fast()
// hands over).  The errno helpers of the C library return: __math_oflow +-inf, __math_uflow +-0, __math_divzero +-inf,
// __math_invalid (x - x) / (x - x).
template <class TAB>
__device__ inline double pow_any(double x, double y, const TAB& T) {
    uint64_t sign_bias = 0;
    uint64_t ix = pow_bits(x);
    const uint64_t iy = pow_bits(y);
    uint32_t topx = (uint32_t)(ix >> 52);
    const uint32_t topy = (uint32_t)(iy >> 52);
    if (topx - 0x001u >= 0x7ffu - 0x001u || (topy & 0x7ffu) - 0x3beu >= 0x43eu - 0x3beu) {
        if (pow_zeroinfnan(iy)) {
            if (2 * iy == 0) return pow_signaling(ix) ? x + y : 1.0;
            if (ix == 0x3ff0000000000000ull) return pow_signaling(iy) ? x + y : 1.0;
            if (2 * ix > 2 * 0x7ff0000000000000ull || 2 * iy > 2 * 0x7ff0000000000000ull) return x + y;
            if (2 * ix == 2 * 0x3ff0000000000000ull) return 1.0;
            if ((2 * ix < 2 * 0x3ff0000000000000ull) == !(iy >> 63)) return 0.0;   // |x| < 1 && y == inf or |x| > 1 && y == -inf
            return y * y;
        }
        if (pow_zeroinfnan(ix)) {
            double x2 = x * x;
            bool neg = false;
            if ((ix >> 63) && pow_checkint(iy) == 1) { x2 = -x2; neg = true; }
            if (2 * ix == 0 && (iy >> 63)) return neg ? -__builtin_inf() : __builtin_inf();
            return (iy >> 63) ? 1.0 / x2 : x2;
        }
        if (ix >> 63) {                                                 // finite x < 0
            const int yint = pow_checkint(iy);
            if (yint == 0) return (x - x) / (x - x);
            if (yint == 1) sign_bias = 0x800ull << 7;
            ix &= 0x7fffffffffffffffull;
            topx &= 0x7ffu;
        }
        if ((topy & 0x7ffu) - 0x3beu >= 0x43eu - 0x3beu) {
            if (ix == 0x3ff0000000000000ull) return 1.0;
            if ((topy & 0x7ffu) < 0x3beu) return ix > 0x3ff0000000000000ull ? 1.0 + y : 1.0 - y;   // |y| < 2^-65
            return (ix > 0x3ff0000000000000ull) == (topy < 0x800u) ? __builtin_inf() : 0.0;
        }
        if (topx == 0) {                                                // subnormal x: normalise
            ix = pow_bits(x * 0x1p52);
            ix &= 0x7fffffffffffffffull;
            ix -= 52ull << 52;
        }
    }
    double lo;
    const double hi = pow_log_inline(ix, lo, T);
    const double ehi = y * hi;
    const double elo = __builtin_fma(y, lo, __builtin_fma(y, hi, -ehi));
    return pow_exp_any(ehi, elo, sign_bias, T);
}

// pow(x, y) as shading calls it: a positive normal base and a normal exponent with |y| in [2^-65, 2^63) run straight-line
// code (the Schlick weight passes 1 - cos_theta_i and 5); zero, negative, subnormal, infinite or NaN bases, other
// exponents and results outside exp_inline's common path sit behind a wave-level branch into pow_any().
template <class TAB>
__device__ __forceinline__ double p3d_pow_fast(double x, double y, const TAB& T) {
    const uint64_t ix = pow_bits(x), iy = pow_bits(y);
    const uint32_t topx = (uint32_t)(ix >> 52), topy = (uint32_t)(iy >> 52);
    const bool args_ok = topx - 0x001u < 0x7ffu - 0x001u && (topy & 0x7ffu) - 0x3beu < 0x43eu - 0x3beu;
    // bypassed lanes compute finite or NaN garbage (the table indices are masked into range)
    double lo;
    const double hi = pow_log_inline(ix, lo, T);
    const double ehi = y * hi;
    const double elo = __builtin_fma(y, lo, __builtin_fma(y, hi, -ehi));
    bool special;
    double r = pow_exp_common(ehi, elo, 0, T, special);
    const bool fine = args_ok && !special;
#ifndef P3D_POW_HOST_CHECK
    if (__ballot(!fine) != 0) {
        asm volatile("");                        // keeps this a branch: the special cases stay off the common path
#else
    {
#endif
        if (!fine) r = pow_any(x, y, T);
    }
    return r;
}

// any arguments (the debug probe)
__device__ __forceinline__ double p3d_pow(double x, double y) { return p3d_pow_fast(x, y, PowTab()); }

// KR with SCHLICK_APPROX, RT/main.cpp:700-701, in g++'s operation order: rI = ((ior_1 - newIor) / (ior_1 + newIor))^2
// in float (pow(x, 2) folded to a float square), 1 - cos_theta_i in float, widened for pow(double, 5.0), (1 - rI) in
// float, widened, multiplied and (double)rI added in double -- no fused multiply-add -- and one rounding to float.
template <class TAB>
__device__ __forceinline__ float p3d_schlick_kr(float ior_1, float newIor, float cos_theta_i, const TAB& T) {
    const float q = (ior_1 - newIor) / (ior_1 + newIor);
    const float rI = q * q;
    const double p = p3d_pow_fast((double)(1.0f - cos_theta_i), 5.0, T);
    return (float)((double)rI + (double)(1.0f - rI) * p);
}

}  // namespace p3d
#endif
