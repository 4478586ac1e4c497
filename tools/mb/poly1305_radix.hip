// tools/mb/poly1305_radix.hip -- microbenchmark behind the radix choice of the ChaCha20-Poly1305 kernels:
// the rate of the Poly1305 step h = (h + m) * r mod 2^130 - 5 with a general (unclamped) multiplier, one dependent chain
// per lane as in the record kernels, for two representations:
//   A  5 x 26-bit limbs, 25 products accumulated in 64 bits (picotls_amd/csrc/chacha/poly1305.h, what the engine uses)
//   B  5 x 32-bit words (130 bits in 4 words + 2 bits), 25 products accumulated column-wise in 96 bits, two folds by 5
// Both chains start from the same values and must end equal mod p (checked on the host). Prints one JSON line.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I picotls_amd/csrc tools/mb/poly1305_radix.hip -o tools/mb/poly1305_radix.bin
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef uint32_t u32;
typedef uint64_t u64;
#include "chacha/poly1305.h"

struct W {
    u32 v[5];  // value = sum v[i] << 32 i, loose: below 2^131
};

__device__ __forceinline__ W w_mul(const W &a, const W &b)
{
    u32 t[10];
    u64 acc = 0;
    u32 hi = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int j = k - i;
            if (j >= 0 && j < 5) {
                const u64 p = (u64)a.v[i] * b.v[j];
                acc += p;
                hi += acc < p;
            }
        }
        t[k] = (u32)acc;
        acc = acc >> 32 | (u64)hi << 32;
        hi = 0;
    }
    t[9] = (u32)acc;
    // low 130 bits + 5 * (the rest), then the same once more for what that left above bit 130
    W r;
    u64 c = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const u32 h = t[k + 4] >> 2 | t[k + 5] << 30, lo = k < 4 ? t[k] : t[4] & 3;
        c += (u64)lo + (u64)h * 5;
        r.v[k] = (u32)c;
        c >>= 32;
    }
    c = (u64)(r.v[4] >> 2) * 5;
    r.v[4] &= 3;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        c += r.v[k];
        r.v[k] = (u32)c;
        c >>= 32;
    }
    return r;
}

__device__ __forceinline__ void w_add_block(W &h, u32 w0, u32 w1, u32 w2, u32 w3)
{
    u64 c = (u64)h.v[0] + w0;
    h.v[0] = (u32)c;
    c = (c >> 32) + h.v[1] + w1;
    h.v[1] = (u32)c;
    c = (c >> 32) + h.v[2] + w2;
    h.v[2] = (u32)c;
    c = (c >> 32) + h.v[3] + w3;
    h.v[3] = (u32)c;
    h.v[4] += (u32)(c >> 32) + 1;
}

// which: 0 = A, 1 = B. Every lane: h = 0; iters times h = (h + m) * r with m = (seed, lane, i, 7) and r = a fixed loose
// element; out[thread] = the five limbs / words.
__global__ __launch_bounds__(256) void chain_kernel(int which, u32 seed, u32 iters, u32 *out)
{
    const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 rw[4] = {0x0a1b2c3du ^ seed, 0x4e5f6071u, 0x8293a4b5u, 0xc6d7e8f9u};
    if (which == 0) {
        Fe r = fe_zero(), h = fe_zero();
        fe_add_block(r, rw[0], rw[1], rw[2], rw[3], 1);
        for (u32 i = 0; i < iters; ++i) {
            fe_add_block(h, seed, tid, i, 7, 1);
            h = fe_mul(h, r);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
            out[5 * tid + k] = h.v[k];
    } else {
        W r = {{rw[0], rw[1], rw[2], rw[3], 1}}, h = {{0, 0, 0, 0, 0}};
        for (u32 i = 0; i < iters; ++i) {
            w_add_block(h, seed, tid, i, 7);
            h = w_mul(h, r);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
            out[5 * tid + k] = h.v[k];
    }
}

#define CHECK(e)                                                                                                       \
    do {                                                                                                               \
        hipError_t e_ = (e);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_));                                                    \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

typedef unsigned __int128 u128;

static void to_p(const u32 *v, int bits, u64 out[3])  // value mod p as (lo, mid, top 2 bits), by schoolbook on the host
{
    // value = sum v[i] << (bits * i), below 2^160: reduce with 2^130 = 5
    u128 lo = 0, hi = 0;  // lo: bits 0..127, hi: the rest
    for (int i = 4; i >= 0; --i) {
        hi = hi << bits | lo >> (128 - bits);
        lo <<= bits;
        const u128 old = lo;
        lo += v[i];
        hi += lo < old;
    }
    for (int pass = 0; pass < 3; ++pass) {  // fold bits >= 130
        const u128 top = hi >> 2;
        hi &= 3;
        const u128 old = lo;
        lo += top * 5;
        hi += lo < old;
    }
    // canonical: subtract p once if >= p
    const u128 old = lo;
    u128 l5 = lo + 5, h5 = hi + (l5 < old);
    if (h5 >> 2) {
        lo = l5;
        hi = h5 & 3;
    }
    out[0] = (u64)lo, out[1] = (u64)(lo >> 64), out[2] = (u64)hi;
}

int main(int argc, char **argv)
{
    const u32 iters = argc > 1 ? (u32)atoi(argv[1]) : 20000, reps = 7;
    int dev = 0, ncu = 0, mhz = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    CHECK(hipDeviceGetAttribute(&mhz, hipDeviceAttributeClockRate, dev));
    mhz /= 1000;
    const unsigned grid = (unsigned)ncu * 4, threads = grid * 256;
    u32 *out[2];
    CHECK(hipMalloc(&out[0], threads * 20));
    CHECK(hipMalloc(&out[1], threads * 20));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    double best[2] = {1e30, 1e30}, sum[2] = {0, 0};
    for (u32 rep = 0; rep < reps + 1; ++rep) {  // arms interleaved; the first round is the warm-up
        for (int which = 0; which < 2; ++which) {
            CHECK(hipEventRecord(e0, 0));
            chain_kernel<<<grid, 256>>>(which, 12345, iters, out[which]);
            CHECK(hipGetLastError());
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep != 0) {
                sum[which] += ms;
                if (ms < best[which])
                    best[which] = ms;
            }
        }
    }
    std::vector<u32> a(threads * 5), b(threads * 5);
    CHECK(hipMemcpy(a.data(), out[0], threads * 20, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), out[1], threads * 20, hipMemcpyDeviceToHost));
    unsigned differ = 0;
    for (unsigned t = 0; t < threads; ++t) {
        u64 pa[3], pb[3];
        to_p(&a[5 * t], 26, pa);
        to_p(&b[5 * t], 32, pb);
        differ += pa[0] != pb[0] || pa[1] != pb[1] || pa[2] != pb[2];
    }
    const double steps = (double)threads * iters;
    printf("{\"bench\": \"poly1305_radix\", \"cus\": %d, \"clock_mhz_attr\": %d, \"threads\": %u, \"iters\": %u, "
           "\"limbs26_ms_mean\": %.3f, \"limbs26_ms_best\": %.3f, \"limbs26_gsteps_per_s\": %.1f, "
           "\"words32_ms_mean\": %.3f, \"words32_ms_best\": %.3f, \"words32_gsteps_per_s\": %.1f, \"chains_differ\": %u}\n",
           ncu, mhz, threads, iters, sum[0] / reps, best[0], steps / (sum[0] / reps) / 1e6, sum[1] / reps, best[1],
           steps / (sum[1] / reps) / 1e6, differ);
    return differ == 0 ? 0 : 1;
}
