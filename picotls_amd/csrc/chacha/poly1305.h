// picotls_amd/csrc/chacha/poly1305.h -- Poly1305 (RFC 8439 §2.5) on 5 x 26-bit limbs, for the ChaCha20-Poly1305 kernels.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included after engine/common.h).
//
// An element of GF(2^130 - 5) is five u32 limbs of 26 bits, value = sum v[i] << 26 i. Between operations the limbs are
// "loose": below 2^26 plus a small excess (what one carry pass leaves), so sums of up to 16 elements plus a message
// block still fit 32 bits and the 25 products of a multiplication, 5 r folded in, fit 64 bits (v_mad_u64_u32).
// Unlike the textbook form the multiplier need not be a clamped r: the kernels multiply by powers of r, which are loose
// elements like any other. tools/mb/poly1305_radix.hip times this radix against 32-bit limbs.
#ifndef PTLS_MI355X_CHACHA_POLY1305_H
#define PTLS_MI355X_CHACHA_POLY1305_H

#define P26 0x3ffffffu

struct Fe {
    u32 v[5];
};

__device__ __forceinline__ Fe fe_zero()
{
    Fe z = {{0, 0, 0, 0, 0}};
    return z;
}

__device__ __forceinline__ Fe fe_one()
{
    Fe z = {{1, 0, 0, 0, 0}};
    return z;
}

__device__ __forceinline__ Fe fe_select(bool c, const Fe &a, const Fe &b)
{
    Fe o;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        o.v[i] = c ? a.v[i] : b.v[i];
    return o;
}

// h += the 16-byte block (w0..w3 little endian) + hibit << 128 (hibit = 1 for every block of the AEAD's padded stream)
__device__ __forceinline__ void fe_add_block(Fe &h, u32 w0, u32 w1, u32 w2, u32 w3, u32 hibit)
{
    h.v[0] += w0 & P26;
    h.v[1] += __builtin_amdgcn_alignbit(w1, w0, 26) & P26;
    h.v[2] += __builtin_amdgcn_alignbit(w2, w1, 20) & P26;
    h.v[3] += __builtin_amdgcn_alignbit(w3, w2, 14) & P26;
    h.v[4] += (w3 >> 8) | (hibit << 24);
}

// a * b mod 2^130 - 5, loose in (limbs below 2^31 for a, 2^27 for b), loose out
__device__ __forceinline__ Fe fe_mul(const Fe &a, const Fe &b)
{
    const u32 s1 = b.v[1] * 5, s2 = b.v[2] * 5, s3 = b.v[3] * 5, s4 = b.v[4] * 5;
    u64 d0 = (u64)a.v[0] * b.v[0] + (u64)a.v[1] * s4 + (u64)a.v[2] * s3 + (u64)a.v[3] * s2 + (u64)a.v[4] * s1;
    u64 d1 = (u64)a.v[0] * b.v[1] + (u64)a.v[1] * b.v[0] + (u64)a.v[2] * s4 + (u64)a.v[3] * s3 + (u64)a.v[4] * s2;
    u64 d2 = (u64)a.v[0] * b.v[2] + (u64)a.v[1] * b.v[1] + (u64)a.v[2] * b.v[0] + (u64)a.v[3] * s4 + (u64)a.v[4] * s3;
    u64 d3 = (u64)a.v[0] * b.v[3] + (u64)a.v[1] * b.v[2] + (u64)a.v[2] * b.v[1] + (u64)a.v[3] * b.v[0] + (u64)a.v[4] * s4;
    u64 d4 = (u64)a.v[0] * b.v[4] + (u64)a.v[1] * b.v[3] + (u64)a.v[2] * b.v[2] + (u64)a.v[3] * b.v[1] + (u64)a.v[4] * b.v[0];
    Fe o;
    d1 += d0 >> 26, o.v[0] = (u32)d0 & P26;
    d2 += d1 >> 26, o.v[1] = (u32)d1 & P26;
    d3 += d2 >> 26, o.v[2] = (u32)d2 & P26;
    d4 += d3 >> 26, o.v[3] = (u32)d3 & P26;
    o.v[4] = (u32)d4 & P26;
    const u64 c = (d4 >> 26) * 5 + o.v[0];  // d4 >> 26 is below 2^38
    o.v[0] = (u32)c & P26;
    o.v[1] += (u32)(c >> 26);
    return o;
}

// one full carry pass, the carry out of limb 4 wrapping to limb 0 as 5 (2^130 = 5)
__device__ __forceinline__ void fe_carry(Fe &h)
{
    u32 c;
    c = h.v[0] >> 26, h.v[0] &= P26, h.v[1] += c;
    c = h.v[1] >> 26, h.v[1] &= P26, h.v[2] += c;
    c = h.v[2] >> 26, h.v[2] &= P26, h.v[3] += c;
    c = h.v[3] >> 26, h.v[3] &= P26, h.v[4] += c;
    c = h.v[4] >> 26, h.v[4] &= P26, h.v[0] += c * 5;
}

// tag = ((h mod 2^130 - 5) + s) mod 2^128: reduce once, freeze, add s (RFC 8439 §2.5.1). h loose (limbs below 2^31).
__device__ __forceinline__ void fe_tag(Fe h, const u32 s[4], u32 tag[4])
{
    // three passes leave every limb below 2^26: the first brings the value under 2^130 + 5 * 2^5, the wrap of the second
    // can only meet a value whose low limbs are nearly empty, and the third ripples what that wrap added to limb 0
    fe_carry(h);
    fe_carry(h);
    fe_carry(h);
    // g = h + 5 - 2^130: not negative exactly when h >= p
    Fe g;
    u32 c = 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        g.v[i] = h.v[i] + c;
        c = g.v[i] >> 26;
        g.v[i] &= P26;
    }
    h = fe_select(c != 0, g, h);
    const u32 w0 = h.v[0] | h.v[1] << 26, w1 = h.v[1] >> 6 | h.v[2] << 20, w2 = h.v[2] >> 12 | h.v[3] << 14,
              w3 = h.v[3] >> 18 | h.v[4] << 8;
    u64 f = (u64)w0 + s[0];
    tag[0] = (u32)f;
    f = (u64)w1 + s[1] + (f >> 32);
    tag[1] = (u32)f;
    f = (u64)w2 + s[2] + (f >> 32);
    tag[2] = (u32)f;
    f = (u64)w3 + s[3] + (f >> 32);
    tag[3] = (u32)f;
}

// h mod 2^130 - 5, every limb below 2^26 (the reduction fe_tag makes before it adds s). h loose (limbs below 2^31).
__device__ __forceinline__ Fe fe_reduced(Fe h)
{
    fe_carry(h);
    fe_carry(h);
    fe_carry(h);
    Fe g;
    u32 c = 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        g.v[i] = h.v[i] + c;
        c = g.v[i] >> 26;
        g.v[i] &= P26;
    }
    return fe_select(c != 0, g, h);
}

// r^e by square and multiply from the low bit of e up: one squaring per bit up to e's highest set bit, and one
// multiplication per bit whose result is selected, not branched on, as the kernels select rE. The trip count follows e,
// which is a block count (public). r loose, loose out; e = 0 gives 1.
__device__ __forceinline__ Fe fe_pow(const Fe &r, u64 e)
{
    Fe acc = fe_one(), sq = r;
    for (; e != 0; e >>= 1) {
        acc = fe_select((e & 1) != 0, fe_mul(acc, sq), acc);
        sq = fe_mul(sq, sq);
    }
    return acc;
}

// r of a one-time key: the first 16 bytes clamped (RFC 8439 §2.5: r &= 0x0ffffffc0ffffffc0ffffffc0fffffff)
__device__ __forceinline__ Fe fe_clamped_r(u32 k0, u32 k1, u32 k2, u32 k3)
{
    Fe r = fe_zero();
    fe_add_block(r, k0 & 0x0fffffffu, k1 & 0x0ffffffcu, k2 & 0x0ffffffcu, k3 & 0x0ffffffcu, 0);
    return r;
}

#endif  // PTLS_MI355X_CHACHA_POLY1305_H
