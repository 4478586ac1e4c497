// picotls_amd/csrc/chacha/chacha20.h -- the ChaCha20 block function (RFC 8439 §2.3), the keyset entry of the
// ChaCha20-Poly1305 engine and its byte-granular loads and stores.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included after engine/common.h).
#ifndef PTLS_MI355X_CHACHA_CHACHA20_H
#define PTLS_MI355X_CHACHA_CHACHA20_H

// one keyset entry in HBM (64 bytes, 16-byte aligned): key and static IV as little-endian words
struct ChaChaKey {
    u32 key[8];
    u32 iv[3];
    u32 pad[5];
};
static_assert(sizeof(ChaChaKey) == 64, "ChaChaKey layout");

#define CHACHA_QR(a, b, c, d)                                                                                          \
    a += b, d ^= a, d = __builtin_rotateleft32(d, 16);                                                                 \
    c += d, b ^= c, b = __builtin_rotateleft32(b, 12);                                                                 \
    a += b, d ^= a, d = __builtin_rotateleft32(d, 8);                                                                  \
    c += d, b ^= c, b = __builtin_rotateleft32(b, 7)

// x = the 64-byte keystream block of (key, counter, nonce), as 16 little-endian words
__device__ __forceinline__ void chacha20_block(const u32 key[8], u32 counter, u32 n0, u32 n1, u32 n2, u32 x[16])
{
    const u32 c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
    x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        x[4 + i] = key[i];
    x[12] = counter, x[13] = n0, x[14] = n1, x[15] = n2;
#pragma unroll 2
    for (int i = 0; i < 10; ++i) {
        CHACHA_QR(x[0], x[4], x[8], x[12]);
        CHACHA_QR(x[1], x[5], x[9], x[13]);
        CHACHA_QR(x[2], x[6], x[10], x[14]);
        CHACHA_QR(x[3], x[7], x[11], x[15]);
        CHACHA_QR(x[0], x[5], x[10], x[15]);
        CHACHA_QR(x[1], x[6], x[11], x[12]);
        CHACHA_QR(x[2], x[7], x[8], x[13]);
        CHACHA_QR(x[3], x[4], x[9], x[14]);
    }
    x[0] += c0, x[1] += c1, x[2] += c2, x[3] += c3;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        x[4 + i] += key[i];
    x[12] += counter, x[13] += n0, x[14] += n1, x[15] += n2;
}

// the first n (0..16) bytes at p as four little-endian words, the rest zero; touches nothing beyond p + n. A whole
// block is one 16-byte access at any byte offset (unaligned access mode), a partial one goes byte by byte.
__device__ __forceinline__ u32x4 load_upto16(const uint8_t *p, u32 n)
{
    if (n >= 16)
        return *(const u32x4_u *)p;
    u32x4 w = {0, 0, 0, 0};
#pragma unroll
    for (u32 i = 0; i < 15; ++i) {
        if (i < n) {
            const u32 b = (u32)p[i] << (8 * (i & 3));
            if (i < 4)
                w.x |= b;
            else if (i < 8)
                w.y |= b;
            else if (i < 12)
                w.z |= b;
            else
                w.w |= b;
        }
    }
    return w;
}

__device__ __forceinline__ void store_upto16(uint8_t *p, u32x4 w, u32 n)
{
    if (n >= 16) {
        *(u32x4_u *)p = w;
        return;
    }
#pragma unroll
    for (u32 i = 0; i < 15; ++i) {
        if (i < n) {
            const u32 v = i < 4 ? w.x : i < 8 ? w.y : i < 12 ? w.z : w.w;
            p[i] = (uint8_t)(v >> (8 * (i & 3)));
        }
    }
}

// w with the bytes from n (0..16) on cleared
__device__ __forceinline__ u32x4 keep_bytes(u32x4 w, u32 n)
{
    u32x4 o;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 have = n > 4 * k ? min(n - 4 * k, 4u) : 0;  // bytes of word k that stay
        const u32 m = have >= 4 ? 0xffffffffu : (1u << (8 * have)) - 1;
        o[k] = w[k] & m;
    }
    return o;
}

#endif  // PTLS_MI355X_CHACHA_CHACHA20_H
