// picotls_amd/csrc/chacha/kernels.h -- ChaCha20-Poly1305 (RFC 8439 §2.8) seal / open of a batch of records, the QUIC
// header-protection masks of that suite and the Poly1305 test hook.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included after chacha20.h and poly1305.h).
//
// Shape. One persistent launch per batch; a workgroup claims runs of records from an atomic counter, its
// waves take 64 / G records of the run at a time and a group of G lanes owns one record. Lane j of the group runs the
// ChaCha20 blocks with counter j, j + G, ...: counter 0 (lane 0's first block) is the one-time Poly1305 key, counter
// v >= 1 the keystream of the 64 text bytes from 64 (v - 1), so in each step the group touches G x 64 contiguous bytes.
// No tables: the cipher is add, xor and rotate on registers, nothing is addressed by secret data, and the LDS holds
// only the workgroup's current claim and the four partial sums of its width sample.
//
// Poly1305 across the group. The tag is sum m_i r^(N - i) + s over the 16-byte blocks of pad16(AAD) || pad16(text) ||
// LE64(aadlen) || LE64(textlen). A lane folds the four Poly1305 blocks of each of its 64-byte blocks into its own
// accumulator: (h + m) r three times, then (h + m) r^(4G - 3), which carries it over the other lanes' blocks to its next
// one. The lane that owns text block 0 (lane 1) starts its chain with the AAD blocks. After its last block a lane
// multiplies by r^E, E = the number of text blocks from that block to the end (1 .. 4G - 3), which aligns every lane's
// partial with the position of the length block; the partials are added across the group, the length block is added
// and one multiplication by r, one reduction mod 2^130 - 5 and the addition of s finish the tag. r^(4G - 3) and r^E come
// from log2(4G) - 1 squarings of r per record.
//
// Framing. FRAME 0: ciphertext || tag, the AAD from its own arena. FRAME 1: TLS 1.3 wire records. FRAME 2: QUIC packets
// (RFC 9001 §5.3-5.4): the header in front of the text is the AAD; seal also runs the header-protection
// block on the sample out of text block 0 and masks the header, open takes packet number and lengths from the
// results of chacha_quic_unmask_kernel, launched ahead of it, and writes the unprotected header.
#ifndef PTLS_MI355X_CHACHA_KERNELS_H
#define PTLS_MI355X_CHACHA_KERNELS_H

#define CHACHA_WG 256            // threads per workgroup
#define CHACHA_G_NARROW 4        // lanes per record: QUIC-sized records (19 blocks at 1200 B: 20 with the key block, 5 a lane)
#define CHACHA_G_WIDE 16         // ... and long ones (16 KiB: 257 blocks, 16 or 17 a lane)
#define CHACHA_WIDE_MIN 4096u    // a workgroup takes the wide groups when its sample of the batch averages this length
#define CHACHA_TLS_MAX_PLAIN 16384u

struct ChaChaArgs {
    const ChaChaKey *keys;
    u32 nkeys;
    u32 force_g;  // 0: each workgroup chooses from a sample of the descriptors
    const ptls_mi355x_record_t *recs;
    u64 nrecs;
    const uint8_t *in, *aad;
    uint8_t *out, *ok;
    // [0] the next unclaimed record, [1] workgroups that have finished; both zero between launches (the last workgroup
    // to finish clears them). Null: rounds of records are dealt to the workgroups by index instead.
    unsigned long long *claim;
    u32 *done_flag;  // per-record path: one completion word per workgroup (publish_done)
    u32 done_token;
    // QUIC packets (FRAME 2): the header-protection keys, and the pre-pass's results that the open reads and completes
    u32 hp_nkeys;
    const ChaChaKey *hp_keys;
    ptls_mi355x_quic_result_t *results;
};

// launches per group width (ptls_mi355x_chacha_debug_counters): [0] narrow, [1] wide, counted by workgroup 0
__device__ unsigned long long g_chacha_launches[2];

__device__ __forceinline__ u32 sub_clamp16(u32 n, u32 off) { return n > off ? min(n - off, 16u) : 0u; }

// QUIC seal (RFC 9001 §5.4.1): the mask of `sample` under the packet's header-protection key (the block of
// chacha_hp_kernel) onto the header at out + out_off, which holds the cleartext header already: the first byte takes
// mask[0] & 0x1f (short header) or & 0x0f (long), packet-number byte i takes mask[1 + i].
__device__ __forceinline__ void quic_protect_header(const ChaChaArgs &a, const ptls_mi355x_record_t &r, u32 first, u32 pn_len,
                                                    u32x4 sample)
{
    const ChaChaKey *hk = a.hp_keys + r.key_idx;
    const u32x4 k0 = *(const u32x4 *)&hk->key[0], k1 = *(const u32x4 *)&hk->key[4];
    const u32 key[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    u32 x[16];
    chacha20_block(key, sample.x, sample.y, sample.z, sample.w, x);
    const uint8_t *pin = a.in + r.in_off + r.aad_len - pn_len;
    uint8_t *hout = a.out + r.out_off, *pout = hout + r.aad_len - pn_len;
    const u32 m14 = quic_m14(x[0], x[1]);
    hout[0] = (uint8_t)(first ^ (x[0] & quic_first_mask(first)));
#pragma unroll
    for (u32 i = 0; i < 4; ++i) {
        if (i < pn_len)
            pout[i] = (uint8_t)(pin[i] ^ (m14 >> (8 * i)));
    }
}

template <int G, bool OPEN, int FRAME>
__device__ __forceinline__ void chacha_record(const ChaChaArgs &a, u64 idx, u32 j)
{
    static_assert(G >= 2 && G <= 64 && (G & (G - 1)) == 0, "group width");
    constexpr u32 STRIDE_E = 4 * G - 3;          // exponent that carries a lane from its block's end to its next block
    constexpr int NBITS = __builtin_ctz(4 * G);  // bits of the exponents 1 .. 4G - 3
    const bool valid = idx < a.nrecs;
    ptls_mi355x_record_t r = {};
    if (valid)
        r = a.recs[idx];
    // QUIC packets: the packet-number length, the first byte in the clear and the full packet number (seal: r.seq as
    // given; open: what the pre-pass reconstructed, with the payload length and its verdict, in results[idx])
    [[maybe_unused]] u32 pn_len = 0, first = 0, quic_len = 0;
    [[maybe_unused]] bool quic_good = false;
    if constexpr (FRAME == 2) {
        if constexpr (OPEN) {
            u32x4 q = {0, 0, 0, QUIC_RESULT_REJECTED_W};
            if (valid)
                q = *(const u32x4_u *)(a.results + idx);
            r.seq = quic_result_pn(q), quic_len = quic_result_payload_len(q), pn_len = quic_result_pn_len(q), first = quic_result_first(q);
            quic_good = valid && quic_result_status(q) == PTLS_MI355X_QUIC_OK;
        } else {
            quic_good = quic_seal_admits(r, a.nkeys, a.hp_nkeys);  // (a lane without a packet: r is zero, which this refuses)
            if (quic_good)
                first = a.in[r.in_off];
            pn_len = quic_pn_len(first), quic_len = r.len;
            quic_good = quic_good && quic_seal_admits_pn(r, pn_len);
        }
    }
    const u32 A = FRAME == 1 ? (u32)TLS_HEADER_SIZE : FRAME == 2 ? r.aad_len + (OPEN ? pn_len : 0u) : PTLS_MI355X_RECORD_AAD_LEN(&r);
    // text bytes (TLS seal: the payload and the inner content type)
    const u32 T = FRAME == 2 ? quic_len : r.len + (FRAME == 1 && !OPEN ? 1u : 0u);
    // a descriptor beyond the limits is rejected: nothing is written for it and open reports ok = 0
    const bool good = FRAME == 2 ? quic_good && r.key_idx < a.nkeys
                                 : valid && r.len <= PTLS_MI355X_MAX_RECORD_LEN && A <= PTLS_MI355X_MAX_AAD_LEN && r.key_idx < a.nkeys &&
                                       (FRAME == 0 || OPEN || r.len <= CHACHA_TLS_MAX_PLAIN) && (FRAME != 0 || A == 0 || a.aad != nullptr);
    const ChaChaKey *ke = a.keys + (good ? r.key_idx : 0);
    u32 key[8];
    {
        const u32x4 k0 = *(const u32x4 *)&ke->key[0], k1 = *(const u32x4 *)&ke->key[4];
        key[0] = k0.x, key[1] = k0.y, key[2] = k0.z, key[3] = k0.w;
        key[4] = k1.x, key[5] = k1.y, key[6] = k1.z, key[7] = k1.w;
    }
    // nonce = static IV ^ (0^32 || BE64(seq))
    const u32 n0 = ke->iv[0], n1 = ke->iv[1] ^ bswap32((u32)(r.seq >> 32)), n2 = ke->iv[2] ^ bswap32((u32)r.seq);
    const uint8_t *src = a.in + r.in_off + (FRAME == 2 ? A : FRAME && OPEN ? TLS_HEADER_SIZE : 0);
    uint8_t *dst = a.out + r.out_off + (FRAME == 2 ? A : FRAME && !OPEN ? TLS_HEADER_SIZE : 0);
    const u32 Cb = (T + 63) >> 6, C = (T + 15) >> 4;  // 64-byte blocks, 16-byte blocks of the text

    // the lane's first block: counter j (lane 0: the Poly1305 key block, whose r and s go to the whole group)
    u32 x[16];
    chacha20_block(key, j, n0, n1, n2, x);
    u32 otk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        otk[i] = (u32)__shfl((int)x[i], 0, G);
    const Fe r1 = fe_clamped_r(otk[0], otk[1], otk[2], otk[3]);

    // the lane's last text block and the exponent E that aligns its partial
    const u32 b0 = j == 0 ? (u32)G - 1 : j - 1;
    u32 E = 0;
    if (b0 < Cb) {
        const u32 blast = b0 + ((Cb - 1 - b0) & ~((u32)G - 1));
        const u32 nblast = (min(64u, T - 64 * blast) + 15) >> 4;
        E = C - (4 * blast + nblast - 1);
    }
    Fe rE = fe_select((E & 1) != 0, r1, fe_one()), rS = r1, sq = r1;
#pragma unroll
    for (int bit = 1; bit < NBITS; ++bit) {
        sq = fe_mul(sq, sq);
        rE = fe_select(((E >> bit) & 1) != 0, fe_mul(rE, sq), rE);
        if ((STRIDE_E >> bit) & 1)
            rS = fe_mul(rS, sq);
    }

    Fe h = fe_zero();
    [[maybe_unused]] u32x4 sample = {0, 0, 0, 0};  // QUIC seal, lane 1: the header-protection sample out of text block 0
    // one 64-byte block b of the text, keystream in x: crypt it, then fold its 16-byte blocks into h (FIRST: the call
    // for the lane's first block, the only one that can be text block 0)
    auto text_block = [&](u32 b, auto FIRST) {
        const u32 o = 64 * b, nT = min(64u, T - o);
        const u32 nS = FRAME == 1 && !OPEN ? (r.len > o ? min(64u, r.len - o) : 0u) : nT;  // bytes the input holds
        u32x4 c[4];
        if (nT == 64 && nS == 64) {  // a whole block: four 16-byte accesses, nothing to clamp or mask
#pragma unroll
            for (u32 w = 0; w < 4; ++w) {
                const u32x4 p = *(const u32x4_u *)(src + o + 16 * w);
                const u32x4 ks = {x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]};
                const u32x4 q = p ^ ks;
                *(u32x4_u *)(dst + o + 16 * w) = q;
                c[w] = OPEN ? p : q;
            }
        } else
#pragma unroll
        for (u32 w = 0; w < 4; ++w) {
            const u32 ns = sub_clamp16(nS, 16 * w), nt = sub_clamp16(nT, 16 * w);
            u32x4 p = load_upto16(src + o + 16 * w, ns);
            if (FRAME == 1 && !OPEN && r.len - o - 16 * w < 16) {  // the inner content type follows the payload
                const u32 at = r.len - o - 16 * w, t = (u32)(r.flags & 0xff) << (8 * (at & 3));
#pragma unroll
                for (u32 k = 0; k < 4; ++k)
                    p[k] |= (at >> 2) == k ? t : 0u;
            }
            const u32x4 ks = {x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]};
            const u32x4 q = p ^ ks;
            store_upto16(dst + o + 16 * w, q, nt);
            c[w] = OPEN ? p : keep_bytes(q, nt);  // the ciphertext, zero from its end
        }
        if constexpr (FRAME == 2 && !OPEN && decltype(FIRST)::value) {
            // the 16 ciphertext bytes from 4 - pn_len (used when they all exist: T >= 20 - pn_len)
            const u32 s = 4 - pn_len;
            sample.x = __builtin_amdgcn_alignbyte(c[0].y, c[0].x, s), sample.y = __builtin_amdgcn_alignbyte(c[0].z, c[0].y, s);
            sample.z = __builtin_amdgcn_alignbyte(c[0].w, c[0].z, s), sample.w = __builtin_amdgcn_alignbyte(c[1].x, c[0].w, s);
        }
        const u32 nb = (nT + 15) >> 4;
        if (nb == 4 && b + G < Cb) {
            fe_add_block(h, c[0].x, c[0].y, c[0].z, c[0].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[1].x, c[1].y, c[1].z, c[1].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[2].x, c[2].y, c[2].z, c[2].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[3].x, c[3].y, c[3].z, c[3].w, 1), h = fe_mul(h, rS);
        } else {  // the lane's last block (the only one that may be short)
#pragma unroll
            for (u32 t = 0; t < 4; ++t) {
                if (t < nb) {
                    fe_add_block(h, c[t].x, c[t].y, c[t].z, c[t].w, 1);
                    h = fe_mul(h, fe_select(t + 1 < nb, r1, rE));
                }
            }
        }
    };

    if (good) {
        if (j == 1) {  // the owner of text block 0 starts with the AAD
            if constexpr (FRAME == 2) {
                // the header, 16 bytes at a time: the AAD is the header in the clear, which is also what open writes
                // out; seal copies it out as it is and masks its first byte and packet number once the sample exists
                const uint8_t *hin = a.in + r.in_off;
                uint8_t *hout = a.out + r.out_off;
                for (u32 off = 0; off < A; off += 16) {
                    // The text follows the header in both arenas, so where 16 bytes from here still lie inside header
                    // and text the header's last block is one access each way instead of a byte loop: the text bytes
                    // it carries go out as they came in, into the start of text block 0, which this lane writes (or,
                    // in place, reads: the same bytes) after this.
                    const u32 n = min(16u, A - off);
                    const bool whole = off + 16 <= A + T;
                    u32x4 w = whole ? *(const u32x4_u *)(hin + off) : load_upto16(hin + off, n);
                    if (OPEN) {
                        if (off == 0)
                            w.x = (w.x & ~0xffu) | first;
                        if (off + 16 > r.aad_len) {  // packet-number bytes in this block (they may straddle two)
#pragma unroll
                            for (u32 i = 0; i < 4; ++i) {
                                const u32 at = r.aad_len + i - off;  // (wraps for a byte of an earlier block)
                                if (i < pn_len && at < 16) {
                                    const u32 sh = 8 * (at & 3), v = ((u32)r.seq >> (8 * (pn_len - 1 - i))) & 0xff;
#pragma unroll
                                    for (u32 k = 0; k < 4; ++k)
                                        w[k] = (at >> 2) == k ? (w[k] & ~(0xffu << sh)) | v << sh : w[k];
                                }
                            }
                        }
                    }
                    if (whole)
                        *(u32x4_u *)(hout + off) = w, w = keep_bytes(w, n);
                    else
                        store_upto16(hout + off, w, n);
                    fe_add_block(h, w.x, w.y, w.z, w.w, 1), h = fe_mul(h, r1);
                }
            } else if (FRAME) {
                u32 w0, w1;
                if (OPEN) {  // the header as received
                    const uint8_t *hp = a.in + r.in_off;
                    w0 = (u32)hp[0] | (u32)hp[1] << 8 | (u32)hp[2] << 16 | (u32)hp[3] << 24, w1 = hp[4];
                } else {  // {23, 3, 3, BE16(len + 17)}
                    const u32 wire = r.len + 17;
                    uint8_t *hp = a.out + r.out_off;
                    w0 = 23u | 3u << 8 | 3u << 16 | (wire >> 8) << 24, w1 = wire & 0xff;
                    hp[0] = 23, hp[1] = 3, hp[2] = 3, hp[3] = (uint8_t)(wire >> 8), hp[4] = (uint8_t)wire;
                }
                fe_add_block(h, w0, w1, 0, 0, 1), h = fe_mul(h, r1);
            } else {
                const uint8_t *ap = a.aad + r.aad_off;
                for (u32 off = 0; off < A; off += 16) {
                    const u32x4 w = load_upto16(ap + off, min(16u, A - off));
                    fe_add_block(h, w.x, w.y, w.z, w.w, 1), h = fe_mul(h, r1);
                }
            }
        }
        if (j >= 1 && j - 1 < Cb)
            text_block(j - 1, std::true_type{});
        if constexpr (FRAME == 2 && !OPEN) {
            // The sample lies in text block 0, which this lane holds: the one block under the header-protection key
            // here, before the lane's other blocks. (No lane has a block to spare at 1200 bytes and four lanes, 20
            // blocks, so the owner of the ciphertext takes it and nothing crosses lanes.)
            if (j == 1 && T + pn_len >= 20)
                quic_protect_header(a, r, first, pn_len, sample);
        }
        for (u32 v = j + G; v <= Cb; v += G) {
            chacha20_block(key, v, n0, n1, n2, x);
            text_block(v - 1, std::false_type{});
        }
    }

    // every lane of the wave is here: the partials of the group, summed into all its lanes
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int m = 1; m < G; m <<= 1)
            h.v[i] += (u32)__shfl_xor((int)h.v[i], m, G);
    }
    [[maybe_unused]] u32x4 qtag = {0, 0, 0, 0};  // QUIC seal: the tag, for a sample that reaches into it
    if (good && j == 0) {
        fe_add_block(h, A, 0, T, 0, 1);  // LE64(aadlen) || LE64(textlen)
        h = fe_mul(h, r1);
        u32 tag[4];
        fe_tag(h, &otk[4], tag);
        if (OPEN) {
            // all 16 bytes compared, no early exit
            const u32x4 got = *(const u32x4_u *)(src + T);
            const u32 diff = (got.x ^ tag[0]) | (got.y ^ tag[1]) | (got.z ^ tag[2]) | (got.w ^ tag[3]);
            a.ok[idx] = diff == 0;
            if constexpr (FRAME == 2)  // (the other fields stay as the pre-pass wrote them)
                ((uint8_t *)(a.results + idx))[offsetof(ptls_mi355x_quic_result_t, status)] =
                    diff == 0 ? PTLS_MI355X_QUIC_OK : PTLS_MI355X_QUIC_BAD_MAC;
        } else {
            const u32x4 t = {tag[0], tag[1], tag[2], tag[3]};
            *(u32x4_u *)(dst + T) = t;
            if constexpr (FRAME == 2)
                qtag = t;
        }
    } else if (OPEN && valid && j == 0) {
        a.ok[idx] = 0;  // (a QUIC packet the pre-pass did not pass keeps the status it gave)
    }
    if constexpr (FRAME == 2 && !OPEN) {
        // The rare packet of under 20 - pn_len payload bytes: its sample ends in the tag. Lane 1, which wrote the header
        // and the ciphertext, reads its own (at most 18) ciphertext bytes back, takes the tag from lane 0 and finishes
        // the header: every byte involved is stored by the lane that reads it, and the common arm above keeps nothing
        // in registers for this one.
        const bool late = good && T + pn_len < 20;
        if (__any(late)) {  // (the same in every lane of the wave)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                qtag[k] = (u32)__shfl((int)qtag[k], 0, G);
            if (late && j == 1) {
                const u32x4 c = load_upto16(dst, min(T, 16u));
                const u32 c4 = (T > 16 ? (u32)dst[16] : 0u) | (T > 17 ? (u32)dst[17] << 8 : 0u);
                const u32 s = 4 - pn_len, nc = T - s;  // nc (0 .. 15) ciphertext bytes from s, then the tag
                u64 lo = (u64)__builtin_amdgcn_alignbyte(c.y, c.x, s) | (u64)__builtin_amdgcn_alignbyte(c.z, c.y, s) << 32;
                u64 hi = (u64)__builtin_amdgcn_alignbyte(c.w, c.z, s) | (u64)__builtin_amdgcn_alignbyte(c4, c.w, s) << 32;
                u64 tlo = (u64)qtag.x | (u64)qtag.y << 32, thi = (u64)qtag.z | (u64)qtag.w << 32;
                if (nc >= 8)
                    thi = tlo, tlo = 0;
                if ((nc & 7) != 0) {
                    thi = thi << (8 * (nc & 7)) | tlo >> (64 - 8 * (nc & 7));
                    tlo <<= 8 * (nc & 7);
                }
                lo |= tlo, hi |= thi;
                const u32x4 smp = {(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
                quic_protect_header(a, r, first, pn_len, smp);
            }
        }
    }
}

// The workgroup's share of the batch. One claim is a run of consecutive records, CHACHA_CLAIMS_PER_WG claims a workgroup
// on average: a claim is one atomic on one address for the whole device, which the memory side serves at some 28 ns
// each (a wave claiming its own 64 / G records made 65,536 claims a launch of 2^20 QUIC packets and spent most of the
// launch queueing for them), so a workgroup claims for its four waves at once and in runs of several rounds. The waves
// of a workgroup take the records of a claim round by round, 64 / G each.
#define CHACHA_CLAIMS_PER_WG 8
template <int G, bool OPEN, int FRAME>
__device__ __forceinline__ void chacha_records(const ChaChaArgs &a, unsigned long long *s_base)
{
    constexpr u32 PER_WAVE = 64 / G, PER_ROUND = CHACHA_WG / G;
    const u32 lane = threadIdx.x & 63, j = lane % G, grp = lane / G, wave = threadIdx.x / 64;
    const u64 rounds = a.nrecs / ((u64)gridDim.x * CHACHA_CLAIMS_PER_WG * PER_ROUND);
    const u64 run = a.claim != nullptr ? max(rounds, (u64)1) * PER_ROUND : PER_ROUND;
    // one round of the workgroup per iteration; a new run is claimed when the current one is used up
    u64 cur = (u64)blockIdx.x * PER_ROUND, end = a.claim != nullptr ? 0 : cur + PER_ROUND;
    if (a.claim != nullptr)
        cur = 0;
    for (;;) {
        if (cur >= end) {
            if (a.claim != nullptr) {
                __syncthreads();  // every wave has read the last claim
                if (threadIdx.x == 0)
                    *s_base = atomicAdd(a.claim, (unsigned long long)run);
                __syncthreads();
                const unsigned long long b = *s_base;  // (the same in every lane: kept in scalar registers)
                cur = (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)b) |
                      (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(b >> 32)) << 32;
            } else {  // no counter (the per-record path): rounds dealt by workgroup index
                cur += (u64)(gridDim.x - 1) * PER_ROUND;
            }
            end = cur + run;
        }
        if (cur >= a.nrecs)
            break;
        chacha_record<G, OPEN, FRAME>(a, cur + wave * PER_WAVE + grp, j);
        cur += PER_ROUND;
    }
}

template <bool OPEN, int FRAME>
__global__ __launch_bounds__(CHACHA_WG) void chacha_batch_kernel(ChaChaArgs a)
{
    __shared__ u32 s_len[CHACHA_WG / 64];
    __shared__ unsigned long long s_base;
    unsigned long long *const kclock = ENGINE_HOOKS && blockIdx.x == 0 ? g_kclock_buf : nullptr;
    const u64 kc_t0 = kclock != nullptr ? __builtin_amdgcn_s_memtime() : 0ull;
    const u64 kc_r0 = kclock != nullptr ? __builtin_amdgcn_s_memrealtime() : 0ull;
    u32 g = a.force_g;
    if (g == 0) {
        // the width from the mean length of CHACHA_WG descriptors spread over the batch (every workgroup reads the
        // same ones; nothing depends on the workgroups agreeing, a claim is a run of records whatever G takes it)
        u32 len = min(a.recs[(u64)threadIdx.x * a.nrecs / CHACHA_WG].len, PTLS_MI355X_MAX_RECORD_LEN >> 8);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            len += (u32)__shfl_xor((int)len, m);
        if ((threadIdx.x & 63) == 0)
            s_len[threadIdx.x / 64] = len;
        __syncthreads();
        u32 sum = 0;
#pragma unroll
        for (int w = 0; w < CHACHA_WG / 64; ++w)
            sum += s_len[w];
        g = sum / CHACHA_WG >= CHACHA_WIDE_MIN ? CHACHA_G_WIDE : CHACHA_G_NARROW;
    }
    if (g == CHACHA_G_WIDE)
        chacha_records<CHACHA_G_WIDE, OPEN, FRAME>(a, &s_base);
    else
        chacha_records<CHACHA_G_NARROW, OPEN, FRAME>(a, &s_base);
    if (ENGINE_HOOKS && blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(&g_chacha_launches[g == CHACHA_G_WIDE ? 1 : 0], 1ull);
    if (a.claim != nullptr) {
        __syncthreads();  // this workgroup has made its last claim
        if (threadIdx.x == 0 && atomicAdd(a.claim + 1, 1ull) == gridDim.x - 1) {
            atomicExch(a.claim, 0ull);
            atomicExch(a.claim + 1, 0ull);
        }
    }
    if (kclock != nullptr && threadIdx.x == 0) {
        const u64 t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        const u32 i = atomicAdd(&g_kclock_n, 1u);
        if (i < g_kclock_cap) {
            kclock[4 * i + 0] = kc_t0, kclock[4 * i + 1] = t1;
            kclock[4 * i + 2] = kc_r0, kclock[4 * i + 3] = r1;
        }
    }
    publish_done(a.done_flag, a.done_token);
}

// ---- Spread launches: an unframed batch of a few records, or a lone long record, whose long records
// are cut into pieces that 16-lane groups all over the device take, where chacha_batch_kernel gives a record of any
// length to one group.
//
// Plan. Every workgroup derives the same plan from the descriptors (the host cannot read them): a record of min_len
// bytes or more that chacha_record would not reject is cut into pieces of chacha_spread_piece() bytes, every other
// record is one whole item for chacha_record at the width of chacha_batch_kernel's sample rule. Whole records are dealt
// to the groups from the last workgroup down, pieces from the first up, by index: no workgroup waits for another.
//
// A piece [lo, hi) of the text is chacha_record's computation one level up: every lane runs block 0 for r (and s, which
// only the finisher uses), lane j the keystream blocks lo / 64 + j, + 16, ..., folding its 16-byte blocks into its own
// chain (stride r^61, then r^E to the piece's end); piece 0's lane 0 starts with the AAD. The group's sum times r^D,
// D = the 16-byte text blocks behind the piece, is the piece's share of the tag polynomial:
//     tag = ((sum_p partial_p r^D_p) + lenblock) r + s.
//
// Combine. The partials of a workgroup's neighbouring groups that belong to one record are added in LDS, and the sums go
// as five 64-bit limb sums into the record's accumulator (atomic adds, nothing to carry below 2^38 summands), then a
// fence, then the count of pieces: the workgroup whose count completes the record fences again, takes the sums with
// atomic exchanges that leave zero behind, carries them into loose limbs and finishes the tag as chacha_record does. The
// accumulators and counts are zero again when the launch ends.
#define CHACHA_SPREAD_MAX_RECS 255u       // descriptors the plan reads: one per thread of a workgroup (the last stays free)
#define CHACHA_SPREAD_PIECE 1024u         // bytes a piece: one step of a 16-lane group; doubled while a record has more
#define CHACHA_SPREAD_MAX_PIECES PTLS_MI355X_CHACHA_SPREAD_MAX_PIECES  // ... pieces than this
#define CHACHA_SPREAD_MIN_BATCH 1024u     // records from this length are cut: in a batch (100 x 1200 B 27.1 -> 22.9 us),
#define CHACHA_SPREAD_MIN_SINGLE 1024u    // on the per-record path (1200 B 36.4 -> 25.6 us; profiles/chacha20_spread.md)
#define CHACHA_SPREAD_ACC_WORDS 6         // per record: five limb sums and the count of its finished pieces
#define CHACHA_SPREAD_SCRATCH_BYTES ((CHACHA_SPREAD_MAX_RECS + 1) * CHACHA_SPREAD_ACC_WORDS * sizeof(unsigned long long))

struct ChaChaSpreadArgs {
    ChaChaArgs a;  // claim is unused: the items are dealt by index
    u32 piece;     // the piece length of records of up to piece x CHACHA_SPREAD_MAX_PIECES bytes (a multiple of 1024)
    u32 min_len;   // records from this length are cut (at least 1)
    unsigned long long *acc;  // CHACHA_SPREAD_ACC_WORDS per record, zero between launches
};

// [0] spread launches, [1] pieces run, [2] records finished by a combine, [3] whole records run in spread launches
__device__ unsigned long long g_chacha_spread_stats[4];

// the piece length of a record of len bytes: `base` doubled until at most CHACHA_SPREAD_MAX_PIECES pieces cover it
__host__ __device__ inline u32 chacha_spread_piece(u32 len, u32 base)
{
    u64 p = base;
    while (((u64)len + p - 1) / p > CHACHA_SPREAD_MAX_PIECES)
        p <<= 1;
    return (u32)p;
}

// Piece [lo, hi) of record r (not rejected; lo a multiple of 1024, hi its end or the text's) on a group of 16 lanes, j
// the lane: crypts the bytes and returns, in every lane, the piece's share of the tag polynomial as a loose element.
// otk: keystream block 0's first eight words (r || s).
template <bool OPEN>
__device__ __forceinline__ Fe chacha_piece(const ChaChaArgs &a, const ptls_mi355x_record_t &r, u32 lo, u32 hi, u32 j, u32 otk[8])
{
    constexpr u32 G = CHACHA_G_WIDE, STRIDE_E = 4 * G - 3;
    constexpr int NBITS = __builtin_ctz(4 * G);
    const u32 A = PTLS_MI355X_RECORD_AAD_LEN(&r), T = r.len;
    const ChaChaKey *ke = a.keys + r.key_idx;
    u32 key[8];
    {
        const u32x4 k0 = *(const u32x4 *)&ke->key[0], k1 = *(const u32x4 *)&ke->key[4];
        key[0] = k0.x, key[1] = k0.y, key[2] = k0.z, key[3] = k0.w;
        key[4] = k1.x, key[5] = k1.y, key[6] = k1.z, key[7] = k1.w;
    }
    const u32 n0 = ke->iv[0], n1 = ke->iv[1] ^ bswap32((u32)(r.seq >> 32)), n2 = ke->iv[2] ^ bswap32((u32)r.seq);
    const uint8_t *src = a.in + r.in_off;
    uint8_t *dst = a.out + r.out_off;
    // 16-byte blocks of the text and up to the piece's end; the piece's 64-byte blocks [Cb0, Cb1)
    const u32 C = (T + 15) >> 4, Cend = (hi + 15) >> 4, Cb0 = lo >> 6, Cb1 = (hi + 63) >> 6;

    u32 x[16];
    chacha20_block(key, 0, n0, n1, n2, x);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        otk[i] = x[i];
    const Fe r1 = fe_clamped_r(otk[0], otk[1], otk[2], otk[3]);

    // the lane's last block of the piece and the exponent E that aligns its partial with the piece's end
    const u32 bf = Cb0 + j;
    u32 E = 0;
    if (bf < Cb1) {
        const u32 blast = bf + ((Cb1 - 1 - bf) & ~(G - 1));
        const u32 nblast = (min(64u, hi - 64 * blast) + 15) >> 4;
        E = Cend - (4 * blast + nblast - 1);
    }
    Fe rE = fe_select((E & 1) != 0, r1, fe_one()), rS = r1, sq = r1;
#pragma unroll
    for (int bit = 1; bit < NBITS; ++bit) {
        sq = fe_mul(sq, sq);
        rE = fe_select(((E >> bit) & 1) != 0, fe_mul(rE, sq), rE);
        if ((STRIDE_E >> bit) & 1)
            rS = fe_mul(rS, sq);
    }

    Fe h = fe_zero();
    if (lo == 0 && j == 0) {  // the owner of text block 0 starts with the AAD
        const uint8_t *ap = a.aad + r.aad_off;
        for (u32 off = 0; off < A; off += 16) {
            const u32x4 w = load_upto16(ap + off, min(16u, A - off));
            fe_add_block(h, w.x, w.y, w.z, w.w, 1), h = fe_mul(h, r1);
        }
    }
    for (u32 b = bf; b < Cb1; b += G) {
        chacha20_block(key, b + 1, n0, n1, n2, x);
        const u32 o = 64 * b, nT = min(64u, hi - o);
        u32x4 c[4];
        if (nT == 64) {  // a whole block: four 16-byte accesses, nothing to clamp or mask
#pragma unroll
            for (u32 w = 0; w < 4; ++w) {
                const u32x4 p = *(const u32x4_u *)(src + o + 16 * w);
                const u32x4 ks = {x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]};
                const u32x4 q = p ^ ks;
                *(u32x4_u *)(dst + o + 16 * w) = q;
                c[w] = OPEN ? p : q;
            }
        } else
#pragma unroll
        for (u32 w = 0; w < 4; ++w) {
            const u32 nt = sub_clamp16(nT, 16 * w);
            const u32x4 p = load_upto16(src + o + 16 * w, nt);
            const u32x4 ks = {x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]};
            const u32x4 q = p ^ ks;
            store_upto16(dst + o + 16 * w, q, nt);
            c[w] = OPEN ? p : keep_bytes(q, nt);  // the ciphertext, zero from its end
        }
        const u32 nb = (nT + 15) >> 4;
        if (nb == 4 && b + G < Cb1) {
            fe_add_block(h, c[0].x, c[0].y, c[0].z, c[0].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[1].x, c[1].y, c[1].z, c[1].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[2].x, c[2].y, c[2].z, c[2].w, 1), h = fe_mul(h, r1);
            fe_add_block(h, c[3].x, c[3].y, c[3].z, c[3].w, 1), h = fe_mul(h, rS);
        } else {  // the lane's last block of the piece (the only one that may be short)
#pragma unroll
            for (u32 t = 0; t < 4; ++t) {
                if (t < nb) {
                    fe_add_block(h, c[t].x, c[t].y, c[t].z, c[t].w, 1);
                    h = fe_mul(h, fe_select(t + 1 < nb, r1, rE));
                }
            }
        }
    }
    // the partials of the group, summed into all its lanes (every lane of the group is here), then carried over the
    // C - Cend text blocks behind the piece
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int m = 1; m < (int)G; m <<= 1)
            h.v[i] += (u32)__shfl_xor((int)h.v[i], m, G);
    }
    return fe_mul(h, fe_pow(r1, C - Cend));
}

template <bool OPEN>
__global__ __launch_bounds__(CHACHA_WG) void chacha_spread_kernel(ChaChaSpreadArgs sa)
{
    constexpr u32 NWAVES = CHACHA_WG / 64, GROUPS = CHACHA_WG / CHACHA_G_WIDE;
    static_assert(CHACHA_SPREAD_MAX_RECS < CHACHA_WG, "one descriptor per thread");
    __shared__ u32 s_len[NWAVES];
    __shared__ u32 s_wave[2][NWAVES];     // the plan's scan: pieces and whole records per wave
    __shared__ u32 s_incl[CHACHA_WG];     // pieces of the records [0, t]
    __shared__ u32 s_whole[CHACHA_WG];    // the whole records, in batch order
    __shared__ u32 s_rec[GROUPS];         // a round's partials: the record of each group's piece (none: ~0)
    __shared__ u32 s_limb[GROUPS][5];
    __shared__ u32 s_stat[2];             // pieces and whole records this workgroup ran
    const ChaChaArgs &a = sa.a;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid / 64, n = (u32)a.nrecs;

    // the width of the whole records: chacha_batch_kernel's rule
    u32 gw = a.force_g;
    if (gw == 0) {
        u32 len = min(a.recs[(u64)tid * a.nrecs / CHACHA_WG].len, PTLS_MI355X_MAX_RECORD_LEN >> 8);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            len += (u32)__shfl_xor((int)len, m);
        if (lane == 0)
            s_len[wave] = len;
    }
    // the plan: thread t reads descriptor t
    u32 np = 0, wh = 0;
    if (tid < n) {
        const ptls_mi355x_record_t r = a.recs[tid];
        const u32 A = PTLS_MI355X_RECORD_AAD_LEN(&r);
        const bool good = r.len <= PTLS_MI355X_MAX_RECORD_LEN && A <= PTLS_MI355X_MAX_AAD_LEN && r.key_idx < a.nkeys &&
                          (A == 0 || a.aad != nullptr);
        if (good && r.len >= sa.min_len) {
            const u32 piece = chacha_spread_piece(r.len, sa.piece);
            np = (r.len + piece - 1) / piece;
        } else {
            wh = 1;
        }
    }
    u32 ip = np, iw = wh;  // inclusive sums over the wave, then over the workgroup
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 tp = (u32)__shfl_up((int)ip, d), tw = (u32)__shfl_up((int)iw, d);
        if (lane >= (u32)d)
            ip += tp, iw += tw;
    }
    if (lane == 63)
        s_wave[0][wave] = ip, s_wave[1][wave] = iw;
    if (tid < 2)
        s_stat[tid] = 0;
    __syncthreads();
    u32 totp = 0, totw = 0;
#pragma unroll
    for (u32 w = 0; w < NWAVES; ++w) {
        if (w < wave)
            ip += s_wave[0][w], iw += s_wave[1][w];
        totp += s_wave[0][w], totw += s_wave[1][w];
    }
    s_incl[tid] = ip;
    if (wh)
        s_whole[iw - 1] = tid;
    if (gw == 0) {
        u32 sum = 0;
#pragma unroll
        for (u32 w = 0; w < NWAVES; ++w)
            sum += s_len[w];
        gw = sum / CHACHA_WG >= CHACHA_WIDE_MIN ? CHACHA_G_WIDE : CHACHA_G_NARROW;
    }
    __syncthreads();

    // whole records: a round of the workgroup is CHACHA_WG / G of them, dealt from the last workgroup down
    const auto whole = [&](auto GW) {
        constexpr u32 G = decltype(GW)::value, PER_WAVE = 64 / G, PER_ROUND = CHACHA_WG / G;
        for (u32 base = (gridDim.x - 1 - blockIdx.x) * PER_ROUND; base < totw; base += gridDim.x * PER_ROUND) {
            const u32 k = base + wave * PER_WAVE + lane / G;
            if (ENGINE_HOOKS && k < totw && lane % G == 0)
                atomicAdd(&s_stat[1], 1u);
            chacha_record<(int)G, OPEN, 0>(a, k < totw ? (u64)s_whole[k] : a.nrecs, lane % G);
        }
    };
    if (gw == CHACHA_G_WIDE)
        whole(std::integral_constant<u32, CHACHA_G_WIDE>{});
    else
        whole(std::integral_constant<u32, CHACHA_G_NARROW>{});

    // pieces: a round is one per group, GROUPS consecutive ones a workgroup
    const u32 g = tid / CHACHA_G_WIDE, j = tid % CHACHA_G_WIDE;
    for (u32 base = blockIdx.x * GROUPS; base < totp; base += gridDim.x * GROUPS) {  // (the same trips in every group)
        const u32 item = base + g;
        const bool has = item < totp;
        u32 t = ~0u, first = 0, otk[8] = {};
        ptls_mi355x_record_t r = {};
        Fe part = fe_zero();
        if (has) {
            u32 lo = 0, hi = n - 1;  // the record of the item: the first t with s_incl[t] > item
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (s_incl[mid] > item)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            t = lo, first = t != 0 ? s_incl[t - 1] : 0u;
            r = a.recs[t];
            const u32 piece = chacha_spread_piece(r.len, sa.piece), at = (item - first) * piece;
            part = chacha_piece<OPEN>(a, r, at, min(r.len, at + piece), j, otk);
            if (j == 0) {
                s_rec[g] = t;
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    s_limb[g][i] = part.v[i];
            }
        } else if (j == 0) {
            s_rec[g] = ~0u;
        }
        __syncthreads();
        if (has && j == 0 && (g == 0 || s_rec[g - 1] != t)) {  // the first of the workgroup's groups on record t
            unsigned long long sum[5];
#pragma unroll
            for (int i = 0; i < 5; ++i)
                sum[i] = part.v[i];
            u32 run = 1;
            for (u32 k = g + 1; k < GROUPS && s_rec[k] == t; ++k, ++run) {
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    sum[i] += s_limb[k][i];
            }
            if (ENGINE_HOOKS)
                atomicAdd(&s_stat[0], run);
            unsigned long long *acc = sa.acc + (size_t)CHACHA_SPREAD_ACC_WORDS * t;
#pragma unroll
            for (int i = 0; i < 5; ++i)
                atomicAdd(acc + i, sum[i]);
            __threadfence();  // the sums are visible device-wide before the count that publishes them
            if (atomicAdd(acc + 5, (unsigned long long)run) + run == s_incl[t] - first) {
                // these pieces completed the record: every other piece's sums are in (they were counted after a fence)
                __threadfence();
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    sum[i] = atomicExch(acc + i, 0ull);  // (not a cached read; zero for the next launch)
                atomicExch(acc + 5, 0ull);
                // limb sums of up to CHACHA_SPREAD_MAX_PIECES loose elements: one carry pass in 64 bits leaves a loose one
                sum[1] += sum[0] >> 26, sum[2] += sum[1] >> 26, sum[3] += sum[2] >> 26, sum[4] += sum[3] >> 26;
                Fe h;
                h.v[0] = ((u32)sum[0] & P26) + (u32)(sum[4] >> 26) * 5;  // (2^130 = 5; the carry out is small)
#pragma unroll
                for (int i = 1; i < 5; ++i)
                    h.v[i] = (u32)sum[i] & P26;
                const u32 A = PTLS_MI355X_RECORD_AAD_LEN(&r), T = r.len;
                fe_add_block(h, A, 0, T, 0, 1);  // LE64(aadlen) || LE64(textlen)
                h = fe_mul(h, fe_clamped_r(otk[0], otk[1], otk[2], otk[3]));
                u32 tag[4];
                fe_tag(h, &otk[4], tag);
                if (OPEN) {
                    // all 16 bytes compared, no early exit
                    const u32x4 got = *(const u32x4_u *)(a.in + r.in_off + T);
                    a.ok[t] = ((got.x ^ tag[0]) | (got.y ^ tag[1]) | (got.z ^ tag[2]) | (got.w ^ tag[3])) == 0;
                } else {
                    const u32x4 tg = {tag[0], tag[1], tag[2], tag[3]};
                    *(u32x4_u *)(a.out + r.out_off + T) = tg;
                }
                if (ENGINE_HOOKS)
                    atomicAdd(&g_chacha_spread_stats[2], 1ull);
            }
        }
        __syncthreads();  // s_rec and s_limb are free again
    }

    if (ENGINE_HOOKS && tid == 0) {
        if (blockIdx.x == 0) {
            atomicAdd(&g_chacha_launches[gw == CHACHA_G_WIDE ? 1 : 0], 1ull);
            atomicAdd(&g_chacha_spread_stats[0], 1ull);
        }
        if (s_stat[0] != 0)
            atomicAdd(&g_chacha_spread_stats[1], (unsigned long long)s_stat[0]);
        if (s_stat[1] != 0)
            atomicAdd(&g_chacha_spread_stats[3], (unsigned long long)s_stat[1]);
    }
    publish_done(a.done_flag, a.done_token);
}

// Test hook (ptls_mi355x_chacha_debug_rpow): r^e on one lane with the pieces' power routine, fully reduced, as 17
// little-endian bytes. r is the 16 bytes as they are (no clamp).
__global__ __launch_bounds__(64) void chacha_rpow_kernel(const uint8_t *r16, u64 e, uint8_t *out17)
{
    if (threadIdx.x != 0)
        return;
    const u32x4 k = *(const u32x4_u *)r16;
    Fe r = fe_zero();
    fe_add_block(r, k.x, k.y, k.z, k.w, 0);
    const Fe h = fe_reduced(fe_pow(r, e));
    const u32x4 o = {h.v[0] | h.v[1] << 26, h.v[1] >> 6 | h.v[2] << 20, h.v[2] >> 12 | h.v[3] << 14, h.v[3] >> 18 | h.v[4] << 8};
    *(u32x4_u *)out17 = o;
    out17[16] = (uint8_t)(h.v[4] >> 24);
}

// QUIC header protection for the ChaCha20 suites: one lane per sample, one block. The sample's first 4 bytes are the
// block counter (little endian) and the next 12 the nonce (picotls' 16-byte ChaCha20 IV, include/picotls.h:95); the mask
// is the first 16 keystream bytes. An entry whose key_idx is out of range gets a zero mask.
__global__ __launch_bounds__(256) void chacha_hp_kernel(const ChaChaKey *keys, u32 nkeys, const ptls_mi355x_hp_t *hp,
                                                        const uint8_t *base, uint8_t *masks, u64 n, u32 *done_flag, u32 done_token)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const ptls_mi355x_hp_t e = hp[i];
        u32x4 m = {0, 0, 0, 0};
        if (e.key_idx < nkeys) {
            const u32x4 s = *(const u32x4_u *)(base + e.sample_off);
            const ChaChaKey *ke = keys + e.key_idx;
            u32 key[8], x[16];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                key[k] = ke->key[k];
            chacha20_block(key, s.x, s.y, s.z, s.w, x);
            m.x = x[0], m.y = x[1], m.z = x[2], m.w = x[3];
        }
        *(u32x4_u *)(masks + 16 * i) = m;
    }
    publish_done(done_flag, done_token);
}

// The pre-pass of ptls_mi355x_chacha_open_quic_packets (RFC 9001 §5.4.2, RFC 9000 A.3), one lane per packet in the shape
// of chacha_hp_kernel: the mask from the sample 4 bytes behind the packet-number offset, the first byte and the packet
// number unmasked, the full packet number from the expected one, the rejections and the key-phase verdict, all into
// results[i], which the FRAME 2 open of chacha_batch_kernel reads for its nonce and lengths. Nothing else is written.
__global__ __launch_bounds__(256) void chacha_quic_unmask_kernel(const ChaChaKey *hp_keys, u32 hp_nkeys, u32 nkeys,
                                                                 const ptls_mi355x_record_t *recs, u64 n, const uint8_t *in,
                                                                 ptls_mi355x_quic_result_t *results)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const ptls_mi355x_record_t r = recs[i];
        u32x4 res = quic_result_rejected();
        if (quic_open_admits(r, nkeys, hp_nkeys)) {
            const uint8_t *p = in + r.in_off, *pn = p + r.aad_len;
            const u32x4 s = *(const u32x4_u *)(pn + 4);
            const ChaChaKey *ke = hp_keys + r.key_idx;
            u32 key[8], x[16];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                key[k] = ke->key[k];
            chacha20_block(key, s.x, s.y, s.z, s.w, x);
            const QuicUnmasked u = quic_unmask(p[0], pn, x[0], quic_m14(x[0], x[1]), r.seq, r.flags);
            res = quic_result_pack(u, r.len - u.pn_len - 16);
        }
        *(u32x4_u *)(results + i) = res;
    }
}

// rekey (ptls_mi355x_chacha_keyset_update): entry idx[i] = src[i]
__global__ __launch_bounds__(256) void chacha_keys_scatter_kernel(const ChaChaKey *src, const u32 *idx, ChaChaKey *dst, u32 n)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        dst[idx[i]] = src[i];
}

// Test hook (ptls_mi355x_chacha_debug_poly1305): plain Poly1305 (RFC 8439 §2.5) of msg under a given one-time key, one
// lane, with the routines the record kernels use. A short last block takes the byte 1 after its end and no 2^128 bit.
__global__ __launch_bounds__(64) void chacha_poly1305_kernel(const uint8_t *key, const uint8_t *msg, u64 len, uint8_t *tag)
{
    if (threadIdx.x != 0)
        return;
    const u32x4 k0 = *(const u32x4_u *)key, k1 = *(const u32x4_u *)(key + 16);
    const Fe r = fe_clamped_r(k0.x, k0.y, k0.z, k0.w);
    const u32 s[4] = {k1.x, k1.y, k1.z, k1.w};
    Fe h = fe_zero();
    for (u64 off = 0; off < len; off += 16) {
        const u32 n = (u32)min((u64)16, len - off);
        u32x4 w = load_upto16(msg + off, n);
        if (n < 16) {
#pragma unroll
            for (u32 k = 0; k < 4; ++k)
                w[k] |= (n >> 2) == k ? 1u << (8 * (n & 3)) : 0u;
        }
        fe_add_block(h, w.x, w.y, w.z, w.w, n == 16);
        h = fe_mul(h, r);
    }
    u32 t[4];
    fe_tag(h, s, t);
    const u32x4 o = {t[0], t[1], t[2], t[3]};
    *(u32x4_u *)tag = o;
}

#endif  // PTLS_MI355X_CHACHA_KERNELS_H
