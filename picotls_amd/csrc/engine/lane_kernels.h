// picotls_amd/csrc/engine/lane_kernels.h -- The record-per-lane batch kernel (gcm_lane_kernel): one whole record per GPU lane.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included in order; not standalone).
#ifndef PTLS_MI355X_ENGINE_LANE_KERNELS_H
#define PTLS_MI355X_ENGINE_LANE_KERNELS_H

// PTLS_MI355X_SCHEDULE_RECORD_PER_LANE: batches in which a connection contributes only a few records. Every other
// batch kernel shares per-key precomputation among a run's records (8 KiB GHASH window tables per H power, a scan and a
// barrier per run); with 1-8 records per key that precomputation is most of the launch. Here nothing is shared: a lane
// reads its record's descriptor, loads the key's round keys into its own registers, builds a 256-byte table of its
// hash key's 4-bit multiples in its own LDS slots and seals or opens the record serially -- AES-CTR four blocks at a
// time behind the counter cache, GHASH as a plain Horner with H (ghash.h gmul_lane). No runs, no scan, no key order, no
// cross-lane step, no barrier after the AES table build; a record costs the same whatever the number of records per
// key. One workgroup of LANE_WG lanes per CU (128 KiB of LDS: the AES T-tables and LANE_WG x 256 B of lane tables), one
// wave per SIMD; workgroup b takes the record tiles b, b + grid, ... of LANE_WG records, lane t record tile * LANE_WG + t.
// The lanes of a wave run in lockstep, so a wave takes as long as its longest record: the schedule suits short records
// of similar length, and a lane works serially, hence the cap PTLS_MI355X_LANE_MAX_LEN on len and AAD.
// Constant time by layout: the AES lookups go to the lane's own bank replica, the GHASH lookups to the
// lane's own bank quad (lds_tables.h build_lane_table), for any key and payload.
#define LANE_WG 256
static_assert(LANE_WG * 256 == LANE_LDS_BYTES - LANE_TAB_BASE, "one 256-byte table per lane");
static_assert(QUIC_DESC_REFUSED > PTLS_MI355X_LANE_MAX_LEN, "lane_record_ok refuses the len of a packet that did not pass");

// record_ok (gcm_kernels.h) with this schedule's limit
template <int FRAME>
__device__ __forceinline__ bool lane_record_ok(const BatchArgs &args, const ptls_mi355x_record_t &r)
{
    return r.len <= PTLS_MI355X_LANE_MAX_LEN && gcm_aad_len<false, FRAME>(r) <= PTLS_MI355X_LANE_MAX_LEN && r.key_idx < args.nkeys;
}

// one accepted record, by one lane; i: its batch index (the ok byte). The TLS framings (FRAME 1, 2: record.h) follow
// gcm_segment byte for byte: the header or the 13-byte AAD is built in registers, a TLS 1.3 seal appends the content type
// to the payload without reading the byte behind it, a framed open stores no plaintext under a header the record layer
// refuses (wr) and computes the tag all the same. Every line of theirs is compiled for them alone.
template <int NR, bool OPEN, int FRAME>
__device__ __forceinline__ void lane_record(const BatchArgs &args, lds_u8 *lds, u32 laneoff, u32 mbase, const ptls_mi355x_record_t &r, u64 i)
{
    constexpr bool SEAL_FRAME = FRAME == 1 && !OPEN, TLS = FRAME == 1 || FRAME == 2, TLS12 = FRAME == 2, HDR = OPEN && TLS;
    const KeyEntry *k = args.keys + r.key_idx;
    u32 rk[NR + 1][4];
#pragma unroll
    for (int q = 0; q <= NR; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            rk[q][c] = k->rk[q][c];
    build_lane_table(lds, mbase, k->h[0]);
    // nonce = iv ^ (0^32 || BE64(seq)), as gcm_segment; TLS 1.2 takes the record's explicit nonce as stored in place of seq
    u32 nw1 = bswap32((u32)(r.seq >> 32)), nw2 = bswap32((u32)r.seq);
    if constexpr (TLS12) {
        const uint8_t *e = args.in + r.in_off + (OPEN ? TLS_HEADER_SIZE : 0);
        nw1 = *(const u32_u *)e;
        nw2 = *(const u32_u *)(e + 4);
    }
    const u32 n0 = k->iv[0] ^ rk[0][0];
    const u32 n1 = k->iv[1] ^ nw1 ^ rk[0][1];
    const u32 n2 = k->iv[2] ^ nw2 ^ rk[0][2];

    // (the text length through record.h's helper in the framed instantiations alone: read through it, r.len cost the
    // unframed and QUIC kernels another register assignment, two SGPRs fewer, with no other change to their code)
    const u32 A = gcm_aad_len<OPEN, FRAME>(r);
    u32 L = r.len;
    if constexpr (TLS)
        L = gcm_text_len<OPEN, FRAME>(r);
    // bytes of text readable at src (a TLS 1.3 seal reads len payload bytes; its last text byte is the content type)
    const u32 Lsrc = SEAL_FRAME ? L - 1 : L;
    const uint8_t *src = args.in + r.in_off + frame_in_skip<OPEN, FRAME>() + quic_skip<FRAME>(A);
    uint8_t *dst = args.out + r.out_off + frame_out_skip<OPEN, FRAME>() + quic_skip<FRAME>(A);
    // a framed open writes no plaintext under a header that tls_unpad_kernel / tls12_check_kernel refuse (segment.h)
    bool wr = true;
    if constexpr (HDR) {
        const uint8_t *h = args.in + r.in_off;
        const u32 w = *(const u32_u *)h, wl = (w >> 24) << 8 | h[4];
        wr = FRAME == 1 ? (w & 0xffffffu) == 0x030317u && wl == L + 16
                        : (w & 0xffff00u) == 0x030300u && wl == L + TLS12_RECORD_IV_SIZE + 16;
    }

    u32 y[4] = {0, 0, 0, 0};
    if constexpr (TLS) {  // one AAD block, from registers but for the TLS 1.3 open's, which is the header as received
        u32x4 X;
        if constexpr (SEAL_FRAME) {  // the record header: built here, written to the wire, and authenticated
            const u32 wl = L + 16;
            X = u32x4{0x00030317u | ((wl >> 8) & 0xffu) << 24, wl & 0xffu, 0, 0};
            store_partial(args.out + r.out_off, X, TLS_HEADER_SIZE);
        } else if constexpr (TLS12) {  // AAD = BE64(seq) || type || 3 || 3 || BE16(len) (build_tls12_aad)
            const u32 type = OPEN ? (u32)args.in[r.in_off] : (r.flags & 0xffu);
            X = u32x4{bswap32((u32)(r.seq >> 32)), bswap32((u32)r.seq), type | 0x030300u | ((L >> 8) & 0xffu) << 24, L & 0xffu};
            if constexpr (!OPEN) {  // the wire header and the explicit nonce
                const u32 wl = TLS12_RECORD_IV_SIZE + L + 16;
                const u32x4 h = {type | 0x030300u | ((wl >> 8) & 0xffu) << 24, (wl & 0xffu) | nw1 << 8, nw1 >> 24 | nw2 << 8, nw2 >> 24};
                store_partial(args.out + r.out_off, h, TLS_HEADER_SIZE + TLS12_RECORD_IV_SIZE);
            }
        } else {
            X = load_partial(args.in + r.in_off, TLS_HEADER_SIZE);
        }
        ghash_lane_fold(mbase, y, X);
    } else {
        // (a QUIC packet's AAD is its header in the clear: the seal's input, or what the open's pre-pass left in the output)
        const uint8_t *aadp = FRAME == 3 ? (OPEN ? (const uint8_t *)args.out + r.out_off : args.in + r.in_off) : args.aad + r.aad_off;
        for (u32 o = 0; o < A; o += 16) {
            const u32 rem = A - o;
            ghash_lane_fold(mbase, y, rem >= 16 ? u32x4(*(const u32x4_u *)(aadp + o)) : load_partial(aadp + o, rem));
        }
    }

    // Step s runs the counters 4s + 1 .. 4s + 4: E(K, J0) (counter 1) is slot 0 of step 0, text block b takes counter
    // b + 2, so a step past the first covers the 64 contiguous text bytes from 16 (4s - 1). The four counters of a step
    // share the cache's 256-counter window except when the last is a multiple of 256: that slot opens the next window,
    // whose cache is built there (a 64 KiB record crosses 16 of them).
    const u32 nb = (L + 15) >> 4, nsteps = (nb + 1 + 3) >> 2;
    CtrCache1 cc = ctr_cache1_init<NR>(lds, laneoff, rk, n0, n1, n2, rk[0][3]);
    u32x4 ekj0 = {0, 0, 0, 0};
    for (u32 s = 0; s < nsteps; ++s) {
        const u32 c0 = 4 * s + 1;
        const int b0 = (int)(4 * s) - 1;  // slot 0's text block
        const bool full = s != 0 && 16u * (u32)(b0 + 4) <= Lsrc;  // four whole text blocks (of the readable source)
        // the step's input is loaded before any of its output is stored (out may alias in)
        u32x4 x[4];
        if (full) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                x[q] = *(const u32x4_u *)(src + 16u * (u32)(b0 + q));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = b0 + q;
                x[q] = u32x4{0, 0, 0, 0};
                if (b >= 0 && b < (int)nb) {
                    const u32 rem = Lsrc - 16u * (u32)b;
                    x[q] = rem >= 16 ? u32x4(*(const u32x4_u *)(src + 16u * (u32)b)) : load_partial(src + 16u * (u32)b, rem);
                    if constexpr (SEAL_FRAME) {  // the inner content type follows the payload (src[len] is never read)
                        if (rem < 16)
                            x[q][rem >> 2] |= (u32)(r.flags & 0xffu) << (8 * (rem & 3));
                    }
                }
            }
        }
        u32 st[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            st[q][0] = n0, st[q][1] = n1, st[q][2] = n2, st[q][3] = bswap32(c0 + (u32)q) ^ rk[0][3];
        aes_ctr_cached_n<NR, 4>(lds, laneoff, rk, cc, st);
        if (((c0 + 3) & 255u) == 0) {
            u32 s1[1][4] = {{n0, n1, n2, bswap32(c0 + 3) ^ rk[0][3]}};
            cc = ctr_cache1_init<NR>(lds, laneoff, rk, n0, n1, n2, s1[0][3]);
            aes_ctr_cached1<NR>(lds, laneoff, rk, cc, s1);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                st[3][c] = s1[0][c];
        }
        // output, and the GHASH inputs (the ciphertext) in x
        if (full) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 o = x[q] ^ u32x4{st[q][0], st[q][1], st[q][2], st[q][3]};
                if (!HDR || wr)
                    *(u32x4_u *)(dst + 16u * (u32)(b0 + q)) = o;
                if (!OPEN)
                    x[q] = o;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = b0 + q;
                const u32x4 ks = {st[q][0], st[q][1], st[q][2], st[q][3]};
                if (b < 0) {
                    ekj0 = ks;
                } else if (b < (int)nb) {
                    const u32 rem = L - 16u * (u32)b;
                    u32x4 o = x[q] ^ ks;
                    if (rem >= 16) {
                        if (!HDR || wr)
                            *(u32x4_u *)(dst + 16u * (u32)b) = o;
                    } else {
                        o = mask_tail(o, rem);
                        if (!HDR || wr)
                            store_partial(dst + 16u * (u32)b, o, rem);
                    }
                    if (!OPEN)
                        x[q] = o;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = b0 + q;
            if (b >= 0 && b < (int)nb)
                ghash_lane_fold(mbase, y, x[q]);
        }
    }
    // the length block, then tag = GHASH ^ E(K, J0)
    const u64 abits = (u64)A * 8, cbits = (u64)L * 8;
    const u32 t[4] = {y[0] ^ (u32)(abits >> 32), y[1] ^ (u32)abits, y[2] ^ (u32)(cbits >> 32), y[3] ^ (u32)cbits};
    gmul_lane(mbase, t, y);
    const u32x4 tag = u32x4{bswap32(y[0]), bswap32(y[1]), bswap32(y[2]), bswap32(y[3])} ^ ekj0;
    if (OPEN) {  // all 16 bytes compared, no early exit; the plaintext is written either way, as fusion does
        const u32x4 d = u32x4(*(const u32x4_u *)(src + L)) ^ tag;
        args.ok[i] = (uint8_t)((d[0] | d[1] | d[2] | d[3]) == 0);
    } else {
        *(u32x4_u *)(dst + L) = tag;
    }
}

// FRAME 0 (unframed records), 1 and 2 (TLS 1.3 and TLS 1.2 wire records, on a keyset with lane_framed set) and 3 (QUIC
// packets: the descriptors are the pre-passes' rewritten ones, aux_kernels.h)
template <int NR, bool OPEN, int FRAME>
__global__ __launch_bounds__(LANE_WG) void gcm_lane_kernel(BatchArgs args)
{
    static_assert(FRAME >= 0 && FRAME <= 3, "unframed records, TLS 1.3 and TLS 1.2 wire records, QUIC packets");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    lds_u8 *lds = (lds_u8 *)smem;
    check_lds_base(smem);
    unsigned long long *const kclock = ENGINE_HOOKS && blockIdx.x == 0 ? g_kclock_buf : nullptr;
    const u64 kc_t0 = kclock != nullptr ? __builtin_amdgcn_s_memtime() : 0ull;
    const u64 kc_r0 = kclock != nullptr ? __builtin_amdgcn_s_memrealtime() : 0ull;
    build_aes_tables(lds);
    __syncthreads();  // (the only barrier: the lane tables are private to their lanes)
    const u32 laneoff = (threadIdx.x & 31) * 4, mbase = lane_tab_base();
    u32 accepted = 0;
    for (u64 tile = blockIdx.x; tile * LANE_WG < args.nrecs; tile += gridDim.x) {
        const u64 i = tile * LANE_WG + threadIdx.x;
        if (i >= args.nrecs)
            continue;
        const ptls_mi355x_record_t r = args.recs[i];
        if (!lane_record_ok<FRAME>(args, r)) {  // rejected as a whole: nothing is written but a failed ok byte
            if (OPEN)
                args.ok[i] = 0;
            continue;
        }
        ++accepted;
        lane_record<NR, OPEN, FRAME>(args, lds, laneoff, mbase, r, i);
    }
    // (test hook, ptls_mi355x_debug_counters) the records this workgroup accepted, one atomic per wave at its end
    if (ENGINE_HOOKS) {
        const u32 sum = wave_incl_sum(accepted);
        if ((threadIdx.x & 63) == 63 && sum != 0)
            atomicAdd(&g_ext_runs[blockIdx.x % EXT_RUN_ROWS][5], (unsigned long long)sum);
    }
    if (kclock != nullptr && threadIdx.x == 0) {  // (vector stores and atomics only)
        const u64 t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        const u32 n = atomicAdd(&g_kclock_n, 1u);
        if (n < g_kclock_cap) {
            kclock[4 * n + 0] = kc_t0, kclock[4 * n + 1] = t1;
            kclock[4 * n + 2] = kc_r0, kclock[4 * n + 3] = r1;
        }
    }
}

#endif  // PTLS_MI355X_ENGINE_LANE_KERNELS_H
