// picotls_amd/csrc/engine/segment.h -- gcm_segment: AES-CTR + GHASH of a range of one record's stream by one 8-lane group.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included in order; not standalone).
#ifndef PTLS_MI355X_ENGINE_SEGMENT_H
#define PTLS_MI355X_ENGINE_SEGMENT_H

// GHASH/CTR work of one G-lane group on steps [m_lo, m_hi) of record r's stream (see file header): lane j owns stream
// positions j + G*m, one AES-CTR block per step (16 LDS lookups per round in flight); its GHASH folds are sequential
// (Horner with H^G; each lane's last position in the segment takes H^(end - position) after the loop). On return every
// lane of the group holds the segment's GHASH partial sum(X_i * H^(end - i)), plus E(K, J0) when the segment holds the
// record's length block: the length lane (lane (N - 1) mod G) encrypts J0 in that step and XORs it into its
// accumulator after the segment end (the length block is the last stream position, H^0 in every later combine), so a
// finished record's GHASH sum is its tag, and E(K, J0) need not stay live through the loop (it waits in the caller's
// LDS slot; live, it was spilled to scratch once per segment). Invalid groups pass m_lo == m_hi.
// With finish (a whole record), a seal writes the tag and an open returns the tag check in okw on the length lane (1 =
// verified, 0 = not; 2 on every other lane and without finish): the caller stores the ok byte, so the record's batch
// index need not stay live through the segment.
//
// Stream layout. Units of the chunked schedule end on step boundaries, so their stream [zero padding | AAD | text |
// length] is front-padded to a multiple of G positions (N = G * K). A whole record (ALIGNED: the lockstep kernel and the
// chunked kernel's whole-record runs) instead takes the front padding that puts its text blocks on 128-byte lines of the
// output: the group then stores one full line per step instead of parts of two (the parts of two cost 14.5 % more HBM
// writes and 2 % of seal time on 16 KiB records, profiles/r2_write_align.txt). Its stream ends where it ends (N any):
// lanes past the length block in the last step are idle, and each lane's last position p multiplies by H^(N - p), 1..G.
//
// Segment end (late round 3): a lane's last multiply by its own power H^e from its own nibble-major table read another
// table row than the lanes beside it, so its bank conflicts depended on the data (profiles/r2_ct_counters.txt). Now
// every lane keeps its last position unmultiplied, the wave's last step skips the Horner multiply, and
// coop_last_powers (ghash.h) applies the powers from window-major tables after the loop: 32 conflict-free lookups per
// lane, E(K, J0) waiting in the caller's LDS slot (ekslot) and added on the length lane. (The per-lane last multiply,
// the round-3 butterfly over uniform tables and the round-2 four-multiply step it replaced are no longer in the source.)
// CT (the kernels' constant-time argument, instantiated true by the chunked, spread and span kernels and false by the
// lockstep one) is read nowhere since the segment ends became one: it only keeps the lockstep kernel's instantiation
// apart from the spread and span kernels'. Sharing one, the step lambdas below gain callers, the compiler inlines them
// otherwise, and the four lockstep kernels' code changes (21 to 38 lines each).
// a 16-byte store of gcm_segment's text output: unconditional but in a framed open (HDR), which skips it for a record
// whose header is refused (wr, set at the function's start)
#define SEG_PUT(p, v)              \
    do {                           \
        if (!HDR || wr)            \
            *(u32x4_u *)(p) = (v); \
    } while (0)
template <int NR, bool OPEN, int FRAME = 0, bool CT = false, bool W8 = false, int GG = ENGINE_G, bool MK4 = false>
__device__ __forceinline__ void gcm_segment(const BatchArgs &args, const lds_u8 *lds, const u32 (&rk)[NR + 1][4], u32 iv0,
                                            u32 iv1, u32 iv2, const ptls_mi355x_record_t &r, bool valid, u32 m_lo,
                                            u32 m_hi, u32 j, u32 laneoff, u32 tsel_horner, u32x4 &acc, bool finish,
                                            u32 &okw, bool aligned, u32 ekslot = 0, bool w8tree = false,
                                            u32 mk_kslot = MK_NONE)
{
    // G lanes per record: ENGINE_G, or 4 in the W8 serial kernel's whole runs (ghash.h, 4-lane groups), whose aligned
    // streams then put text blocks on 64-byte boundaries (a group stores 64 bytes a step)
    constexpr int G = GG;
    static_assert(G == 8 || (G == 4 && W8), "8-lane groups, or 4-lane groups in the W8 kernels");
#if ENGINE_PROFILE
    const unsigned long long tsg0 = stamp();
#endif
    constexpr int GS = G == 8 ? 3 : 2;  // log2 G
    // W8 (a W8 run of the pair's EXT 3 kernel, gcm_chunked_kernel): Horner on the 8-bit H^8 table (gmul8), the lanes'
    // last powers by a serial Horner over the group's ranks with the window-major H table (W8_TAB_H, w8_lane_end)
    // (without W8: Horner on the nibble-major H^8 table, the conflict-free segment end coop_last_powers)
    W8Lane w8 = {};
    if constexpr (W8)
        w8 = w8_lane(lane_here());
    // (round 6) MK4: a multi-key run's record (4-lane groups of the W8 serial kernel): the Horner on its connection's
    // 4-bit H^4 table (gmul4w) and the segment end on its H table, in the table slot mk_kslot names (ghash.h)
    static_assert(!MK4 || (W8 && G == 4), "MK runs are 4-lane W8 runs");
    MK4Lane mk4 = {};
    if constexpr (MK4)
        mk4 = mk4_lane(lane_here());
    auto horner = [&](u32x4 t) -> u32x4 {
        if constexpr (MK4)
            return gmul4w(lds, t, w8, mk4, mk_kslot);
        else
            return gmul8(lds, t, w8);
    };
    constexpr bool SEAL_FRAME = FRAME == 1 && !OPEN, OPEN_FRAME = FRAME == 1 && OPEN, TLS12 = FRAME == 2;
    const u32 L = gcm_text_len<OPEN, FRAME>(r), A = gcm_aad_len<OPEN, FRAME>(r);
    // bytes of text readable at src (a framed seal reads len payload bytes; its last text byte is the content type)
    const u32 Lsrc = SEAL_FRAME ? L - 1 : L;
    const u32 na = (A + 15) >> 4, nb = (L + 15) >> 4;
    const u32 total = na + nb + 1;
    const uint8_t *src = args.in + r.in_off + frame_in_skip<OPEN, FRAME>() + quic_skip<FRAME>(A);
    uint8_t *dst = args.out + r.out_off + frame_out_skip<OPEN, FRAME>() + quic_skip<FRAME>(A);
    // A framed open writes no plaintext for a record whose header the record layer refuses (TLS 1.3: not {23, 3, 3,
    // BE16(len + 16)}; TLS 1.2: not {type, 3, 3, BE16(8 + len + 16)}, the checks of tls_unpad_kernel and
    // tls12_check_kernel): its range of the output stays as it was. Its tag is computed all the same, since those
    // kernels report a failed tag ahead of a bad header. HDR is false in every other instantiation, whose stores
    // (SEG_PUT) are then unconditional.
    constexpr bool HDR = OPEN && (FRAME == 1 || FRAME == 2);
    bool wr = true;
    if constexpr (HDR) {
        if (valid) {
            const uint8_t *h = args.in + r.in_off;
            const u32 w = *(const u32_u *)h, wl = (w >> 24) << 8 | h[4];
            wr = FRAME == 1 ? (w & 0xffffffu) == 0x030317u && wl == L + 16
                            : (w & 0xffff00u) == 0x030300u && wl == L + TLS12_RECORD_IV_SIZE + 16;
        }
    }
    int P;
    u32 N;
    if (aligned) {  // text block b at position P + na + b, and (dst / 16 + b) mod G == that position mod G
        const u32 K0 = (total + G - 1) / G;
        P = (int)(((u32)((uintptr_t)dst >> 4) - na) & (G - 1));
        // (round 6) a 4-lane open puts text block 0 at a step's start instead: the steps before it need no keystream
        // (the seal's aligned output gives it the same padding), and the steady steps hold their blocks until a line is
        // whole (LINE below)
        if constexpr (OPEN && G == 4)
            P = (int)((0u - na) & (G - 1));
        // ... unless that costs a record shorter than ALIGN_MIN_STEPS steps one more step (its wave would take it too:
        // -6 % on 1200-byte records), which keeps the padding of a multiple of G positions
        if ((u32)P + total > K0 * G && K0 < ALIGN_MIN_STEPS)
            P = (int)(K0 * G - total);
        N = (u32)P + total;
        if (valid)
            m_hi = (N + G - 1) / G;
    } else {  // (padded to a multiple of ENGINE_G positions for any G: 4-lane groups take the 8-lane units' bounds)
        const u32 K = (total + ENGINE_G - 1) / ENGINE_G;
        P = (int)(K * ENGINE_G) - (int)total;
        N = K * ENGINE_G;
    }
    // this lane's last step in the segment and its power there: at the record's end H^(N - p) for its last position p,
    // at a unit's end (a step boundary) H^(G - j)
    const bool at_end = aligned;
    const int m_last = !valid ? -1 : at_end ? ((int)N - 1 - (int)j) >> GS : (int)m_hi - 1;
    const u32 e_last = at_end ? N - ((u32)G * (u32)m_last + j) : (u32)G - j;  // 1..G
    // the first step in which some lane of the group is at its last position (the steady range ends before it)
    const int m_first_last = at_end ? ((int)N - G) >> GS : (int)m_hi - 1;
    const u32 jl = (N - 1) & (G - 1);  // the length block's lane

    const u32 Smax = wave_max_perg<G>(m_hi - m_lo);  // m_lo, m_hi are uniform within a group

    // nonce = iv ^ (0^32 || BE64(seq)) (lib/picotls.c:6587-6601); TLS 1.2 takes the explicit nonce of the record in
    // place of seq, read as stored (big endian), so its two words need no swap
    u32 nw1 = bswap32((u32)(r.seq >> 32)), nw2 = bswap32((u32)r.seq);
    if (TLS12) {
        const uint8_t *e = args.in + r.in_off + (OPEN ? TLS_HEADER_SIZE : 0);
        nw1 = *(const u32_u *)e;
        nw2 = *(const u32_u *)(e + 4);
    }
    const u32 n0 = iv0 ^ rk[0][0];
    const u32 n1 = iv1 ^ nw1 ^ rk[0][1];
    const u32 n2 = iv2 ^ nw2 ^ rk[0][2];
    // (a QUIC packet's AAD is its header in the clear: the seal's input, or what the open's pre-pass left in the output)
    constexpr bool QUIC = FRAME == 3;
    const uint8_t *aadp = QUIC         ? (OPEN ? (const uint8_t *)args.out + r.out_off : args.in + r.in_off)
                          : OPEN_FRAME ? args.in + r.in_off
                                       : args.aad + r.aad_off;

    acc = u32x4{0, 0, 0, 0};

    CtrCache1 cc1 = {};  // (the counter cache runs one block per lane and step)
    u32 cc1_key = 0xffffffffu;  // counter >> 8 of the cached window (none yet)

    // data block of lane j at step m: b = j + G*m - P - na; a full 16-byte input block is loaded one step ahead, so
    // its HBM latency hides under the AES of the current step
    auto full_block = [&](u32 m, int &b) -> bool {
        b = (int)(j + G * m) - P - (int)na;
        return m < m_hi && b >= 0 && b < (int)nb && Lsrc - 16u * (u32)b >= 16;
    };
    // (a loop of one trip, what the loop over the blocks of a step left: written as a plain block, the compiler nests
    // the load's branches and every kernel's code changes)
    u32x4 nxt = {0, 0, 0, 0};
    for (int i = 0; i < 1; ++i) {
        int b;
        if (full_block(m_lo, b))
            nxt = *(const u32x4_u *)(src + 16u * (u32)b);
    }

    // step m, part 1: the next step's input prefetch and this step's counter block (refreshing the counter cache when
    // the lane enters a new 256-counter window). (Round 5: the W8 kernels' unframed steps outside the steady range as one
    // pass, the non-text inputs loaded ahead of the AES, measured within +-0.5 % of these two parts on quic1200 and
    // mixed, profiles/r5/g4_ab.txt, and was not kept.)
    u32x4 cur;
    auto setup_step = [&](u32 m0, u32 (&st)[1][4], bool wave_ks) {
        cur = nxt;
        int bn;
        if (full_block(m0 + 1, bn))
            nxt = *(const u32x4_u *)(src + 16u * (u32)bn);
        // AES-CTR input: data positions encrypt counter 2+b, all others J0 (kept by the length lane as E(K, J0))
        const int logical = (int)(j + G * m0) - P;
        const int b = logical - (int)na;
        const bool is_data = m0 < m_hi && logical >= (int)na && b < (int)nb;
        st[0][0] = n0, st[0][1] = n1, st[0][2] = n2;
        const u32 ctr = is_data ? (u32)(b + 2) : 1u;
        st[0][3] = bswap32(ctr) ^ rk[0][3];
        if (wave_ks && (ctr >> 8) != cc1_key) {  // entering a new 256-counter window (divergent; skipped when no lane does)
            cc1 = ctr_cache1_init<NR>(lds, laneoff, rk, n0, n1, n2, st[0][3]);
            cc1_key = ctr >> 8;
        }
    };
    // step m, part 2: with the keystream block ks, write the output and return the GHASH input block X of position
    // j + G*m
    auto finish_step = [&](u32 m, const u32x4 &ks) -> u32x4 {
        const bool act = m < m_hi;
        const int logical = (int)(j + G * m) - P;
        const int b = logical - (int)na;
        const bool is_data = act && logical >= (int)na && b < (int)nb;
        const bool is_aad = act && logical >= 0 && logical < (int)na;
        const bool is_len = act && logical == (int)(na + nb);
        u32x4 X = {0, 0, 0, 0};
        // steady state: every active lane of the wave holds a full 16-byte text block (one uniform branch, no
        // per-case dispatch)
        const bool full = is_data && Lsrc - 16u * (u32)b >= 16;
        if (__all(!act || full)) {
            const u32x4 o = cur ^ ks;
            if (act)
                SEG_PUT(dst + 16u * (u32)b, o);
            return OPEN ? cur : o;
        }
        if (is_data) {
            const u32 rem = L - 16u * (u32)b;
            uint8_t *op = dst + 16u * (u32)b;
            if (rem >= 16 && (!SEAL_FRAME || Lsrc - 16u * (u32)b >= 16)) {
                const u32x4 v = cur;
                const u32x4 o = v ^ ks;
                SEG_PUT(op, o);
                X = OPEN ? v : o;
            } else {
                const u32 srem = Lsrc - 16u * (u32)b;
                u32x4 v = load_partial(src + 16u * (u32)b, srem);
                if (SEAL_FRAME)  // the inner content type follows the payload
                    v[srem >> 2] |= (u32)(r.flags & 0xffu) << (8 * (srem & 3));
                const u32x4 o = rem >= 16 ? v ^ ks : mask_tail(v ^ ks, rem);
                if (rem >= 16)
                    SEG_PUT(op, o);
                else if (!HDR || wr)
                    store_partial(op, o, rem);
                X = OPEN ? v : o;
            }
        } else if (is_aad) {
            if (SEAL_FRAME) {  // the record header: built here, written to the wire, and authenticated
                const u32 wl = L + 16;
                X = u32x4{0x00030317u | ((wl >> 8) & 0xffu) << 24, wl & 0xffu, 0, 0};
                store_partial(args.out + r.out_off, X, TLS_HEADER_SIZE);
            } else if (TLS12) {  // AAD = BE64(seq) || type || 3 || 3 || BE16(len) (build_tls12_aad)
                const u32 type = OPEN ? (u32)args.in[r.in_off] : (r.flags & 0xffu);
                X = u32x4{bswap32((u32)(r.seq >> 32)), bswap32((u32)r.seq), type | 0x030300u | ((L >> 8) & 0xffu) << 24,
                          L & 0xffu};
                if (!OPEN) {  // the wire header and the explicit nonce
                    const u32 wl = TLS12_RECORD_IV_SIZE + L + 16;
                    const u32x4 h = {type | 0x030300u | ((wl >> 8) & 0xffu) << 24, (wl & 0xffu) | nw1 << 8,
                                     nw1 >> 24 | nw2 << 8, nw2 >> 24};
                    store_partial(args.out + r.out_off, h, TLS_HEADER_SIZE + TLS12_RECORD_IV_SIZE);
                }
            } else {
                const u32 rem = A - 16u * (u32)logical;
                const uint8_t *ap = aadp + 16u * (u32)logical;
                X = rem >= 16 ? *(const u32x4_u *)ap : load_partial(ap, rem);
            }
        } else if (is_len) {
            // (formed here, not hoisted: the loop-invariant length block was kept live through the loop and spilled)
            u32 Ah = A, Lh = L;
            asm volatile("" : "+v"(Ah), "+v"(Lh));
            const u64 abits = (u64)Ah * 8, cbits = (u64)Lh * 8;
            X[0] = bswap32((u32)(abits >> 32));
            X[1] = bswap32((u32)abits);
            X[2] = bswap32((u32)(cbits >> 32));
            X[3] = bswap32((u32)cbits);
            // (E(K, J0) kept in LDS until after the loop: live through it, it was spilled)
            *(lds_u32x4 *)(const_cast<lds_u8 *>(lds) + ekslot) = ks;
        }
        return X;
    };

    // Steady state: the steps [sa, sb) (relative to m_lo, wave-uniform) in which every lane of every group of the wave
    // holds a full text block, the next step's block is full too (the prefetch needs no check) and no group is at its
    // segment's last step (Horner with H^G throughout). They run without the per-lane position logic: the counter,
    // source and destination just advance by one step, about 30 VALU operations fewer per block.
    const int D0 = P + (int)na;         // stream position of text block 0
    const int nbf = (int)(Lsrc >> 4);   // full text blocks
    const int ms = (D0 + G - 1) / G;    // first step whose 8 positions are all >= D0
    const int me = nbf + D0 >= G ? (nbf + D0 - G) / G : -1;  // last step whose 8 positions are all full text
    int sa = max(ms, (int)m_lo) - (int)m_lo;
    int sb = min(me - 1, m_first_last - 1) + 1 - (int)m_lo;
    if (!valid || m_hi <= m_lo)
        sa = 1, sb = 0;
    sa = wave_smax_perg<G>(sa);
    sb = wave_smin_perg<G>(sb);

    // (round 6, PROGRESS_PRIO) the waves of a SIMD issue by the work they have left in the segment: the one furthest
    // behind first, so that equal claims end together instead of in the issue order's age skew (a run's last wave
    // otherwise finishes alone on its SIMD)
    auto progress_prio = [&](u32 left) {
        if constexpr (TREE_PRIO_BAND && W8) {
            if (w8tree) {
                const u32 q = left / TREE_PRIO_BAND;
                const u32 lvl = q >= 3 ? 3u : q;
                if (lvl == 3)
                    __builtin_amdgcn_s_setprio(3);
                else if (lvl == 2)
                    __builtin_amdgcn_s_setprio(2);
                else if (lvl == 1)
                    __builtin_amdgcn_s_setprio(1);
                else
                    __builtin_amdgcn_s_setprio(0);
                return;
            }
        }
        if constexpr (PROGRESS_PRIO && W8) {
            if (w8tree)  // (the tree kernel's long whole runs take TREE_PRIO_BAND above: bands of 4 measured -2.3 %)
                return;
            if (left > 3u * PROGRESS_PRIO)
                __builtin_amdgcn_s_setprio(3);
            else if (left > 2u * PROGRESS_PRIO)
                __builtin_amdgcn_s_setprio(2);
            else if (left > 1u * PROGRESS_PRIO)
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
    };
#if ENGINE_PROFILE
    const unsigned long long tsg1 = stamp();
    unsigned long long tsteady = 0;
#endif
    for (u32 s0 = 0; s0 < Smax; ++s0) {
        progress_prio(Smax - s0);
        if ((int)s0 == sa && sb > sa) {
#if ENGINE_PROFILE
            const unsigned long long tst0 = stamp();
#endif
            const int b0 = (int)(j + G * (m_lo + (u32)sa)) - D0;  // this lane's text block at step sa
            u32 off = 16u * (u32)b0;                               // its byte offset in the text
            u32 ctr = (u32)b0 + 2;
            // PAIR (a 4-lane seal): the block held from the previous step (the first half of its line), stored with this
            // one. Half lines stored a step apart leave the L2 as two write-backs of the line (tools/mb/wcal.hip:
            // 1.07-1.08x the bytes; paired, 1.00x)
            constexpr bool LINE = OPEN && G == 4;
            constexpr bool PAIR = G == 4 && !LINE;
            u32x4 held = {0, 0, 0, 0};
            bool have = false;
            // LINE (a 4-lane open, its steps aligned to the text, not to the output): held = the lane's block
            // in a line's first half, held2 its block in the second half (the next step's). The line is whole at the
            // second half's step, or one step later for a lane past its first half's line offset ("late": j >
            // (dst + off) / 16 mod 4, the line's last block falls in the next step); then the lane stores both. Late
            // lanes store from dst - 64, so both kinds store at p - 64 and p
            u32x4 held2 = {0, 0, 0, 0};
            bool late = false;
            uint8_t *dst_l = dst;
            if constexpr (LINE) {
                late = j > (((u32)(uintptr_t)(dst + off) >> 4) & 3u);
                dst_l = dst - (late ? 64 : 0);
            }
            // pair8: an 8-lane group whose steps straddle lines (a cut run's unit, counted from the stream's end) --
            // the lanes past the line boundary (the same lanes every step) hold their blocks one step, so each line is
            // stored by one step's instructions; uniform over the wave: no lane straddles in an aligned stream
            const bool holder = G == 8 && ((u32)(uintptr_t)(dst + off) & 127u) < 16u * j;
            // (unframed batches: the TLS-framed kernels measured slower with it, TLS 1.2 1200-byte seal -1.4 %)
            const bool pair8 = G == 8 && W8 && FRAME == 0 && !aligned && __any(holder);
            for (int s = sa; s < sb; ++s) {
                if ((s & 3) == 0)
                    progress_prio(Smax - (u32)s);
                cur = nxt;
                nxt = *(const u32x4_u *)(src + off + 16 * G);
                u32 st[1][4] = {{n0, n1, n2, bswap32(ctr) ^ rk[0][3]}};
                if ((ctr >> 8) != cc1_key) {
                    cc1 = ctr_cache1_init<NR>(lds, laneoff, rk, n0, n1, n2, st[0][3]);
                    cc1_key = ctr >> 8;
                }
                aes_ctr_cached1<NR>(lds, laneoff, rk, cc1, st);
                __builtin_amdgcn_sched_barrier(0);
                const u32x4 o = cur ^ u32x4{st[0][0], st[0][1], st[0][2], st[0][3]};
                if constexpr (LINE) {
                    const bool first = (((u32)(uintptr_t)(dst + off)) & 64u) == 0;
                    if (!first)
                        held2 = o;
                    if (first == late) {  // the held line is whole at this step (held from inside the range only)
                        uint8_t *p = dst_l + off;
                        if (s >= sa + 1 + (int)late)
                            SEG_PUT(p - 64, held);
                        if (!late || s > sa)
                            SEG_PUT(p, held2);
                    }
                    if (first)
                        held = o;
                } else if constexpr (PAIR) {
                    if ((((uintptr_t)(dst + off)) & 64u) == 0 && s + 1 < sb) {
                        held = o;
                        have = true;
                    } else {
                        if (have)
                            *(u32x4_u *)(dst + off - 16 * G) = held;
                        *(u32x4_u *)(dst + off) = o;
                        have = false;
                    }
                } else if (pair8) {
                    if (have)
                        *(u32x4_u *)(dst + off - 16 * G) = held;
                    have = holder && s + 1 < sb;
                    if (have)
                        held = o;
                    else
                        *(u32x4_u *)(dst + off) = o;
                } else {
                    SEG_PUT(dst + off, o);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (W8)
                    acc = horner(acc ^ (OPEN ? cur : o));
                else
                    acc = gmul_tab(lds, acc ^ (OPEN ? cur : o), tsel_horner);
                __builtin_amdgcn_sched_barrier(0);
                ctr += G;
                off += 16 * G;
            }
            if constexpr (LINE) {  // the blocks still held after the range's last step
                uint8_t *p = dst + off - 16 * G;
                if ((((u32)(uintptr_t)p) & 64u) == 0) {
                    SEG_PUT(p, held);
                } else if (late) {
                    SEG_PUT(p, held2);
                    if (sb - 1 > sa)
                        SEG_PUT(p - 64, held);
                }
            }
            s0 = (u32)sb;  // (a block in the range's last step is stored at once: nothing is held past it)
#if ENGINE_PROFILE
            tsteady += stamp() - tst0;
#endif
        }
        const u32 m0 = m_lo + s0;
        // (round 5) a step in which no lane of the wave holds a text or length position (front padding and AAD only:
        // the first step of 4-lane groups on short records) needs no keystream and skips the AES; the lengths decide
        // it, not the data
        const int lg = (int)(j + G * m0) - P;
        // (4-lane groups, and the 8-lane groups of the EXT 3 kernel's long whole records, w8tree: an aligned open of
        // records with one AAD block starts every record with such a step, and so does the seal's wave whose records
        // share that padding; in the other 8-lane kernels such a step is rare, and the test cost the TLS 1.3 open
        // kernel spills, as it does EXT 3's TLS 1.2 seal: 16 bytes a lane)
        const bool wave_ks = (G != 4 && !(w8tree && !TLS12)) || __any(m0 < m_hi && lg >= (int)na && lg <= (int)(na + nb)) != 0;
        u32 st[1][4];
        setup_step(m0, st, wave_ks);
        if (wave_ks)
            aes_ctr_cached1<NR>(lds, laneoff, rk, cc1, st);
        __builtin_amdgcn_sched_barrier(0);
        const u32x4 X = finish_step(m0, u32x4{st[0][0], st[0][1], st[0][2], st[0][3]});
        // scheduling fence: keeps the 32 table loads of this fold from being hoisted next to the other work (that
        // hoisting spills them to scratch)
        __builtin_amdgcn_sched_barrier(0);
        const bool last_here = (int)m0 == m_last;
        // every lane multiplies by H^G, the uniform Horner table, except at its last position, which takes its power
        // H^e_last after the loop (coop_last_powers, w8_lane_end); in the wave's last step no lane needs the multiply
        const u32x4 t = acc ^ X;
        u32x4 prod = t;
        if (s0 + 1 < Smax) {
            if constexpr (W8)
                prod = horner(t);
            else
                prod = gmul_tab(lds, t, tsel_horner);
            if (last_here)
                prod = t;
        }
        if ((int)m0 <= m_last)
            acc = prod;
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr ((PROGRESS_PRIO != 0 || TREE_PRIO_BAND != 0) && W8)
        __builtin_amdgcn_s_setprio(0);
#if ENGINE_PROFILE
    const unsigned long long tsg2 = stamp();
#endif

    static_assert(G == 8 || W8, "dpp_xor8 reduces groups of 8 lanes");
    // (round 5) an open's received tag is loaded before the segment end, whose lookups hide its latency (loaded after
    // it, the wave waited for it at every record's end: 2.3 % of the 1200-byte open)
    u32x4 rt = {0, 0, 0, 0};
    if (OPEN && finish && valid && j == jl)
        rt = *(const u32x4_u *)(src + L);
    if constexpr (W8) {
        // sum over the group of a_l H^(e_l) (rank r = 8 - e owes H^(8 - r)): ((v_0 H + v_1) H + ... + v_7) H by eight
        // group multiplies with the one window-major table H (4 conflict-free lookups per lane each: 32, as
        // coop_last_powers, with one table instead of seven)
        // (the EXT 3 kernel's long whole records too: its butterfly over the ranks with H and H^2 nibble-major, 160
        // lookups a lane for three short levels, measured behind this chain once its waves were dealt records of one
        // padding and issued in priority bands -- tls16k -0.9 %, profiles/long_deal_ab.txt -- and is gone)
        const u32 rank = valid ? (u32)G - e_last : j;
        if constexpr (G == 4)
            acc = w8_lane_end4(lds, acc, lane_here(), rank, MK4 ? mk_htab(mk_kslot) : (u32)W8_TAB_H);
        else
            acc = w8_lane_end(lds, acc, lane_here(), rank);
        if (valid && m_hi * G >= N && j == jl)  // the segment holds the length block: E(K, J0), on its lane
            acc ^= u32x4(*(const lds_u32x4 *)(lds + ekslot));
    } else {
        // the lanes' powers H^(e_last - 1), conflict-free (ghash.h); ranks rotated by N mod 8
        const u32 rank = valid ? (u32)G - e_last : j;
        acc = coop_last_powers(lds, acc, lane_here(), (j - rank) & (G - 1));
        // XOR over the G lanes of the group
#pragma unroll
        for (int c = 0; c < 4; ++c)
            acc[c] = dpp_xor8(acc[c]);
        acc = gmul_group_w(lds, acc, LDS_AES_BYTES, lane_here());  // the group's sum times H (table 0, window-major)
        if (valid && m_hi * G >= N && j == jl)  // the segment holds the length block: E(K, J0), on its lane
            acc ^= u32x4(*(const lds_u32x4 *)(lds + ekslot));
    }
    // whole record (finish): tag = GHASH ^ E(K, J0), written after the ciphertext (seal) or compared with the
    // received one (open)
    okw = 2;
    if (finish && valid && j == jl) {
        const u32x4 tag = acc;
        if (OPEN) {
            const u32x4 d = rt ^ tag;
            okw = (d[0] | d[1] | d[2] | d[3]) == 0;
        } else {
            *(u32x4_u *)(dst + L) = tag;
        }
    }
#if ENGINE_PROFILE
    if (W8 && !w8tree && lane_here() == 0) {  // [16] setup, [17] steps, [18] end of the serial W8 kernels' segments, [19] segments
        const unsigned long long tsg3 = stamp();
        PROF_ADD(16, tsg1 - tsg0), PROF_ADD(17, tsg2 - tsg1), PROF_ADD(18, tsg3 - tsg2), PROF_ADD(19, 1);
        // [20] the wave's steps, [21] of them in the steady form
        PROF_ADD(20, Smax), PROF_ADD(21, sb > sa ? (u32)(sb - sa) : 0u), PROF_ADD(22, tsteady);
    }
#endif
}

#undef SEG_PUT

#endif  // PTLS_MI355X_ENGINE_SEGMENT_H
