// picotls_amd/csrc/quic/header.h -- QUIC packet protection's header rules (RFC 9001 §5.4, RFC 9000 A.3), suite-neutral:
// what of the first byte a mask covers, the packet-number length, the admission rules of a seal and an open descriptor,
// the unmasking of first byte and packet number with the packet-number window and the key-phase verdict, and the
// 16-byte result word. The mask itself is the suite's (AES-ECB: engine/aux_kernels.h; a ChaCha20 block:
// chacha/kernels.h). Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (after engine/common.h).
// The contract these state is DESIGN.md §10.6.
#ifndef PTLS_MI355X_QUIC_HEADER_H
#define PTLS_MI355X_QUIC_HEADER_H

// the first byte's protected bits: the low 4 of a long header, the low 5 of a short one
__device__ __forceinline__ u32 quic_first_mask(uint8_t first) { return (first & 0x80) != 0 ? 0x0fu : 0x1fu; }

__device__ __forceinline__ u32 quic_pn_len(uint8_t first) { return (first & 3) + 1; }

// mask[1 .. 4], which go onto the packet-number bytes, from the mask's first two words
__device__ __forceinline__ u32 quic_m14(u32 x0, u32 x1) { return x0 >> 8 | x1 << 24; }

// The admission rules take the keysets' sizes by reference: each is read where its comparison stands, behind the checks
// before it, as in the kernels these rules were written out in (by value, the FRAME 2 seal of chacha_batch_kernel took
// a 129th VGPR and lost a wave of occupancy).
// Open. len: the packet number, the ciphertext and the tag; 4 + 16 of them are the sample's bytes at the least
__device__ __forceinline__ bool quic_open_admits(const ptls_mi355x_record_t &r, const u32 &nkeys, const u32 &hp_nkeys)
{
    return r.len >= 20 && r.len <= PTLS_MI355X_MAX_RECORD_LEN && r.aad_len >= 1 && r.key_idx < nkeys && r.key_idx < hp_nkeys;
}

// Seal, before the first byte is read (aad_len: the header with its packet number, in the clear) ...
__device__ __forceinline__ bool quic_seal_admits(const ptls_mi355x_record_t &r, const u32 &nkeys, const u32 &hp_nkeys)
{
    return r.aad_len >= 2 && r.flags == 0 && r.len <= PTLS_MI355X_MAX_RECORD_LEN && r.key_idx < nkeys && r.key_idx < hp_nkeys;
}

// ... and after: the header holds a byte before the packet number, and packet number and payload cover a sample's first 4 bytes
__device__ __forceinline__ bool quic_seal_admits_pn(const ptls_mi355x_record_t &r, u32 pn_len)
{
    return r.aad_len >= 1 + pn_len && pn_len + r.len >= 4;
}

// RFC 9000 A.3: the candidate in the expected number's window, moved a window up or down when that is closer
__device__ __forceinline__ u64 quic_decode_pn(u64 expect, u32 trunc, u32 pn_len)
{
    const u64 win = 1ull << (8 * pn_len), hwin = win >> 1;
    u64 cand = (expect & ~(win - 1)) | trunc;
    if (cand + hwin <= expect && cand < (1ull << 62) - win)
        cand += win;
    else if (cand > expect + hwin && cand >= win)
        cand -= win;
    return cand;
}

// a short header whose key-phase bit is not the expected one (flags bit 0)
__device__ __forceinline__ bool quic_key_phase_differs(u32 first, u32 flags)
{
    return (first & 0x80) == 0 && ((first >> 2) & 1) != (flags & 1u);
}

struct QuicUnmasked {
    u32 first, pn_len;  // the first byte in the clear, 1 .. 4
    u64 pn;             // the full packet number
    bool phase;         // a short header whose key-phase bit is not the expected one (flags bit 0)
};

// `first` as it arrived, the packet-number bytes at pn, mask[0] and mask[1 .. 4], the expected packet number
// (quic_unmask_kernel, engine/aux_kernels.h, puts the same parts together itself)
__device__ __forceinline__ QuicUnmasked quic_unmask(u32 first, const uint8_t *pn, u32 mask0, u32 m14, u64 expect, u32 flags)
{
    first ^= mask0 & quic_first_mask(first);
    const u32 pn_len = quic_pn_len(first);
    u32 trunc = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        if (k < pn_len)
            trunc = trunc << 8 | (((u32)pn[k] ^ (m14 >> (8 * k))) & 0xff);
    }
    return QuicUnmasked{first, pn_len, quic_decode_pn(expect, trunc, pn_len), quic_key_phase_differs(first, flags)};
}

// ptls_mi355x_quic_result_t as one 16-byte word: pn low, pn high, payload_len, pn_len | first_byte << 8 | status << 16.
// Rejected: that status and nothing else, {0, 0, 0, QUIC_RESULT_REJECTED_W} (also what a lane without a packet starts from)
#define QUIC_RESULT_REJECTED_W ((u32)PTLS_MI355X_QUIC_REJECTED << 16)
__device__ __forceinline__ u32x4 quic_result_rejected() { return u32x4{0, 0, 0, QUIC_RESULT_REJECTED_W}; }

// (status OK until the tag check, which writes the status byte alone)
__device__ __forceinline__ u32x4 quic_result_pack(const QuicUnmasked &u, u32 payload_len)
{
    return u32x4{(u32)u.pn, (u32)(u.pn >> 32), payload_len,
                 u.pn_len | u.first << 8 | (u32)(u.phase ? PTLS_MI355X_QUIC_KEY_PHASE : PTLS_MI355X_QUIC_OK) << 16};
}

// the word's fields, as the FRAME 2 open of chacha_batch_kernel reads them back. (The load with its rejected default
// stands in that kernel: behind a function, or with quic_result_rejected() for the default, the kernel's registers are
// numbered anew through the whole record, which an unchanged kernel is not worth.)
__device__ __forceinline__ u64 quic_result_pn(u32x4 q) { return (u64)q.x | (u64)q.y << 32; }
__device__ __forceinline__ u32 quic_result_payload_len(u32x4 q) { return q.z; }
__device__ __forceinline__ u32 quic_result_pn_len(u32x4 q) { return q.w & 0xff; }
__device__ __forceinline__ u32 quic_result_first(u32x4 q) { return (q.w >> 8) & 0xff; }
__device__ __forceinline__ u32 quic_result_status(u32x4 q) { return (q.w >> 16) & 0xff; }

#endif  // PTLS_MI355X_QUIC_HEADER_H
