/*
 * picotls/mi355x_quic.h -- QUIC packet protection under AES-GCM for the MI355X (gfx950) record engine: the AEAD and the
 * header protection of a batch of packets in one call, the AES-GCM form of ptls_mi355x_chacha_seal_quic_packets /
 * _open_quic_packets (picotls/mi355x_chacha20.h). The keysets, the 40-byte descriptors, the suite-neutral result type
 * ptls_mi355x_quic_result_t and the PTLS_MI355X_QUIC_* codes are those of picotls/mi355x.h; like the ChaCha20 pair, the
 * calls live with their suite, in a header of their own, and in the same libptls_mi355x.so.
 */
#ifndef picotls_mi355x_quic_h
#define picotls_mi355x_quic_h

#include <stddef.h>

#include "picotls/mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/**
 * QUIC packet protection under AES-GCM (RFC 9001 §5.3-5.4), batched: the AEAD and the header protection of a packet in
 * one call, asynchronous on `stream`. The contract is that of the ChaCha20 pair (picotls/mi355x_chacha20.h), with the
 * mask of ptls_mi355x_hp_mask_batch, AES-ECB(hp key, sample). Descriptors are ptls_mi355x_record_t; key_idx selects the
 * AEAD key in ks and the header-protection key in hp_ks (an AES keyset on ks's device whose IVs are unused; it may be ks
 * itself, and its key size may differ from ks's); aad_off is ignored. Packets may sit at any byte offset (offsets are
 * the 64-bit in_off / out_off), out_off == in_off on one arena (in place) is allowed, and nothing is read or written
 * outside a packet's own bytes.
 *
 * seal: in + in_off holds the cleartext packet, a header of aad_len bytes followed by len payload bytes. The last
 * pn_len = (header[0] & 3) + 1 header bytes are the truncated packet number as it goes on the wire, seq is the full
 * packet number (nonce = static IV ^ BE64(seq)), flags must be 0. out + out_off receives aad_len + len + 16 bytes:
 * protected header || ciphertext || tag. The AAD is the cleartext header; the 16-byte sample starts at packet offset
 * aad_len - pn_len + 4 (it may reach into the tag), the first byte takes mask[0] & 0x1f (short header, bit 7 clear) or
 * & 0x0f (long header) and pn byte i takes mask[1 + i].
 * Rejected (nothing written): aad_len < 1 + pn_len, pn_len + len < 4 (no full sample, RFC 9001 §5.4.2), key_idx not
 * below both keysets' sizes, len above PTLS_MI355X_MAX_RECORD_LEN, flags != 0.
 *
 * open: in + in_off holds the protected packet, aad_len is the offset of its packet-number field (>= 1) and len the
 * number of bytes from there to the packet's end (pn || ciphertext || tag; len >= 20, else rejected). seq is the
 * expected packet number (the largest processed in the packet-number space, plus 1), from which the full number is
 * reconstructed as in RFC 9000 A.3; flags bit 0 is the expected key phase (short headers only). out + out_off receives
 * the unprotected header (aad_len + pn_len bytes) || plaintext. ok[i] = 1 only when the packet authenticated;
 * results[i] gives the packet number, the lengths, the unprotected first byte and a PTLS_MI355X_QUIC_* status. A short
 * header whose key-phase bit differs from the expected one gets KEY_PHASE and ok = 0 and is not decrypted (nothing is
 * written for it): the caller resubmits it under the other key generation. On BAD_MAC the bytes in out, within the
 * packet's own output region, are unspecified. ok and results are both required.
 *
 * Three launches on `stream` each, no host work between them: a pre-pass over the descriptors (open: the header
 * unmasking of every packet), the batch, and a finish (seal: the header protection; open: the statuses).
 * Return 0 on success (an empty batch touches nothing), a negative value on invalid arguments or launch failure.
 */
int ptls_mi355x_seal_quic_packets(ptls_mi355x_keyset_t *ks, ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_record_t *recs,
                                  size_t nrecs, const void *in, void *out, void *stream);
int ptls_mi355x_open_quic_packets(ptls_mi355x_keyset_t *ks, ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_record_t *recs,
                                  size_t nrecs, const void *in, void *out, uint8_t *ok, ptls_mi355x_quic_result_t *results,
                                  void *stream);

#ifdef __cplusplus
}
#endif

#endif
