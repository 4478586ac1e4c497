/*
 * picotls/mi355x_chacha20.h -- MI355X (gfx950) ChaCha20-Poly1305 record engine for picotls: the C ABI of the second AEAD
 * family picotls negotiates (TLS_CHACHA20_POLY1305_SHA256, the QUIC ChaCha20 header protection, HPKE's
 * PTLS_HPKE_AEAD_CHACHA20POLY1305), beside the AES-GCM engine of picotls/mi355x.h and in the same libptls_mi355x.so.
 *
 * The calls mirror the AES-GCM ones: the same 40-byte ptls_mi355x_record_t descriptors, the same pointer rules (device
 * addresses, streams as void * holding a hipStream_t), the same limits and rejections, the same TLS 1.3 wire layout and
 * result struct. Record i of a batch gives exactly what one picotls call gives:
 *     ptls_mi355x_chacha_seal_batch  record i == ptls_aead_encrypt(ctx[key_idx], out + out_off, in + in_off, len, seq,
 *                                                aad + aad_off, aad_len)      on ptls_openssl_chacha20poly1305
 *                                                (lib/openssl.c:2524-2555, lib/chacha20poly1305.h:51-145)
 *     ptls_mi355x_chacha_open_batch  record i == ptls_aead_decrypt(...) != SIZE_MAX
 * with nonce = static_iv(key_idx) ^ (0^32 || BE64(seq)) (ptls_aead__build_iv, lib/picotls.c:6587).
 *
 * There is no per-key precomputation: a keyset entry is the 32-byte key and the 12-byte static IV, and the Poly1305 key
 * of a record comes from its own keystream block 0. The cipher has no tables and no secret-dependent addresses, so
 * every call is constant-time by construction.
 *
 * The picotls objects (ptls_mi355x_chacha20, ptls_mi355x_chacha20poly1305) are declared in
 * picotls/mi355x_chacha20_picotls.h, which needs picotls.h; this header does not.
 */
#ifndef picotls_mi355x_chacha20_h
#define picotls_mi355x_chacha20_h

#include "picotls/mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTLS_MI355X_CHACHA_KEY_SIZE 32
#define PTLS_MI355X_CHACHA_IV_SIZE 12
#define PTLS_MI355X_CHACHA_TAG_SIZE 16

typedef struct st_ptls_mi355x_chacha_keyset_t ptls_mi355x_chacha_keyset_t;

/**
 * Creates a keyset of nkeys ChaCha20-Poly1305 traffic keys on the current HIP device. keys: nkeys * 32 bytes, ivs:
 * nkeys * 12 bytes, both host memory. The call waits until the arrays have been copied (for its own copy, not for other
 * work on the device). Returns NULL on invalid arguments or device failure.
 */
ptls_mi355x_chacha_keyset_t *ptls_mi355x_chacha_keyset_new(const void *keys, const void *ivs, size_t nkeys);
/**
 * Destroys a keyset. Device key material is cleared in stream order after every launch already made with the keyset,
 * on any stream; the call itself does not wait.
 */
void ptls_mi355x_chacha_keyset_free(ptls_mi355x_chacha_keyset_t *ks);
size_t ptls_mi355x_chacha_keyset_size(const ptls_mi355x_chacha_keyset_t *ks);
/* the HIP device the keyset's entries live on (the current device when it was created) */
int ptls_mi355x_chacha_keyset_device(const ptls_mi355x_chacha_keyset_t *ks);
/**
 * Replaces the key and static IV of the n entries key_idx[0..n) (host arrays: n * 32 key bytes, n * 12 IV bytes).
 * Stream-ordered like ptls_mi355x_keyset_update: launches made with the keyset before the call use the old entries,
 * launches made after it the new ones; the call waits for the keyset's launches in flight and for its own copies.
 * Returns 0, or -1 on invalid arguments / out-of-range or repeated indices (nothing changed) or device failure.
 */
int ptls_mi355x_chacha_keyset_update(ptls_mi355x_chacha_keyset_t *ks, const uint32_t *key_idx, const void *keys, const void *ivs,
                                     size_t n);
/* static IV accessors (do_get_iv / do_set_iv); set_iv is ordered like keyset_update. Return 0 on success. */
int ptls_mi355x_chacha_keyset_get_iv(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *iv);
int ptls_mi355x_chacha_keyset_set_iv(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, const void *iv);

/**
 * Seals / opens nrecs records in one launch, asynchronous on `stream`. Descriptors, pointers, limits and rejections as
 * for ptls_mi355x_seal_batch / ptls_mi355x_open_batch: seal reads len bytes at in + in_off and writes len + 16 bytes
 * (ciphertext || tag) at out + out_off; open reads len + 16 bytes and writes len; in, out and aad may sit at any byte
 * offset, and out_off == in_off on one arena (in place) is allowed. A record whose len or AAD exceeds
 * PTLS_MI355X_MAX_RECORD_LEN / PTLS_MI355X_MAX_AAD_LEN or whose key_idx is not below the keyset size is rejected:
 * nothing is written for it and open reports ok = 0.
 * open: ok[i] = 1 when record i authenticated, 0 otherwise (all 16 tag bytes are compared, without an early exit). The
 * batch open decrypts while it authenticates, so it may leave decrypted bytes in out for a record whose tag fails; the
 * caller must not use them (the per-record ptls_mi355x_chacha_decrypt below never hands them out).
 * Returns 0 on success, a negative value on invalid arguments or launch failure.
 */
int ptls_mi355x_chacha_seal_batch(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                  const void *aad, void *out, void *stream);
int ptls_mi355x_chacha_open_batch(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                  const void *aad, void *out, uint8_t *ok, void *stream);

/**
 * TLS 1.3 record protection, batched: the wire layout, the meaning of len / flags and the results of
 * ptls_mi355x_seal_tls_records / ptls_mi355x_open_tls_records, under ChaCha20-Poly1305. seal: header {23, 3, 3,
 * BE16(len + 17)} || ciphertext of payload || content type (flags & 0xff) || tag at out + out_off, len <= 16384.
 * open: the wire record at in + in_off, recs[i].len = header length field - 16; the header as received is the AAD.
 */
int ptls_mi355x_chacha_seal_tls_records(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs,
                                        const void *in, void *out, void *stream);
int ptls_mi355x_chacha_open_tls_records(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs,
                                        const void *in, void *out, uint8_t *ok, ptls_mi355x_tls_result_t *results, void *stream);

/**
 * QUIC header protection of the ChaCha20 suites, batched: mask[i] (16 bytes at masks + 16 i) = the first 16 keystream
 * bytes of ChaCha20 under key hp[i].key_idx of hp_ks (its IVs are unused), with the 16-byte sample at base + sample_off
 * as picotls' ChaCha20 IV: block counter = the sample's first 4 bytes (little endian), nonce = the other 12
 * (include/picotls.h:95; ptls_cipher_init + ptls_cipher_encrypt of zeros on ptls_openssl_chacha20). A QUIC stack uses
 * 5 of the 16 bytes. Entries with key_idx >= the keyset size get a zero mask.
 */
int ptls_mi355x_chacha_hp_mask_batch(ptls_mi355x_chacha_keyset_t *hp_ks, const ptls_mi355x_hp_t *hp, size_t n, const void *base,
                                     void *masks, void *stream);

/**
 * QUIC packet protection (RFC 9001 §5.3-5.4), batched: the AEAD and the header protection of a packet in one call,
 * asynchronous on `stream`. Descriptors are ptls_mi355x_record_t; key_idx selects the AEAD key in ks and the
 * header-protection key in hp_ks (a keyset whose IVs are unused, on ks's device; it may be ks itself); aad_off is
 * ignored. Packets may sit at any byte offset, out_off == in_off on one arena (in place) is allowed, and nothing is read
 * or written outside a packet's own bytes.
 *
 * seal: in + in_off holds the cleartext packet, a header of aad_len bytes followed by len payload bytes. The last
 * pn_len = (header[0] & 3) + 1 header bytes are the truncated packet number as it goes on the wire, seq is the full
 * packet number (nonce = static IV ^ BE64(seq)), flags must be 0. out + out_off receives aad_len + len + 16 bytes:
 * protected header || ciphertext || tag. The AAD is the cleartext header; the 16-byte sample starts at packet offset
 * aad_len - pn_len + 4 (it may reach into the tag), the mask is that of ptls_mi355x_chacha_hp_mask_batch, the first
 * byte takes mask[0] & 0x1f (short header, bit 7 clear) or & 0x0f (long header) and pn byte i takes mask[1 + i].
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
 * written for it): the caller resubmits it under the other key generation. On BAD_MAC the bytes in out are
 * unspecified. ok and results are both required. Two launches on `stream` (the header unmasking of every packet, then
 * the batch), no host work between them.
 * Return 0 on success, a negative value on invalid arguments or launch failure.
 */
int ptls_mi355x_chacha_seal_quic_packets(ptls_mi355x_chacha_keyset_t *ks, ptls_mi355x_chacha_keyset_t *hp_ks,
                                         const ptls_mi355x_record_t *recs, size_t nrecs, const void *in, void *out, void *stream);
int ptls_mi355x_chacha_open_quic_packets(ptls_mi355x_chacha_keyset_t *ks, ptls_mi355x_chacha_keyset_t *hp_ks,
                                         const ptls_mi355x_record_t *recs, size_t nrecs, const void *in, void *out, uint8_t *ok,
                                         ptls_mi355x_quic_result_t *results, void *stream);

/**
 * Synchronous single-record helpers on HOST buffers (a batch of one through the engine's pinned staging pool); they
 * back the picotls objects and mirror ptls_aead_encrypt / ptls_aead_decrypt. encrypt writes inlen + 16 bytes (output
 * may alias input). decrypt takes inlen = len + 16 and returns the plaintext length, or SIZE_MAX on a tag mismatch,
 * inlen < 16 or an engine error; on SIZE_MAX the caller's output is left untouched (lib/chacha20poly1305.h:140-145).
 */
int ptls_mi355x_chacha_encrypt(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen,
                               uint64_t seq, const void *aad, size_t aadlen);
int ptls_mi355x_chacha_encrypt_v(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const ptls_mi355x_iovec_t *input,
                                 size_t incnt, uint64_t seq, const void *aad, size_t aadlen);
size_t ptls_mi355x_chacha_decrypt(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen,
                                  uint64_t seq, const void *aad, size_t aadlen);
/* one header-protection mask on HOST buffers: mask (16 bytes) from sample (16 bytes) under key key_idx of hp_ks */
int ptls_mi355x_chacha_hp_mask(ptls_mi355x_chacha_keyset_t *hp_ks, size_t key_idx, void *mask, const void *sample);

/**
 * Test and measurement hooks (not the picotls boundary).
 * debug_poly1305: runs the device Poly1305 routine on HOST buffers under the 32-byte one-time key key32 (r || s).
 * debug_force: group_lanes 0 = automatic, else 4 or 16 lanes per record; max_workgroups 0 = automatic, else a cap on
 * the launch grid (small batches then reach every variant and the claim loop). Process-wide.
 * debug_counters: out[0] = launches that ran 4-lane groups, out[1] = 16-lane groups (as seen by workgroup 0). Waits for
 * the device.
 */
int ptls_mi355x_chacha_debug_poly1305(const void *key32, const void *msg, size_t len, void *tag16);
int ptls_mi355x_chacha_debug_force(int group_lanes, int max_workgroups);
int ptls_mi355x_chacha_debug_counters(uint64_t *out, int reset);

/**
 * Spread launches: an unframed batch of few records, and a per-record call with a long record, cut their long records
 * into pieces that groups all over the device seal or open, and the last piece of a record to finish combines the
 * pieces' Poly1305 partials into its tag. A record is cut into at most this many pieces; the piece length is the
 * compiled base length doubled until that holds.
 */
#define PTLS_MI355X_CHACHA_SPREAD_MAX_PIECES 1024
/**
 * debug_spread: piece_bytes 0 = the compiled base piece length, else a multiple of 1024; min_len 0 = the compiled
 * minimum lengths (records from that length are cut), else one value for batches and per-record calls alike; force
 * nonzero = a group width forced with debug_force no longer keeps a batch or a call off the spread kernel. All zeros
 * is automatic. Process-wide.
 * debug_spread_counters: out[0] = spread launches, out[1] = pieces run, out[2] = records whose tag a combine finished,
 * out[3] = whole (uncut) records run in spread launches. Waits for the device.
 * debug_spread_params: out[0] = the minimum length in a batch, out[1] = on the per-record path, out[2] = the largest
 * batch that takes a spread launch (records), out[3] = the base piece length.
 * debug_rpow: r^e mod 2^130 - 5 with the device routine the pieces use, on HOST buffers: r16 = 16 little-endian bytes
 * taken as they are (no clamp), out17 = the fully reduced result as 17 little-endian bytes.
 */
int ptls_mi355x_chacha_debug_spread(int piece_bytes, int min_len, int force);
int ptls_mi355x_chacha_debug_spread_counters(uint64_t *out, int reset);
int ptls_mi355x_chacha_debug_spread_params(uint32_t *out);
int ptls_mi355x_chacha_debug_rpow(const void *r16, uint64_t e, void *out17);

#ifdef __cplusplus
}
#endif

#endif
