/*
 * picotls/mi355x_chacha20_picotls.h -- picotls algorithm objects backed by the MI355X ChaCha20-Poly1305 engine
 * (libptls_mi355x_picotls.so).
 *
 * Drop-in counterparts of ptls_openssl_chacha20 / ptls_openssl_chacha20poly1305 (include/picotls/openssl.h,
 * lib/openssl.c:2524-2555): same names, key / IV / tag sizes, limits and TLS 1.2 IV sizes {12, 0}; the AEAD's ctr_cipher
 * is the ChaCha20 object and its ecb_cipher is NULL. Every callback of ptls_aead_context_t is implemented on the GPU
 * engine as a batch of one; the deprecated do_encrypt_init / update / final are NULL. The ChaCha20 cipher object serves
 * QUIC header protection: ptls_cipher_init with the 16-byte IV (counter || nonce), then one ptls_cipher_encrypt of up to
 * 16 bytes. Use the batch entry points of picotls/mi355x_chacha20.h for throughput.
 */
#ifndef picotls_mi355x_chacha20_picotls_h
#define picotls_mi355x_chacha20_picotls_h

#include "picotls.h" /* from the picotls installation (-I <picotls>/include) */
#include "mi355x_chacha20.h"

#ifdef __cplusplus
extern "C" {
#endif

extern ptls_cipher_algorithm_t ptls_mi355x_chacha20;
extern ptls_aead_algorithm_t ptls_mi355x_chacha20poly1305;

/**
 * Returns the engine keyset behind an AEAD context created from ptls_mi355x_chacha20poly1305 (key index 0), so that a
 * caller can move from per-record calls to ptls_mi355x_chacha_seal_batch / _open_batch on the same traffic key.
 */
ptls_mi355x_chacha_keyset_t *ptls_mi355x_chacha_aead_get_keyset(ptls_aead_context_t *ctx);

#ifdef __cplusplus
}
#endif

#endif
