/*
 * picotls_amd/csrc/ptls_mi355x_chacha20.c -- the picotls plugin objects for the MI355X ChaCha20-Poly1305 engine.
 *
 * Counterparts of ptls_openssl_chacha20 / ptls_openssl_chacha20poly1305 (lib/openssl.c:2524-2555; the AEAD construction
 * of lib/chacha20poly1305.h:51-145) on top of include/picotls/mi355x_chacha20.h, in the manner of ptls_mi355x.c:
 *   setup_crypto     key == NULL: IV-only update; callbacks; one engine keyset of one key per context
 *   do_encrypt       -> ptls_mi355x_chacha_encrypt, then the supplementary (header protection) block as
 *                       ptls_aead__do_encrypt does (include/picotls.h:2136-2146)
 *   do_encrypt_v     -> ptls_mi355x_chacha_encrypt_v
 *   do_decrypt       -> ptls_mi355x_chacha_decrypt (SIZE_MAX leaves the output untouched)
 *   do_get_iv/set_iv -> the context's copy / ptls_mi355x_chacha_keyset_set_iv
 *   ctr cipher       ChaCha20 with picotls' 16-byte IV (counter || nonce); like the engine's AES-CTR objects it serves
 *                    QUIC header protection: one transform of up to 16 bytes per init
 * The deprecated do_encrypt_init / update / final are NULL, as in the AES-GCM objects.
 *
 * Failure behaviour as in ptls_mi355x.c: a seal the engine cannot complete zeroes its whole output (fail closed), a
 * cipher that cannot produce its keystream aborts, decrypt reports SIZE_MAX.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "picotls/mi355x_chacha20_picotls.h"

static void chacha_fatal(const char *what)
{
    fprintf(stderr, "picotls MI355X engine: %s failed: %s\n", what, ptls_mi355x_last_error());
    abort();
}

struct mi355x_chacha_aead_context {
    ptls_aead_context_t super;
    ptls_mi355x_chacha_keyset_t *ks;
    uint8_t static_iv[PTLS_CHACHA20POLY1305_IV_SIZE];
};

struct mi355x_chacha_ctr_context {
    ptls_cipher_context_t super;
    ptls_mi355x_chacha_keyset_t *ks;
    uint8_t bits[16];
    int is_ready;
};

/* ------------------------------------------------------------------ ChaCha20 (<= 16 bytes per init) */

static void chacha20_dispose(ptls_cipher_context_t *_ctx)
{
    struct mi355x_chacha_ctr_context *ctx = (struct mi355x_chacha_ctr_context *)_ctx;
    ptls_mi355x_chacha_keyset_free(ctx->ks);
    ptls_clear_memory(ctx->bits, sizeof(ctx->bits));
}

static void chacha20_init(ptls_cipher_context_t *_ctx, const void *iv)
{
    struct mi355x_chacha_ctr_context *ctx = (struct mi355x_chacha_ctr_context *)_ctx;
    if (ptls_mi355x_chacha_hp_mask(ctx->ks, 0, ctx->bits, iv) != 0)
        chacha_fatal("ChaCha20 keystream");
    ctx->is_ready = 1;
}

static void chacha20_transform(ptls_cipher_context_t *_ctx, void *output, const void *input, size_t len)
{
    struct mi355x_chacha_ctr_context *ctx = (struct mi355x_chacha_ctr_context *)_ctx;
    if (!(ctx->is_ready && len <= 16))
        chacha_fatal("ChaCha20 transform (supported once per init, up to 16 bytes)");
    ctx->is_ready = 0;
    const uint8_t *in = input;
    uint8_t *out = output;
    for (size_t i = 0; i < len; ++i)
        out[i] = in[i] ^ ctx->bits[i];
}

static int chacha20_setup(ptls_cipher_context_t *_ctx, int is_enc, const void *key)
{
    (void)is_enc; /* a stream cipher is its own inverse */
    struct mi355x_chacha_ctr_context *ctx = (struct mi355x_chacha_ctr_context *)_ctx;
    static const uint8_t zero_iv[PTLS_CHACHA20POLY1305_IV_SIZE] = {0};
    if ((ctx->ks = ptls_mi355x_chacha_keyset_new(key, zero_iv, 1)) == NULL)
        return PTLS_ERROR_LIBRARY;
    ctx->super.do_dispose = chacha20_dispose;
    ctx->super.do_init = chacha20_init;
    ctx->super.do_transform = chacha20_transform;
    ctx->is_ready = 0;
    return 0;
}

/* ------------------------------------------------------------------ ChaCha20-Poly1305 */

static void chachapoly_dispose_crypto(ptls_aead_context_t *_ctx)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    ptls_mi355x_chacha_keyset_free(ctx->ks);
    ctx->ks = NULL;
    ptls_clear_memory(ctx->static_iv, sizeof(ctx->static_iv));
}

static void chachapoly_get_iv(ptls_aead_context_t *_ctx, void *iv)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    memcpy(iv, ctx->static_iv, sizeof(ctx->static_iv));
}

static void chachapoly_set_iv(ptls_aead_context_t *_ctx, const void *iv)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    memcpy(ctx->static_iv, iv, sizeof(ctx->static_iv));
    /* a wrong IV on the device would seal under a nonce the caller did not ask for: nothing safe to return */
    if (ptls_mi355x_chacha_keyset_set_iv(ctx->ks, 0, iv) != 0)
        chacha_fatal("set_iv");
}

static void chachapoly_encrypt(ptls_aead_context_t *_ctx, void *output, const void *input, size_t inlen, uint64_t seq,
                               const void *aad, size_t aadlen, ptls_aead_supplementary_encryption_t *supp)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    if (ptls_mi355x_chacha_encrypt(ctx->ks, 0, output, input, inlen, seq, aad, aadlen) != 0) {
        /* a seal that did not happen leaves zeros, never plaintext or a partial result */
        memset(output, 0, inlen + PTLS_CHACHA20POLY1305_TAG_SIZE);
        if (supp != NULL)
            memset(supp->output, 0, sizeof(supp->output));
        return;
    }
    if (supp != NULL) {
        /* the sample may point into the freshly written ciphertext, so it is read only now (include/picotls.h:446-449) */
        supp->ctx->do_init(supp->ctx, supp->input);
        memset(supp->output, 0, sizeof(supp->output));
        supp->ctx->do_transform(supp->ctx, supp->output, supp->output, sizeof(supp->output));
    }
}

static void chachapoly_encrypt_v(ptls_aead_context_t *_ctx, void *output, ptls_iovec_t *input, size_t incnt, uint64_t seq,
                                 const void *aad, size_t aadlen)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    if (ptls_mi355x_chacha_encrypt_v(ctx->ks, 0, output, (const ptls_mi355x_iovec_t *)input, incnt, seq, aad, aadlen) != 0) {
        size_t total = 0;
        for (size_t i = 0; i < incnt; ++i)
            total += input[i].len;
        memset(output, 0, total + PTLS_CHACHA20POLY1305_TAG_SIZE);
    }
}

static size_t chachapoly_decrypt(ptls_aead_context_t *_ctx, void *output, const void *input, size_t inlen, uint64_t seq,
                                 const void *aad, size_t aadlen)
{
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;
    if (inlen < PTLS_CHACHA20POLY1305_TAG_SIZE)
        return SIZE_MAX;
    return ptls_mi355x_chacha_decrypt(ctx->ks, 0, output, input, inlen, seq, aad, aadlen);
}

static int chachapoly_setup(ptls_aead_context_t *_ctx, int is_enc, const void *key, const void *iv)
{
    (void)is_enc; /* one context type serves both directions */
    struct mi355x_chacha_aead_context *ctx = (struct mi355x_chacha_aead_context *)_ctx;

    memcpy(ctx->static_iv, iv, sizeof(ctx->static_iv));
    if (key == NULL)
        return 0;

    if ((ctx->ks = ptls_mi355x_chacha_keyset_new(key, iv, 1)) == NULL)
        return PTLS_ERROR_LIBRARY;
    ctx->super.dispose_crypto = chachapoly_dispose_crypto;
    ctx->super.do_get_iv = chachapoly_get_iv;
    ctx->super.do_set_iv = chachapoly_set_iv;
    ctx->super.do_encrypt_init = NULL;
    ctx->super.do_encrypt_update = NULL;
    ctx->super.do_encrypt_final = NULL;
    ctx->super.do_encrypt = chachapoly_encrypt;
    ctx->super.do_encrypt_v = chachapoly_encrypt_v;
    ctx->super.do_decrypt = chachapoly_decrypt;
    return 0;
}

ptls_mi355x_chacha_keyset_t *ptls_mi355x_chacha_aead_get_keyset(ptls_aead_context_t *ctx)
{
    return ((struct mi355x_chacha_aead_context *)ctx)->ks;
}

ptls_cipher_algorithm_t ptls_mi355x_chacha20 = {"CHACHA20", PTLS_CHACHA20_KEY_SIZE, 1, PTLS_CHACHA20_IV_SIZE,
                                                sizeof(struct mi355x_chacha_ctr_context), chacha20_setup};
ptls_aead_algorithm_t ptls_mi355x_chacha20poly1305 = {"CHACHA20-POLY1305",
                                                      PTLS_CHACHA20POLY1305_CONFIDENTIALITY_LIMIT,
                                                      PTLS_CHACHA20POLY1305_INTEGRITY_LIMIT,
                                                      &ptls_mi355x_chacha20,
                                                      NULL,
                                                      PTLS_CHACHA20_KEY_SIZE,
                                                      PTLS_CHACHA20POLY1305_IV_SIZE,
                                                      PTLS_CHACHA20POLY1305_TAG_SIZE,
                                                      {PTLS_TLS12_CHACHAPOLY_FIXED_IV_SIZE, PTLS_TLS12_CHACHAPOLY_RECORD_IV_SIZE},
                                                      0,
                                                      0,
                                                      sizeof(struct mi355x_chacha_aead_context),
                                                      chachapoly_setup};
