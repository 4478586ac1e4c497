/*
 * tests/c/test_chacha_vtable.c -- the ChaCha20-Poly1305 picotls objects of the MI355X engine driven through picotls' own
 * core (ptls_aead_new_direct, ptls_aead_encrypt / _encrypt_v / ptls_aead_decrypt / ptls_aead_xor_iv, ptls_cipher_new /
 * ptls_cipher_init / ptls_cipher_encrypt; lib/picotls.c in oracle/_ref/libtls12_ref.so) side by side with
 * ptls_openssl_chacha20poly1305 / ptls_openssl_chacha20 of the same library. TAP-like output; exit status 1 on failure.
 *
 * The fusion AES-GCM seal also runs once before the engine is first used and again at the end: a reference that changes
 * in the engine's process fails here.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "picotls.h"
#include "picotls/fusion.h"
#include "picotls/openssl.h"
#include "picotls/mi355x_chacha20_picotls.h"

static int ntest, nfail;

#define OK(cond, ...)                                                                                                  \
    do {                                                                                                               \
        ++ntest;                                                                                                       \
        if (cond) {                                                                                                    \
            printf("ok %d - ", ntest);                                                                                 \
        } else {                                                                                                       \
            ++nfail;                                                                                                   \
            printf("not ok %d - ", ntest);                                                                             \
        }                                                                                                              \
        printf(__VA_ARGS__);                                                                                           \
        printf("\n");                                                                                                  \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;

static void fill(uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
        p[i] = (uint8_t)rng_state;
    }
}

/* fusion's seal of a fixed record: taken before the engine is first used, compared at the end */
static void fusion_probe(uint8_t *out)
{
    static const uint8_t key[16] = {1, 2, 3}, iv[12] = {4, 5, 6}, aad[13] = {7};
    uint8_t pt[1200];
    memset(pt, 0x5a, sizeof(pt));
    ptls_aead_context_t *c = ptls_aead_new_direct(&ptls_fusion_aes128gcm, 1, key, iv);
    ptls_aead_encrypt(c, out, pt, sizeof(pt), 42, aad, sizeof(aad));
    ptls_aead_free(c);
}

static void fields_test(void)
{
    const ptls_aead_algorithm_t *m = &ptls_mi355x_chacha20poly1305, *o = &ptls_openssl_chacha20poly1305;
    OK(strcmp(m->name, o->name) == 0 && m->confidentiality_limit == o->confidentiality_limit &&
           m->integrity_limit == o->integrity_limit && m->key_size == o->key_size && m->iv_size == o->iv_size &&
           m->tag_size == o->tag_size && m->tls12.fixed_iv_size == o->tls12.fixed_iv_size &&
           m->tls12.record_iv_size == o->tls12.record_iv_size && m->non_temporal == o->non_temporal &&
           m->align_bits == o->align_bits,
       "chacha20poly1305 scalar fields match ptls_openssl_chacha20poly1305");
    OK(m->ctr_cipher == &ptls_mi355x_chacha20 && m->ecb_cipher == NULL && o->ecb_cipher == NULL && m->setup_crypto != NULL &&
           m->context_size >= sizeof(ptls_aead_context_t),
       "ctr_cipher is the ChaCha20 object, ecb_cipher NULL");
    const ptls_cipher_algorithm_t *mc = &ptls_mi355x_chacha20, *oc = &ptls_openssl_chacha20;
    OK(strcmp(mc->name, oc->name) == 0 && mc->key_size == oc->key_size && mc->block_size == oc->block_size &&
           mc->iv_size == oc->iv_size && mc->setup_crypto != NULL && mc->context_size >= sizeof(ptls_cipher_context_t),
       "chacha20 scalar fields match ptls_openssl_chacha20");
}

static void pair_test(void)
{
    static const size_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1200, 4096, 16384, 16385, 70000};
    static uint8_t pt[70000], a[70016], b[70016], back[70000], aad[64];
    uint8_t key[32], iv[12];
    fill(key, sizeof(key)), fill(iv, sizeof(iv));
    ptls_aead_context_t *me = ptls_aead_new_direct(&ptls_mi355x_chacha20poly1305, 1, key, iv);
    ptls_aead_context_t *md = ptls_aead_new_direct(&ptls_mi355x_chacha20poly1305, 0, key, iv);
    ptls_aead_context_t *oe = ptls_aead_new_direct(&ptls_openssl_chacha20poly1305, 1, key, iv);
    ptls_aead_context_t *od = ptls_aead_new_direct(&ptls_openssl_chacha20poly1305, 0, key, iv);
    OK(me != NULL && md != NULL && oe != NULL && od != NULL, "contexts created");
    if (me == NULL || md == NULL || oe == NULL || od == NULL)
        return;
    OK(me->do_encrypt_init == NULL && me->do_encrypt_update == NULL && me->do_encrypt_final == NULL && me->do_encrypt != NULL &&
           me->do_encrypt_v != NULL && me->do_decrypt != NULL && me->do_get_iv != NULL && me->do_set_iv != NULL &&
           me->dispose_crypto != NULL,
       "callbacks: one-shot ones set, init / update / final NULL");
    OK(ptls_mi355x_chacha_aead_get_keyset(me) != NULL && ptls_mi355x_chacha_keyset_size(ptls_mi355x_chacha_aead_get_keyset(me)) == 1,
       "aead_get_keyset");
    for (size_t i = 0; i < sizeof(lens) / sizeof(lens[0]); ++i) {
        const size_t n = lens[i], an = i * 3 % 41;
        const uint64_t seq = (uint64_t)i << 40 | i;
        fill(pt, n), fill(aad, an);
        memset(a, 0xaa, n + 16), memset(b, 0xbb, n + 16);
        ptls_aead_encrypt(me, a, pt, n, seq, aad, an);
        ptls_aead_encrypt(oe, b, pt, n, seq, aad, an);
        OK(memcmp(a, b, n + 16) == 0, "encrypt len %zu == openssl", n);
        /* encrypt_v over three vectors */
        ptls_iovec_t v[3] = {{pt, n / 3}, {pt + n / 3, 0}, {pt + n / 3, n - n / 3}};
        memset(a, 0xaa, n + 16);
        ptls_aead_encrypt_v(me, a, v, 3, seq, aad, an);
        OK(memcmp(a, b, n + 16) == 0, "encrypt_v len %zu == openssl", n);
        /* cross decrypt */
        memset(back, 0xcc, n);
        OK(ptls_aead_decrypt(md, back, b, n + 16, seq, aad, an) == n && memcmp(back, pt, n) == 0, "mi355x opens openssl len %zu", n);
        OK(ptls_aead_decrypt(od, back, a, n + 16, seq, aad, an) == n && memcmp(back, pt, n) == 0, "openssl opens mi355x len %zu", n);
        /* a failed decrypt returns SIZE_MAX and leaves the output as it was */
        memset(back, 0xcc, n);
        a[n + 16 - 1 - n / 2] ^= 4;
        size_t r = ptls_aead_decrypt(md, back, a, n + 16, seq, aad, an), same = 1;
        for (size_t k = 0; k < n; ++k)
            same &= back[k] == 0xcc;
        OK(r == SIZE_MAX && same, "tampered len %zu rejected, output untouched", n);
    }
    OK(ptls_aead_decrypt(md, back, a, 15, 0, NULL, 0) == SIZE_MAX, "inlen < 16 rejected");
    /* xor_iv on both, then equal again */
    uint8_t mask[12], iv_m[12], iv_o[12];
    fill(mask, sizeof(mask));
    ptls_aead_xor_iv(me, mask, sizeof(mask));
    ptls_aead_xor_iv(oe, mask, sizeof(mask));
    ptls_aead_get_iv(me, iv_m), ptls_aead_get_iv(oe, iv_o);
    OK(memcmp(iv_m, iv_o, 12) == 0, "get_iv after xor_iv");
    fill(pt, 1200);
    ptls_aead_encrypt(me, a, pt, 1200, 9, aad, 13);
    ptls_aead_encrypt(oe, b, pt, 1200, 9, aad, 13);
    OK(memcmp(a, b, 1216) == 0, "encrypt after xor_iv == openssl");
    OK(ptls_aead_decrypt(md, back, a, 1216, 9, aad, 13) == SIZE_MAX, "the other context still has the old IV");
    ptls_aead_set_iv(md, iv_m);
    OK(ptls_aead_decrypt(md, back, a, 1216, 9, aad, 13) == 1200 && memcmp(back, pt, 1200) == 0, "set_iv");
    ptls_aead_free(me), ptls_aead_free(md), ptls_aead_free(oe), ptls_aead_free(od);
}

static void cipher_test(void)
{
    uint8_t key[32], iv[16], zero[16] = {0}, m[16], o[16], hdr[5], hm[5], ho[5];
    int same = 1;
    fill(key, sizeof(key));
    ptls_cipher_context_t *mc = ptls_cipher_new(&ptls_mi355x_chacha20, 1, key), *oc = ptls_cipher_new(&ptls_openssl_chacha20, 1, key);
    OK(mc != NULL && oc != NULL, "cipher contexts created");
    if (mc == NULL || oc == NULL)
        return;
    for (int i = 0; i < 64; ++i) {
        fill(iv, sizeof(iv));
        ptls_cipher_init(mc, iv), ptls_cipher_init(oc, iv);
        ptls_cipher_encrypt(mc, m, zero, 16), ptls_cipher_encrypt(oc, o, zero, 16);
        same &= memcmp(m, o, 16) == 0;
        /* as QUIC uses it: 5 bytes of a header */
        fill(hdr, sizeof(hdr));
        ptls_cipher_init(mc, iv), ptls_cipher_init(oc, iv);
        ptls_cipher_encrypt(mc, hm, hdr, 5), ptls_cipher_encrypt(oc, ho, hdr, 5);
        same &= memcmp(hm, ho, 5) == 0;
    }
    OK(same, "64 header-protection masks == ptls_openssl_chacha20");
    ptls_cipher_free(mc), ptls_cipher_free(oc);
}

/* ptls_aead_encrypt_s: the supplementary (header protection) block computed from the sealed output */
static void supp_test(void)
{
    uint8_t key[32], hpkey[32], iv[12], pt[1200], a[1216], b[1216], aad[13];
    fill(key, 32), fill(hpkey, 32), fill(iv, 12), fill(pt, sizeof(pt)), fill(aad, sizeof(aad));
    ptls_aead_context_t *me = ptls_aead_new_direct(&ptls_mi355x_chacha20poly1305, 1, key, iv);
    ptls_aead_context_t *oe = ptls_aead_new_direct(&ptls_openssl_chacha20poly1305, 1, key, iv);
    ptls_cipher_context_t *mc = ptls_cipher_new(&ptls_mi355x_chacha20, 1, hpkey), *oc = ptls_cipher_new(&ptls_openssl_chacha20, 1, hpkey);
    if (me == NULL || oe == NULL || mc == NULL || oc == NULL) {
        OK(0, "supp contexts created");
        return;
    }
    ptls_aead_supplementary_encryption_t sm = {mc, a + 4, {0}}, so = {oc, b + 4, {0}};
    ptls_aead_encrypt_s(me, a, pt, sizeof(pt), 3, aad, sizeof(aad), &sm);
    ptls_aead_encrypt_s(oe, b, pt, sizeof(pt), 3, aad, sizeof(aad), &so);
    OK(memcmp(a, b, sizeof(a)) == 0 && memcmp(sm.output, so.output, sizeof(sm.output)) == 0, "encrypt_s with supp == openssl");
    ptls_aead_free(me), ptls_aead_free(oe), ptls_cipher_free(mc), ptls_cipher_free(oc);
}

int main(void)
{
    if (!ptls_fusion_is_supported_by_cpu()) {
        printf("1..0 # SKIP fusion not supported by this CPU\n");
        return 0;
    }
    uint8_t before[1216], after[1216];
    fusion_probe(before); /* before the engine is first used */
    fields_test();
    pair_test();
    cipher_test();
    supp_test();
    fusion_probe(after);
    OK(memcmp(before, after, sizeof(before)) == 0, "fusion's seal is the same before and after the engine ran");
    printf("1..%d\n# %d failed\n", ntest, nfail);
    return nfail == 0 ? 0 : 1;
}
