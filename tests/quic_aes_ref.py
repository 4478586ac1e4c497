"""Reference for QUIC packet protection under AES-GCM (RFC 9001 §5.3-5.4, RFC 9000 A.3): the AES primitives, bound to
quic_ref's protect and unprotect under that module's names and signatures. Two independent sources behind ``impl``:

  "ossl"    AES-GCM and AES-ECB of the system libcrypto through ctypes (EVP_aes_{128,256}_gcm, EVP_aes_{128,256}_ecb),
            found the way chacha_ref finds it;
  "oracle"  oracle.GcmOracle.seal / .open / .aes_encrypt, the project's own plain-C restatement (oracle/gcm_ref.c).

The key size (16 or 32 bytes) is that of the key passed; the header-protection key may have another size than the AEAD
key. Statuses are those of include/picotls/mi355x.h (PTLS_MI355X_QUIC_*). decode_pn and the status constants are
quic_ref's. No RFC 9001 Appendix A vector is included: none is available to this tree to reproduce byte for byte from
both sources, so the two sources are checked against each other instead (test_quic_aes_ref.py)."""
from __future__ import annotations

import ctypes
import functools

import chacha_ref as R
import quic_ref
from quic_ref import BAD_MAC, KEY_PHASE, OK, REJECTED, Opened, _apply_mask, decode_pn  # noqa: F401

_oracle = None
_evp_ready = False


def _gcm_oracle():
    global _oracle
    if _oracle is None:
        from oracle import GcmOracle

        _oracle = GcmOracle()
    return _oracle


def _evp():
    global _evp_ready
    c = R._libcrypto()
    if not _evp_ready:
        for name in ("EVP_aes_128_gcm", "EVP_aes_256_gcm", "EVP_aes_128_ecb", "EVP_aes_256_ecb"):
            getattr(c, name).restype = ctypes.c_void_p
        c.EVP_CIPHER_CTX_set_padding.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _evp_ready = True
    return c


def _cipher(c, key: bytes, mode: str):
    assert len(key) in (16, 32)
    return getattr(c, f"EVP_aes_{len(key) * 8}_{mode}")()


def ossl_gcm_seal(key: bytes, nonce: bytes, pt: bytes, aad: bytes) -> bytes:
    c = _evp()
    with R._Ctx() as k:
        ctx = k.ctx
        assert c.EVP_CipherInit_ex(ctx, _cipher(c, key, "gcm"), None, None, None, 1) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, R._EVP_CTRL_AEAD_SET_IVLEN, 12, None) == 1
        assert c.EVP_CipherInit_ex(ctx, None, None, key, nonce, 1) == 1
        if aad:
            R._update(c, ctx, aad, False)
        ct = R._update(c, ctx, pt) if pt else b""
        n = ctypes.c_int(0)
        fin = ctypes.create_string_buffer(16)
        assert c.EVP_CipherFinal_ex(ctx, fin, ctypes.byref(n)) == 1
        tag = ctypes.create_string_buffer(16)
        assert c.EVP_CIPHER_CTX_ctrl(ctx, R._EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        return ct + tag.raw


def ossl_gcm_open(key: bytes, nonce: bytes, sealed: bytes, aad: bytes) -> bytes | None:
    c = _evp()
    ct, tag = sealed[:-16], sealed[-16:]
    with R._Ctx() as k:
        ctx = k.ctx
        assert c.EVP_CipherInit_ex(ctx, _cipher(c, key, "gcm"), None, None, None, 0) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, R._EVP_CTRL_AEAD_SET_IVLEN, 12, None) == 1
        assert c.EVP_CipherInit_ex(ctx, None, None, key, nonce, 0) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, R._EVP_CTRL_AEAD_SET_TAG, 16, tag) == 1
        if aad:
            R._update(c, ctx, aad, False)
        pt = R._update(c, ctx, ct) if ct else b""
        n = ctypes.c_int(0)
        fin = ctypes.create_string_buffer(16)
        if c.EVP_CipherFinal_ex(ctx, fin, ctypes.byref(n)) != 1:
            return None
        return pt


def ossl_aes_ecb(key: bytes, block: bytes) -> bytes:
    c = _evp()
    assert len(block) == 16
    with R._Ctx() as k:
        ctx = k.ctx
        assert c.EVP_CipherInit_ex(ctx, _cipher(c, key, "ecb"), None, key, None, 1) == 1
        assert c.EVP_CIPHER_CTX_set_padding(ctx, 0) == 1
        return R._update(c, ctx, block)[:16]


def gcm_seal(key: bytes, iv: bytes, seq: int, aad: bytes, pt: bytes, impl: str = "ossl") -> bytes:
    """ciphertext || tag under nonce = iv ^ BE64(seq)."""
    if impl == "oracle":
        return _gcm_oracle().seal(key, iv, seq, aad, pt)
    assert impl == "ossl"
    return ossl_gcm_seal(key, R.nonce_for(iv, seq), pt, aad)


def gcm_open(key: bytes, iv: bytes, seq: int, aad: bytes, sealed: bytes, impl: str = "ossl") -> bytes | None:
    if impl == "oracle":
        return _gcm_oracle().open(key, iv, seq, aad, sealed)
    assert impl == "ossl"
    return ossl_gcm_open(key, R.nonce_for(iv, seq), sealed, aad)


def hp_mask(hp: bytes, sample: bytes, impl: str = "ossl") -> bytes:
    """AES-ECB(hp key, sample), of which the first 5 bytes are used (RFC 9001 §5.4.3)."""
    assert len(sample) == 16
    if impl == "oracle":
        return _gcm_oracle().aes_encrypt(hp, sample)[:5]
    assert impl == "ossl"
    return ossl_aes_ecb(hp, sample)[:5]


AES_GCM = quic_ref.Suite(gcm_seal, gcm_open, hp_mask)
# quic_ref's protect(key, iv, hp, pn, header, payload, impl="ossl") and unprotect(key, iv, hp, expected_pn, pn_off, packet,
# phase=0, impl="ossl"), over AES-GCM and AES-ECB
protect = functools.partial(quic_ref.protect, suite=AES_GCM)
unprotect = functools.partial(quic_ref.unprotect, suite=AES_GCM)
