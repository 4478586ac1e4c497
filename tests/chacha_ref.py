"""References for the ChaCha20-Poly1305 tests.

(a) OpenSSL: the system libcrypto through ctypes (EVP_chacha20_poly1305, EVP_chacha20), the backend picotls itself uses
    for the suite.
(b) plain Python: RFC 8439 restated with bigints (slow, independent of (a)).
(c) the RFC 8439 / 7539 vectors of tests/golden/chacha20poly1305_kat.json.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import json
import os
import struct

import numpy as np

P1305 = (1 << 130) - 5
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chacha20poly1305_kat.json")


def load_kat() -> dict:
    with open(KAT_PATH) as fh:
        return json.load(fh)


def nonce_for(iv: bytes, seq: int) -> bytes:
    """static_iv ^ (0^32 || BE64(seq)) (ptls_aead__build_iv)."""
    s = bytes(4) + struct.pack(">Q", seq)
    return bytes(a ^ b for a, b in zip(iv, s))


# ------------------------------------------------------------------------------------------------ (b) plain Python


def _rotl(x: int, n: int) -> int:
    return ((x << n) | (x >> (32 - n))) & 0xffffffff


def _qr(s: list, a: int, b: int, c: int, d: int) -> None:
    s[a] = (s[a] + s[b]) & 0xffffffff
    s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & 0xffffffff
    s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & 0xffffffff
    s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & 0xffffffff
    s[b] = _rotl(s[b] ^ s[c], 7)


def py_chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574, *struct.unpack("<8I", key), counter & 0xffffffff,
            *struct.unpack("<3I", nonce)]
    s = list(init)
    for _ in range(10):
        _qr(s, 0, 4, 8, 12), _qr(s, 1, 5, 9, 13), _qr(s, 2, 6, 10, 14), _qr(s, 3, 7, 11, 15)
        _qr(s, 0, 5, 10, 15), _qr(s, 1, 6, 11, 12), _qr(s, 2, 7, 8, 13), _qr(s, 3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & 0xffffffff for a, b in zip(s, init)))


def py_chacha20_xor(key: bytes, counter: int, nonce: bytes, data: bytes) -> bytes:
    out = bytearray()
    for i in range(0, len(data), 64):
        ks = py_chacha20_block(key, counter + i // 64, nonce)
        out += bytes(a ^ b for a, b in zip(data[i:i + 64], ks))
    return bytes(out)


def py_poly1305_acc(key32: bytes, msg: bytes) -> int:
    """The accumulator before the final reduction is taken mod 2^128 (an integer below p)."""
    r = int.from_bytes(key32[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    acc = 0
    for i in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P1305
    return acc


def py_poly1305(key32: bytes, msg: bytes) -> bytes:
    s = int.from_bytes(key32[16:], "little")
    return ((py_poly1305_acc(key32, msg) + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def py_seal(key: bytes, nonce: bytes, pt: bytes, aad: bytes = b"") -> bytes:
    otk = py_chacha20_block(key, 0, nonce)[:32]
    ct = py_chacha20_xor(key, 1, nonce, pt)
    mac = _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return ct + py_poly1305(otk, mac)


def py_open(key: bytes, nonce: bytes, sealed: bytes, aad: bytes = b"") -> bytes | None:
    ct, tag = sealed[:-16], sealed[-16:]
    otk = py_chacha20_block(key, 0, nonce)[:32]
    mac = _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    if py_poly1305(otk, mac) != tag:
        return None
    return py_chacha20_xor(key, 1, nonce, ct)


# ------------------------------------------------------------------------------------------------ (a) OpenSSL

_EVP_CTRL_AEAD_SET_IVLEN, _EVP_CTRL_AEAD_GET_TAG, _EVP_CTRL_AEAD_SET_TAG = 0x9, 0x10, 0x11
_crypto = None


def _libcrypto():
    global _crypto
    if _crypto is None:
        name = ctypes.util.find_library("crypto")
        if name is None:
            raise RuntimeError("libcrypto not found")
        c = ctypes.CDLL(name)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        c.EVP_CIPHER_CTX_new.restype = vp
        c.EVP_CIPHER_CTX_free.argtypes = [vp]
        c.EVP_chacha20_poly1305.restype = vp
        c.EVP_chacha20.restype = vp
        c.EVP_CipherInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p, ci]
        c.EVP_CipherUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ci), ctypes.c_char_p, ci]
        c.EVP_CipherFinal_ex.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ci)]
        c.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ci, ci, ctypes.c_char_p]
        _crypto = c
    return _crypto


class _Ctx:
    def __init__(self):
        self.c = _libcrypto()
        self.ctx = self.c.EVP_CIPHER_CTX_new()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.EVP_CIPHER_CTX_free(self.ctx)


def _update(c, ctx, data: bytes, want_out: bool = True) -> bytes:
    n = ctypes.c_int(0)
    out = ctypes.create_string_buffer(len(data) + 16) if want_out else None
    if c.EVP_CipherUpdate(ctx, out, ctypes.byref(n), data, len(data)) != 1:
        raise RuntimeError("EVP_CipherUpdate failed")
    return out.raw[:n.value] if want_out else b""


def ossl_seal(key: bytes, nonce: bytes, pt: bytes, aad: bytes = b"") -> bytes:
    with _Ctx() as k:
        c, ctx = k.c, k.ctx
        assert c.EVP_CipherInit_ex(ctx, c.EVP_chacha20_poly1305(), None, None, None, 1) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, _EVP_CTRL_AEAD_SET_IVLEN, 12, None) == 1
        assert c.EVP_CipherInit_ex(ctx, None, None, key, nonce, 1) == 1
        if aad:
            _update(c, ctx, aad, False)
        ct = _update(c, ctx, pt) if pt else b""
        n = ctypes.c_int(0)
        fin = ctypes.create_string_buffer(16)
        assert c.EVP_CipherFinal_ex(ctx, fin, ctypes.byref(n)) == 1
        tag = ctypes.create_string_buffer(16)
        assert c.EVP_CIPHER_CTX_ctrl(ctx, _EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        return ct + tag.raw


def ossl_open(key: bytes, nonce: bytes, sealed: bytes, aad: bytes = b"") -> bytes | None:
    ct, tag = sealed[:-16], sealed[-16:]
    with _Ctx() as k:
        c, ctx = k.c, k.ctx
        assert c.EVP_CipherInit_ex(ctx, c.EVP_chacha20_poly1305(), None, None, None, 0) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, _EVP_CTRL_AEAD_SET_IVLEN, 12, None) == 1
        assert c.EVP_CipherInit_ex(ctx, None, None, key, nonce, 0) == 1
        assert c.EVP_CIPHER_CTX_ctrl(ctx, _EVP_CTRL_AEAD_SET_TAG, 16, tag) == 1
        if aad:
            _update(c, ctx, aad, False)
        pt = _update(c, ctx, ct) if ct else b""
        n = ctypes.c_int(0)
        fin = ctypes.create_string_buffer(16)
        if c.EVP_CipherFinal_ex(ctx, fin, ctypes.byref(n)) != 1:
            return None
        return pt


def ossl_chacha20(key: bytes, iv16: bytes, data: bytes) -> bytes:
    """EVP_chacha20 with the 16-byte IV (LE32 block counter || 12-byte nonce): what ptls_openssl_chacha20 runs."""
    with _Ctx() as k:
        c, ctx = k.c, k.ctx
        assert c.EVP_CipherInit_ex(ctx, c.EVP_chacha20(), None, key, iv16, 1) == 1
        return _update(c, ctx, data)


# ------------------------------------------------------------------------------------------------ batches


def seal_records(keys, ivs, recs, pt, aad, out, seal=ossl_seal) -> None:
    """Reference of chacha_seal_batch: writes ciphertext || tag of every record of ``recs`` (RECORD_DTYPE) into the numpy
    arena ``out``; keys / ivs are lists of bytes indexed by key_idx."""
    for r in recs:
        k = int(r["key_idx"])
        i, o, n = int(r["in_off"]), int(r["out_off"]), int(r["len"])
        a, an = int(r["aad_off"]), int(r["aad_len"]) | int(r["flags"]) << 16
        sealed = seal(keys[k], nonce_for(ivs[k], int(r["seq"])), pt[i:i + n].tobytes(), aad[a:a + an].tobytes())
        out[o:o + n + 16] = np.frombuffer(sealed, np.uint8)
