"""Reference for QUIC packet protection (RFC 9001 §5.3-5.4, RFC 9000 A.3): protect and unprotect, written once over a
Suite (an AEAD seal and open and a header-protection mask), decode_pn, Opened and the statuses.

The module's own names are the ChaCha20-Poly1305 binding, built only from what chacha_ref has: OpenSSL (ossl_seal /
ossl_open / ossl_chacha20) and, as an independent second source, the plain-Python restatements (py_seal / py_open /
py_chacha20_block). ``impl`` picks the source: "ossl" or "py". quic_aes_ref binds the same functions to AES-GCM.

Statuses are those of include/picotls/mi355x.h (PTLS_MI355X_QUIC_*)."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Callable

import chacha_ref as R

OK, BAD_MAC, REJECTED, KEY_PHASE = 0, 1, 2, 3
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quic_chacha20_kat.json")


def load_kat() -> dict:
    with open(KAT_PATH) as fh:
        return json.load(fh)


def hp_mask(hp: bytes, sample: bytes, impl: str = "ossl") -> bytes:
    """The first 5 keystream bytes of ChaCha20 under the header-protection key, counter = the sample's first 4 bytes
    (little endian), nonce = the other 12 (RFC 9001 §5.4.4)."""
    assert len(sample) == 16
    if impl == "py":
        return R.py_chacha20_block(hp, int.from_bytes(sample[:4], "little"), sample[4:])[:5]
    return R.ossl_chacha20(hp, sample, bytes(5))


def _seal(key: bytes, iv: bytes, seq: int, aad: bytes, pt: bytes, impl: str = "ossl") -> bytes:
    return (R.py_seal if impl == "py" else R.ossl_seal)(key, R.nonce_for(iv, seq), pt, aad)


def _open(key: bytes, iv: bytes, seq: int, aad: bytes, sealed: bytes, impl: str = "ossl") -> bytes | None:
    return (R.py_open if impl == "py" else R.ossl_open)(key, R.nonce_for(iv, seq), sealed, aad)


@dataclass(frozen=True)
class Suite:
    """What protect / unprotect take from a cipher suite, each with a trailing ``impl`` that picks the source."""
    seal: Callable[..., bytes]            # (key, iv, seq, aad, pt, impl) -> ciphertext || tag, nonce = iv ^ BE64(seq)
    open: Callable[..., "bytes | None"]   # (key, iv, seq, aad, sealed, impl) -> plaintext, None on a bad tag
    hp_mask: Callable[..., bytes]         # (hp, sample, impl) -> mask[0 .. 4]


CHACHA20 = Suite(_seal, _open, hp_mask)


def _apply_mask(first: int, mask: bytes) -> int:
    return first ^ (mask[0] & (0x0f if first & 0x80 else 0x1f))  # (bit 7 is not protected)


def decode_pn(expected_pn: int, truncated_pn: int, pn_len: int) -> int:
    """RFC 9000 A.3 (expected_pn = the largest packet number processed + 1; pn_len in bytes)."""
    win = 1 << (8 * pn_len)
    hwin = win // 2
    cand = (expected_pn & ~(win - 1)) | truncated_pn
    if cand <= expected_pn - hwin and cand < (1 << 62) - win:
        return cand + win
    if cand > expected_pn + hwin and cand >= win:
        return cand - win
    return cand


def protect(key: bytes, iv: bytes, hp: bytes, pn: int, header: bytes, payload: bytes, impl: str = "ossl",
            suite: Suite = CHACHA20) -> bytes:
    """header (cleartext, ending in the truncated packet number of (header[0] & 3) + 1 bytes) || payload to the protected
    packet: header' || ciphertext || tag."""
    pn_len = (header[0] & 3) + 1
    assert len(header) >= 1 + pn_len and pn_len + len(payload) >= 4
    sealed = suite.seal(key, iv, pn, header, payload, impl)
    pn_off = len(header) - pn_len
    sample = (header[pn_off:] + sealed)[4:20]
    mask = suite.hp_mask(hp, sample, impl)
    out = bytearray(header)
    out[0] = _apply_mask(header[0], mask)
    for i in range(pn_len):
        out[pn_off + i] ^= mask[1 + i]
    return bytes(out) + sealed


@dataclass
class Opened:
    status: int
    pn: int = 0
    pn_len: int = 0
    first_byte: int = 0
    header: bytes = b""  # the unprotected header, through the packet number
    payload: bytes | None = None  # None unless status == OK


def unprotect(key: bytes, iv: bytes, hp: bytes, expected_pn: int, pn_off: int, packet: bytes, phase: int = 0,
              impl: str = "ossl", suite: Suite = CHACHA20) -> Opened:
    """The receiver's side: packet is the whole protected packet, pn_off the offset of its packet-number field."""
    if pn_off < 1 or len(packet) - pn_off < 20:
        return Opened(REJECTED)
    mask = suite.hp_mask(hp, packet[pn_off + 4:pn_off + 20], impl)
    first = _apply_mask(packet[0], mask)
    pn_len = (first & 3) + 1
    trunc = bytes(packet[pn_off + i] ^ mask[1 + i] for i in range(pn_len))
    pn = decode_pn(expected_pn, int.from_bytes(trunc, "big"), pn_len)
    header = bytes([first]) + packet[1:pn_off] + trunc
    res = Opened(OK, pn, pn_len, first, header)
    if not first & 0x80 and (first >> 2) & 1 != phase & 1:
        res.status = KEY_PHASE
        return res
    res.payload = suite.open(key, iv, pn, header, packet[pn_off + pn_len:], impl)
    if res.payload is None:
        res.status = BAD_MAC
    return res
