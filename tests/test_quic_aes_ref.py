"""CPU-side checks of QUIC packet protection under AES-GCM: the two sources of tests/quic_aes_ref.py (the system
libcrypto, the project's plain-C oracle) against each other for both key sizes, the round trip, every rejection and
key-phase verdict, and the boundary (the header, exports, QUIC_ABI_FUNCTIONS, the Python wrappers). No device calls.

No RFC 9001 Appendix A vector is included: none is available to this tree to reproduce byte for byte from both sources
(quic_aes_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import picotls_amd as pa
import quic_aes_ref as Q

IMPLS = ("ossl", "oracle")
NAMES = {"ptls_mi355x_seal_quic_packets", "ptls_mi355x_open_quic_packets"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(rng, first_bits: int, pn_len: int, pn: int, middle: int) -> bytes:
    return bytes([first_bits | (pn_len - 1)]) + rng.bytes(middle) + (pn & ((1 << 8 * pn_len) - 1)).to_bytes(pn_len, "big")


@pytest.mark.parametrize("key_size", (16, 32))
def test_primitives_agree(key_size):
    rng = np.random.default_rng(key_size)
    for n in (0, 1, 15, 16, 17, 100):
        key, iv, aad, pt = rng.bytes(key_size), rng.bytes(12), rng.bytes(int(rng.integers(0, 40))), rng.bytes(n)
        seq = int(rng.integers(0, 2**62))
        sealed = Q.gcm_seal(key, iv, seq, aad, pt, "ossl")
        assert sealed == Q.gcm_seal(key, iv, seq, aad, pt, "oracle") and len(sealed) == n + 16
        for impl in IMPLS:
            assert Q.gcm_open(key, iv, seq, aad, sealed, impl) == pt
            assert Q.gcm_open(key, iv, seq ^ 1, aad, sealed, impl) is None
        block = rng.bytes(16)
        assert Q.hp_mask(key, block, "ossl") == Q.hp_mask(key, block, "oracle")
    # FIPS-197 C.1 / C.3: the block cipher itself, on both sources
    pt = bytes.fromhex("00112233445566778899aabbccddeeff")
    want = {16: "69c4e0d86a7b0430d8cdb78070b4c55a", 32: "8ea2b7ca516745bfeafc49904b496089"}[key_size]
    for impl in IMPLS:
        assert Q.hp_mask(bytes(range(key_size)), pt, impl) == bytes.fromhex(want)[:5]


@pytest.mark.parametrize("key_size", (16, 32))
def test_both_sources_agree_on_random_packets(key_size):
    """A few hundred packets: every pn_len, payloads from 4 - pn_len up, short and long headers, and the header-protection
    key of the other size on every third packet."""
    rng = np.random.default_rng(9001 + key_size)
    for i in range(240):
        hp_size = 48 - key_size if i % 3 == 0 else key_size
        key, iv, hp = rng.bytes(key_size), rng.bytes(12), rng.bytes(hp_size)
        pn_len = i % 4 + 1
        long_hdr = i % 5 == 0
        first = 0xc0 if long_hdr else 0x40 | (i & 4)
        pn = int(rng.integers(0, 2**62))
        header = _header(rng, first, pn_len, pn, int(rng.integers(0, 21)) if not long_hdr else int(rng.integers(6, 50)))
        lo = 4 - pn_len
        payload = rng.bytes(lo + i // 8 if i < 160 else int(rng.integers(lo, 1500)))
        packet = Q.protect(key, iv, hp, pn, header, payload, "ossl")
        assert packet == Q.protect(key, iv, hp, pn, header, payload, "oracle")
        assert packet[0] & 0x80 == first & 0x80 and len(packet) == len(header) + len(payload) + 16
        assert packet[1:len(header) - pn_len] == header[1:-pn_len]  # only the first byte and the packet number are masked
        for impl in IMPLS:
            got = Q.unprotect(key, iv, hp, pn, len(header) - pn_len, packet, (first >> 2) & 1, impl)
            assert (got.status, got.pn, got.pn_len, got.first_byte) == (Q.OK, pn, pn_len, header[0])
            assert got.header == header and got.payload == payload


@pytest.mark.parametrize("impl", IMPLS)
def test_verdicts(impl):
    rng = np.random.default_rng(5)
    key, iv, hp = rng.bytes(16), rng.bytes(12), rng.bytes(16)
    pn = 0x1234567
    header = _header(rng, 0x40, 2, pn, 8)
    packet = Q.protect(key, iv, hp, pn, header, rng.bytes(30), impl)
    pn_off = len(header) - 2
    assert Q.unprotect(key, iv, hp, pn, pn_off, packet, 0, impl).status == Q.OK
    # a short header under the other expected phase: not opened
    got = Q.unprotect(key, iv, hp, pn, pn_off, packet, 1, impl)
    assert got.status == Q.KEY_PHASE and got.payload is None and got.pn == pn
    # a long header ignores the expected phase
    lh = _header(rng, 0xc0, 2, pn, 20)
    lp = Q.protect(key, iv, hp, pn, lh, rng.bytes(30), impl)
    assert Q.unprotect(key, iv, hp, pn, len(lh) - 2, lp, 1, impl).status == Q.OK
    # tampering outside the sample: the first byte's unprotected bits, the DCID, the packet number, ciphertext, tag
    for pos in (1, pn_off, len(packet) - 1, pn_off + 4 + 16):
        bad = bytearray(packet)
        bad[pos] ^= 0x10
        assert Q.unprotect(key, iv, hp, pn, pn_off, bytes(bad), 0, impl).status == Q.BAD_MAC, pos
    # an expected number more than half a window off: A.3 lands a window away and the tag fails
    got = Q.unprotect(key, iv, hp, pn + (1 << 16), pn_off, packet, 0, impl)
    assert got.status == Q.BAD_MAC and got.pn == pn + (1 << 16)
    # rejections: no byte before the packet number, fewer than 20 bytes from it to the end
    assert Q.unprotect(key, iv, hp, pn, 0, packet, 0, impl).status == Q.REJECTED
    assert Q.unprotect(key, iv, hp, pn, len(packet) - 19, packet, 0, impl).status == Q.REJECTED
    assert Q.unprotect(key, iv, hp, pn, len(packet) - 20, packet, 0, impl).status != Q.REJECTED
    # the sender's: no full sample, a header without room for the packet number
    with pytest.raises(AssertionError):
        Q.protect(key, iv, hp, pn, _header(rng, 0x40, 1, pn, 3), b"ab", impl)
    with pytest.raises(AssertionError):
        Q.protect(key, iv, hp, pn, bytes([0x43, 1, 2, 3]), bytes(20), impl)


def test_quic_calls_are_exported():
    """The AES-GCM pair: declared in picotls/mi355x_quic.h (a header of their own: mi355x.h keeps the suite-neutral types
    only, as test_quic_ref holds it to), listed in QUIC_ABI_FUNCTIONS, exported, callable."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "picotls", "mi355x_quic.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(ptls_mi355x_\w+)\s*\(", text)) == NAMES == set(pa.QUIC_ABI_FUNCTIONS)
    assert not NAMES & (set(pa.ABI_FUNCTIONS) | set(pa.CHACHA_ABI_FUNCTIONS) | set(pa.DEBUG_FUNCTIONS))
    from picotls_amd import build as b

    assert os.path.join(ROOT, "include", "picotls", "mi355x_quic.h") in b.HEADERS
    out = subprocess.run(["nm", "-D", "--defined-only", pa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = pa.load_library()
    for n in NAMES:
        assert getattr(lib, n) is not None
    assert callable(pa.seal_quic_packets) and callable(pa.open_quic_packets)
    # invalid arguments are refused before any device call: NULL keysets return -1
    assert lib.ptls_mi355x_seal_quic_packets(None, None, None, 0, None, None, None) == -1
    assert lib.ptls_mi355x_open_quic_packets(None, None, None, 0, None, None, None, None, None) == -1
    with pytest.raises(pa.EngineError):
        pa.seal_quic_packets(None, None, 0, 0, 0, 0)
