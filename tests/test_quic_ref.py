"""CPU-side checks of QUIC packet protection: the reference of tests/quic_ref.py against the RFC 9001 A.5 packet and the
RFC 9000 A.3 example on both of its sources, and the boundary (result struct, status codes, exports) against the header
text. No device calls."""
import os
import re
import subprocess

import numpy as np
import pytest

import picotls_amd as pa
import quic_ref as Q
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, QUIC_REJECTED, QUIC_RESULT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPLS = ("ossl", "py")


def _kat():
    v = Q.load_kat()["packet"]
    return {k: (bytes.fromhex(x) if isinstance(x, str) else x) for k, x in v.items()}


@pytest.mark.parametrize("impl", IMPLS)
def test_rfc9001_a5_packet(impl):
    v = _kat()
    assert Q.hp_mask(v["hp"], v["sample"], impl) == v["mask"]
    packet = Q.protect(v["key"], v["iv"], v["hp"], v["pn"], v["header"], v["payload"], impl)
    assert packet == v["packet"]
    assert packet[5:21] == v["sample"]  # in this vector the sample covers the tag
    for expected in (v["pn"], v["pn"] - 1, v["pn"] + 1):
        got = Q.unprotect(v["key"], v["iv"], v["hp"], expected, 1, packet, 0, impl)
        assert (got.status, got.pn, got.pn_len, got.first_byte) == (Q.OK, v["pn"], 3, 0x42)
        assert got.header == v["header"] and got.payload == v["payload"]
    # the key-phase bit of 0x42 is 0: expected phase 1 is a KEY_PHASE verdict, nothing opened
    got = Q.unprotect(v["key"], v["iv"], v["hp"], v["pn"], 1, packet, 1, impl)
    assert got.status == Q.KEY_PHASE and got.payload is None
    bad = bytearray(packet)
    bad[4] ^= 1  # the one ciphertext byte, ahead of the sample (a flip inside the sample changes the mask as well)
    assert Q.unprotect(v["key"], v["iv"], v["hp"], v["pn"], 1, bytes(bad), 0, impl).status == Q.BAD_MAC
    assert Q.unprotect(v["key"], v["iv"], v["hp"], v["pn"], 2, packet, 0, impl).status == Q.REJECTED  # 19 bytes from pn_off


def test_both_sources_agree_on_random_packets():
    rng = np.random.default_rng(9001)
    for i in range(40):
        key, iv, hp = rng.bytes(32), rng.bytes(12), rng.bytes(32)
        pn_len = i % 4 + 1
        long_hdr = i % 5 == 0
        first = (0xc0 if long_hdr else 0x40 | (i & 4)) | (pn_len - 1)
        pn = int(rng.integers(0, 2**62))
        header = bytes([first]) + rng.bytes(int(rng.integers(0, 21))) + (pn & ((1 << 8 * pn_len) - 1)).to_bytes(pn_len, "big")
        payload = rng.bytes(int(rng.integers(max(4 - pn_len, 0), 80)))
        packet = Q.protect(key, iv, hp, pn, header, payload, "ossl")
        assert packet == Q.protect(key, iv, hp, pn, header, payload, "py")
        assert packet[0] & 0x80 == first & 0x80 and len(packet) == len(header) + len(payload) + 16
        for impl in IMPLS:
            got = Q.unprotect(key, iv, hp, pn, len(header) - pn_len, packet, (first >> 2) & 1, impl)
            assert (got.status, got.pn, got.header, got.payload) == (Q.OK, pn, header, payload)


def test_decode_pn_rfc9000_a3():
    v = Q.load_kat()["decode_pn"]
    largest = int(v["largest"], 16)
    assert Q.decode_pn(largest + 1, int(v["truncated"], 16), v["pn_len"]) == int(v["pn"], 16) == 0xa82f9b32


@pytest.mark.parametrize("pn_len", (1, 2, 3, 4))
def test_decode_pn_window_edges(pn_len):
    """A packet number within half a window of the expected one comes back exactly, at both edges of the window, near 0
    (where there is no window below) and near 2^62 - 1 (none above)."""
    win = 1 << (8 * pn_len)
    hwin = win // 2
    top = (1 << 62) - 1
    for expected in (0, 1, hwin - 1, hwin, hwin + 1, win, 3 * win + 5, 0xa82f30eb, (1 << 40) + hwin, top - win, top - hwin, top - 1, top):
        # RFC 9000 A.3 recovers every pn with expected - hwin < pn <= expected + hwin
        for pn in (expected - hwin + 1, expected - hwin + 2, expected - 1, expected, expected + 1, expected + hwin - 1, expected + hwin):
            if 0 <= pn <= top:
                assert Q.decode_pn(expected, pn & (win - 1), pn_len) == pn, (expected, pn)
    assert Q.decode_pn(0, win - 1, pn_len) == win - 1  # no step below zero
    assert Q.decode_pn(top, 0, pn_len) == top + 1 - win  # no step past 2^62 - 1


def test_result_struct_and_statuses_match_the_header():
    text = open(os.path.join(ROOT, "include", "picotls", "mi355x.h")).read()
    for name, value in (("OK", QUIC_OK), ("BAD_MAC", QUIC_BAD_MAC), ("REJECTED", QUIC_REJECTED), ("KEY_PHASE", QUIC_KEY_PHASE)):
        m = re.search(rf"#define\s+PTLS_MI355X_QUIC_{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == value == getattr(Q, name), name
    body = re.search(r"typedef struct st_ptls_mi355x_quic_result_t \{(.*?)\} ptls_mi355x_quic_result_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint(?:8|16|32|64)_t)\s+(\w+)\s*;", body)
    ctype = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "uint64_t": "<u8"}
    assert [(n, np.dtype(ctype[t])) for t, n in fields] == [(n, QUIC_RESULT_DTYPE[n]) for n in QUIC_RESULT_DTYPE.names]
    assert QUIC_RESULT_DTYPE.itemsize == 16 and pa.QUIC_RESULT_DTYPE is QUIC_RESULT_DTYPE
    # the suite-neutral header declares types only; the calls live with their suite
    assert "quic_packets" not in " ".join(pa.ABI_FUNCTIONS)


def test_quic_calls_are_exported():
    names = {"ptls_mi355x_chacha_seal_quic_packets", "ptls_mi355x_chacha_open_quic_packets"}
    assert names <= set(pa.CHACHA_ABI_FUNCTIONS)
    out = subprocess.run(["nm", "-D", "--defined-only", pa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert names <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = pa.load_library()
    for n in names:
        assert getattr(lib, n) is not None
    assert callable(pa.chacha_seal_quic_packets) and callable(pa.chacha_open_quic_packets)
