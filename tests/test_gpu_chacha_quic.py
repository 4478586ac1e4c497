"""QUIC packet protection under ChaCha20-Poly1305 on the GPU (ptls_mi355x_chacha_seal_quic_packets /
_open_quic_packets): every comparison is byte for byte against tests/quic_ref.py (OpenSSL; a subset of each batch also
against its plain-Python source). Arenas start as 0xAA and are compared whole, so a write outside a packet shows. Every
test runs at both forced group widths, the batch ones also with the grid capped at two workgroups so that the claim loop
turns. The references of a test are computed once and shared by its modes."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import picotls_amd as pa
import quic_ref as Q
from gpu_util import dev, empty
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, QUIC_REJECTED, QUIC_RESULT_DTYPE, RECORD_DTYPE

pytestmark = pytest.mark.gpu

FILL = 0xAA
WIDTHS = pa.CHACHA_GROUP_WIDTHS
MODES = [(w, 0) for w in WIDTHS] + [(w, 2) for w in WIDTHS]  # (group width, cap on the launch grid)
TOP = (1 << 62) - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def forced():
    """debug_force for the test, back to automatic after it"""
    yield pa.chacha_debug_force
    pa.chacha_debug_force(0, 0)


@dataclass
class Keys:
    keys: list
    ivs: list
    hps: list

    @classmethod
    def make(cls, rng, n):
        return cls([rng.bytes(32) for _ in range(n)], [rng.bytes(12) for _ in range(n)], [rng.bytes(32) for _ in range(n)])

    def keysets(self):
        return pa.ChaChaKeyset(b"".join(self.keys), b"".join(self.ivs)), pa.ChaChaKeyset(b"".join(self.hps), bytes(12 * len(self.hps)))


@dataclass
class Pkt:
    k: int
    pn: int
    header: bytes   # cleartext, ending in the truncated packet number
    payload: bytes
    packet: bytes   # the protected packet (reference)
    expected: int   # the receiver's expected packet number
    phase: int

    @property
    def pn_len(self):
        return (self.header[0] & 3) + 1


def header_for(rng, pn, pn_len, body_len, long=False, phase=0):
    """first byte || body_len random bytes (a DCID, or a long header's fields) || the truncated packet number"""
    if long:
        first = 0xc0 | int(rng.integers(0, 4)) << 4 | int(rng.integers(0, 4)) << 2 | (pn_len - 1)
    else:
        first = 0x40 | int(rng.integers(0, 2)) << 5 | int(rng.integers(0, 4)) << 3 | phase << 2 | (pn_len - 1)
    return bytes([first]) + rng.bytes(body_len) + (pn & ((1 << 8 * pn_len) - 1)).to_bytes(pn_len, "big")


def make_pkt(K, rng, k, pn, pn_len, body_len, payload_len, long=False, phase=0, expected=None, hps=None):
    header = header_for(rng, pn, pn_len, body_len, long, phase)
    payload = rng.bytes(payload_len)
    packet = Q.protect(K.keys[k], K.ivs[k], (hps or K.hps)[k], pn, header, payload)
    return Pkt(k, pn, header, payload, packet, pn if expected is None else expected, phase)


def place(sizes, residues=None):
    """offsets of items of these sizes with at least 16 untouched bytes around each; item i at residues[i] mod 16"""
    offs, at = [], 16
    for i, n in enumerate(sizes):
        at = (at + 15) // 16 * 16 + (residues[i] if residues is not None else 0)
        offs.append(at)
        at += n + 16
    return offs, at + 32


def filled(nbytes):
    return np.full(max(nbytes, 1), FILL, np.uint8)


def put(arena, off, data):
    arena[off:off + len(data)] = np.frombuffer(data, np.uint8)


def seal_recs(pkts, in_offs, out_offs):
    recs = np.zeros(len(pkts), RECORD_DTYPE)
    for r, p, i, o in zip(recs, pkts, in_offs, out_offs):
        r["in_off"], r["out_off"], r["seq"], r["len"], r["key_idx"], r["aad_len"] = i, o, p.pn, len(p.payload), p.k, len(p.header)
    recs["aad_off"] = 0xdeadbeef  # ignored
    return recs


def open_recs(pkts, in_offs, out_offs):
    recs = np.zeros(len(pkts), RECORD_DTYPE)
    for r, p, i, o in zip(recs, pkts, in_offs, out_offs):
        r["in_off"], r["out_off"], r["seq"], r["key_idx"], r["flags"] = i, o, p.expected, p.k, p.phase
        r["aad_len"], r["len"] = len(p.header) - p.pn_len, len(p.packet) - (len(p.header) - p.pn_len)
    recs["aad_off"] = 0xdeadbeef
    return recs


def gpu_seal(ks, hp_ks, recs, arena_in, arena_out):
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    pa.chacha_seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), len(recs), d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def gpu_open(ks, hp_ks, recs, arena_in, arena_out):
    n = len(recs)
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    d_ok, d_res = empty(n + 16, FILL), empty(16 * n + 16, FILL)
    pa.chacha_open_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(),
                                _stream())
    torch.cuda.synchronize()
    ok, res = d_ok.cpu().numpy(), d_res.cpu().numpy()
    assert (ok[n:] == FILL).all() and (res[16 * n:] == FILL).all(), "ok or results written past the batch"
    return d_out.cpu().numpy(), ok[:n], res[:16 * n].view(QUIC_RESULT_DTYPE)


def result_tuple(r):
    return tuple(int(r[f]) for f in ("pn", "payload_len", "pn_len", "first_byte", "status", "reserved"))


def check_packets(ks, hp_ks, pkts, in_res=None, out_res=None, back_res=None):
    """seal of the cleartext packets == the reference packets over the whole 0xAA arena; open of those restores header ||
    payload with ok all 1 and the reference's results"""
    n = len(pkts)
    clear = [p.header + p.payload for p in pkts]
    in_offs, in_size = place([len(c) for c in clear], in_res)
    out_offs, out_size = place([len(p.packet) for p in pkts], out_res)
    arena_in, want = filled(in_size), filled(out_size)
    for c, p, i, o in zip(clear, pkts, in_offs, out_offs):
        put(arena_in, i, c)
        put(want, o, p.packet)
    got = gpu_seal(ks, hp_ks, seal_recs(pkts, in_offs, out_offs), arena_in, filled(out_size))
    bad = [i for i, (p, o) in enumerate(zip(pkts, out_offs)) if got[o:o + len(p.packet)].tobytes() != p.packet]
    assert not bad, f"sealed packets differ from the reference: {[(i, pkts[i].pn_len, len(pkts[i].header), len(pkts[i].payload)) for i in bad[:8]]}"
    assert np.array_equal(got, want), "bytes outside the packets were written"
    back_offs, back_size = place([len(c) for c in clear], back_res)
    want_back = filled(back_size)
    for c, o in zip(clear, back_offs):
        put(want_back, o, c)
    back, ok, res = gpu_open(ks, hp_ks, open_recs(pkts, out_offs, back_offs), got, filled(back_size))
    assert ok.tolist() == [1] * n, f"open refused packets {np.flatnonzero(ok != 1)[:8]}"
    bad = [i for i, (c, o) in enumerate(zip(clear, back_offs)) if back[o:o + len(c)].tobytes() != c]
    assert not bad, f"opened packets differ: {[(i, pkts[i].pn_len, len(pkts[i].header), len(pkts[i].payload)) for i in bad[:8]]}"
    assert np.array_equal(back, want_back), "bytes outside the opened packets were written"
    for i, p in enumerate(pkts):
        assert result_tuple(res[i]) == (p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK, 0), i


def assert_python_source_agrees(K, pkts, subset, hps=None):
    for i in subset:
        p = pkts[i]
        assert Q.protect(K.keys[p.k], K.ivs[p.k], (hps or K.hps)[p.k], p.pn, p.header, p.payload, "py") == p.packet, i


# ---- 1. RFC 9001 A.5


@pytest.mark.parametrize("width", WIDTHS)
def test_rfc9001_a5_vector(width, forced):
    v = {k: (bytes.fromhex(x) if isinstance(x, str) else x) for k, x in Q.load_kat()["packet"].items()}
    ks, hp_ks = pa.ChaChaKeyset(v["key"], v["iv"]), pa.ChaChaKeyset(v["hp"], bytes(12))
    forced(width, 0)
    assert v["packet"][5:21] == v["sample"]  # the sample covers the tag
    for expected in (v["pn"], v["pn"] - 1):
        p = Pkt(0, v["pn"], v["header"], v["payload"], v["packet"], expected, 0)
        check_packets(ks, hp_ks, [p])
    ks.free(), hp_ks.free()


# ---- 2. every small shape


@functools.lru_cache(maxsize=None)
def _every_shape():
    rng = np.random.default_rng(2000)
    K = Keys.make(rng, 2)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        lens = list(range(4 - pn_len, 151)) + [191, 192, 193, 255, 256, 257, 1200, 1452, 4095, 4096, 4097, 16384, 65527]
        for i, ln in enumerate(lens):
            long = i % 7 == 3
            body = 6 + i % 40 if long else i % 21  # short headers: DCIDs of 0 .. 20 bytes
            pkts.append(make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long, phase=(i >> 1) & 1))
    assert_python_source_agrees(K, pkts, list(range(0, len(pkts), 9)) + [i for i, p in enumerate(pkts) if len(p.payload) == 1200])
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_every_small_shape(width, cap, forced):
    K, pkts = _every_shape()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    pa.chacha_debug_counters(reset=True)
    check_packets(ks, hp_ks, pkts)
    ran = pa.chacha_debug_counters(reset=True)
    assert ran[width] == 2 and sum(ran.values()) == 2, ran  # one seal launch, one batch launch of the open, at the forced width
    ks.free(), hp_ks.free()


# ---- 3. AAD block edges


@functools.lru_cache(maxsize=None)
def _aad_edges():
    rng = np.random.default_rng(3000)
    K = Keys.make(rng, 1)
    pkts = []
    for hlen in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300):  # (17, 33, 49: a 4-byte packet number across a block edge)
        for pn_len in (1, 2, 3, 4):
            for ln in (3, 20, 1200):
                long = hlen == 300 or (hlen + pn_len) % 3 == 0
                pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), pn_len, hlen - 1 - pn_len, ln, long))
    assert all(len(p.header) in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300) for p in pkts)
    assert_python_source_agrees(K, pkts, range(0, len(pkts), 5))
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_aad_block_edges(width, cap, forced):
    K, pkts = _aad_edges()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    check_packets(ks, hp_ks, pkts)
    ks.free(), hp_ks.free()


# ---- 4. the sample reaching the tag


@functools.lru_cache(maxsize=None)
def _sample_in_tag():
    rng = np.random.default_rng(4000)
    K = Keys.make(rng, 2)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        for ln in range(4 - pn_len, 20 - pn_len):  # pn_len + len >= 4 and len < 20 - pn_len
            for body in (0, 8, 20):
                pkts.append(make_pkt(K, rng, len(pkts) & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long=body == 20))
    assert len(pkts) == 64 * 3
    assert_python_source_agrees(K, pkts, range(0, len(pkts), 3))
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_sample_reaches_the_tag(width, cap, forced):
    K, pkts = _sample_in_tag()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    res = [(3 * i + 1) % 16 for i in range(len(pkts))]
    check_packets(ks, hp_ks, pkts, in_res=res, out_res=res[::-1], back_res=res)
    ks.free(), hp_ks.free()


# ---- 5. byte offsets and in place


@functools.lru_cache(maxsize=None)
def _offset_pkts():
    rng = np.random.default_rng(5000)
    K = Keys.make(rng, 1)
    pkts = []
    for ln in (5, 63, 64, 65, 1200):
        for k in range(16):
            pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), k % 4 + 1, (5 * k) % 21, ln, long=k == 7))
    assert_python_source_agrees(K, pkts, range(0, len(pkts), 8))
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_odd_offsets(width, cap, forced):
    K, pkts = _offset_pkts()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    n = len(pkts)
    check_packets(ks, hp_ks, pkts, in_res=[i % 16 for i in range(n)], out_res=[(i + 5) % 16 for i in range(n)],
                  back_res=[(i + 11) % 16 for i in range(n)])
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("width, cap", MODES)
def test_in_place_seal_then_open(width, cap, forced):
    K, pkts = _offset_pkts()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    n = len(pkts)
    offs, size = place([len(p.packet) for p in pkts], [(7 * i + 3) % 16 for i in range(n)])
    arena, sealed = filled(size), filled(size)
    for p, o in zip(pkts, offs):
        put(arena, o, p.header + p.payload)  # room for the tag behind every packet
        put(sealed, o, p.packet)
    d_arena = dev(arena)
    d_recs = dev(seal_recs(pkts, offs, offs))
    pa.chacha_seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), sealed), "in-place seal"
    d_recs = dev(open_recs(pkts, offs, offs))
    d_ok, d_res = empty(n, FILL), empty(16 * n, FILL)
    pa.chacha_open_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), d_ok.data_ptr(),
                                d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().tolist() == [1] * n
    opened = sealed.copy()  # header || payload back where they were, the 16 bytes behind them as the seal left them
    for p, o in zip(pkts, offs):
        put(opened, o, p.header + p.payload)
    assert np.array_equal(d_arena.cpu().numpy(), opened), "in-place open"
    res = d_res.cpu().numpy().view(QUIC_RESULT_DTYPE)
    assert [result_tuple(r) for r in res] == [(p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK, 0) for p in pkts]
    ks.free(), hp_ks.free()


# ---- 6. many connections


@functools.lru_cache(maxsize=None)
def _many_connections():
    rng = np.random.default_rng(6000)
    nk = 300
    K = Keys.make(rng, nk)
    order = rng.permutation(np.repeat(np.arange(nk), 2))
    pkts = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, int(rng.integers(3, 1300)),
                     phase=int(rng.integers(0, 2))) for k in order]
    same = [make_pkt(K, rng, int(k), p.pn, p.pn_len, 8, len(p.payload), phase=p.phase, hps=K.keys) for k, p in zip(order, pkts)]
    assert_python_source_agrees(K, pkts, range(0, len(pkts), 40))
    assert_python_source_agrees(K, same, range(0, len(same), 60), hps=K.keys)
    return K, pkts, same


@pytest.mark.parametrize("width, cap", MODES)
def test_many_connections(width, cap, forced):
    K, pkts, same = _many_connections()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    check_packets(ks, hp_ks, pkts)
    check_packets(ks, ks, same)  # hp_ks the same object as ks: connection k's header-protection key is its AEAD key
    ks.free(), hp_ks.free()


# ---- 7. packet-number reconstruction on the device


@functools.lru_cache(maxsize=None)
def _pn_cases():
    rng = np.random.default_rng(7000)
    K = Keys.make(rng, 1)
    good, lost = [], []
    for pn_len in (1, 2, 3, 4):
        win = 1 << (8 * pn_len)
        hwin = win // 2
        base = int(rng.integers(1 << 33, 1 << 61)) & ~(win - 1)
        cases = [
            (base + 5, base - 3),                 # expected low in its window, the packet late: the candidate steps down
            (base + win - 4, base + win + 2),     # expected high in its window, the packet ahead: steps up
            (base + hwin, base + hwin + 9),       # stays
            (base + hwin, base + 1), (base + hwin, base + win - 1),  # stays, at both ends of the window
            (base + hwin, base + win),            # expected + hwin: the last number still recovered
            (0, 0), (0, hwin), (1, 0), (hwin + 3, 4),  # near zero: there is no window below
            (TOP, TOP), (TOP, TOP - hwin + 1), (TOP - 1, TOP), (TOP - win, TOP - hwin),  # near 2^62 - 1: none above
        ]
        for expected, pn in cases:
            assert Q.decode_pn(expected, pn & (win - 1), pn_len) == pn, (pn_len, expected, pn)
            good.append(make_pkt(K, rng, 0, pn, pn_len, 8, 30, expected=expected))
        # out of the window: the device must reconstruct what A.3 gives, a different number, so the packet fails
        for expected, pn in ((base + hwin, base - hwin), (base + 5, base + 5 + hwin + 1)):
            assert Q.decode_pn(expected, pn & (win - 1), pn_len) != pn
            lost.append(make_pkt(K, rng, 0, pn, pn_len, 8, 30, expected=expected))
    return K, good, lost


@pytest.mark.parametrize("width, cap", MODES)
def test_packet_number_reconstruction(width, cap, forced):
    K, good, lost = _pn_cases()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    pkts = good + lost
    in_offs, in_size = place([len(p.packet) for p in pkts])
    out_offs, out_size = place([len(p.packet) - 16 for p in pkts])
    arena = filled(in_size)
    for p, o in zip(pkts, in_offs):
        put(arena, o, p.packet)
    back, ok, res = gpu_open(ks, hp_ks, open_recs(pkts, in_offs, out_offs), arena, filled(out_size))
    for i, p in enumerate(pkts):
        win = 1 << (8 * p.pn_len)
        want_pn = Q.decode_pn(p.expected, p.pn & (win - 1), p.pn_len)
        assert int(res[i]["pn"]) == want_pn, (i, p.pn_len, p.expected, p.pn)
        if i < len(good):
            assert want_pn == p.pn and int(ok[i]) == 1 and int(res[i]["status"]) == QUIC_OK, (i, p.pn_len, p.expected, p.pn)
            assert back[out_offs[i]:out_offs[i] + len(p.packet) - 16].tobytes() == p.header + p.payload
        else:
            assert int(ok[i]) == 0 and int(res[i]["status"]) == QUIC_BAD_MAC, (i, p.pn_len, p.expected, p.pn)
    ks.free(), hp_ks.free()


# ---- 8. tampering


def _open_mixed(ks, hp_ks, K, pkts, packets, recs_edit=None):
    """opens ``packets`` (pkts' reference packets, some altered) and checks every one against the reference's verdict
    on the same bytes: ok, results, the output of those that opened, nothing written outside; returns the statuses"""
    n = len(pkts)
    in_offs, in_size = place([len(x) for x in packets])
    out_offs, out_size = place([len(x) - 16 for x in packets])
    arena = filled(in_size)
    for x, o in zip(packets, in_offs):
        put(arena, o, x)
    recs = open_recs(pkts, in_offs, out_offs)
    if recs_edit is not None:
        recs_edit(recs)
    back, ok, res = gpu_open(ks, hp_ks, recs, arena, filled(out_size))
    want_back = filled(out_size)
    for i, (p, x) in enumerate(zip(pkts, packets)):
        r = recs[i]
        k = int(r["key_idx"])
        o, region = out_offs[i], int(r["aad_len"]) + int(r["len"]) - 16
        if k >= len(K.keys) or k >= len(K.hps):
            w = Q.Opened(Q.REJECTED)
        else:
            w = Q.unprotect(K.keys[k], K.ivs[k], K.hps[k], int(r["seq"]), int(r["aad_len"]), x[:int(r["aad_len"]) + int(r["len"])],
                            int(r["flags"]) & 1)
        assert int(res[i]["status"]) == w.status and int(ok[i]) == (1 if w.status == Q.OK else 0), (i, w.status, result_tuple(res[i]))
        if w.status == Q.OK:
            put(want_back, o, w.header + w.payload)
            assert result_tuple(res[i]) == (w.pn, len(w.payload), w.pn_len, w.first_byte, QUIC_OK, 0), i
        elif w.status == Q.BAD_MAC:
            want_back[o:o + region] = back[o:o + region]  # unspecified bytes, within the packet's own output region
            assert result_tuple(res[i])[:4] == (w.pn, int(r["len"]) - w.pn_len - 16, w.pn_len, w.first_byte), i
        elif w.status == Q.KEY_PHASE:
            assert result_tuple(res[i])[:4] == (w.pn, int(r["len"]) - w.pn_len - 16, w.pn_len, w.first_byte), i
    assert np.array_equal(back, want_back), "a packet that did not open was written to, or bytes outside the packets were"
    return [int(s) for s in res["status"]]


@functools.lru_cache(maxsize=None)
def _tamper_pkts():
    rng = np.random.default_rng(8000)
    K = Keys.make(rng, 2)
    pkts = [make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), i % 4 + 1, 8 + i % 5, int(rng.integers(40, 1500)), long=i % 4 == 3,
                     phase=(i >> 2) & 1) for i in range(64)]
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_tampering(width, cap, forced):
    K, pkts = _tamper_pkts()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    rng = np.random.default_rng(8001)
    for kind in ("first", "pn", "dcid", "ciphertext", "tag"):
        hit = rng.random(64) < 0.4
        hit[int(rng.integers(0, 64))] = True
        packets = []
        for p, h in zip(pkts, hit):
            x = bytearray(p.packet)
            if h:
                hl = len(p.header)
                if kind == "first":
                    # a protected bit of the first byte: the packet-number length or a reserved bit (the key-phase bit
                    # of a short header has a verdict of its own, test_key_phase)
                    x[0] ^= 1 << int(rng.choice([0, 1, 2, 3] if p.header[0] & 0x80 else [0, 1, 3, 4]))
                elif kind == "pn":
                    x[hl - 1 - int(rng.integers(0, p.pn_len))] ^= 1 << int(rng.integers(0, 8))
                elif kind == "dcid":
                    x[1 + int(rng.integers(0, hl - 1 - p.pn_len))] ^= 1 << int(rng.integers(0, 8))
                elif kind == "ciphertext":
                    # behind the sample (the 16 bytes from ciphertext offset 4 - pn_len): a flip inside it changes the
                    # mask too, and with it a short header's key-phase bit half the time (the case below)
                    x[hl + int(rng.integers(20, len(p.payload)))] ^= 1 << int(rng.integers(0, 8))
                else:
                    x[len(x) - 1 - int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
            packets.append(bytes(x))
        status = _open_mixed(ks, hp_ks, K, pkts, packets)
        assert status == [QUIC_BAD_MAC if h else QUIC_OK for h in hit], kind  # every tampered packet fails, no other
    # a flip inside the sample: the packet fails with the verdict the reference gives for the same bytes (BAD_MAC, or
    # KEY_PHASE where the changed mask turns a short header's key-phase bit), every other packet opens
    packets = []
    for i, p in enumerate(pkts):
        x = bytearray(p.packet)
        if i % 2:
            x[len(p.header) + 4 - p.pn_len + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        packets.append(bytes(x))
    status = _open_mixed(ks, hp_ks, K, pkts, packets)
    assert all((s == QUIC_OK) == (i % 2 == 0) for i, s in enumerate(status)) and QUIC_BAD_MAC in status and QUIC_KEY_PHASE in status
    ks.free(), hp_ks.free()


# ---- 9. rejections


@pytest.mark.parametrize("width, cap", MODES)
def test_rejections(width, cap, forced):
    rng = np.random.default_rng(9000)
    K = Keys.make(rng, 3)
    K.hps = K.hps[:2]  # key_idx 2 is beyond hp_ks only, 3 beyond both
    ks, hp_ks = K.keysets()
    forced(width, cap)
    Kfull = Keys(K.keys, K.ivs, K.hps + [bytes(32)])
    pkts = [make_pkt(Kfull, rng, i % 2, int(rng.integers(0, 2**62)), i % 4 + 1, 8, 40 + 13 * i) for i in range(12)]
    n = len(pkts)
    clear = [p.header + p.payload for p in pkts]
    in_offs, in_size = place([len(c) for c in clear])
    out_offs, out_size = place([len(p.packet) for p in pkts])
    arena_in, want = filled(in_size), filled(out_size)
    recs = seal_recs(pkts, in_offs, out_offs)
    bad = {1: "sample", 3: "header", 5: "key beyond hp_ks", 7: "key beyond both", 8: "flags", 10: "len"}
    recs[1]["len"] = 3 - pkts[1].pn_len          # pn_len + len = 3: no full sample
    recs[3]["aad_len"] = pkts[3].pn_len          # aad_len < 1 + pn_len
    recs[5]["key_idx"], recs[7]["key_idx"] = 2, 3
    recs[8]["flags"] = 1
    recs[10]["len"] = (1 << 30) + 1
    for i, (c, p, a, o) in enumerate(zip(clear, pkts, in_offs, out_offs)):
        put(arena_in, a, c)
        if i not in bad:
            put(want, o, p.packet)
    got = gpu_seal(ks, hp_ks, recs, arena_in, filled(out_size))
    assert np.array_equal(got, want), "a rejected descriptor was written for, or a neighbour was not sealed"

    # open: all twelve reference packets, six descriptors out of the limits
    arena = filled(out_size)
    for p, o in zip(pkts, out_offs):
        put(arena, o, p.packet)
    back_offs, back_size = place([len(c) for c in clear])
    opn = open_recs(pkts, out_offs, back_offs)
    opn[1]["len"] = 19       # 19 bytes from the packet number on: no room for a sample
    opn[3]["aad_len"] = 0    # no first byte ahead of the packet number
    opn[5]["key_idx"], opn[7]["key_idx"] = 2, 3
    opn[8]["len"] = 0
    opn[10]["len"] = (1 << 30) + 1
    back, ok, res = gpu_open(ks, hp_ks, opn, arena, filled(back_size))
    want_back = filled(back_size)
    for i, (c, o) in enumerate(zip(clear, back_offs)):
        if i not in bad:
            put(want_back, o, c)
    assert ok.tolist() == [0 if i in bad else 1 for i in range(n)]
    assert [int(s) for s in res["status"]] == [QUIC_REJECTED if i in bad else QUIC_OK for i in range(n)]
    assert np.array_equal(back, want_back), "a rejected packet was written for, or a neighbour was not opened"
    ks.free(), hp_ks.free()


# ---- 10. invalid arguments


@pytest.mark.parametrize("width", WIDTHS)
def test_invalid_arguments(width, forced):
    rng = np.random.default_rng(10000)
    K = Keys.make(rng, 1)
    ks, hp_ks = K.keysets()
    forced(width, 0)
    p = make_pkt(K, rng, 0, 5, 2, 8, 100)
    arena = filled(256)
    put(arena, 16, p.packet)
    d_recs, d_in, d_out = dev(open_recs([p], [16], [16])), dev(arena), dev(filled(256))
    d_ok, d_res = empty(1, FILL), empty(16, FILL)
    lib = pa.load_library()
    args = (d_recs.data_ptr(), 1, d_in.data_ptr(), d_out.data_ptr())
    assert lib.ptls_mi355x_chacha_open_quic_packets(ks.handle, hp_ks.handle, *args, d_ok.data_ptr(), None, None) == -1  # results
    assert lib.ptls_mi355x_chacha_open_quic_packets(ks.handle, hp_ks.handle, *args, None, d_res.data_ptr(), None) == -1   # ok
    assert lib.ptls_mi355x_chacha_open_quic_packets(ks.handle, None, *args, d_ok.data_ptr(), d_res.data_ptr(), None) == -1  # hp_ks
    assert lib.ptls_mi355x_chacha_seal_quic_packets(ks.handle, None, *args, None) == -1
    assert lib.ptls_mi355x_chacha_seal_quic_packets(None, hp_ks.handle, *args, None) == -1
    with pytest.raises(pa.EngineError):
        pa.chacha_open_quic_packets(ks, hp_ks, *args, d_ok.data_ptr(), 0, _stream())
    with pytest.raises(pa.EngineError):
        pa.chacha_seal_quic_packets(ks, None, *args, _stream())
    # an empty batch is no error and touches nothing
    assert lib.ptls_mi355x_chacha_seal_quic_packets(ks.handle, hp_ks.handle, None, 0, None, None, None) == 0
    assert lib.ptls_mi355x_chacha_open_quic_packets(ks.handle, hp_ks.handle, None, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_ok.cpu().numpy() == FILL).all() and (d_res.cpu().numpy() == FILL).all()
    ks.free(), hp_ks.free()


# ---- 11. key phase


@functools.lru_cache(maxsize=None)
def _phase_pkts():
    rng = np.random.default_rng(11000)
    K = Keys.make(rng, 1)
    pkts = []
    for i in range(16):
        pkts.append(make_pkt(K, rng, 0, 1000 + i, i % 4 + 1, 8, 20 + 70 * i, long=i % 4 == 2, phase=(i >> 2) & 1))
    return K, pkts


@pytest.mark.parametrize("width, cap", MODES)
def test_key_phase(width, cap, forced):
    K, pkts = _phase_pkts()
    ks, hp_ks = K.keysets()
    forced(width, cap)
    packets = [p.packet for p in pkts]

    def flip_all(recs):
        recs["flags"] ^= 1

    # the wrong expected phase: short headers get KEY_PHASE, ok = 0 and keep their sentinel (checked whole-arena in
    # _open_mixed); long headers ignore the bit and open
    status = _open_mixed(ks, hp_ks, K, pkts, packets, recs_edit=flip_all)
    assert status == [QUIC_OK if p.header[0] & 0x80 else QUIC_KEY_PHASE for p in pkts]
    # the same packets with the right phase all open
    assert _open_mixed(ks, hp_ks, K, pkts, packets) == [QUIC_OK] * len(pkts)
    ks.free(), hp_ks.free()


# ---- 12. ordering


@pytest.mark.parametrize("width", WIDTHS)
def test_free_and_rekey_of_hp_ks_right_after_launch_are_ordered(width, forced):
    """In the shape of test_free_and_rekey_right_after_launch_are_ordered (test_gpu_chacha.py), for the second keyset of
    the call: a rekey and a free of hp_ks made right after a launch on a side stream order themselves behind it, so the
    packets carry the old header-protection key's masks."""
    rng = np.random.default_rng(12000 + width)
    n = 2000
    forced(width, 0)
    K = Keys.make(rng, 1)
    side = torch.cuda.Stream("cuda:0")
    pns = [int(x) for x in rng.integers(0, 2**62, n)]
    headers = [header_for(rng, pn, i % 4 + 1, 8) for i, pn in enumerate(pns)]
    payloads = [rng.bytes(1200) for _ in range(n)]
    in_offs, in_size = place([len(h) + 1200 for h in headers])
    out_offs, out_size = place([len(h) + 1216 for h in headers])
    arena_in = filled(in_size)
    recs = np.zeros(n, RECORD_DTYPE)
    for r, h, pl, pn, i, o in zip(recs, headers, payloads, pns, in_offs, out_offs):
        put(arena_in, i, h + pl)
        r["in_off"], r["out_off"], r["seq"], r["len"], r["aad_len"] = i, o, pn, 1200, len(h)
    d_recs, d_in = dev(recs), dev(arena_in)
    ks = pa.ChaChaKeyset(K.keys[0], K.ivs[0])
    outs = []
    for _ in range(3):
        hp1, hp2 = rng.bytes(32), rng.bytes(32)
        hp_ks = pa.ChaChaKeyset(hp1, bytes(12))
        d_first, d_second = empty(out_size, FILL), empty(out_size, FILL)
        side.wait_stream(torch.cuda.current_stream())  # the inputs and the filled outputs are ready
        pa.chacha_seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_first.data_ptr(), side.cuda_stream)
        hp_ks.update([0], hp2, bytes(12))  # immediately, with the batch most likely still running
        pa.chacha_seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_second.data_ptr(), _stream())
        hp_ks.free()
        outs.append(((hp1, d_first), (hp2, d_second)))
    torch.cuda.synchronize()
    for rnd, pair in enumerate(outs):
        for which, (hp, d_out) in zip(("launch before the rekey", "launch after the rekey"), pair):
            got = d_out.cpu().numpy()
            want = filled(out_size)
            for h, pl, pn, o in zip(headers, payloads, pns, out_offs):
                put(want, o, Q.protect(K.keys[0], K.ivs[0], hp, pn, h, pl))
            bad = [i for i, (h, o) in enumerate(zip(headers, out_offs)) if not np.array_equal(got[o:o + len(h) + 1216], want[o:o + len(h) + 1216])]
            assert not bad, f"round {rnd}, {which}: {len(bad)} of {n} packets differ from the reference, first {bad[:4]}"
            assert np.array_equal(got, want)
    ks.free()
