"""What the GPU tests of QUIC packet protection share (test_gpu_chacha_quic.py, test_gpu_quic_aes.py): the packets and
their placement in 0xAA arenas, the descriptors, the seal and open calls with their checks against the reference, and the
case generators. Everything is parametrised by a Suite; a generator's packets depend on the suite and its own arguments
only, so its result is cached and shared by the tests (and modes) that use it. Not a test module."""
import functools
from dataclasses import dataclass
from typing import Any, Callable

import numpy as np
import torch

from gpu_util import dev, empty
from picotls_amd.records import QUIC_OK, QUIC_RESULT_DTYPE, RECORD_DTYPE

FILL = 0xAA
TOP = (1 << 62) - 1


@dataclass(frozen=True)
class Suite:
    keyset: Callable[[bytes, bytes, int], Any]  # (keys, ivs, key size) -> an engine keyset
    key_size: int
    hp_size: int       # the header-protection keys' size ...
    alt_hp_size: int   # ... and the one of sample_in_tag (AES: the other size than the AEAD keys')
    seal: Callable     # the engine's calls: (ks, hp_ks, recs, n, in, out, stream), and with ok, results before stream
    open: Callable
    ref: Any           # the reference module: protect, unprotect, decode_pn, Opened, the statuses
    second: str        # ref's second source (its ``impl``)
    seed: int          # added to every generator's seed


def stream():
    return torch.cuda.current_stream().cuda_stream


@dataclass
class Keys:
    suite: Suite
    keys: list
    ivs: list
    hps: list

    @classmethod
    def make(cls, suite, rng, n, hp_size=None):
        return cls(suite, [rng.bytes(suite.key_size) for _ in range(n)], [rng.bytes(12) for _ in range(n)],
                   [rng.bytes(hp_size or suite.hp_size) for _ in range(n)])

    def keysets(self):
        return (self.suite.keyset(b"".join(self.keys), b"".join(self.ivs), len(self.keys[0])),
                self.suite.keyset(b"".join(self.hps), bytes(12 * len(self.hps)), len(self.hps[0])))


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
    packet = K.suite.ref.protect(K.keys[k], K.ivs[k], (hps or K.hps)[k], pn, header, payload)
    return Pkt(k, pn, header, payload, packet, pn if expected is None else expected, phase)


def place(sizes, residues=None, align=16):
    """offsets of items of these sizes with at least 16 untouched bytes around each; item i at residues[i] mod align"""
    offs, at = [], align
    for i, n in enumerate(sizes):
        at = (at + align - 1) // align * align + (residues[i] if residues is not None else 0)
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


def gpu_seal(suite, ks, hp_ks, recs, arena_in, arena_out):
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    suite.seal(ks, hp_ks, d_recs.data_ptr(), len(recs), d_in.data_ptr(), d_out.data_ptr(), stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def gpu_open(suite, ks, hp_ks, recs, arena_in, arena_out):
    n = len(recs)
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    d_ok, d_res = empty(n + 16, FILL), empty(16 * n + 16, FILL)
    suite.open(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), stream())
    torch.cuda.synchronize()
    ok, res = d_ok.cpu().numpy(), d_res.cpu().numpy()
    assert (ok[n:] == FILL).all() and (res[16 * n:] == FILL).all(), "ok or results written past the batch"
    return d_out.cpu().numpy(), ok[:n], res[:16 * n].view(QUIC_RESULT_DTYPE)


def result_tuple(r):
    return tuple(int(r[f]) for f in ("pn", "payload_len", "pn_len", "first_byte", "status", "reserved"))


def want_results(pkts):
    """the results of opening the reference packets: everything as sealed, status OK, reserved 0"""
    want = np.zeros(len(pkts), QUIC_RESULT_DTYPE)
    for w, p in zip(want, pkts):
        w["pn"], w["payload_len"], w["pn_len"], w["first_byte"], w["status"] = p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK
    return want


def _shape(pkts, i):
    return i, pkts[i].pn_len, len(pkts[i].header), len(pkts[i].payload)


def check_packets(suite, ks, hp_ks, pkts, in_res=None, out_res=None, back_res=None, align=16):
    """seal of the cleartext packets == the reference packets over the whole 0xAA arena; open of those restores header ||
    payload with ok all 1 and the reference's results"""
    n = len(pkts)
    clear = [p.header + p.payload for p in pkts]
    in_offs, in_size = place([len(c) for c in clear], in_res, align)
    out_offs, out_size = place([len(p.packet) for p in pkts], out_res, align)
    arena_in, want = filled(in_size), filled(out_size)
    for c, p, i, o in zip(clear, pkts, in_offs, out_offs):
        put(arena_in, i, c)
        put(want, o, p.packet)
    got = gpu_seal(suite, ks, hp_ks, seal_recs(pkts, in_offs, out_offs), arena_in, filled(out_size))
    if not np.array_equal(got, want):
        bad = [i for i, (p, o) in enumerate(zip(pkts, out_offs)) if got[o:o + len(p.packet)].tobytes() != p.packet]
        assert not bad, f"{len(bad)} sealed packets differ from the reference: {[_shape(pkts, i) for i in bad[:8]]}"
        assert False, "bytes outside the packets were written"
    back_offs, back_size = place([len(c) for c in clear], back_res, align)
    want_back = filled(back_size)
    for c, o in zip(clear, back_offs):
        put(want_back, o, c)
    back, ok, res = gpu_open(suite, ks, hp_ks, open_recs(pkts, out_offs, back_offs), got, filled(back_size))
    assert ok.tolist() == [1] * n, f"open refused packets {[_shape(pkts, int(i)) for i in np.flatnonzero(ok != 1)[:8]]}"
    if not np.array_equal(back, want_back):
        bad = [i for i, (c, o) in enumerate(zip(clear, back_offs)) if back[o:o + len(c)].tobytes() != c]
        assert not bad, f"{len(bad)} opened packets differ: {[_shape(pkts, i) for i in bad[:8]]}"
        assert False, "bytes outside the opened packets were written"
    bad = np.flatnonzero(res != want_results(pkts))
    assert bad.size == 0, [(int(i), result_tuple(res[i])) for i in bad[:8]]


def assert_second_source_agrees(K, pkts, subset, hps=None):
    for i in subset:
        p = pkts[i]
        assert K.suite.ref.protect(K.keys[p.k], K.ivs[p.k], (hps or K.hps)[p.k], p.pn, p.header, p.payload, K.suite.second) == p.packet, i


def open_mixed(ks, hp_ks, K, pkts, packets, recs_edit=None):
    """opens ``packets`` (pkts' reference packets, some altered) and checks every one against the reference's verdict
    on the same bytes: ok, results, the output of those that opened, nothing written outside; returns the statuses"""
    Q = K.suite.ref
    in_offs, in_size = place([len(x) for x in packets])
    out_offs, out_size = place([len(x) - 16 for x in packets])
    arena = filled(in_size)
    for x, o in zip(packets, in_offs):
        put(arena, o, x)
    recs = open_recs(pkts, in_offs, out_offs)
    if recs_edit is not None:
        recs_edit(recs)
    back, ok, res = gpu_open(K.suite, ks, hp_ks, recs, arena, filled(out_size))
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


# ---- the case generators: (Keys, packets ...) of a suite


@functools.lru_cache(maxsize=None)
def every_shape(suite):
    rng = np.random.default_rng(2000 + suite.seed)
    K = Keys.make(suite, rng, 2)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        lens = list(range(4 - pn_len, 151)) + [191, 192, 193, 255, 256, 257, 1200, 1452, 4095, 4096, 4097, 16384, 65527]
        for i, ln in enumerate(lens):
            long = i % 7 == 3
            body = 6 + i % 40 if long else i % 21  # short headers: DCIDs of 0 .. 20 bytes
            pkts.append(make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long, phase=(i >> 1) & 1))
    assert_second_source_agrees(K, pkts, list(range(0, len(pkts), 9)) + [i for i, p in enumerate(pkts) if len(p.payload) == 1200])
    return K, pkts


@functools.lru_cache(maxsize=None)
def aad_edges(suite):
    rng = np.random.default_rng(3000 + suite.seed)
    K = Keys.make(suite, rng, 1)
    pkts = []
    for hlen in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300):  # (17, 33, 49: a 4-byte packet number across a block edge)
        for pn_len in (1, 2, 3, 4):
            for ln in (3, 20, 1200):
                long = hlen == 300 or (hlen + pn_len) % 3 == 0
                pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), pn_len, hlen - 1 - pn_len, ln, long))
    assert all(len(p.header) in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300) for p in pkts)
    assert_second_source_agrees(K, pkts, range(0, len(pkts), 5))
    return K, pkts


@functools.lru_cache(maxsize=None)
def sample_in_tag(suite):
    rng = np.random.default_rng(4000 + suite.seed)
    K = Keys.make(suite, rng, 2, hp_size=suite.alt_hp_size)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        for ln in range(4 - pn_len, 20 - pn_len):  # pn_len + len >= 4 and len < 20 - pn_len
            for body in (0, 8, 20):
                pkts.append(make_pkt(K, rng, len(pkts) & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long=body == 20))
    assert len(pkts) == 64 * 3
    assert_second_source_agrees(K, pkts, range(0, len(pkts), 3))
    return K, pkts


@functools.lru_cache(maxsize=None)
def offset_pkts(suite, per_len, second_every):
    """per_len packets of each of five lengths, packet-number lengths and DCID lengths in rotation, every 16th a long header"""
    rng = np.random.default_rng(5000 + suite.seed)
    K = Keys.make(suite, rng, 1)
    pkts = []
    for ln in (5, 63, 64, 65, 1200):
        for k in range(per_len):
            pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), k % 4 + 1, (5 * k) % 21, ln, long=k % 16 == 7))
    assert_second_source_agrees(K, pkts, range(0, len(pkts), second_every))
    return K, pkts


@functools.lru_cache(maxsize=None)
def many_connections(suite, runs_of_8=False):
    """300 connections x 2 packets in random order; the same with each connection's AEAD key as its header-protection
    key; with runs_of_8, also 300 connections x 8 uniform packets in random order"""
    rng = np.random.default_rng(6000 + suite.seed)
    nk = 300
    K = Keys.make(suite, rng, nk)
    order = rng.permutation(np.repeat(np.arange(nk), 2))
    pkts = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, int(rng.integers(3, 1300)),
                     phase=int(rng.integers(0, 2))) for k in order]
    same = [make_pkt(K, rng, int(k), p.pn, p.pn_len, 8, len(p.payload), phase=p.phase, hps=K.keys) for k, p in zip(order, pkts)]
    mk = []
    if runs_of_8:
        order8 = rng.permutation(np.repeat(np.arange(nk), 8))
        mk = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, 1200) for k in order8]
    assert_second_source_agrees(K, pkts, range(0, len(pkts), 40))
    assert_second_source_agrees(K, same, range(0, len(same), 60), hps=K.keys)
    assert_second_source_agrees(K, mk, range(0, len(mk), 150))
    return K, pkts, same, mk


@functools.lru_cache(maxsize=None)
def pn_cases(suite):
    """packets whose number the expected one recovers (good) and packets out of its window (lost)"""
    Q = suite.ref
    rng = np.random.default_rng(7000 + suite.seed)
    K = Keys.make(suite, rng, 1)
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


@functools.lru_cache(maxsize=None)
def tamper_pkts(suite, n):
    rng = np.random.default_rng(8000 + suite.seed)
    K = Keys.make(suite, rng, 2)
    pkts = [make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), i % 4 + 1, 8 + i % 5, int(rng.integers(40, 1500)), long=i % 4 == 3,
                     phase=(i >> 2) & 1) for i in range(n)]
    return K, pkts


def tampered(rng, pkts, hit, kind):
    """pkts' reference packets, those of ``hit`` with one bit flipped in the part ``kind`` names"""
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
                # mask too, and with it a short header's key-phase bit half the time (tampered_in_sample)
                x[hl + int(rng.integers(20, len(p.payload)))] ^= 1 << int(rng.integers(0, 8))
            else:
                x[len(x) - 1 - int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        packets.append(bytes(x))
    return packets


def tampered_in_sample(rng, pkts):
    """every second packet with one bit flipped inside its sample"""
    packets = []
    for i, p in enumerate(pkts):
        x = bytearray(p.packet)
        if i % 2:
            x[len(p.header) + 4 - p.pn_len + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        packets.append(bytes(x))
    return packets


@functools.lru_cache(maxsize=None)
def phase_pkts(suite):
    rng = np.random.default_rng(11000 + suite.seed)
    K = Keys.make(suite, rng, 1)
    pkts = []
    for i in range(16):
        pkts.append(make_pkt(K, rng, 0, 1000 + i, i % 4 + 1, 8, 20 + 70 * i, long=i % 4 == 2, phase=(i >> 2) & 1))
    return K, pkts


# ---- checks both suites run on their own packets and modes


def check_in_place(suite, ks, hp_ks, pkts):
    """seal and then open with in == out: the packets where the cleartext was, and back"""
    n = len(pkts)
    offs, size = place([len(p.packet) for p in pkts], [(7 * i + 3) % 16 for i in range(n)])
    arena, sealed = filled(size), filled(size)
    for p, o in zip(pkts, offs):
        put(arena, o, p.header + p.payload)  # room for the tag behind every packet
        put(sealed, o, p.packet)
    d_arena = dev(arena)
    d_recs = dev(seal_recs(pkts, offs, offs))
    suite.seal(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), sealed), "in-place seal"
    d_recs = dev(open_recs(pkts, offs, offs))
    d_ok, d_res = empty(n, FILL), empty(16 * n, FILL)
    suite.open(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), stream())
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().tolist() == [1] * n
    opened = sealed.copy()  # header || payload back where they were, the 16 bytes behind them as the seal left them
    for p, o in zip(pkts, offs):
        put(opened, o, p.header + p.payload)
    assert np.array_equal(d_arena.cpu().numpy(), opened), "in-place open"
    res = d_res.cpu().numpy().view(QUIC_RESULT_DTYPE)
    assert [result_tuple(r) for r in res] == [(p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK, 0) for p in pkts]


def check_pn_reconstruction(suite, ks, hp_ks, good, lost):
    """pn_cases on the device: A.3's number in results for every packet; the good ones open, the lost ones fail the tag"""
    Q = suite.ref
    pkts = good + lost
    in_offs, in_size = place([len(p.packet) for p in pkts])
    out_offs, out_size = place([len(p.packet) - 16 for p in pkts])
    arena = filled(in_size)
    for p, o in zip(pkts, in_offs):
        put(arena, o, p.packet)
    back, ok, res = gpu_open(suite, ks, hp_ks, open_recs(pkts, in_offs, out_offs), arena, filled(out_size))
    for i, p in enumerate(pkts):
        win = 1 << (8 * p.pn_len)
        want_pn = Q.decode_pn(p.expected, p.pn & (win - 1), p.pn_len)
        assert int(res[i]["pn"]) == want_pn, (i, p.pn_len, p.expected, p.pn)
        if i < len(good):
            assert want_pn == p.pn and int(ok[i]) == 1 and int(res[i]["status"]) == Q.OK, (i, p.pn_len, p.expected, p.pn)
            assert back[out_offs[i]:out_offs[i] + len(p.packet) - 16].tobytes() == p.header + p.payload
        else:
            assert int(ok[i]) == 0 and int(res[i]["status"]) == Q.BAD_MAC, (i, p.pn_len, p.expected, p.pn)


def check_key_phase(ks, hp_ks, K, pkts):
    packets = [p.packet for p in pkts]

    def flip_all(recs):
        recs["flags"] ^= 1

    # the wrong expected phase: short headers get KEY_PHASE, ok = 0 and keep their sentinel (checked whole-arena in
    # open_mixed); long headers ignore the bit and open
    status = open_mixed(ks, hp_ks, K, pkts, packets, recs_edit=flip_all)
    assert status == [K.suite.ref.OK if p.header[0] & 0x80 else K.suite.ref.KEY_PHASE for p in pkts]
    # the same packets with the right phase all open
    assert open_mixed(ks, hp_ks, K, pkts, packets) == [K.suite.ref.OK] * len(pkts)


def check_rejections(suite, reps, before_launch=lambda: None):
    """twelve packets ``reps`` times over, six descriptors in twelve outside the limits: nothing is written for those,
    their neighbours are sealed and opened. before_launch() runs once the keysets exist."""
    Q = suite.ref
    rng = np.random.default_rng(9000 + suite.seed)
    K = Keys.make(suite, rng, 3)
    K.hps = K.hps[:2]  # key_idx 2 is beyond hp_ks only, 3 beyond both
    ks, hp_ks = K.keysets()
    before_launch()
    Kfull = Keys(suite, K.keys, K.ivs, K.hps + [bytes(suite.hp_size)])
    pkts = [make_pkt(Kfull, rng, i % 2, int(rng.integers(0, 2**62)), i % 4 + 1, 8, 40 + 13 * i) for i in range(12)] * reps
    n = len(pkts)
    clear = [p.header + p.payload for p in pkts]
    in_offs, in_size = place([len(c) for c in clear])
    out_offs, out_size = place([len(p.packet) for p in pkts])
    arena_in, want = filled(in_size), filled(out_size)
    recs = seal_recs(pkts, in_offs, out_offs)
    bad = {1: "sample", 3: "header", 5: "key beyond hp_ks", 7: "key beyond both", 8: "flags", 10: "len"}
    for b in range(0, n, 12):
        recs[b + 1]["len"] = 3 - pkts[1].pn_len          # pn_len + len = 3: no full sample
        recs[b + 3]["aad_len"] = pkts[3].pn_len          # aad_len < 1 + pn_len
        recs[b + 5]["key_idx"], recs[b + 7]["key_idx"] = 2, 3
        recs[b + 8]["flags"] = 1
        recs[b + 10]["len"] = (1 << 30) + 1
    for i, (c, p, a, o) in enumerate(zip(clear, pkts, in_offs, out_offs)):
        put(arena_in, a, c)
        if i % 12 not in bad:
            put(want, o, p.packet)
    got = gpu_seal(suite, ks, hp_ks, recs, arena_in, filled(out_size))
    assert np.array_equal(got, want), "a rejected descriptor was written for, or a neighbour was not sealed"

    # open: the reference packets, six descriptors in twelve out of the limits
    arena = filled(out_size)
    for p, o in zip(pkts, out_offs):
        put(arena, o, p.packet)
    back_offs, back_size = place([len(c) for c in clear])
    opn = open_recs(pkts, out_offs, back_offs)
    for b in range(0, n, 12):
        opn[b + 1]["len"] = 19       # 19 bytes from the packet number on: no room for a sample
        opn[b + 3]["aad_len"] = 0    # no first byte ahead of the packet number
        opn[b + 5]["key_idx"], opn[b + 7]["key_idx"] = 2, 3
        opn[b + 8]["len"] = 0
        opn[b + 10]["len"] = (1 << 30) + 1
    back, ok, res = gpu_open(suite, ks, hp_ks, opn, arena, filled(back_size))  # (checks that ok and results end at n)
    want_back = filled(back_size)
    for i, (c, o) in enumerate(zip(clear, back_offs)):
        if i % 12 not in bad:
            put(want_back, o, c)
    assert ok.tolist() == [0 if i % 12 in bad else 1 for i in range(n)]
    assert [int(s) for s in res["status"]] == [Q.REJECTED if i % 12 in bad else Q.OK for i in range(n)]
    assert np.array_equal(back, want_back), "a rejected packet was written for, or a neighbour was not opened"
    ks.free(), hp_ks.free()
