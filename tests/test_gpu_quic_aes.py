"""QUIC packet protection under AES-GCM on the GPU (ptls_mi355x_seal_quic_packets / ptls_mi355x_open_quic_packets), in
the sections of test_gpu_chacha_quic.py: every comparison is byte for byte against tests/quic_aes_ref.py (the system
libcrypto; a subset of each batch also against its second source, the project's plain-C oracle). Arenas start as 0xAA
and are compared whole, so a write outside a packet shows. Every case runs for AES-128 and AES-256; the references of a
case are computed once per key size and shared by its tests. debug_counters shows which kernel kinds ran where a case
exists to reach one.

Two of the kinds need more than the shapes the cases name, because of rules the dispatcher had before this frame and
keeps: a whole run in 4-lane groups needs 128 records in a workgroup's range (32,768 and more in a batch on 256 CUs), and
a multi-key run starts from a connection of three or more uniform records (MK_MIN_FIRST). 300 x 1200 B and 300
connections x 2 packets therefore run in cut runs (measured: w8_g4 = 0, w8_mk = 0 for them); each of those two tests runs
its named shape and a second batch that reaches the kind, and asserts the counter on that one."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import picotls_amd as pa
import quic_aes_ref as Q
from gpu_util import dev, empty
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, QUIC_REJECTED, QUIC_RESULT_DTYPE, RECORD_DTYPE

pytestmark = pytest.mark.gpu

FILL = 0xAA
KEY_SIZES = (16, 32)
TOP = (1 << 62) - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


@dataclass
class Keys:
    keys: list
    ivs: list
    hps: list

    @classmethod
    def make(cls, rng, n, key_size, hp_size=None):
        return cls([rng.bytes(key_size) for _ in range(n)], [rng.bytes(12) for _ in range(n)],
                   [rng.bytes(hp_size or key_size) for _ in range(n)])

    def keysets(self):
        return (pa.Keyset(b"".join(self.keys), b"".join(self.ivs), len(self.keys[0])),
                pa.Keyset(b"".join(self.hps), bytes(12 * len(self.hps)), len(self.hps[0])))


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


def gpu_seal(ks, hp_ks, recs, arena_in, arena_out):
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    pa.seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), len(recs), d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def gpu_open(ks, hp_ks, recs, arena_in, arena_out):
    n = len(recs)
    d_recs, d_in, d_out = dev(recs), dev(arena_in), dev(arena_out)
    d_ok, d_res = empty(n + 16, FILL), empty(16 * n + 16, FILL)
    pa.open_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    ok, res = d_ok.cpu().numpy(), d_res.cpu().numpy()
    assert (ok[n:] == FILL).all() and (res[16 * n:] == FILL).all(), "ok or results written past the batch"
    return d_out.cpu().numpy(), ok[:n], res[:16 * n].view(QUIC_RESULT_DTYPE)


def result_tuple(r):
    return tuple(int(r[f]) for f in ("pn", "payload_len", "pn_len", "first_byte", "status", "reserved"))


def _shape(pkts, i):
    return i, pkts[i].pn_len, len(pkts[i].header), len(pkts[i].payload)


def check_packets(ks, hp_ks, pkts, in_res=None, out_res=None, back_res=None, align=16):
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
    got = gpu_seal(ks, hp_ks, seal_recs(pkts, in_offs, out_offs), arena_in, filled(out_size))
    if not np.array_equal(got, want):
        bad = [i for i, (p, o) in enumerate(zip(pkts, out_offs)) if got[o:o + len(p.packet)].tobytes() != p.packet]
        assert not bad, f"{len(bad)} sealed packets differ from the reference: {[_shape(pkts, i) for i in bad[:8]]}"
        assert False, "bytes outside the packets were written"
    back_offs, back_size = place([len(c) for c in clear], back_res, align)
    want_back = filled(back_size)
    for c, o in zip(clear, back_offs):
        put(want_back, o, c)
    back, ok, res = gpu_open(ks, hp_ks, open_recs(pkts, out_offs, back_offs), got, filled(back_size))
    assert ok.tolist() == [1] * n, f"open refused packets {[_shape(pkts, int(i)) for i in np.flatnonzero(ok != 1)[:8]]}"
    if not np.array_equal(back, want_back):
        bad = [i for i, (c, o) in enumerate(zip(clear, back_offs)) if back[o:o + len(c)].tobytes() != c]
        assert not bad, f"{len(bad)} opened packets differ: {[_shape(pkts, i) for i in bad[:8]]}"
        assert False, "bytes outside the opened packets were written"
    want_res = np.zeros(n, QUIC_RESULT_DTYPE)
    for w, p in zip(want_res, pkts):
        w["pn"], w["payload_len"], w["pn_len"], w["first_byte"], w["status"] = p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK
    bad = np.flatnonzero(res != want_res)
    assert bad.size == 0, [(int(i), result_tuple(res[i])) for i in bad[:8]]


def assert_oracle_source_agrees(K, pkts, subset, hps=None):
    for i in subset:
        p = pkts[i]
        assert Q.protect(K.keys[p.k], K.ivs[p.k], (hps or K.hps)[p.k], p.pn, p.header, p.payload, "oracle") == p.packet, i


def counted(fn):
    """fn() between two resets of the debug counters: its launches and runs by kind"""
    pa.debug_counters(reset=True)
    fn()
    return pa.debug_counters(reset=True)


# ---- 1. every small shape


@functools.lru_cache(maxsize=None)
def _every_shape(key_size):
    rng = np.random.default_rng(2000 + key_size)
    K = Keys.make(rng, 2, key_size)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        lens = list(range(4 - pn_len, 151)) + [191, 192, 193, 255, 256, 257, 1200, 1452, 4095, 4096, 4097, 16384, 65527]
        for i, ln in enumerate(lens):
            long = i % 7 == 3
            body = 6 + i % 40 if long else i % 21  # short headers: DCIDs of 0 .. 20 bytes
            pkts.append(make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long, phase=(i >> 1) & 1))
    assert_oracle_source_agrees(K, pkts, list(range(0, len(pkts), 9)) + [i for i, p in enumerate(pkts) if len(p.payload) == 1200])
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_every_small_shape_one_batch(key_size):
    """above 256 packets: the serial W8 kernel (many-key form: two keys), and never the long-record kernel"""
    K, pkts = _every_shape(key_size)
    assert len(pkts) >= 256
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    assert c["launches"]["w8_serial"] == 2 and c["launches"]["w8_tree"] == 0 and c["launches"]["chunked"] == 0, c
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_every_small_shape_in_slices(key_size):
    """the same packets in slices of under 256: the 4-bit kernel (EXT 0)"""
    K, pkts = _every_shape(key_size)
    ks, hp_ks = K.keysets()
    step = 131
    c = counted(lambda: [check_packets(ks, hp_ks, pkts[a:a + step]) for a in range(0, len(pkts), step)])
    nslices = (len(pkts) + step - 1) // step
    assert c["launches"]["chunked"] == 2 * nslices and c["launches"]["w8_serial"] == 0, c
    ks.free(), hp_ks.free()


# ---- 2. AAD block edges


@functools.lru_cache(maxsize=None)
def _aad_edges(key_size):
    rng = np.random.default_rng(3000 + key_size)
    K = Keys.make(rng, 1, key_size)
    pkts = []
    for hlen in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300):  # (17, 33, 49: a 4-byte packet number across a block edge)
        for pn_len in (1, 2, 3, 4):
            for ln in (3, 20, 1200):
                long = hlen == 300 or (hlen + pn_len) % 3 == 0
                pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), pn_len, hlen - 1 - pn_len, ln, long))
    assert all(len(p.header) in (7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300) for p in pkts)
    assert_oracle_source_agrees(K, pkts, range(0, len(pkts), 5))
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_aad_block_edges(key_size):
    K, pkts = _aad_edges(key_size)
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts)                 # 132 packets: the 4-bit kernel
    check_packets(ks, hp_ks, pkts + pkts[::-1])    # 264: the serial W8 kernel
    ks.free(), hp_ks.free()


# ---- 3. the sample reaching the tag


@functools.lru_cache(maxsize=None)
def _sample_in_tag(key_size):
    rng = np.random.default_rng(4000 + key_size)
    K = Keys.make(rng, 2, key_size, hp_size=48 - key_size)  # (the header-protection keys of the other size)
    pkts = []
    for pn_len in (1, 2, 3, 4):
        for ln in range(4 - pn_len, 20 - pn_len):  # pn_len + len >= 4 and len < 20 - pn_len
            for body in (0, 8, 20):
                pkts.append(make_pkt(K, rng, len(pkts) & 1, int(rng.integers(0, 2**62)), pn_len, body, ln, long=body == 20))
    assert len(pkts) == 64 * 3
    assert_oracle_source_agrees(K, pkts, range(0, len(pkts), 3))
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_sample_reaches_the_tag(key_size):
    K, pkts = _sample_in_tag(key_size)
    ks, hp_ks = K.keysets()
    res = [(3 * i + 1) % 16 for i in range(len(pkts))]
    check_packets(ks, hp_ks, pkts, in_res=res, out_res=res[::-1], back_res=res)
    twice = pkts + pkts  # 384 packets: the serial W8 kernel
    res = [(5 * i + 2) % 16 for i in range(len(twice))]
    check_packets(ks, hp_ks, twice, in_res=res, out_res=res[::-1], back_res=res)
    ks.free(), hp_ks.free()


# ---- 4. byte offsets and in place


@functools.lru_cache(maxsize=None)
def _offset_pkts(key_size):
    rng = np.random.default_rng(5000 + key_size)
    K = Keys.make(rng, 1, key_size)
    pkts = []
    for ln in (5, 63, 64, 65, 1200):
        for k in range(64):
            pkts.append(make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), k % 4 + 1, (5 * k) % 21, ln, long=k % 16 == 7))
    assert_oracle_source_agrees(K, pkts, range(0, len(pkts), 16))
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_odd_offsets(key_size):
    K, pkts = _offset_pkts(key_size)
    ks, hp_ks = K.keysets()
    for sub in (pkts[::4], pkts):  # 80 packets (the 4-bit kernel), 320 (the serial W8 kernel)
        n = len(sub)
        check_packets(ks, hp_ks, sub, in_res=[i % 16 for i in range(n)], out_res=[(i + 5) % 16 for i in range(n)],
                      back_res=[(i + 11) % 16 for i in range(n)])
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_in_place_seal_then_open(key_size):
    K, all_pkts = _offset_pkts(key_size)
    ks, hp_ks = K.keysets()
    for pkts in (all_pkts[::4], all_pkts):
        n = len(pkts)
        offs, size = place([len(p.packet) for p in pkts], [(7 * i + 3) % 16 for i in range(n)])
        arena, sealed = filled(size), filled(size)
        for p, o in zip(pkts, offs):
            put(arena, o, p.header + p.payload)  # room for the tag behind every packet
            put(sealed, o, p.packet)
        d_arena = dev(arena)
        d_recs = dev(seal_recs(pkts, offs, offs))
        pa.seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert np.array_equal(d_arena.cpu().numpy(), sealed), "in-place seal"
        d_recs = dev(open_recs(pkts, offs, offs))
        d_ok, d_res = empty(n, FILL), empty(16 * n, FILL)
        pa.open_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_arena.data_ptr(), d_arena.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(),
                             _stream())
        torch.cuda.synchronize()
        assert d_ok.cpu().numpy().tolist() == [1] * n
        opened = sealed.copy()  # header || payload back where they were, the 16 bytes behind them as the seal left them
        for p, o in zip(pkts, offs):
            put(opened, o, p.header + p.payload)
        assert np.array_equal(d_arena.cpu().numpy(), opened), "in-place open"
        res = d_res.cpu().numpy().view(QUIC_RESULT_DTYPE)
        assert [result_tuple(r) for r in res] == [(p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK, 0) for p in pkts]
    ks.free(), hp_ks.free()


# ---- 5. one key: whole runs in 4-lane groups


@functools.lru_cache(maxsize=None)
def _one_key(key_size):
    rng = np.random.default_rng(5500 + key_size)
    K = Keys.make(rng, 1, key_size)
    pkts = [make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), i % 4 + 1, 8, 1200, phase=i & 1) for i in range(300)]
    assert_oracle_source_agrees(K, pkts, range(0, 300, 30))
    return K, pkts


@functools.lru_cache(maxsize=None)
def _one_key_block(key_size, n, payload_len):
    rng = np.random.default_rng(5600 + key_size + payload_len)
    K = Keys.make(rng, 1, key_size)
    pkts = [make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), i % 4 + 1, 8 + i % 3, payload_len, long=i % 11 == 0) for i in range(n)]
    assert_oracle_source_agrees(K, pkts, range(0, n, n // 8))
    return K, pkts


def check_tiled(ks, hp_ks, pkts, reps, in_shift, out_shift, back_shift):
    """check_packets for ``reps`` copies of ``pkts`` side by side in one batch, every arena a block of whole 128-byte lines
    repeated and the descriptors repeated with it (numpy tiling: tens of thousands of packets without a Python loop over
    them); packet i of a block at shift[i] within its line"""
    n = len(pkts)
    clear = [p.header + p.payload for p in pkts]

    def block(sizes, shift):
        offs, size = place(sizes, shift, 128)
        return offs, (size + 127) // 128 * 128

    in_offs, in_size = block([len(c) for c in clear], in_shift)
    out_offs, out_size = block([len(p.packet) for p in pkts], out_shift)
    back_offs, back_size = block([len(c) for c in clear], back_shift)
    arena_in, want, want_back = filled(in_size), filled(out_size), filled(back_size)
    for c, p, i, o, b in zip(clear, pkts, in_offs, out_offs, back_offs):
        put(arena_in, i, c), put(want, o, p.packet), put(want_back, b, c)

    def tiled(recs, isz, osz):
        t = np.tile(recs, reps)
        rep = np.repeat(np.arange(reps, dtype=np.uint64), n)
        t["in_off"] += rep * np.uint64(isz)
        t["out_off"] += rep * np.uint64(osz)
        return t

    def same(got, want_block, size, what):
        whole = np.tile(want_block, reps)
        if not np.array_equal(got, whole):
            at = int(np.flatnonzero(got != whole)[0])
            assert False, f"{what}: first difference in copy {at // size} at block offset {at % size}"

    got = gpu_seal(ks, hp_ks, tiled(seal_recs(pkts, in_offs, out_offs), in_size, out_size), np.tile(arena_in, reps), filled(out_size * reps))
    same(got, want, out_size, "seal")
    back, ok, res = gpu_open(ks, hp_ks, tiled(open_recs(pkts, out_offs, back_offs), out_size, back_size), got, filled(back_size * reps))
    assert (ok == 1).all(), f"open refused packets {np.flatnonzero(ok != 1)[:8]}"
    same(back, want_back, back_size, "open")
    want_res = np.zeros(n, QUIC_RESULT_DTYPE)
    for w, p in zip(want_res, pkts):
        w["pn"], w["payload_len"], w["pn_len"], w["first_byte"], w["status"] = p.pn, len(p.payload), p.pn_len, p.header[0], QUIC_OK
    assert np.array_equal(res, np.tile(want_res, reps)), "results"


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_one_key_300_packets(key_size):
    K, pkts = _one_key(key_size)
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    print("300 x 1200 B, one key:", c)
    assert c["launches"]["w8_serial"] == 2 and c["runs"]["w8_serial"] > 0, c
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_one_key_whole_runs_in_4_lane_groups(key_size):
    """A one-key batch with 128 and more packets in every workgroup's range runs whole packets in 4-lane groups. Outputs
    shifted by 16 x (i mod 8) within their 128-byte lines: the G4 open's line-hold path and the seal's
    paired stores at every line offset. 600-byte payloads (10 4-lane steps: the steady loop runs)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    K, pkts = _one_key_block(key_size, 136, 600)
    ks, hp_ks = K.keysets()
    n = len(pkts)
    c = counted(lambda: check_tiled(ks, hp_ks, pkts, ncu, [(i * 7) % 128 for i in range(n)], [16 * (i % 8) for i in range(n)],
                                    [16 * ((i + 3) % 8) for i in range(n)]))
    assert c["runs"]["w8_g4"] > 0 and c["launches"]["w8_tree"] == 0, c
    ks.free(), hp_ks.free()


def test_one_key_whole_runs_of_long_packets():
    """Whole runs of packets of 8 KiB and more stay with the serial kernel (no long-record kernel for this frame). AES-128
    only: the batch is 128 packets per CU of 8200 bytes."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    K, pkts = _one_key_block(16, 128, 8200)
    ks, hp_ks = K.keysets()
    n = len(pkts)
    c = counted(lambda: check_tiled(ks, hp_ks, pkts, ncu, None, [16 * (i % 8) for i in range(n)], [16 * ((i + 5) % 8) for i in range(n)]))
    assert c["runs"]["w8_g4"] > 0 and c["launches"]["w8_tree"] == 0 and c["launches"]["w8_serial"] == 2, c
    ks.free(), hp_ks.free()


# ---- 6. many connections


@functools.lru_cache(maxsize=None)
def _many_connections(key_size):
    rng = np.random.default_rng(6000 + key_size)
    nk = 300
    K = Keys.make(rng, nk, key_size)
    order = rng.permutation(np.repeat(np.arange(nk), 2))
    pkts = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, int(rng.integers(3, 1300)),
                     phase=int(rng.integers(0, 2))) for k in order]
    same = [make_pkt(K, rng, int(k), p.pn, p.pn_len, 8, len(p.payload), phase=p.phase, hps=K.keys) for k, p in zip(order, pkts)]
    # connections of 8 uniform packets in random order: regrouped on the device, then joined into multi-key runs
    order8 = rng.permutation(np.repeat(np.arange(nk), 8))
    mk = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, 1200) for k in order8]
    assert_oracle_source_agrees(K, pkts, range(0, len(pkts), 40))
    assert_oracle_source_agrees(K, same, range(0, len(same), 60), hps=K.keys)
    assert_oracle_source_agrees(K, mk, range(0, len(mk), 150))
    return K, pkts, same, mk


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_many_connections(key_size):
    K, pkts, same, mk = _many_connections(key_size)
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    print("300 connections x 2 packets:", c)
    assert c["launches"]["w8_serial"] == 2, c
    check_packets(ks, ks, same)  # hp_ks the same object as ks: connection k's header-protection key is its AEAD key
    c = counted(lambda: check_packets(ks, hp_ks, mk))
    print("300 connections x 8 packets:", c)
    assert c["runs"]["w8_mk"] > 0, c
    ks.free(), hp_ks.free()


# ---- 7. a few long packets among short ones (cut runs)

# (length, header length, key size, packets per connection) of test_w8_multi_key_runs_vs_fusion's six shapes; a header
# holds at least its first byte and a 4-byte packet number
CUT_SHAPES = [(1200, 13, 16, 64), (1200, 13, 32, 64), (37, 5, 16, 48), (600, 21, 16, 17), (3000, 13, 32, 100), (1, 5, 16, 5)]


@functools.lru_cache(maxsize=None)
def _cut_runs(length, hlen, key_size, per_key):
    rng = np.random.default_rng(7700 + length + per_key)
    n = 640
    nk = (n + per_key - 1) // per_key
    K = Keys.make(rng, nk, key_size)
    pkts = []
    for i in range(n):
        pn_len = max(i % 4 + 1, 4 - length)
        ln = int(rng.integers(8192, 20000)) if i % 97 == 13 else length  # a few packets of 8 KiB and more
        pkts.append(make_pkt(K, rng, i // per_key, int(rng.integers(0, 2**62)), pn_len, hlen - 1 - pn_len, ln, long=i % 5 == 0))
    assert_oracle_source_agrees(K, pkts, range(0, n, 40))
    return K, pkts


@pytest.mark.parametrize("length, hlen, key_size, per_key", CUT_SHAPES)
def test_long_packets_among_short_ones(length, hlen, key_size, per_key):
    K, pkts = _cut_runs(length, hlen, key_size, per_key)
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    assert c["launches"]["w8_serial"] == 2 and c["launches"]["w8_tree"] == 0, c
    ks.free(), hp_ks.free()


# ---- 8. packet-number reconstruction on the device


@functools.lru_cache(maxsize=None)
def _pn_cases(key_size):
    rng = np.random.default_rng(7000 + key_size)
    K = Keys.make(rng, 1, key_size)
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


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_packet_number_reconstruction(key_size):
    K, good, lost = _pn_cases(key_size)
    ks, hp_ks = K.keysets()
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


# ---- 9. tampering


def _open_mixed(ks, hp_ks, K, pkts, packets, recs_edit=None):
    """opens ``packets`` (pkts' reference packets, some altered) and checks every one against the reference's verdict
    on the same bytes: ok, results, the output of those that opened, nothing written outside; returns the statuses"""
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
def _tamper_pkts(key_size):
    rng = np.random.default_rng(8000 + key_size)
    K = Keys.make(rng, 2, key_size)
    n = 288  # (above 256: the serial W8 kernel and, two keys in alternation, the regroup's permutation of the ok bytes)
    pkts = [make_pkt(K, rng, i & 1, int(rng.integers(0, 2**62)), i % 4 + 1, 8 + i % 5, int(rng.integers(40, 1500)), long=i % 4 == 3,
                     phase=(i >> 2) & 1) for i in range(n)]
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_tampering(key_size):
    K, pkts = _tamper_pkts(key_size)
    ks, hp_ks = K.keysets()
    n = len(pkts)
    rng = np.random.default_rng(8001)
    for kind in ("first", "pn", "dcid", "ciphertext", "tag"):
        hit = rng.random(n) < 0.4
        hit[int(rng.integers(0, n))] = True
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
        # (a slice of under 256 packets as well: the 4-bit kernel's ok bytes)
        for a, b in ((0, n), (0, 64)):
            status = _open_mixed(ks, hp_ks, K, pkts[a:b], packets[a:b])
            assert status == [QUIC_BAD_MAC if h else QUIC_OK for h in hit[a:b]], kind  # every tampered packet fails, no other
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


# ---- 10. key phase


@functools.lru_cache(maxsize=None)
def _phase_pkts(key_size):
    rng = np.random.default_rng(11000 + key_size)
    K = Keys.make(rng, 1, key_size)
    pkts = []
    for i in range(16):
        pkts.append(make_pkt(K, rng, 0, 1000 + i, i % 4 + 1, 8, 20 + 70 * i, long=i % 4 == 2, phase=(i >> 2) & 1))
    return K, pkts


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_key_phase(key_size):
    K, pkts = _phase_pkts(key_size)
    ks, hp_ks = K.keysets()

    def flip_all(recs):
        recs["flags"] ^= 1

    for rep in (1, 20):  # 16 packets (the 4-bit kernel), 320 (the serial W8 kernel)
        some = pkts * rep
        packets = [p.packet for p in some]
        # the wrong expected phase: short headers get KEY_PHASE, ok = 0 and keep their sentinel (checked whole-arena in
        # _open_mixed); long headers ignore the bit and open
        status = _open_mixed(ks, hp_ks, K, some, packets, recs_edit=flip_all)
        assert status == [QUIC_OK if p.header[0] & 0x80 else QUIC_KEY_PHASE for p in some]
        # the same packets with the right phase all open
        assert _open_mixed(ks, hp_ks, K, some, packets) == [QUIC_OK] * len(some)
    ks.free(), hp_ks.free()


# ---- 11. rejections


@pytest.mark.parametrize("key_size", KEY_SIZES)
@pytest.mark.parametrize("reps", (1, 25))  # 12 descriptors (the 4-bit kernel), 300 (the serial W8 kernel)
def test_rejections(key_size, reps):
    rng = np.random.default_rng(9000 + key_size)
    K = Keys.make(rng, 3, key_size)
    K.hps = K.hps[:2]  # key_idx 2 is beyond hp_ks only, 3 beyond both
    ks, hp_ks = K.keysets()
    Kfull = Keys(K.keys, K.ivs, K.hps + [bytes(key_size)])
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
    got = gpu_seal(ks, hp_ks, recs, arena_in, filled(out_size))
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
    back, ok, res = gpu_open(ks, hp_ks, opn, arena, filled(back_size))  # (checks that ok and results end at n)
    want_back = filled(back_size)
    for i, (c, o) in enumerate(zip(clear, back_offs)):
        if i % 12 not in bad:
            put(want_back, o, c)
    assert ok.tolist() == [0 if i % 12 in bad else 1 for i in range(n)]
    assert [int(s) for s in res["status"]] == [QUIC_REJECTED if i % 12 in bad else QUIC_OK for i in range(n)]
    assert np.array_equal(back, want_back), "a rejected packet was written for, or a neighbour was not opened"
    ks.free(), hp_ks.free()


# ---- 12. invalid arguments


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_invalid_arguments(key_size):
    rng = np.random.default_rng(10000 + key_size)
    K = Keys.make(rng, 1, key_size)
    ks, hp_ks = K.keysets()
    p = make_pkt(K, rng, 0, 5, 2, 8, 100)
    arena = filled(256)
    put(arena, 16, p.packet)
    d_recs, d_in, d_out = dev(open_recs([p], [16], [16])), dev(arena), dev(filled(256))
    d_ok, d_res = empty(1, FILL), empty(16, FILL)
    lib = pa.load_library()
    args = (d_recs.data_ptr(), 1, d_in.data_ptr(), d_out.data_ptr())
    assert lib.ptls_mi355x_open_quic_packets(ks.handle, hp_ks.handle, *args, d_ok.data_ptr(), None, None) == -1  # results
    assert lib.ptls_mi355x_open_quic_packets(ks.handle, hp_ks.handle, *args, None, d_res.data_ptr(), None) == -1   # ok
    assert lib.ptls_mi355x_open_quic_packets(ks.handle, None, *args, d_ok.data_ptr(), d_res.data_ptr(), None) == -1  # hp_ks
    assert lib.ptls_mi355x_open_quic_packets(None, hp_ks.handle, *args, d_ok.data_ptr(), d_res.data_ptr(), None) == -1  # ks
    assert lib.ptls_mi355x_seal_quic_packets(ks.handle, None, *args, None) == -1
    assert lib.ptls_mi355x_seal_quic_packets(None, hp_ks.handle, *args, None) == -1
    with pytest.raises(pa.EngineError):
        pa.open_quic_packets(ks, hp_ks, *args, d_ok.data_ptr(), 0, _stream())
    with pytest.raises(pa.EngineError):
        pa.seal_quic_packets(ks, None, *args, _stream())
    # an empty batch is no error and touches nothing
    assert lib.ptls_mi355x_seal_quic_packets(ks.handle, hp_ks.handle, None, 0, None, None, None) == 0
    assert lib.ptls_mi355x_open_quic_packets(ks.handle, hp_ks.handle, None, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_ok.cpu().numpy() == FILL).all() and (d_res.cpu().numpy() == FILL).all()
    ks.free(), hp_ks.free()


def test_hp_ks_on_another_device_is_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    rng = np.random.default_rng(10500)
    K = Keys.make(rng, 1, 16)
    ks = pa.Keyset(K.keys[0], K.ivs[0], 16)
    with torch.cuda.device(1):
        hp_ks = pa.Keyset(K.hps[0], bytes(12), 16)
    p = make_pkt(K, rng, 0, 5, 2, 8, 100)
    arena = filled(256)
    put(arena, 16, p.header + p.payload)
    d_recs, d_in, d_out = dev(seal_recs([p], [16], [16])), dev(arena), dev(filled(256))
    lib = pa.load_library()
    assert lib.ptls_mi355x_seal_quic_packets(ks.handle, hp_ks.handle, d_recs.data_ptr(), 1, d_in.data_ptr(), d_out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    ks.free(), hp_ks.free()


# ---- 13. ordering


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_free_and_rekey_of_hp_ks_right_after_launch_are_ordered(key_size):
    """A rekey and a free of hp_ks made right after a launch on a side stream order themselves behind it, so the packets
    carry the old header-protection key's masks (the shape of the ChaCha20 pair's test)."""
    rng = np.random.default_rng(12000 + key_size)
    n = 2000
    K = Keys.make(rng, 1, key_size)
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
    ks = pa.Keyset(K.keys[0], K.ivs[0], key_size)
    outs = []
    for _ in range(3):
        hp1, hp2 = rng.bytes(key_size), rng.bytes(key_size)
        hp_ks = pa.Keyset(hp1, bytes(12), key_size)
        d_first, d_second = empty(out_size, FILL), empty(out_size, FILL)
        side.wait_stream(torch.cuda.current_stream())  # the inputs and the filled outputs are ready
        pa.seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_first.data_ptr(), side.cuda_stream)
        hp_ks.update([0], hp2, bytes(12))  # immediately, with the batch most likely still running
        pa.seal_quic_packets(ks, hp_ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_second.data_ptr(), _stream())
        hp_ks.free()
        outs.append(((hp1, d_first), (hp2, d_second)))
    torch.cuda.synchronize()
    # (the AEAD part of a packet does not depend on the header-protection key: sealed once, masked per key)
    sealed = [Q.gcm_seal(K.keys[0], K.ivs[0], pn, h, pl) for h, pl, pn in zip(headers, payloads, pns)]
    assert Q.protect(K.keys[0], K.ivs[0], outs[0][0][0], pns[0], headers[0], payloads[0]) == _masked(headers[0], sealed[0], outs[0][0][0])
    for rnd, pair in enumerate(outs):
        for which, (hp, d_out) in zip(("launch before the rekey", "launch after the rekey"), pair):
            got = d_out.cpu().numpy()
            want = filled(out_size)
            for h, sl, o in zip(headers, sealed, out_offs):
                put(want, o, _masked(h, sl, hp))
            bad = [i for i, (h, o) in enumerate(zip(headers, out_offs)) if not np.array_equal(got[o:o + len(h) + 1216], want[o:o + len(h) + 1216])]
            assert not bad, f"round {rnd}, {which}: {len(bad)} of {n} packets differ from the reference, first {bad[:4]}"
            assert np.array_equal(got, want)
    ks.free()


def _masked(header, sealed, hp):
    """quic_aes_ref.protect's header protection on an AEAD output computed before (checked against protect itself above)"""
    pn_len = (header[0] & 3) + 1
    pn_off = len(header) - pn_len
    mask = Q.hp_mask(hp, (header[pn_off:] + sealed)[4:20])
    out = bytearray(header)
    out[0] = Q._apply_mask(header[0], mask)
    for i in range(pn_len):
        out[pn_off + i] ^= mask[1 + i]
    return bytes(out) + sealed
