"""QUIC packet protection under AES-GCM on the GPU (ptls_mi355x_seal_quic_packets / ptls_mi355x_open_quic_packets), with
the packets, checks and case generators of tests/quic_util.py that the ChaCha20 pair's tests use too (the sections are
those of test_gpu_chacha_quic.py): every comparison is byte for byte against tests/quic_aes_ref.py (the system
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

import numpy as np
import pytest
import torch

import picotls_amd as pa
import quic_aes_ref as Q
import quic_util as U
from gpu_util import dev, empty
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, RECORD_DTYPE
from quic_util import FILL, Keys, filled, gpu_open, gpu_seal, header_for, make_pkt, open_recs, place, put, seal_recs

pytestmark = pytest.mark.gpu

KEY_SIZES = (16, 32)
# (sample_in_tag's header-protection keys are of the other size)
SUITES = {size: U.Suite(keyset=pa.Keyset, key_size=size, hp_size=size, alt_hp_size=48 - size, seal=pa.seal_quic_packets,
                        open=pa.open_quic_packets, ref=Q, second="oracle", seed=size) for size in KEY_SIZES}
_stream = U.stream


def check_packets(ks, hp_ks, pkts, **kw):
    U.check_packets(SUITES[ks.key_size], ks, hp_ks, pkts, **kw)


def counted(fn):
    """fn() between two resets of the debug counters: its launches and runs by kind"""
    pa.debug_counters(reset=True)
    fn()
    return pa.debug_counters(reset=True)


# ---- 1. every small shape


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_every_small_shape_one_batch(key_size):
    """above 256 packets: the serial W8 kernel (many-key form: two keys), and never the long-record kernel"""
    K, pkts = U.every_shape(SUITES[key_size])
    assert len(pkts) >= 256
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    assert c["launches"]["w8_serial"] == 2 and c["launches"]["w8_tree"] == 0 and c["launches"]["chunked"] == 0, c
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_every_small_shape_in_slices(key_size):
    """the same packets in slices of under 256: the 4-bit kernel (EXT 0)"""
    K, pkts = U.every_shape(SUITES[key_size])
    ks, hp_ks = K.keysets()
    step = 131
    c = counted(lambda: [check_packets(ks, hp_ks, pkts[a:a + step]) for a in range(0, len(pkts), step)])
    nslices = (len(pkts) + step - 1) // step
    assert c["launches"]["chunked"] == 2 * nslices and c["launches"]["w8_serial"] == 0, c
    ks.free(), hp_ks.free()


# ---- 2. AAD block edges


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_aad_block_edges(key_size):
    K, pkts = U.aad_edges(SUITES[key_size])
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts)                 # 132 packets: the 4-bit kernel
    check_packets(ks, hp_ks, pkts + pkts[::-1])    # 264: the serial W8 kernel
    ks.free(), hp_ks.free()


# ---- 3. the sample reaching the tag


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_sample_reaches_the_tag(key_size):
    K, pkts = U.sample_in_tag(SUITES[key_size])
    ks, hp_ks = K.keysets()
    res = [(3 * i + 1) % 16 for i in range(len(pkts))]
    check_packets(ks, hp_ks, pkts, in_res=res, out_res=res[::-1], back_res=res)
    twice = pkts + pkts  # 384 packets: the serial W8 kernel
    res = [(5 * i + 2) % 16 for i in range(len(twice))]
    check_packets(ks, hp_ks, twice, in_res=res, out_res=res[::-1], back_res=res)
    ks.free(), hp_ks.free()


# ---- 4. byte offsets and in place


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_odd_offsets(key_size):
    K, pkts = U.offset_pkts(SUITES[key_size], 64, 16)
    ks, hp_ks = K.keysets()
    for sub in (pkts[::4], pkts):  # 80 packets (the 4-bit kernel), 320 (the serial W8 kernel)
        n = len(sub)
        check_packets(ks, hp_ks, sub, in_res=[i % 16 for i in range(n)], out_res=[(i + 5) % 16 for i in range(n)],
                      back_res=[(i + 11) % 16 for i in range(n)])
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_in_place_seal_then_open(key_size):
    K, all_pkts = U.offset_pkts(SUITES[key_size], 64, 16)
    ks, hp_ks = K.keysets()
    for pkts in (all_pkts[::4], all_pkts):
        U.check_in_place(SUITES[key_size], ks, hp_ks, pkts)
    ks.free(), hp_ks.free()


# ---- 5. one key: whole runs in 4-lane groups


@functools.lru_cache(maxsize=None)
def _one_key(key_size):
    rng = np.random.default_rng(5500 + key_size)
    K = Keys.make(SUITES[key_size], rng, 1)
    pkts = [make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), i % 4 + 1, 8, 1200, phase=i & 1) for i in range(300)]
    U.assert_second_source_agrees(K, pkts, range(0, 300, 30))
    return K, pkts


@functools.lru_cache(maxsize=None)
def _one_key_block(key_size, n, payload_len):
    rng = np.random.default_rng(5600 + key_size + payload_len)
    K = Keys.make(SUITES[key_size], rng, 1)
    pkts = [make_pkt(K, rng, 0, int(rng.integers(0, 2**62)), i % 4 + 1, 8 + i % 3, payload_len, long=i % 11 == 0) for i in range(n)]
    U.assert_second_source_agrees(K, pkts, range(0, n, n // 8))
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

    got = gpu_seal(SUITES[ks.key_size], ks, hp_ks, tiled(seal_recs(pkts, in_offs, out_offs), in_size, out_size), np.tile(arena_in, reps), filled(out_size * reps))
    same(got, want, out_size, "seal")
    back, ok, res = gpu_open(SUITES[ks.key_size], ks, hp_ks, tiled(open_recs(pkts, out_offs, back_offs), out_size, back_size), got, filled(back_size * reps))
    assert (ok == 1).all(), f"open refused packets {np.flatnonzero(ok != 1)[:8]}"
    same(back, want_back, back_size, "open")
    assert np.array_equal(res, np.tile(U.want_results(pkts), reps)), "results"


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


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_many_connections(key_size):
    K, pkts, same, mk = U.many_connections(SUITES[key_size], runs_of_8=True)
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
    K = Keys.make(SUITES[key_size], rng, nk)
    pkts = []
    for i in range(n):
        pn_len = max(i % 4 + 1, 4 - length)
        ln = int(rng.integers(8192, 20000)) if i % 97 == 13 else length  # a few packets of 8 KiB and more
        pkts.append(make_pkt(K, rng, i // per_key, int(rng.integers(0, 2**62)), pn_len, hlen - 1 - pn_len, ln, long=i % 5 == 0))
    U.assert_second_source_agrees(K, pkts, range(0, n, 40))
    return K, pkts


@pytest.mark.parametrize("length, hlen, key_size, per_key", CUT_SHAPES)
def test_long_packets_among_short_ones(length, hlen, key_size, per_key):
    K, pkts = _cut_runs(length, hlen, key_size, per_key)
    ks, hp_ks = K.keysets()
    c = counted(lambda: check_packets(ks, hp_ks, pkts))
    assert c["launches"]["w8_serial"] == 2 and c["launches"]["w8_tree"] == 0, c
    ks.free(), hp_ks.free()


# ---- 8. packet-number reconstruction on the device


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_packet_number_reconstruction(key_size):
    K, good, lost = U.pn_cases(SUITES[key_size])
    ks, hp_ks = K.keysets()
    U.check_pn_reconstruction(SUITES[key_size], ks, hp_ks, good, lost)
    ks.free(), hp_ks.free()


# ---- 9. tampering


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_tampering(key_size):
    K, pkts = U.tamper_pkts(SUITES[key_size], 288)
    ks, hp_ks = K.keysets()
    n = len(pkts)
    rng = np.random.default_rng(8001)
    for kind in ("first", "pn", "dcid", "ciphertext", "tag"):
        hit = rng.random(n) < 0.4
        hit[int(rng.integers(0, n))] = True
        packets = U.tampered(rng, pkts, hit, kind)
        # (a slice of under 256 packets as well: the 4-bit kernel's ok bytes)
        for a, b in ((0, n), (0, 64)):
            status = U.open_mixed(ks, hp_ks, K, pkts[a:b], packets[a:b])
            assert status == [QUIC_BAD_MAC if h else QUIC_OK for h in hit[a:b]], kind  # every tampered packet fails, no other
    # a flip inside the sample: the packet fails with the verdict the reference gives for the same bytes (BAD_MAC, or
    # KEY_PHASE where the changed mask turns a short header's key-phase bit), every other packet opens
    packets = U.tampered_in_sample(rng, pkts)
    status = U.open_mixed(ks, hp_ks, K, pkts, packets)
    assert all((s == QUIC_OK) == (i % 2 == 0) for i, s in enumerate(status)) and QUIC_BAD_MAC in status and QUIC_KEY_PHASE in status
    ks.free(), hp_ks.free()


# ---- 10. key phase


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_key_phase(key_size):
    K, pkts = U.phase_pkts(SUITES[key_size])
    ks, hp_ks = K.keysets()
    for rep in (1, 20):  # 16 packets (the 4-bit kernel), 320 (the serial W8 kernel)
        U.check_key_phase(ks, hp_ks, K, pkts * rep)
    ks.free(), hp_ks.free()


# ---- 11. rejections


@pytest.mark.parametrize("key_size", KEY_SIZES)
@pytest.mark.parametrize("reps", (1, 25))  # 12 descriptors (the 4-bit kernel), 300 (the serial W8 kernel)
def test_rejections(key_size, reps):
    U.check_rejections(SUITES[key_size], reps)


# ---- 12. invalid arguments


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_invalid_arguments(key_size):
    rng = np.random.default_rng(10000 + key_size)
    K = Keys.make(SUITES[key_size], rng, 1)
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
    K = Keys.make(SUITES[16], rng, 1)
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
    K = Keys.make(SUITES[key_size], rng, 1)
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
