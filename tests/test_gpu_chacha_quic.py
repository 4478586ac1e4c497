"""QUIC packet protection under ChaCha20-Poly1305 on the GPU (ptls_mi355x_chacha_seal_quic_packets /
_open_quic_packets): every comparison is byte for byte against tests/quic_ref.py (OpenSSL; a subset of each batch also
against its plain-Python source). Arenas start as 0xAA and are compared whole, so a write outside a packet shows. Every
test runs at both forced group widths, the batch ones also with the grid capped at two workgroups so that the claim loop
turns. The packets, the checks and the case generators are those of tests/quic_util.py, shared with the AES-GCM pair's
tests; the references of a case are computed once and shared by its modes."""
import numpy as np
import pytest
import torch

import picotls_amd as pa
import quic_ref as Q
import quic_util as U
from gpu_util import dev, empty
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, RECORD_DTYPE
from quic_util import FILL, Keys, Pkt, filled, header_for, make_pkt, open_recs, place, put

pytestmark = pytest.mark.gpu

S = U.Suite(keyset=lambda keys, ivs, size: pa.ChaChaKeyset(keys, ivs), key_size=32, hp_size=32, alt_hp_size=32,
            seal=pa.chacha_seal_quic_packets, open=pa.chacha_open_quic_packets, ref=Q, second="py", seed=0)
WIDTHS = pa.CHACHA_GROUP_WIDTHS
MODES = [(w, 0) for w in WIDTHS] + [(w, 2) for w in WIDTHS]  # (group width, cap on the launch grid)
_stream = U.stream


@pytest.fixture
def forced():
    """debug_force for the test, back to automatic after it"""
    yield pa.chacha_debug_force
    pa.chacha_debug_force(0, 0)


def check_packets(ks, hp_ks, pkts, **kw):
    U.check_packets(S, ks, hp_ks, pkts, **kw)


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


@pytest.mark.parametrize("width, cap", MODES)
def test_every_small_shape(width, cap, forced):
    K, pkts = U.every_shape(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    pa.chacha_debug_counters(reset=True)
    check_packets(ks, hp_ks, pkts)
    ran = pa.chacha_debug_counters(reset=True)
    assert ran[width] == 2 and sum(ran.values()) == 2, ran  # one seal launch, one batch launch of the open, at the forced width
    ks.free(), hp_ks.free()


# ---- 3. AAD block edges


@pytest.mark.parametrize("width, cap", MODES)
def test_aad_block_edges(width, cap, forced):
    K, pkts = U.aad_edges(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    check_packets(ks, hp_ks, pkts)
    ks.free(), hp_ks.free()


# ---- 4. the sample reaching the tag


@pytest.mark.parametrize("width, cap", MODES)
def test_sample_reaches_the_tag(width, cap, forced):
    K, pkts = U.sample_in_tag(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    res = [(3 * i + 1) % 16 for i in range(len(pkts))]
    check_packets(ks, hp_ks, pkts, in_res=res, out_res=res[::-1], back_res=res)
    ks.free(), hp_ks.free()


# ---- 5. byte offsets and in place


@pytest.mark.parametrize("width, cap", MODES)
def test_odd_offsets(width, cap, forced):
    K, pkts = U.offset_pkts(S, 16, 8)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    n = len(pkts)
    check_packets(ks, hp_ks, pkts, in_res=[i % 16 for i in range(n)], out_res=[(i + 5) % 16 for i in range(n)],
                  back_res=[(i + 11) % 16 for i in range(n)])
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("width, cap", MODES)
def test_in_place_seal_then_open(width, cap, forced):
    K, pkts = U.offset_pkts(S, 16, 8)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    U.check_in_place(S, ks, hp_ks, pkts)
    ks.free(), hp_ks.free()


# ---- 6. many connections


@pytest.mark.parametrize("width, cap", MODES)
def test_many_connections(width, cap, forced):
    K, pkts, same, _ = U.many_connections(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    check_packets(ks, hp_ks, pkts)
    check_packets(ks, ks, same)  # hp_ks the same object as ks: connection k's header-protection key is its AEAD key
    ks.free(), hp_ks.free()


# ---- 7. packet-number reconstruction on the device


@pytest.mark.parametrize("width, cap", MODES)
def test_packet_number_reconstruction(width, cap, forced):
    K, good, lost = U.pn_cases(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    U.check_pn_reconstruction(S, ks, hp_ks, good, lost)
    ks.free(), hp_ks.free()


# ---- 8. tampering


@pytest.mark.parametrize("width, cap", MODES)
def test_tampering(width, cap, forced):
    K, pkts = U.tamper_pkts(S, 64)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    rng = np.random.default_rng(8001)
    for kind in ("first", "pn", "dcid", "ciphertext", "tag"):
        hit = rng.random(64) < 0.4
        hit[int(rng.integers(0, 64))] = True
        packets = U.tampered(rng, pkts, hit, kind)
        status = U.open_mixed(ks, hp_ks, K, pkts, packets)
        assert status == [QUIC_BAD_MAC if h else QUIC_OK for h in hit], kind  # every tampered packet fails, no other
    # a flip inside the sample: the packet fails with the verdict the reference gives for the same bytes (BAD_MAC, or
    # KEY_PHASE where the changed mask turns a short header's key-phase bit), every other packet opens
    packets = U.tampered_in_sample(rng, pkts)
    status = U.open_mixed(ks, hp_ks, K, pkts, packets)
    assert all((s == QUIC_OK) == (i % 2 == 0) for i, s in enumerate(status)) and QUIC_BAD_MAC in status and QUIC_KEY_PHASE in status
    ks.free(), hp_ks.free()


# ---- 9. rejections


@pytest.mark.parametrize("width, cap", MODES)
def test_rejections(width, cap, forced):
    U.check_rejections(S, 1, before_launch=lambda: forced(width, cap))  # 12 descriptors


# ---- 10. invalid arguments


@pytest.mark.parametrize("width", WIDTHS)
def test_invalid_arguments(width, forced):
    rng = np.random.default_rng(10000)
    K = Keys.make(S, rng, 1)
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


@pytest.mark.parametrize("width, cap", MODES)
def test_key_phase(width, cap, forced):
    K, pkts = U.phase_pkts(S)
    ks, hp_ks = K.keysets()
    forced(width, cap)
    U.check_key_phase(ks, hp_ks, K, pkts)
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
    K = Keys.make(S, rng, 1)
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
