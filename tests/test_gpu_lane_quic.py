"""QUIC packet protection (ptls_mi355x_seal_quic_packets / ptls_mi355x_open_quic_packets) with the AEAD keyset set to the
record-per-lane schedule: the packets, case generators and checks of tests/quic_util.py that test_gpu_quic_aes.py runs,
byte for byte against tests/quic_aes_ref.py over whole 0xAA arenas, for AES-128 and AES-256. The generators are cached per
suite, and a suite here differs from test_gpu_quic_aes.py's only in how it makes its keysets, so it has a seed of its
own and its references are computed once for this file. Every batch call is checked through the debug counters: the lane
kernel ran (FRAME 3) and no chunked kernel did."""
import numpy as np
import pytest
import torch

import picotls_amd as pa
import quic_aes_ref as Q
import quic_util as U
from picotls_amd.records import QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK
from quic_util import Keys, make_pkt

pytestmark = pytest.mark.gpu

KEY_SIZES = (16, 32)
OTHER_KINDS = ("chunked", "spread", "seal_hp", "w8_tree", "w8_serial", "lockstep", "span")


def lane_keyset(keys, ivs, key_size):
    """(the header-protection keyset gets the schedule too: its ECB masks do not depend on it)"""
    ks = pa.Keyset(keys, ivs, key_size)
    ks.set_schedule("record_per_lane")
    return ks


SUITES = {size: U.Suite(keyset=lane_keyset, key_size=size, hp_size=size, alt_hp_size=48 - size, seal=pa.seal_quic_packets,
                        open=pa.open_quic_packets, ref=Q, second="oracle", seed=700 + size) for size in KEY_SIZES}


def lane_ran(fn, calls=None):
    """fn() between two resets of the debug counters: only the lane kernel made batch launches (``calls`` of them)"""
    pa.debug_counters(reset=True)
    out = fn()
    c = pa.debug_counters(reset=True)
    assert c["launches"]["lane"] >= 1 and all(c["launches"][k] == 0 for k in OTHER_KINDS), c
    assert calls is None or c["launches"]["lane"] == calls, c
    return out


def check_packets(ks, hp_ks, pkts, **kw):
    lane_ran(lambda: U.check_packets(SUITES[ks.key_size], ks, hp_ks, pkts, **kw), calls=2)


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_every_small_shape(key_size):
    """short and long headers, pn_len 1-4, every payload length to 150 and lengths up to 65,527"""
    K, pkts = U.every_shape(SUITES[key_size])
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts)
    check_packets(ks, hp_ks, pkts[:131])  # one ragged tile
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_aad_block_edges(key_size):
    K, pkts = U.aad_edges(SUITES[key_size])
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts + pkts[::-1])
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_sample_reaches_the_tag(key_size):
    K, pkts = U.sample_in_tag(SUITES[key_size])
    ks, hp_ks = K.keysets()
    res = [(3 * i + 1) % 16 for i in range(len(pkts))]
    check_packets(ks, hp_ks, pkts, in_res=res, out_res=res[::-1], back_res=res)
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_odd_offsets_and_in_place(key_size):
    K, pkts = U.offset_pkts(SUITES[key_size], 64, 16)
    ks, hp_ks = K.keysets()
    n = len(pkts)
    check_packets(ks, hp_ks, pkts, in_res=[i % 16 for i in range(n)], out_res=[(i + 5) % 16 for i in range(n)],
                  back_res=[(i + 11) % 16 for i in range(n)])
    lane_ran(lambda: U.check_in_place(SUITES[key_size], ks, hp_ks, pkts), calls=2)
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_many_connections_of_two_packets(key_size):
    """300 connections x 2 packets in random order, the same with each connection's AEAD key as its header-protection
    key, and 300 connections x 8 packets"""
    K, pkts, same, mk = U.many_connections(SUITES[key_size], runs_of_8=True)
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts)
    check_packets(ks, ks, same)
    check_packets(ks, hp_ks, mk)
    ks.free(), hp_ks.free()


def test_two_packets_per_connection_over_2000_connections():
    """the shape the schedule is for: 4,000 packets, two per connection, the connections in no order"""
    suite = SUITES[16]
    rng = np.random.default_rng(7300)
    nk = 2000
    K = Keys.make(suite, rng, nk)
    order = rng.permutation(np.repeat(np.arange(nk), 2))
    pkts = [make_pkt(K, rng, int(k), int(rng.integers(0, 2**62)), int(rng.integers(1, 5)), 8, int(rng.integers(20, 1300)),
                     long=i % 9 == 0, phase=int(rng.integers(0, 2))) for i, k in enumerate(order)]
    U.assert_second_source_agrees(K, pkts, range(0, len(pkts), 250))
    ks, hp_ks = K.keysets()
    check_packets(ks, hp_ks, pkts)
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_packet_number_reconstruction(key_size):
    K, good, lost = U.pn_cases(SUITES[key_size])
    ks, hp_ks = K.keysets()
    lane_ran(lambda: U.check_pn_reconstruction(SUITES[key_size], ks, hp_ks, good, lost), calls=1)
    ks.free(), hp_ks.free()


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
        status = lane_ran(lambda: U.open_mixed(ks, hp_ks, K, pkts, packets), calls=1)
        assert status == [QUIC_BAD_MAC if h else QUIC_OK for h in hit], kind  # every tampered packet fails, no other
    packets = U.tampered_in_sample(rng, pkts)
    status = lane_ran(lambda: U.open_mixed(ks, hp_ks, K, pkts, packets), calls=1)
    assert all((s == QUIC_OK) == (i % 2 == 0) for i, s in enumerate(status)) and QUIC_BAD_MAC in status and QUIC_KEY_PHASE in status
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
def test_key_phase(key_size):
    K, pkts = U.phase_pkts(SUITES[key_size])
    ks, hp_ks = K.keysets()
    for rep in (1, 20):
        lane_ran(lambda: U.check_key_phase(ks, hp_ks, K, pkts * rep), calls=2)
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("key_size", KEY_SIZES)
@pytest.mark.parametrize("reps", (1, 25))
def test_rejections(key_size, reps):
    """six descriptors in twelve outside the limits (a len of 2^30 + 1 among them, which the pre-pass refuses; what the
    pre-pass refuses reaches the lane kernel as a len it refuses too): nothing is written for them"""
    started = []

    def before_launch():
        pa.debug_counters(reset=True)
        started.append(True)

    U.check_rejections(SUITES[key_size], reps, before_launch=before_launch)
    c = pa.debug_counters(reset=True)
    assert started and c["launches"]["lane"] == 2 and all(c["launches"][k] == 0 for k in OTHER_KINDS), c
    assert c["runs"]["lane_records"] == 2 * 6 * reps, c  # the six good packets of every twelve, sealed and opened
