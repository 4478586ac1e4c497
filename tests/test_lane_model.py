"""CPU model of the record-per-lane kernel's GHASH (picotls_amd/csrc/engine/lane_kernels.h, ghash.h gmul_lane,
lds_tables.h build_lane_table): Shoup's 4-bit multiply on a table of the hash key's 16 multiples with
the reduction in closed form, the serial Horner over [AAD | text | length], and the table's LDS address map, which is
conflict-free for any data. The multiply is restated here word for word as the kernel does it (big-endian 32-bit words,
the same shifts) and checked against the C oracle (oracle/gcm_ref.c). The GPU suite checks the kernel end to end against
lib/fusion.c (tests/test_gpu_lane.py)."""
import itertools

import numpy as np
import pytest

from oracle import GcmOracle

M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def oracle():
    return GcmOracle()


def words(b: bytes):  # a 16-byte GHASH element as the kernel's big-endian words
    return [int.from_bytes(b[4 * q:4 * q + 4], "big") for q in range(4)]


def unwords(w) -> bytes:
    return b"".join(x.to_bytes(4, "big") for x in w)


def alignbit(hi, lo, s):  # v_alignbit_b32: the low 32 bits of {hi, lo} >> s
    return ((hi << 32 | lo) >> s) & M32


def mulx(b):  # gf_mulx_be (common.h)
    lsb = b[3] & 1
    return [(b[0] >> 1) ^ (0xE1000000 if lsb else 0), (b[1] >> 1) | (b[0] << 31) & M32, (b[2] >> 1) | (b[1] << 31) & M32,
            (b[3] >> 1) | (b[2] << 31) & M32]


def lane_table(h: bytes):  # build_lane_table: M[n] = sum over the set bits of n (bit 3 = x^0) of x^q H
    v = [words(h)]
    for _ in range(3):
        v.append(mulx(v[-1]))
    tab = []
    for n in range(16):
        e = [0, 0, 0, 0]
        for m in range(4):
            if (n >> (3 - m)) & 1:
                e = [a ^ b for a, b in zip(e, v[m])]
        tab.append(e)
    return tab


def gmul_lane(tab, t):  # gmul_lane: 32 nibble steps Z = (Z >> 4) ^ R(Z & 15) ^ M[nibble], last nibble first
    z = [0, 0, 0, 0]
    for p in range(31, -1, -1):
        n = (t[p >> 3] >> (28 - 4 * (p & 7))) & 15
        if p != 31:
            top = (z[3] << 28) & M32
            z = [(z[0] >> 4) ^ top ^ (top >> 1) ^ (top >> 2) ^ (top >> 7), alignbit(z[0], z[1], 4), alignbit(z[1], z[2], 4),
                 alignbit(z[2], z[3], 4)]
        z = [a ^ b for a, b in zip(z, tab[n])]
    return z


def reduction_constants():  # the method's R table as the closed form gives it: what 4 bits shifted out put back into word 0
    out = []
    for rem in range(16):
        top = rem << 28
        out.append(top ^ (top >> 1) ^ (top >> 2) ^ (top >> 7))
    return out


def test_reduction_constants_are_the_4bit_methods():
    # the table every 4-bit GHASH implementation carries ("last4"), as 16-bit values at the top of the element
    last4 = [0x0000, 0x1c20, 0x3840, 0x2460, 0x7080, 0x6ca0, 0x48c0, 0x54e0, 0xe100, 0xfd20, 0xd940, 0xc560, 0x9180, 0x8da0,
             0xa9c0, 0xb5e0]
    assert reduction_constants() == [v << 16 for v in last4]


def test_lane_multiply_equals_the_oracle(oracle):
    rng = np.random.default_rng(11)
    ones, zero = b"\xff" * 16, bytes(16)
    single = [(1 << k).to_bytes(16, "big") for k in range(128)]
    pairs = [(rng.bytes(16), rng.bytes(16)) for _ in range(1000)]
    pairs += [(ones, ones), (ones, zero), (zero, ones)]
    pairs += [(ones, s) for s in single] + [(s, ones) for s in single]
    pairs += [(single[int(a)], single[int(b)]) for a, b in rng.integers(0, 128, (200, 2))]
    for h, x in pairs:
        assert unwords(gmul_lane(lane_table(h), words(x))) == oracle.gf128_mul(x, h), (h.hex(), x.hex())


def lane_ghash(h: bytes, aad: bytes, text: bytes) -> bytes:
    """lane_record's GHASH: Y = (Y ^ X) H over the zero-padded AAD blocks, the text blocks and the length block."""
    tab = lane_table(h)
    y = [0, 0, 0, 0]

    def fold(block):
        nonlocal y
        y = gmul_lane(tab, [a ^ b for a, b in zip(y, words(block.ljust(16, b"\0")))])

    for o in range(0, len(aad), 16):
        fold(aad[o:o + 16])
    for o in range(0, len(text), 16):
        fold(text[o:o + 16])
    abits, cbits = 8 * len(aad), 8 * len(text)
    y = gmul_lane(tab, [y[0] ^ abits >> 32, y[1] ^ abits & M32, y[2] ^ cbits >> 32, y[3] ^ cbits & M32])
    return unwords(y)


def test_serial_horner_equals_the_oracles_ghash(oracle):
    rng = np.random.default_rng(12)
    cases = [(a, t) for a in (0, 1, 13, 16, 17, 40) for t in (0, 1, 15, 16, 17, 63, 64, 65, 300)] + [(65536, 0), (0, 4097)]
    for alen, tlen in cases:
        h, aad, text = rng.bytes(16), rng.bytes(alen), rng.bytes(tlen)
        pad = lambda b: b + bytes(-len(b) % 16)
        stream = pad(aad) + pad(text) + (8 * alen).to_bytes(8, "big") + (8 * tlen).to_bytes(8, "big")
        assert lane_ghash(h, aad, text) == oracle.ghash(h, stream), (alen, tlen)


# The LDS address map (lds_tables.h lane_tab_base): entry n of lane l of wave w at 65536 + w * 16384 + n * 1024 + l * 16
def entry_addr(w, l, n):
    return 65536 + w * 16384 + n * 1024 + l * 16


# ds_read_b128 is served in four groups of 16 lanes, one LDS cycle each when their bank quads are disjoint; the bank of
# byte address a is (a / 4) mod 64
READ_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
                    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
                    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def test_the_service_groups_partition_the_wave():
    assert sorted(itertools.chain(*READ_B128_GROUPS)) == list(range(64))
    assert all(len(g) == 16 for g in READ_B128_GROUPS)


def test_table_lookups_are_conflict_free_for_any_nibbles():
    # a lane's bank quad does not depend on n, so one check per lane covers every assignment of nibbles to lanes: the
    # 16 x 16 (lane, nibble) pairs of a group give exactly 16 distinct quads, one per lane
    for w in range(4):
        for group in READ_B128_GROUPS:
            quads = {}
            for l in group:
                per_lane = {frozenset((entry_addr(w, l, n) // 4 + k) % 64 for k in range(4)) for n in range(16)}
                assert len(per_lane) == 1, (w, l)
                quads[l] = next(iter(per_lane))
            for a, b in itertools.combinations(group, 2):
                assert not (quads[a] & quads[b]), (w, a, b)
    # ... and spot assignments, as the hardware would see them
    rng = np.random.default_rng(13)
    for _ in range(200):
        w, group = int(rng.integers(0, 4)), READ_B128_GROUPS[int(rng.integers(0, 4))]
        banks = [(entry_addr(w, l, int(rng.integers(0, 16))) // 4 + k) % 64 for l in group for k in range(4)]
        assert len(set(banks)) == 64


def test_table_build_store_phases_cover_distinct_banks():
    # ds_write_b128 is served in 8 phases of 8 contiguous lanes; the bank of byte address a is (a / 4) mod 32. Every
    # lane stores the same n in one instruction
    for w in range(4):
        for n in range(16):
            for l0 in range(0, 64, 8):
                banks = [(entry_addr(w, l, n) // 4 + k) % 32 for l in range(l0, l0 + 8) for k in range(4)]
                assert len(set(banks)) == 32, (w, n, l0)


def test_the_tables_fill_the_second_64k_exactly():
    spans = sorted(entry_addr(w, l, n) for w in range(4) for l in range(64) for n in range(16))
    assert spans == list(range(65536, 131072, 16))
