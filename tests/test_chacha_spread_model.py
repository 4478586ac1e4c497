"""The plan and the algebra of the ChaCha20-Poly1305 spread launches, without a GPU: chacha_spread_plan's cuts obey the
device plan's invariants, and a tag assembled piece by piece from those cuts with Python integers (each piece's Horner
sum aligned with its own end, times r^D for the D 16-byte text blocks behind it) is OpenSSL's tag."""
import os
import re
import struct

import numpy as np

import chacha_ref as R
import picotls_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P1305
# the lengths of tests/test_gpu_chacha_spread.py's piece-edge test, at its forced piece and minimum
EDGE_LENS = [k * 1024 + d for k in (1, 2, 3, 4) for d in (-1, 0, 1, 15, 16, 17, 63, 64, 65)] + [0, 1, 1200]
EDGE_AADS = (0, 5, 13, 16, 33, 300)
EDGE_PARAMS = {"min_len": 2048, "piece": 1024, "max_pieces": pa.CHACHA_SPREAD_MAX_PIECES}


def test_max_pieces_matches_the_header():
    with open(os.path.join(ROOT, "include", "picotls", "mi355x_chacha20.h")) as fh:
        m = re.search(r"#define PTLS_MI355X_CHACHA_SPREAD_MAX_PIECES (\d+)", fh.read())
    assert m is not None and int(m.group(1)) == pa.CHACHA_SPREAD_MAX_PIECES


def test_plan_invariants():
    rng = np.random.default_rng(1)
    for min_len, piece in ((2048, 1024), (16384, 1024), (16384, 4096), (1, 1024), (65536, 2048)):
        params = {"min_len": min_len, "piece": piece, "max_pieces": pa.CHACHA_SPREAD_MAX_PIECES}
        lens = [0, 1, min_len - 1, min_len, min_len + 1, piece * pa.CHACHA_SPREAD_MAX_PIECES - 1, piece * pa.CHACHA_SPREAD_MAX_PIECES,
                piece * pa.CHACHA_SPREAD_MAX_PIECES + 1, (1 << 30) - 1, 1 << 30] + EDGE_LENS
        lens += [int(x) for x in rng.integers(0, 1 << 30, 40)] + [int(x) for x in rng.integers(0, 1 << 18, 40)]
        plan = pa.chacha_spread_plan(lens, params)
        assert len(plan) == len(lens)
        for n, cuts in zip(lens, plan):
            if n < min_len:
                assert cuts == [], n  # below the minimum: whole
                continue
            assert 1 <= len(cuts) <= pa.CHACHA_SPREAD_MAX_PIECES, (n, len(cuts))
            assert cuts[0][0] == 0 and cuts[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), n  # the pieces tile [0, n)
            sizes = {hi - lo for lo, hi in cuts[:-1]}
            assert len(sizes) <= 1 and all(s % 1024 == 0 and s % piece == 0 for s in sizes), (n, sizes)
            assert 0 < cuts[-1][1] - cuts[-1][0] <= (sizes.pop() if sizes else max(n, 1))
            # the smallest doubling of the base piece that stays under the cap
            size = cuts[0][1] if len(cuts) > 1 else None
            if size is not None and size > piece:
                assert -(-n // (size // 2)) > pa.CHACHA_SPREAD_MAX_PIECES, (n, size)
    assert pa.chacha_spread_plan([1 << 30], {"min_len": 1, "piece": 1024})[0][0] == (0, 1 << 20)  # 1024 pieces of 1 MiB
    assert pa.chacha_spread_plan([(1 << 30) + 1], EDGE_PARAMS) == [[]]  # beyond the record limit: rejected, one whole item


def tag_by_pieces(otk: bytes, ct: bytes, aad: bytes, cuts) -> bytes:
    r = int.from_bytes(otk[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    s = int.from_bytes(otk[16:32], "little")
    total, nblocks = 0, (len(ct) + 15) // 16
    for lo, hi in cuts:
        blocks = []
        if lo == 0:  # piece 0 starts with the AAD
            a = aad + bytes(-len(aad) % 16)
            blocks += [a[i:i + 16] for i in range(0, len(a), 16)]
        c = ct[lo:hi] + bytes(-(hi - lo) % 16)
        blocks += [c[i:i + 16] for i in range(0, len(c), 16)]
        h = 0
        for blk in blocks:  # Horner inside the piece: aligned with the piece's end
            h = (h + int.from_bytes(blk + b"\x01", "little")) * r % P
        total += h * pow(r, nblocks - (hi + 15) // 16, P)  # a plain sum: no order among the pieces
    total = (total + int.from_bytes(struct.pack("<QQ", len(aad), len(ct)) + b"\x01", "little")) * r % P
    return ((total + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def test_tag_from_pieces_is_openssls():
    rng = np.random.default_rng(2)
    plan = pa.chacha_spread_plan(EDGE_LENS, EDGE_PARAMS)
    cut = 0
    for i, (n, cuts) in enumerate(zip(EDGE_LENS, plan)):
        key, nonce, pt, aad = rng.bytes(32), rng.bytes(12), rng.bytes(n), rng.bytes(EDGE_AADS[i % len(EDGE_AADS)])
        sealed = R.ossl_seal(key, nonce, pt, aad)
        if not cuts:
            assert n < EDGE_PARAMS["min_len"]
            continue
        cut += 1
        assert len(cuts) == -(-n // 1024)
        assert tag_by_pieces(R.py_chacha20_block(key, 0, nonce), sealed[:n], aad, cuts) == sealed[n:], (n, len(aad))
    assert cut == 26  # k = 2: all but 2047; k = 3, 4: all
