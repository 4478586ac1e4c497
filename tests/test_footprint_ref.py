"""The references keep the write footprint: on byte-adjacent records (RecordBatch.build_offsets: no padding, odd bases)
in arenas pre-filled with random bytes, lib/fusion.c on 8 threads and the plain-C oracle leave identical whole arenas on
seal, fusion's open writes the records' plaintext bytes and nothing else, and the OpenSSL ChaCha20-Poly1305 reference
does the same. test_gpu_footprint.py relies on this when it compares whole arenas with the references' without a mask.
CPU only."""
import os

import numpy as np
import pytest

import chacha_ref as R
from footprint_util import assert_arena, packed_case, rand_bytes, span_mask, tamper
from oracle import FusionRef, GcmOracle

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))
needs_fusion = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libfusion_ref.so not built (needs /root/reference)")


def _lens(rng):
    # every length 0..299, then 300 random ones up to 20,000 bytes; AADs of 0..39 bytes
    return np.concatenate([np.arange(300), rng.integers(0, 20001, 300)]), rng.integers(0, 40, 600)


@needs_fusion
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("key_size", [16, 32])
def test_fusion_and_oracle_keep_the_footprint(key_size, in_place):
    rng = np.random.default_rng(4100 + key_size + in_place)
    lens, aads = _lens(rng)
    c = packed_case(rng, lens, aads, key_size, nkeys=3, in_place=in_place)
    s = c.b.seal
    assert int(s["seq"].max()) >> 63 == 1  # (full 64-bit sequence numbers)
    ref, oracle = FusionRef(), GcmOracle()
    src0 = c.src.copy()
    want = c.fill.copy()
    ref.run_batch(True, c.keys, c.ivs, key_size, s, c.src, c.aad, want, nthreads=8)
    other = c.fill.copy()
    oracle.seal_batch(c.keys, c.ivs, key_size, s, c.src, c.aad, other)
    assert_arena(want, other, c.sealed_offs, c.sealed_sizes, "fusion's sealed arena against the oracle's")
    assert np.array_equal(c.src, src0)  # (the inputs are read only)
    outside = ~span_mask(c.sealed_offs, c.sealed_sizes, want.size)
    assert outside.sum() == 3 + 64 and np.array_equal(want[outside], c.fill[outside])
    # every record also equals fusion's single-record seal of its own text and AAD
    for i in range(0, c.n, 7):
        k, o, ln, a, al = (int(s[f][i]) for f in ("key_idx", "out_off", "len", "aad_off", "aad_len"))
        p = int(s["in_off"][i])
        assert want[o:o + ln + 16].tobytes() == ref.seal(c.keys[k * key_size:(k + 1) * key_size].tobytes(),
                                                         c.ivs[12 * k:12 * k + 12].tobytes(), int(s["seq"][i]),
                                                         c.aad[a:a + al].tobytes(), src0[p:p + ln].tobytes()), i

    # open: three tampered records (ciphertext, tag, AAD); the plaintext is written for them too
    bad, badaad, victims, (ct_v, at, bit) = tamper(rng, c, want)
    plain = c.src.copy()  # what the open must restore: the plaintext, with the flipped ciphertext bit (CTR)
    plain[int(s["in_off"][ct_v]) + at] ^= bit
    ok = np.full(c.n, 0xAA, np.uint8)
    if in_place:
        back = bad.copy()
        ref.run_batch(False, c.keys, c.ivs, key_size, c.b.open, bad, badaad, back, ok=ok, nthreads=8)
        text = span_mask(c.plain_offs, c.plain_sizes, back.size)
        expect = np.where(text, plain, bad)  # tags and tail as the seal left them
    else:
        pfill = rand_bytes(rng, c.b.pt_bytes)
        back = pfill.copy()
        ref.run_batch(False, c.keys, c.ivs, key_size, c.b.open, bad, badaad, back, ok=ok, nthreads=8)
        text = span_mask(c.plain_offs, c.plain_sizes, back.size)
        expect = np.where(text, plain, pfill)
    assert_arena(back, expect, c.plain_offs, c.plain_sizes, "fusion's opened arena")
    want_ok = np.ones(c.n, np.uint8)
    want_ok[victims] = 0
    assert np.array_equal(ok, want_ok)
    back2, ok2 = (bad.copy() if in_place else pfill.copy()), np.full(c.n, 0xAA, np.uint8)
    oracle.open_batch(c.keys, c.ivs, key_size, c.b.open, bad, badaad, back2, ok2)
    assert np.array_equal(ok2, want_ok)
    good = span_mask(c.plain_offs[want_ok == 1], c.plain_sizes[want_ok == 1], back.size)
    assert np.array_equal(back2[good], expect[good]) and np.array_equal(back2[~text], expect[~text])


@pytest.mark.parametrize("in_place", [False, True])
def test_chacha_reference_keeps_the_footprint(in_place):
    rng = np.random.default_rng(4200 + in_place)
    lens = np.concatenate([np.arange(130), rng.integers(0, 5000, 30)])
    c = packed_case(rng, lens, rng.integers(0, 40, len(lens)), 32, nkeys=2, in_place=in_place)
    keys = [c.keys[32 * k:32 * k + 32].tobytes() for k in range(2)]
    ivs = [c.ivs[12 * k:12 * k + 12].tobytes() for k in range(2)]
    s = c.b.seal
    want = c.fill.copy()
    R.seal_records(keys, ivs, s, c.src, c.aad, want)
    outside = ~span_mask(c.sealed_offs, c.sealed_sizes, want.size)
    assert outside.sum() == 3 + 64 and np.array_equal(want[outside], c.fill[outside])
    for i in range(c.n):  # OpenSSL opens every record back; a tenth of them also equal the plain-Python restatement
        k, o, ln, a, al, p = (int(s[f][i]) for f in ("key_idx", "out_off", "len", "aad_off", "aad_len", "in_off"))
        nonce = R.nonce_for(ivs[k], int(s["seq"][i]))
        assert R.ossl_open(keys[k], nonce, want[o:o + ln + 16].tobytes(), c.aad[a:a + al].tobytes()) == c.src[p:p + ln].tobytes(), i
        if i % 10 == 0:
            assert want[o:o + ln + 16].tobytes() == R.py_seal(keys[k], nonce, c.src[p:p + ln].tobytes(), c.aad[a:a + al].tobytes()), i
