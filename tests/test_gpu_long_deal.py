"""Whole runs of long uniform records in the W8 pair's EXT 3 kernel, whose waves take their eight records with a stride
of eight within each 64 records of a run (gcm_kernels.h claim_unit), so that packed records share their front padding
within a wave, and whose segments skip the AES of a step that holds only padding and AAD and end by the serial chain
over the lanes' ranks, whatever the records' paddings (segment.h, ghash.h w8_lane_end). Every sealed
record, tag, opened byte and ok byte against lib/fusion.c, with tampered ciphertext, tag and AAD bits.

Shapes: 33,280 records (130 per workgroup at 256 CUs: two full blocks of 64 and a block of two, so the last claims hold
invalid groups) of at least 65 steps. Packed outputs rotate the padding with the record index; a stride that is a
multiple of 128 gives one padding; an odd stride leaves the output unaligned to 16 bytes; a shuffled record order
gives a wave records of different paddings (the bounds then come from the wave's lanes, as before the dealing)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import picotls_amd as pa  # noqa: E402
from oracle import FusionRef  # noqa: E402
from picotls_amd.records import RecordBatch  # noqa: E402
from gpu_util import dev, empty, gpu_open, gpu_seal  # noqa: E402

pytestmark = pytest.mark.gpu

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))
N = 256 * 130


@pytest.fixture(scope="module")
def ref():
    assert torch.cuda.is_available(), "no GPU visible"
    pa.load_library()
    if not HAVE_REF:
        pytest.skip("oracle/_ref/libfusion_ref.so not shipped")
    return FusionRef()


def _layout(b, lens, layout, rng):
    """The batch's descriptors with the sealed records (the seal's outputs) and the opened plaintexts (the open's) laid
    out as `layout` says; returns (seal, open, sealed_bytes, pt_out_bytes)."""
    n = len(lens)
    seal, opn = b.seal.copy(), b.open.copy()
    sealed_bytes, out_bytes = b.sealed_bytes, b.pt_bytes
    if layout in ("stride128", "odd"):
        slot = (int(lens.max()) + 16 + 127) // 128 * 128 + (0 if layout == "stride128" else 9)
        base = 0 if layout == "stride128" else 3
        off = (np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(base))
        seal["out_off"], opn["in_off"], opn["out_off"] = off, off, off
        sealed_bytes = out_bytes = n * slot + base
    elif layout == "shuffled":
        p = rng.permutation(n)
        seal, opn = seal[p], opn[p]
    else:
        assert layout == "packed"
    return seal, opn, sealed_bytes, out_bytes


def _check(ref, rng, lens, aads, key_size, nkeys, layout="packed", tamper=12, tree_runs=200, only_tree=True):
    lens, n = np.asarray(lens), len(lens)
    key_idx = np.sort(rng.integers(0, nkeys, n)) if nkeys > 1 else None
    b = RecordBatch.build(lens, np.asarray(aads), seqs=rng.integers(0, 2**62, n, dtype=np.uint64), key_idx=key_idx)
    seal, opn, sealed_bytes, out_bytes = _layout(b, lens, layout, rng)
    keys = np.frombuffer(rng.bytes(nkeys * key_size), np.uint8)
    ivs = np.frombuffer(rng.bytes(nkeys * 12), np.uint8)
    pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
    aad = np.frombuffer(rng.bytes(max(b.aad_bytes, 1)), np.uint8)
    ks = pa.Keyset(keys, ivs, key_size)
    pa.debug_counters(reset=True)
    sealed = gpu_seal(ks, seal, pt, aad, sealed_bytes)
    c_seal = pa.debug_counters(reset=True)
    want = np.zeros(sealed_bytes, np.uint8)
    ref.run_batch(True, keys, ivs, key_size, seal, pt, aad, want, nthreads=8)
    if not np.array_equal(sealed, want):
        bad_recs = [i for i in range(n) if not np.array_equal(
            sealed[int(seal[i]["out_off"]):int(seal[i]["out_off"]) + int(seal[i]["len"]) + 16],
            want[int(seal[i]["out_off"]):int(seal[i]["out_off"]) + int(seal[i]["len"]) + 16])]
        pytest.fail(f"{len(bad_recs)} sealed records differ from fusion, first {bad_recs[:8]}")
    # open fusion's records with tampered ciphertext, tag and AAD bits; the plaintext is written either way, as fusion
    bad, badaad = want.copy(), aad.copy()
    victims = rng.choice(n, tamper, replace=False)
    for t, v in enumerate(victims):
        o, ln, al = int(opn[v]["in_off"]), int(opn[v]["len"]), int(opn[v]["aad_len"])
        if t % 3 == 0:
            bad[o + int(rng.integers(0, ln))] ^= 1 << int(rng.integers(0, 8))
        elif t % 3 == 1 or al == 0:
            bad[o + ln + int(rng.integers(0, 16))] ^= 0x20
        else:
            badaad[int(opn[v]["aad_off"]) + int(rng.integers(0, al))] ^= 2
    back, ok = gpu_open(ks, opn, bad, badaad, out_bytes, out_fill=0x5A)
    c_open = pa.debug_counters(reset=True)
    expect_ok = np.ones(n, np.uint8)
    expect_ok[victims] = 0
    ref_back, ref_ok = np.full(out_bytes, 0x5A, np.uint8), np.zeros(n, np.uint8)
    _, fails = ref.run_batch(False, keys, ivs, key_size, opn, bad, badaad, ref_back, ok=ref_ok, nthreads=8)
    assert fails == tamper and np.array_equal(ref_ok, expect_ok)
    assert np.array_equal(ok, expect_ok)
    assert np.array_equal(back, ref_back)
    for c in (c_seal, c_open):  # the runs were EXT 3's
        assert c["launches"]["w8_tree"] == 1 and c["runs"]["w8_tree"] >= tree_runs, c
        if only_tree:
            assert c["runs"]["w8_serial"] == 0, c
    ks.free()


@pytest.mark.parametrize("length,aad", [(8200, 0), (8192, 5), (8177, 16), (16385, 21), (16384, 5)])
def test_long_runs_lengths_and_aads_vs_fusion(ref, length, aad):
    # packed records: the front padding rotates with the record index (by one position a record at 16 KiB + tag); 0 to
    # 2 AAD blocks; a partial last text block (8177, 16385) and a text of whole blocks
    rng = np.random.default_rng(9100 + length + aad)
    _check(ref, rng, np.full(N, length), np.full(N, aad), 16, 1)


def test_long_runs_mixed_lengths_within_the_uniform_slack_vs_fusion(ref):
    # 65 to 67 steps in one run (UNIFORM_SLACK 2), AADs of 0 to 21 bytes: a wave's records differ in steps and padding
    rng = np.random.default_rng(9201)
    _check(ref, rng, rng.integers(8200, 8430, N), rng.choice([0, 5, 16, 21], N), 16, 1)


@pytest.mark.parametrize("layout,length,aad", [("stride128", 8200, 5), ("odd", 8192, 21), ("shuffled", 16384, 5),
                                               ("shuffled", 8177, 0)])
def test_long_runs_output_layouts_vs_fusion(ref, layout, length, aad):
    # one padding for every record (a stride of a multiple of 128), outputs unaligned to 16 bytes (an odd stride), and a
    # record order in which the records of a wave have different paddings (shuffled)
    rng = np.random.default_rng(9300 + length + aad + len(layout))
    _check(ref, rng, np.full(N, length), np.full(N, aad), 16, 1, layout=layout)


def test_long_runs_aes256_three_keys_vs_fusion(ref):
    # three connections: a workgroup whose range holds a key change cuts the shorter side into units (EXT 4)
    rng = np.random.default_rng(9401)
    _check(ref, rng, np.full(N, 8200), np.full(N, 5), 32, 3, tree_runs=180, only_tree=False)


def test_long_runs_batch_not_a_multiple_of_the_block_vs_fusion(ref):
    # 33,317 records: ranges of 130 and 131 records, the last block of each run partly invalid
    rng = np.random.default_rng(9501)
    n = N + 37
    _check(ref, rng, np.full(n, 8200), np.full(n, 16), 16, 1)


def _framed(ref, rng, tls12):
    """33,280 framed records of 8200 payload bytes, sealed (every wire byte) and opened back. Expected wire records from
    fusion's batch over the same AEAD inputs: TLS 1.3 header || AEAD(payload || type) under the header as AAD; TLS 1.2
    header || explicit nonce || AEAD(payload) with the nonce as sequence number under BE64(seq) || type || 3 || 3 ||
    BE16(len)."""
    n, ln = N, 8200
    key, fixed = rng.bytes(16), rng.bytes(4)
    iv = fixed + bytes(8) if tls12 else fixed + rng.bytes(8)
    seqs = rng.integers(0, 2**40, n).astype(np.uint64)
    nonces = rng.integers(0, 2**62, n).astype(np.uint64)
    payload = np.frombuffer(rng.bytes(n * ln), np.uint8).reshape(n, ln)
    pre, text, over = (8, ln, 13 + 16) if tls12 else (0, ln + 1, 5 + 16)
    # the engine's input arena: (TLS 1.2: the explicit nonce, big endian, then) the payload
    arena = np.zeros((n, pre + ln), np.uint8)
    arena[:, pre:] = payload
    if tls12:
        arena[:, :8] = nonces.astype(">u8").view(np.uint8).reshape(n, 8)
    recs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    recs["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(pre + ln)
    recs["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(text + over)
    recs["len"], recs["seq"], recs["flags"] = ln, seqs, 23
    # fusion's inputs: the AEAD plaintexts, the AADs, and outputs after each wire header
    fpt = np.full((n, text), 23, np.uint8)
    fpt[:, :ln] = payload
    wl = text + 16 + (8 if tls12 else 0)
    hdr = np.zeros((n, 5), np.uint8)
    hdr[:] = [23, 3, 3, wl >> 8, wl & 0xFF]
    if tls12:
        faad = np.zeros((n, 16), np.uint8)
        faad[:, :8] = seqs.astype(">u8").view(np.uint8).reshape(n, 8)
        faad[:, 8:13] = [23, 3, 3, ln >> 8, ln & 0xFF]
        alen = 13
    else:
        faad = np.zeros((n, 16), np.uint8)
        faad[:, :5] = hdr
        alen = 5
    frecs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    frecs["in_off"] = np.arange(n, dtype=np.uint64) * np.uint64(text)
    frecs["out_off"] = recs["out_off"] + np.uint64(over - 16)
    frecs["aad_off"] = np.arange(n) * 16
    frecs["len"], frecs["aad_len"], frecs["seq"] = text, alen, nonces if tls12 else seqs
    want = np.zeros(n * (text + over), np.uint8)
    keys, ivs = np.frombuffer(key, np.uint8), np.frombuffer(iv, np.uint8)
    ref.run_batch(True, keys, ivs, 16, frecs, fpt.reshape(-1), faad.reshape(-1), want, nthreads=8)
    w2 = want.reshape(n, text + over)
    w2[:, :5] = hdr
    if tls12:
        w2[:, 5:13] = arena[:, :8]
    ks = pa.Keyset(key, iv, 16)
    s = torch.cuda.current_stream().cuda_stream
    d_recs, d_in, d_out = dev(recs), dev(arena), empty(want.size, 0xEE)
    pa.debug_counters(reset=True)
    (pa.seal_tls12_records if tls12 else pa.seal_tls_records)(ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), s)
    torch.cuda.synchronize()
    c_seal = pa.debug_counters(reset=True)
    out = d_out.cpu().numpy()
    if not np.array_equal(out, want):
        bad = np.nonzero((out.reshape(n, -1) != w2).any(axis=1))[0]
        pytest.fail(f"{len(bad)} wire records differ from fusion, first {list(bad[:8])}")
    # open the wire records, three of them tampered: ciphertext, tag, and an authenticated byte before the ciphertext
    # (TLS 1.3: the header's length, part of the AAD; TLS 1.2: the explicit nonce)
    wire = want.copy().reshape(n, text + over)
    victims = rng.choice(n, 3, replace=False)
    wire[victims[0], over - 16 + 100] ^= 4
    wire[victims[1], -1] ^= 0x80
    wire[victims[2], 12 if tls12 else 4] ^= 1
    orecs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    orecs["in_off"], orecs["len"], orecs["seq"] = recs["out_off"], text, seqs
    orecs["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(text)
    d_recs2, d_wire, d_plain = dev(orecs), dev(wire), empty(n * text + 1)
    d_ok, d_res = empty(n, 0x77), empty(8 * n, 0x77)
    (pa.open_tls12_records if tls12 else pa.open_tls_records)(ks, d_recs2.data_ptr(), n, d_wire.data_ptr(), d_plain.data_ptr(),
                                                               d_ok.data_ptr(), d_res.data_ptr(), s)
    torch.cuda.synchronize()
    c_open = pa.debug_counters(reset=True)
    expect_ok = np.ones(n, np.uint8)
    expect_ok[victims] = 0
    assert np.array_equal(d_ok.cpu().numpy(), expect_ok)
    res = d_res.cpu().numpy().view(pa.TLS_RESULT_DTYPE)
    good = expect_ok == 1
    assert (res["status"][good] == pa.TLS_OK).all() and (res["plain_len"][good] == ln).all()
    assert (res["status"][~good] != pa.TLS_OK).all()
    plain = d_plain.cpu().numpy()[:n * text].reshape(n, text)
    assert np.array_equal(plain[good][:, :ln], payload[good])
    for c in (c_seal, c_open):
        assert c["launches"]["w8_tree"] == 1 and c["runs"]["w8_tree"] >= 200 and c["runs"]["w8_serial"] == 0, c
    ks.free()


def test_long_runs_tls13_framed_vs_fusion(ref):
    _framed(ref, np.random.default_rng(9601), tls12=False)


def test_long_runs_tls12_framed_vs_fusion(ref):
    _framed(ref, np.random.default_rng(9602), tls12=True)
