"""Every AEAD kernel family writes its records' bytes and nothing else.

include/picotls/mi355x.h gives byte offsets with no alignment rule, so a caller may pack records back to back and seal or
open in place. Here record i + 1 starts on the byte after record i ends (RecordBatch.build_offsets: odd bases, no padding,
so the offsets take every residue mod 16 and mod 64), the output arenas start as random bytes, and the whole arena is
compared with the one the reference wrote into (lib/fusion.c, or OpenSSL for ChaCha20-Poly1305), with no mask: a store
that reaches one byte past [out_off, out_off + len + 16) on seal, or [out_off, out_off + len) on open, lands in a
neighbouring record, a tag or the tail, all of them random bytes, and shows. ok bytes, TLS results and header-protection
masks have a filled tail too. test_footprint_ref.py pins that the references themselves keep the footprint.

Each case asserts through the debug counters that the kernel family it is meant for ran. Every case runs the packed
layout and the in-place one (in_off == out_off; after the open the arena is the sealed arena with only the plaintext
bytes replaced)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import chacha_ref as R  # noqa: E402
import picotls_amd as pa  # noqa: E402
from footprint_util import TAIL, assert_arena, packed_case, rand_bytes, span_mask, tamper  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import FusionRef  # noqa: E402
from test_gpu_fuzz import _lengths  # noqa: E402

pytestmark = pytest.mark.gpu

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))
OK_FILL = 0xAA  # (neither 0 nor 1: an ok byte that was never written shows)
LAYOUTS = pytest.mark.parametrize("in_place", [False, True], ids=["packed", "in_place"])
# the smallest batches with whole runs: one persistent workgroup per CU (256) walks a contiguous range, and a range
# holds a whole run from WHOLE_MIN_RECS = 128 records (130 per workgroup, as test_gpu_w8.py's whole-run batches)
WHOLE_RUN_BATCH = 256 * 130


@pytest.fixture(scope="module", autouse=True)
def engine():
    assert torch.cuda.is_available(), "no GPU visible"
    pa.load_library()
    torch.cuda.init()


@pytest.fixture(scope="module")
def ref():
    if not HAVE_REF:
        pytest.skip("oracle/_ref/libfusion_ref.so not shipped")
    return FusionRef()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _seal_batch(ks, d_recs, n, d_in, d_aad, d_out):
    pa.seal_batch(ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())


def _routed(routing, phase):
    """Prints the launch's non-zero counters (pytest -rP shows them), then asserts the kernel family."""
    cnt = pa.debug_counters(reset=True)
    print(phase, {kind: {k: int(v) for k, v in d.items() if v} for kind, d in cnt.items()})
    routing(cnt, phase)


def check(ref, rng, c, routing, schedule=None, rejected=(), do_seal=_seal_batch):
    """The one checker: seals case ``c`` (footprint_util.PackedCase) over its random fill and compares the whole arena
    with fusion's, then opens fusion's arena with three tampered records (a ciphertext, a tag and an AAD bit) into
    another random fill (in place: over the sealed arena) and compares the whole plaintext arena with fusion's, the ok
    bytes exactly and their tail. ``routing(counters, phase)`` asserts the kernel family on the seal's and the open's
    counters. ``rejected``: records whose descriptors the caller made invalid (nothing written, ok = 0); fusion runs
    the others."""
    b, n, key_size = c.b, c.n, c.key_size
    good = np.setdiff1d(np.arange(n), np.asarray(rejected, np.int64))
    ks = pa.Keyset(c.keys, c.ivs, key_size)
    if schedule is not None:
        ks.set_schedule(schedule, allow_variable_time=True)
    want = c.fill.copy()
    ref.run_batch(True, c.keys, c.ivs, key_size, b.seal[good], c.src, c.aad, want, nthreads=8)
    d_seal, d_aad = dev(b.seal), dev(c.aad)
    d_in = dev(c.src)
    d_out = d_in if c.in_place else dev(c.fill)
    pa.debug_counters(reset=True)
    do_seal(ks, d_seal, n, d_in, d_aad, d_out)
    torch.cuda.synchronize()
    _routed(routing, "seal")
    assert_arena(d_out.cpu().numpy(), want, c.sealed_offs, c.sealed_sizes, "sealed arena against fusion's")
    if not c.in_place:
        assert np.array_equal(d_in.cpu().numpy(), c.src), "the seal wrote to its input arena"
    assert np.array_equal(d_aad.cpu().numpy(), c.aad), "the seal wrote to the AAD arena"
    del d_in, d_out

    bad, badaad, victims, _ = tamper(rng, c, want, candidates=good)
    want_ok = np.zeros(n, np.uint8)
    want_ok[good] = 1
    want_ok[victims] = 0
    ref_ok = np.full(len(good), OK_FILL, np.uint8)
    pfill = bad if c.in_place else rand_bytes(rng, b.pt_bytes)
    ref_back = pfill.copy()
    ref.run_batch(False, c.keys, c.ivs, key_size, b.open[good], bad, badaad, ref_back, ok=ref_ok, nthreads=8)
    assert np.array_equal(ref_ok, want_ok[good])
    d_open, d_badaad, d_bad = dev(b.open), dev(badaad), dev(bad)
    d_back = d_bad if c.in_place else dev(pfill)
    d_ok = dev(np.full(n + TAIL, OK_FILL, np.uint8))
    pa.debug_counters(reset=True)
    pa.open_batch(ks, d_open.data_ptr(), n, d_bad.data_ptr(), d_badaad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(routing, "open")
    ok, back = d_ok.cpu().numpy(), d_back.cpu().numpy()
    assert np.array_equal(ok[:n], want_ok), f"ok bytes differ at records {np.flatnonzero(ok[:n] != want_ok)[:8]}"
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"
    if c.in_place:
        assert_arena(back, ref_back, c.sealed_offs, c.sealed_sizes, "arena opened in place (a record's last 16 bytes: its tag)")
    else:
        assert_arena(back, ref_back, c.plain_offs, c.plain_sizes, "opened arena against fusion's")
    if c.in_place:  # only plaintext bytes replaced: tags, rejected records and the tail as the seal left them
        kept = ~span_mask(c.plain_offs[good], c.plain_sizes[good], back.size)
        assert np.array_equal(back[kept], bad[kept]), "the in-place open changed bytes outside the records' texts"
    else:
        assert np.array_equal(d_bad.cpu().numpy(), bad), "the open wrote to its input arena"
    ks.free()


def _no_w8(c, phase):
    assert c["launches"]["w8_serial"] == 0 and c["launches"]["w8_tree"] == 0, f"{phase}: {c}"


def _serial_only(c, phase):
    assert c["launches"]["w8_serial"] >= 1 and c["launches"]["w8_tree"] == 0, f"{phase}: {c}"


# ------------------------------------------------------------------------------------------------ the batch kernels


@LAYOUTS
@pytest.mark.parametrize("nkeys", [1, 7])
@pytest.mark.parametrize("key_size", [16, 32])
@pytest.mark.parametrize("schedule", ["chunked", "lockstep"])
def test_4bit_kernels(ref, schedule, key_size, nkeys, in_place):
    """Under W8_MIN_RECS = 256 records the 4-bit kernels run: 255 records of every length 0..254, AADs of 0..40 bytes,
    on the chunked and the lockstep schedule."""
    rng = np.random.default_rng(5000 + key_size + nkeys + 100 * in_place + (1000 if schedule == "lockstep" else 0))
    c = packed_case(rng, np.arange(255), np.arange(255) % 41, key_size, nkeys, in_place)

    def routing(cnt, phase):
        _no_w8(cnt, phase)
        assert (cnt["launches"]["lockstep"] >= 1) == (schedule == "lockstep"), f"{phase}: {cnt}"

    check(ref, rng, c, routing, schedule=schedule)


@LAYOUTS
@pytest.mark.parametrize("nkeys", [1, 3])
def test_w8_serial_cut_runs_beside_rejected_descriptors(ref, nkeys, in_place):
    """The W8 serial kernel alone (EXT 4; too few records per workgroup for whole runs): 2,500 records of the fuzz
    tests' length mix in cut runs, so that units, pair8 holders and record ends meet neighbours at every residue. Two
    descriptors carry a len above PTLS_MI355X_MAX_RECORD_LEN and one a key index outside the keyset: their ranges keep
    the fill (in place: the caller's bytes) and their ok bytes are 0."""
    rng = np.random.default_rng(5100 + nkeys + 10 * in_place)
    n = 2500
    c = packed_case(rng, _lengths(rng, n), rng.integers(0, 41, n), 16 if nkeys == 1 else 32, nkeys, in_place)
    rejected = [701, 1502, 2203]
    for d in (c.b.seal, c.b.open):
        d["len"][701], d["len"][1502] = (1 << 30) + 1, 0xFFFFFFFF
        d["key_idx"][2203] = nkeys + 2
    check(ref, rng, c, _serial_only, rejected=rejected)


@LAYOUTS
@pytest.mark.parametrize("base", [1100, 20])
def test_w8_serial_whole_runs_in_4_lane_groups(ref, base, in_place):
    """Whole runs of the W8 serial kernel in 4-lane groups (paired half-line stores; the open's line holding): records
    of base + U[0, 200) bytes, within UNIFORM_SLACK steps of each other, so the runs stay whole while the byte-adjacent
    offsets take every residue mod 16 and mod 64. A workgroup takes whole runs from WHOLE_MIN_RECS = 128 records of its
    own (ENGINE_WG / ENGINE_G, common.h), so the batch is 256 x 130 records, as test_w8_g4_whole_runs_vs_fusion's; with
    256 x 33 the counters showed no whole run at all."""
    rng = np.random.default_rng(5200 + base + in_place)
    n = WHOLE_RUN_BATCH
    c = packed_case(rng, base + rng.integers(0, 200, n), rng.choice([0, 13, 17], n), 16, 1, in_place)

    def routing(cnt, phase):
        assert cnt["runs"]["w8_g4"] > 0, f"{phase}: {cnt}"

    check(ref, rng, c, routing)


@LAYOUTS
def test_w8_tree_kernel(ref, in_place):
    """The EXT 3 (tree) kernel: whole runs of records of at least W8_MIN_STEPS = 64 steps, 256 x 130 records (see
    WHOLE_RUN_BATCH) of 8200 + U[0, 200) bytes under one key."""
    rng = np.random.default_rng(5300 + in_place)
    n = WHOLE_RUN_BATCH
    c = packed_case(rng, 8200 + rng.integers(0, 200, n), np.full(n, 13), 16, 1, in_place)

    def routing(cnt, phase):
        assert cnt["launches"]["w8_tree"] == 1 and cnt["runs"]["w8_tree"] > 0, f"{phase}: {cnt}"

    check(ref, rng, c, routing)


@LAYOUTS
def test_w8_multi_key_runs(ref, in_place):
    """Multi-key runs (connections of fewer records than a workgroup has groups joined into one whole run): 20,000
    records, 17 per connection, of 600 + U[0, 100) bytes, AES-128."""
    rng = np.random.default_rng(5400 + in_place)
    n = 20000
    key_idx = np.arange(n) // 17
    c = packed_case(rng, 600 + rng.integers(0, 100, n), rng.choice([0, 13, 17], n), 16, int(key_idx[-1]) + 1, in_place,
                    key_idx=key_idx)

    def routing(cnt, phase):
        assert cnt["runs"]["w8_mk"] > 0, f"{phase}: {cnt}"

    check(ref, rng, c, routing)


@LAYOUTS
def test_device_regrouping(ref, in_place):
    """3,000 records over 300 keys in random order are grouped by key on the device: the kernels walk a permutation,
    and the ok bytes are written through it to each record's own index, with the tail untouched."""
    rng = np.random.default_rng(5500 + in_place)
    n = 3000
    c = packed_case(rng, rng.integers(0, 5000, n), rng.integers(0, 41, n), 32, 300, in_place, key_idx=rng.integers(0, 300, n))
    check(ref, rng, c, _serial_only)


@LAYOUTS
def test_spread_launch(ref, in_place):
    """A batch of fewer records than CUs whose long records the spare workgroups share in pieces: 600 KiB + 5, 100 and
    1 MiB + 1 bytes, byte-adjacent (with three records every one is tampered in the open: all ok bytes are 0 and the
    plaintext is written all the same, as fusion does)."""
    rng = np.random.default_rng(5600 + in_place)
    c = packed_case(rng, np.array([(600 << 10) + 5, 100, (1 << 20) + 1]), np.array([13, 5, 21]), 32, 1, in_place)

    def routing(cnt, phase):
        assert cnt["launches"]["spread"] >= 1, f"{phase}: {cnt}"

    check(ref, rng, c, routing)


@LAYOUTS
def test_seal_with_header_protection_masks(ref, in_place):
    """seal_batch_hp: 300 QUIC-sized packets of 1185..1215 bytes over 5 connections, the masks of samples in the sealed
    output computed by the seal launch; the masks buffer has a filled tail."""
    rng = np.random.default_rng(5700 + in_place)
    n, nkeys = 300, 5
    lens = rng.integers(1185, 1216, n)
    c = packed_case(rng, lens, rng.integers(8, 30, n), 16, nkeys, in_place)
    s = c.b.seal
    hp_keys = rand_bytes(rng, nkeys * 16)
    sample_in_ct = 4 - rng.integers(1, 5, n)
    hp = np.zeros(n, dtype=pa.HP_DTYPE)
    hp["sample_off"] = s["out_off"] + sample_in_ct.astype(np.uint64)
    hp["key_idx"] = s["key_idx"]
    hp_ks = pa.Keyset(hp_keys, np.zeros(nkeys * 12, np.uint8), 16)
    mfill = rand_bytes(rng, 16 * n + TAIL)
    d_hp, d_masks = dev(hp), dev(mfill)

    def do_seal(ks, d_recs, n_, d_in, d_aad, d_out):
        pa.seal_batch_hp(ks, d_recs.data_ptr(), n_, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), hp_ks, d_hp.data_ptr(),
                         d_masks.data_ptr(), _stream())

    def routing(cnt, phase):
        if phase == "seal":
            assert cnt["launches"]["seal_hp"] >= 1, f"{cnt}"

    check(ref, rng, c, routing, do_seal=do_seal)
    want_masks = mfill.copy()
    for i in range(n):
        k, p, ln, a, al = (int(s[f][i]) for f in ("key_idx", "in_off", "len", "aad_off", "aad_len"))
        _, mask = ref.seal_with_hp(c.keys[16 * k:16 * k + 16].tobytes(), c.ivs[12 * k:12 * k + 12].tobytes(), int(s["seq"][i]),
                                   c.aad[a:a + al].tobytes(), c.src[p:p + ln].tobytes(), hp_keys[16 * k:16 * k + 16].tobytes(),
                                   int(sample_in_ct[i]))
        want_masks[16 * i:16 * i + 16] = np.frombuffer(mask, np.uint8)
    assert_arena(d_masks.cpu().numpy(), want_masks, 16 * np.arange(n), np.full(n, 16), "header-protection masks")
    hp_ks.free()


# ------------------------------------------------------------------------------------------------ the per-record path


@pytest.mark.parametrize("key_size", [16, 32])
def test_per_record_path(ref, key_size):
    """ptls_mi355x_encrypt / decrypt on host buffers (the picotls objects' calls): into a random-filled buffer at an odd
    offset, apart and in place, lengths around the unit sizes and 300,001 bytes, which runs over many workgroups. The
    bytes before the output and after its last byte are untouched."""
    rng = np.random.default_rng(5800 + key_size)
    key, iv = rng.bytes(key_size), rng.bytes(12)
    ks = pa.Keyset(key, iv, key_size)
    ks.set_constant_time(True)
    lib = pa.load_library()
    at = 3

    def ptr(a, off=0):
        return ctypes.c_void_p(a.ctypes.data + off)

    for ln in (0, 1, 15, 17, 2047, 2049, 300001):
        pt, aad, seq = rand_bytes(rng, ln)[:ln], rng.bytes(13), int(rng.integers(0, 2**64, dtype=np.uint64))
        sealed = np.frombuffer(ref.seal(key, iv, seq, aad, pt.tobytes()), np.uint8)
        aadb = np.frombuffer(aad, np.uint8)
        for in_place in (False, True):
            buf = rand_bytes(rng, at + ln + 16 + TAIL)
            if in_place:
                buf[at:at + ln] = pt
            want = buf.copy()
            want[at:at + ln + 16] = sealed
            src = buf[at:] if in_place else pt.copy()
            pa.debug_counters(reset=True)
            assert lib.ptls_mi355x_encrypt(ks.handle, 0, ptr(buf, at), ptr(src), ln, seq, ptr(aadb), 13) == 0, pa._err("encrypt")
            cnt = pa.debug_counters(reset=True)
            assert (cnt["launches"]["span"] >= 1) == (ln >= 262144), (ln, cnt)
            assert_arena(buf, want, [at], [ln + 16], f"encrypt of {ln} bytes, in_place={in_place}")
            # decrypt: fusion's record back into a filled buffer (in place: over the record itself)
            buf = rand_bytes(rng, at + ln + 16 + TAIL)
            if in_place:
                buf[at:at + ln + 16] = sealed
            want = buf.copy()
            want[at:at + ln] = pt
            src = buf[at:] if in_place else sealed.copy()
            got = lib.ptls_mi355x_decrypt(ks.handle, 0, ptr(buf, at), ptr(src), ln + 16, seq, ptr(aadb), 13)
            assert got == ln, (ln, in_place, got)
            assert_arena(buf, want, [at], [ln], f"decrypt of {ln} bytes, in_place={in_place}")
    ks.free()


# ------------------------------------------------------------------------------------------------ framed opens


def _framed_case(ref, rng, version, n, header_failures):
    """n TLS wire records back to back (payloads of 0..16,383 bytes, three connections) sealed by fusion, with a
    ciphertext bit, a tag bit and a header bit (an AAD bit) flipped in three of them and, with ``header_failures``, two
    records whose tag verifies under a header the record layer refuses. Returns the open descriptors, the wire, the
    expected plaintext arena over ``pfill`` (byte-adjacent at stride text from an odd base), ok bytes and results."""
    nkeys = 3
    key_size = 32 if version == 13 else 16
    lens = rng.integers(0, 16384, n)
    types = rng.choice([21, 22, 23], n)
    key_idx = np.arange(n) * nkeys // n
    seqs = rng.integers(0, 2**64, n, dtype=np.uint64)
    text = lens + 1 if version == 13 else lens
    head = 5 if version == 13 else 13  # bytes of the wire record in front of the ciphertext
    aad_len = 5 if version == 13 else 13
    wire_off = np.concatenate([[0], np.cumsum(text + head + 16)[:-1]]).astype(np.int64)
    text_off = np.concatenate([[0], np.cumsum(text)[:-1]]).astype(np.int64)
    total = int(text.sum())
    victims = [int(v) for v in rng.choice(np.flatnonzero(text > 0), 5, replace=False)]
    ct_v, tag_v, hdr_v = victims[:3]
    hdr_fail = victims[3:] if header_failures else []
    keys = rand_bytes(rng, nkeys * key_size)
    if version == 13:
        ivs = rand_bytes(rng, nkeys * 12)
        nonces = seqs
    else:  # the GCM nonce is fixed IV || explicit nonce: fusion's seq is the explicit nonce on a static IV of fixed || 0^64
        ivs = np.concatenate([np.concatenate([rand_bytes(rng, 4), np.zeros(8, np.uint8)]) for _ in range(nkeys)])
        nonces = rng.integers(0, 2**64, n, dtype=np.uint64)
    inner = rand_bytes(rng, total)
    aad = np.zeros(aad_len * n, np.uint8)
    headers = []
    for i in range(n):
        if version == 13:
            inner[text_off[i] + lens[i]] = types[i]
            outer = 22 if i in hdr_fail else 23  # (authenticated: the tag verifies under the refused header)
            hdr = bytes([outer, 3, 3]) + int(text[i] + 16).to_bytes(2, "big")
            aad[5 * i:5 * i + 5] = np.frombuffer(hdr, np.uint8)
        else:
            hdr = bytes([int(types[i]), 3, 3]) + int(lens[i] + 24).to_bytes(2, "big")
            a = int(seqs[i]).to_bytes(8, "big") + bytes([int(types[i]), 3, 3]) + int(lens[i]).to_bytes(2, "big")
            aad[13 * i:13 * i + 13] = np.frombuffer(a, np.uint8)
        headers.append(hdr)
    frecs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    frecs["in_off"], frecs["out_off"], frecs["len"] = text_off, wire_off + head, text
    frecs["aad_off"], frecs["aad_len"], frecs["seq"], frecs["key_idx"] = aad_len * np.arange(n), aad_len, nonces, key_idx
    wire = rand_bytes(rng, int(wire_off[-1] + text[-1] + head + 16) + TAIL)
    ref.run_batch(True, keys, ivs, key_size, frecs, inner, aad, wire, nthreads=8)
    for i in range(n):
        o = int(wire_off[i])
        wire[o:o + 5] = np.frombuffer(headers[i], np.uint8)
        if version == 12:
            wire[o + 5:o + 13] = np.frombuffer(int(nonces[i]).to_bytes(8, "big"), np.uint8)
    for i in hdr_fail:
        if version == 12:
            wire[wire_off[i] + 1] = 2  # (the AAD takes 3, 3 as constants: the tag still verifies)
    at, bit = int(rng.integers(0, int(text[ct_v]))), 1 << int(rng.integers(0, 8))
    wire[wire_off[ct_v] + head + at] ^= bit
    wire[wire_off[tag_v] + head + text[tag_v] + int(rng.integers(0, 16))] ^= 0x20
    wire[wire_off[hdr_v]] ^= 0x04

    base = 3
    orecs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    orecs["in_off"], orecs["out_off"], orecs["len"], orecs["seq"], orecs["key_idx"] = wire_off, base + text_off, text, seqs, key_idx
    pfill = rand_bytes(rng, base + total + TAIL)
    want = pfill.copy()
    want[base:base + total] = inner
    want[base + text_off[ct_v] + at] ^= bit  # (CTR: the flipped ciphertext bit; the plaintext is written all the same)
    # a refused header leaves the range as it was, whether the tag verifies or not (TLS 1.3: the flipped outer type too;
    # TLS 1.2 takes any type, so its flipped type only fails the tag and the plaintext is written)
    for i in hdr_fail + ([hdr_v] if version == 13 else []):
        o = base + int(text_off[i])
        want[o:o + int(text[i])] = pfill[o:o + int(text[i])]
    res = np.zeros(n, dtype=pa.TLS_RESULT_DTYPE)
    res["plain_len"], res["content_type"] = lens, types
    if version == 13:
        unexpected = (lens == 0) & (types != 23)
        res["status"][unexpected] = pa.TLS_UNEXPECTED_MESSAGE
        for v in (ct_v, tag_v, hdr_v):
            res[v] = (0, 0, pa.TLS_BAD_MAC, 0)
        for v in hdr_fail:
            res[v] = (0, 0, pa.TLS_BAD_HEADER, 0)
    else:
        for v in (ct_v, tag_v, hdr_v):
            res[v] = (0, int(wire[wire_off[v]]), pa.TLS_BAD_MAC, 0)
        for v in hdr_fail:
            res[v] = (0, int(types[v]), pa.TLS_BAD_HEADER, 0)
    return keys, ivs, key_size, orecs, wire, pfill, want, res, base + text_off, text


def _framed_open(ref, version, header_failures):
    rng = np.random.default_rng(5900 + version + 100 * header_failures)
    n = 2500
    keys, ivs, key_size, orecs, wire, pfill, want, res, offs, sizes = _framed_case(ref, rng, version, n, header_failures)
    ks = pa.Keyset(keys, ivs, key_size)
    rfill = rand_bytes(rng, 8 * n + TAIL)
    d_recs, d_wire, d_out = dev(orecs), dev(wire), dev(pfill)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    opener = pa.open_tls_records if version == 13 else pa.open_tls12_records
    pa.debug_counters(reset=True)
    opener(ks, d_recs.data_ptr(), n, d_wire.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(_serial_only, "open")
    ok, got_res = d_ok.cpu().numpy(), d_res.cpu().numpy()
    want_res = rfill.copy()
    want_res[:8 * n] = res.view(np.uint8)
    assert_arena(got_res, want_res, 8 * np.arange(n), np.full(n, 8), "TLS results")
    assert np.array_equal(ok[:n], (res["status"] == pa.TLS_OK).astype(np.uint8))
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"
    assert np.array_equal(d_wire.cpu().numpy(), wire), "the open wrote to the wire arena"
    assert_arena(d_out.cpu().numpy(), want, offs, sizes, "opened plaintext arena")
    ks.free()


@pytest.mark.parametrize("version", [13, 12], ids=["tls13", "tls12"])
def test_framed_open(ref, version):
    """open_tls_records / open_tls12_records on 2,500 wire records of 0..16,383 payload bytes packed back to back, the
    plaintexts byte-adjacent at stride text in a random-filled arena that is compared whole; three records fail their
    tag (a ciphertext, a tag and a header bit): their plaintext is written all the same, except under a header that the
    record layer refuses (TLS 1.3's flipped outer type), which leaves the range filled; ok bytes and results exact,
    with filled tails."""
    _framed_open(ref, version, header_failures=False)


@pytest.mark.parametrize("version", [13, 12], ids=["tls13", "tls12"])
def test_framed_open_header_failure_keeps_the_fill(ref, version):
    """The same batch with two records whose tag verifies under a header that the record layer refuses (TLS 1.3: outer
    type 22; TLS 1.2: version byte 2): status BAD_HEADER, ok = 0, and their plaintext ranges keep the fill.
    The open authenticates such a record without storing it (segment.h), since a failed tag is reported ahead of a bad
    header."""
    _framed_open(ref, version, header_failures=True)


# ------------------------------------------------------------------------------------------------ ChaCha20-Poly1305


@LAYOUTS
@pytest.mark.parametrize("width", pa.CHACHA_GROUP_WIDTHS)
def test_chacha20_poly1305(width, in_place):
    """The ChaCha20-Poly1305 kernels at both forced group widths: the 311 lengths of test_gpu_chacha.test_every_length,
    byte-adjacent, against OpenSSL; every record opens back into a filled arena (in place: over the sealed arena)."""
    rng = np.random.default_rng(6000 + width + in_place)
    widest = max(pa.CHACHA_GROUP_WIDTHS)
    lens = list(range(301)) + [widest * 64 - 1, widest * 64, widest * 64 + 1, 1200, 4095, 4096, 4097, 16384, 16385, 16640]
    c = packed_case(rng, lens, [i % 41 for i in range(len(lens))], 32, 2, in_place)
    n, b = c.n, c.b
    keys = [c.keys[32 * k:32 * k + 32].tobytes() for k in range(2)]
    ivs = [c.ivs[12 * k:12 * k + 12].tobytes() for k in range(2)]
    want = c.fill.copy()
    R.seal_records(keys, ivs, b.seal, c.src, c.aad, want)
    ks = pa.ChaChaKeyset(c.keys, c.ivs)
    try:
        pa.chacha_debug_force(width, 0)
        pa.chacha_debug_counters(reset=True)
        d_seal, d_aad, d_in = dev(b.seal), dev(c.aad), dev(c.src)
        d_out = d_in if in_place else dev(c.fill)
        pa.chacha_seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert_arena(d_out.cpu().numpy(), want, c.sealed_offs, c.sealed_sizes, "sealed arena against OpenSSL's")
        pfill = want if in_place else rand_bytes(rng, b.pt_bytes)
        back = pfill.copy()
        for r in b.seal:
            p, o, ln = int(r["in_off"]), int(r["out_off"]), int(r["len"])
            back[p:p + ln] = c.src[p:p + ln]  # (in place p == o: the plaintext back over its ciphertext, the tag kept)
        d_open, d_sealed = dev(b.open), dev(want)
        d_back = d_sealed if in_place else dev(pfill)
        d_ok = dev(np.full(n + TAIL, OK_FILL, np.uint8))
        pa.chacha_open_batch(ks, d_open.data_ptr(), n, d_sealed.data_ptr(), d_aad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(),
                             _stream())
        torch.cuda.synchronize()
        ran = pa.chacha_debug_counters(reset=True)
        assert ran[width] == 2 and sum(ran.values()) == 2, ran  # one seal, one open, both at the forced width
        ok = d_ok.cpu().numpy()
        assert (ok[:n] == 1).all() and (ok[n:] == OK_FILL).all(), ok
        assert_arena(d_back.cpu().numpy(), back, c.plain_offs, c.plain_sizes, "opened arena")
    finally:
        pa.chacha_debug_force(0, 0)
        ks.free()
