"""ChaCha20-Poly1305 on the GPU: every comparison is byte-exact against OpenSSL (chacha_ref (a)), a subset of each test
also against the plain-Python restatement (b). Output arenas start as 0xAA so that stray writes show: whole arenas are
compared, not just the records' bytes."""
import numpy as np
import pytest
import torch

import chacha_ref as R
import picotls_amd as pa
from gpu_util import dev, empty
from picotls_amd.records import HP_DTYPE, RECORD_DTYPE, TLS_BAD_HEADER, TLS_BAD_MAC, TLS_OK, TLS_RESULT_DTYPE, TLS_UNEXPECTED_MESSAGE, RecordBatch

pytestmark = pytest.mark.gpu

FILL = 0xAA
WIDTHS = pa.CHACHA_GROUP_WIDTHS
WIDEST = max(WIDTHS)
MAX_RECORD_LEN = 1 << 30


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _keys(rng, n):
    return [rng.bytes(32) for _ in range(n)], [rng.bytes(12) for _ in range(n)]


def _keyset(keys, ivs):
    return pa.ChaChaKeyset(b"".join(keys), b"".join(ivs))


def gpu_seal(ks, recs, pt, aad, out):
    """Seals into a copy of the arena ``out`` on the device and returns it."""
    d_recs, d_pt, d_aad, d_out = dev(recs), dev(pt if pt.size else np.zeros(1, np.uint8)), dev(aad if aad.size else np.zeros(1, np.uint8)), dev(out)
    pa.chacha_seal_batch(ks, d_recs.data_ptr(), len(recs), d_pt.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def gpu_open(ks, recs, sealed, aad, out):
    d_recs, d_in, d_aad, d_out = dev(recs), dev(sealed), dev(aad if aad.size else np.zeros(1, np.uint8)), dev(out)
    d_ok = empty(len(recs), FILL)
    pa.chacha_open_batch(ks, d_recs.data_ptr(), len(recs), d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(),
                         _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_ok[:len(recs)].cpu().numpy()


def filled(nbytes):
    return np.full(max(nbytes, 1), FILL, np.uint8)


def expect_back(recs, pt, nbytes):
    """the plaintext arena an open of every record of ``recs`` (the seal descriptors) leaves, 0xAA elsewhere"""
    out = filled(nbytes)
    for r in recs:
        i, n = int(r["in_off"]), int(r["len"])
        out[i:i + n] = pt[i:i + n]
    return out


def check_batch(ks, keys, ivs, b, rng, py_subset=()):
    """seal == (a) over the whole 0xAA arena, open restores the plaintext with ok all 1; records py_subset also == (b)"""
    pt = np.frombuffer(rng.bytes(max(b.pt_bytes, 1)), np.uint8)
    aad = np.frombuffer(rng.bytes(max(b.aad_bytes, 1)), np.uint8)
    want = filled(b.sealed_bytes)
    R.seal_records(keys, ivs, b.seal, pt, aad, want)
    got = gpu_seal(ks, b.seal, pt, aad, filled(b.sealed_bytes))
    bad = [i for i, r in enumerate(b.seal) if not np.array_equal(got[int(r["out_off"]):int(r["out_off"]) + int(r["len"]) + 16],
                                                                 want[int(r["out_off"]):int(r["out_off"]) + int(r["len"]) + 16])]
    assert not bad, f"sealed records differ from OpenSSL: {[(i, int(b.seal[i]['len']), int(b.seal[i]['aad_len'])) for i in bad[:8]]}"
    assert np.array_equal(got, want), "bytes outside the records were written"
    for i in py_subset:
        r = b.seal[i]
        k, o, n, a, an = int(r["key_idx"]), int(r["out_off"]), int(r["len"]), int(r["aad_off"]), int(r["aad_len"])
        py = R.py_seal(keys[k], R.nonce_for(ivs[k], int(r["seq"])), pt[int(r["in_off"]):int(r["in_off"]) + n].tobytes(),
                       aad[a:a + an].tobytes())
        assert got[o:o + n + 16].tobytes() == py, f"record {i} (len {n}) differs from the Python reference"
    back, ok = gpu_open(ks, b.open, got, aad, filled(b.pt_bytes))
    assert ok.tolist() == [1] * b.n, f"open rejected records {np.flatnonzero(ok != 1)[:8]}"
    assert np.array_equal(back, expect_back(b.seal, pt, b.pt_bytes)), "open did not restore the plaintext"
    return pt, aad, got


@pytest.fixture
def forced():
    """debug_force for the test, back to automatic after it"""
    yield pa.chacha_debug_force
    pa.chacha_debug_force(0, 0)


# ---- 1. every length (and 12: the forced width is the one that ran)


@pytest.mark.parametrize("width", WIDTHS)
def test_every_length(width, forced):
    rng = np.random.default_rng(100 + width)
    lens = list(range(301)) + [WIDEST * 64 - 1, WIDEST * 64, WIDEST * 64 + 1, 1200, 4095, 4096, 4097, 16384, 16385, 16640]
    aads = [i % 41 for i in range(len(lens))]
    b = RecordBatch.build(lens, aads, seqs=rng.integers(0, 2**62, len(lens), dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    forced(width, 0)
    pa.chacha_debug_counters(reset=True)
    subset = list(range(0, 301, 5)) + [301, 302, 304]  # 64 records: every fifth length, G x 64 - 1, G x 64 and 1200
    check_batch(ks, keys, ivs, b, rng, py_subset=subset)
    ran = pa.chacha_debug_counters(reset=True)
    assert ran[width] == 2 and sum(ran.values()) == 2, ran  # one seal, one open, both at the forced width
    ks.free()


# ---- 2. AAD edges


@pytest.mark.parametrize("width", WIDTHS)
def test_aad_edges(width, forced):
    rng = np.random.default_rng(200 + width)
    cases = [(n, a) for a in (0, 1, 5, 13, 15, 16, 17, 31, 32, 33, 40, 300) for n in (0, 1, 64, 1200)]
    b = RecordBatch.build([c[0] for c in cases], [c[1] for c in cases], seqs=rng.integers(0, 2**62, len(cases), dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    forced(width, 0)
    check_batch(ks, keys, ivs, b, rng, py_subset=range(len(cases)))
    ks.free()


# ---- 3. odd offsets and in place


def _offset_batch():
    """records of lengths {1, 63, 64, 65, 1200} whose in, out and aad offsets take every residue mod 16"""
    recs = np.zeros(5 * 16, RECORD_DTYPE)
    pos = {"in": 0, "out": 0, "aad": 0}

    def place(kind, res, size):
        at = (pos[kind] + 15) // 16 * 16 + 16 + res  # at least 16 untouched bytes between records
        pos[kind] = at + size
        return at

    i = 0
    for n in (1, 63, 64, 65, 1200):
        for k in range(16):
            r = recs[i]
            r["len"], r["aad_len"], r["seq"] = n, 13, 1000 + i
            r["in_off"] = place("in", k, n)
            r["out_off"] = place("out", (k + 5) % 16, n + 16)
            r["aad_off"] = place("aad", (k + 11) % 16, 13)
            i += 1
    return recs, pos["in"] + 32, pos["out"] + 32, pos["aad"] + 32


@pytest.mark.parametrize("width", WIDTHS)
def test_odd_offsets(width, forced):
    rng = np.random.default_rng(300 + width)
    recs, in_bytes, out_bytes, aad_bytes = _offset_batch()
    assert {int(r["in_off"]) % 16 for r in recs} == set(range(16)) == {int(r["out_off"]) % 16 for r in recs}
    assert {int(r["aad_off"]) % 16 for r in recs} == set(range(16))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    forced(width, 0)
    pt = np.frombuffer(rng.bytes(in_bytes), np.uint8)
    aad = np.frombuffer(rng.bytes(aad_bytes), np.uint8)
    want = filled(out_bytes)
    R.seal_records(keys, ivs, recs, pt, aad, want)
    got = gpu_seal(ks, recs, pt, aad, filled(out_bytes))
    assert np.array_equal(got, want)
    for r in recs[::8]:
        o, n, a = int(r["out_off"]), int(r["len"]), int(r["aad_off"])
        assert got[o:o + n + 16].tobytes() == R.py_seal(keys[0], R.nonce_for(ivs[0], int(r["seq"])),
                                                        pt[int(r["in_off"]):int(r["in_off"]) + n].tobytes(), aad[a:a + 13].tobytes())
    opn = recs.copy()
    opn["in_off"], opn["out_off"] = recs["out_off"], recs["in_off"]
    back, ok = gpu_open(ks, opn, got, aad, filled(in_bytes))
    assert ok.tolist() == [1] * len(recs)
    assert np.array_equal(back, expect_back(recs, pt, in_bytes))
    ks.free()


@pytest.mark.parametrize("width", WIDTHS)
def test_in_place(width, forced):
    rng = np.random.default_rng(350 + width)
    recs, _, out_bytes, aad_bytes = _offset_batch()
    recs["in_off"] = recs["out_off"]  # one arena, out_off == in_off, room for the tag behind every record
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    forced(width, 0)
    aad = np.frombuffer(rng.bytes(aad_bytes), np.uint8)
    arena = filled(out_bytes)
    for r in recs:
        o, n = int(r["in_off"]), int(r["len"])
        arena[o:o + n] = np.frombuffer(rng.bytes(n), np.uint8)
    want = arena.copy()
    R.seal_records(keys, ivs, recs, arena, aad, want)
    d_recs, d_aad, d_arena = dev(recs), dev(aad), dev(arena)
    pa.chacha_seal_batch(ks, d_recs.data_ptr(), len(recs), d_arena.data_ptr(), d_aad.data_ptr(), d_arena.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), want), "in-place seal"
    d_ok = empty(len(recs), FILL)
    pa.chacha_open_batch(ks, d_recs.data_ptr(), len(recs), d_arena.data_ptr(), d_aad.data_ptr(), d_arena.data_ptr(),
                         d_ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert d_ok[:len(recs)].cpu().numpy().tolist() == [1] * len(recs)
    restored = want.copy()  # the plaintext back where it was, tags and the bytes between records as the seal left them
    for r in recs:
        o, n = int(r["in_off"]), int(r["len"])
        restored[o:o + n] = arena[o:o + n]
    assert np.array_equal(d_arena.cpu().numpy(), restored), "in-place open"
    ks.free()


# ---- 4. many keys, then a rekey of some


def test_many_keys_and_update():
    rng = np.random.default_rng(400)
    nk = 2048
    keys, ivs = _keys(rng, nk)
    ks = _keyset(keys, ivs)
    assert ks.n == nk
    order = rng.permutation(nk).astype(np.uint32)
    b = RecordBatch.build([1200] * nk, 13, seqs=rng.integers(0, 2**62, nk, dtype=np.uint64), key_idx=order)
    check_batch(ks, keys, ivs, b, rng, py_subset=range(0, nk, 64))
    idx = rng.choice(nk, 100, replace=False).astype(np.uint32)
    new_keys, new_ivs = _keys(rng, 100)
    ks.update(idx, b"".join(new_keys), b"".join(new_ivs))
    for i, k, v in zip(idx, new_keys, new_ivs):
        keys[int(i)], ivs[int(i)] = k, v
        assert ks.get_iv(int(i)) == v
    check_batch(ks, keys, ivs, b, rng, py_subset=[int(np.flatnonzero(order == idx[0])[0])])
    with pytest.raises(pa.EngineError):
        ks.update(np.array([nk], np.uint32), bytes(32), bytes(12))
    ks.free()


# ---- 5. the claim loop


def test_claim_loop(forced):
    rng = np.random.default_rng(500)
    n = 3000
    b = RecordBatch.build([64] * n, 5, seqs=np.arange(n, dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    forced(min(WIDTHS), 2)  # 2 workgroups of 64 groups each for 3,000 records: each claims a dozen runs of records
    pa.chacha_debug_counters(reset=True)
    check_batch(ks, keys, ivs, b, rng, py_subset=range(0, n, 100))
    # a second pair of launches on the same stream finds the claim counters cleared by the first
    check_batch(ks, keys, ivs, b, rng)
    assert pa.chacha_debug_counters(reset=True)[min(WIDTHS)] == 4
    ks.free()


# ---- 6. tampering


def test_tampering():
    rng = np.random.default_rng(600)
    lens = [int(x) for x in rng.integers(1, 2000, 60)] + [1, 16, 64, 4096]
    b = RecordBatch.build(lens, 13, seqs=rng.integers(0, 2**62, 64, dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    _, aad, sealed = check_batch(ks, keys, ivs, b, rng)
    for kind in ("first", "middle", "last", "tag", "aad", "seq"):
        hit = rng.random(64) < 0.4
        hit[rng.integers(0, 64)] = True
        s, a, recs = sealed.copy(), aad.copy(), b.open.copy()
        for i in np.flatnonzero(hit):
            o, n, bit = int(recs[i]["in_off"]), int(recs[i]["len"]), 1 << int(rng.integers(0, 8))
            if kind == "aad":
                a[int(recs[i]["aad_off"]) + int(rng.integers(0, 13))] ^= bit
            elif kind == "seq":
                recs[i]["seq"] ^= np.uint64(1 << int(rng.integers(0, 62)))
            else:
                s[o + {"first": 0, "middle": n // 2, "last": n - 1, "tag": n + int(rng.integers(0, 16))}[kind]] ^= bit
        _, ok = gpu_open(ks, recs, s, a, filled(b.pt_bytes))
        assert ok.tolist() == [0 if h else 1 for h in hit], kind  # every tampered record rejected, no other
    ks.free()


# ---- 7. rejected descriptors


def test_rejected_descriptors():
    rng = np.random.default_rng(700)
    keys, ivs = _keys(rng, 3)
    ks = _keyset(keys, ivs)
    b = RecordBatch.build([100, 200, 300, 400, 500, 64], 13, seqs=np.arange(6, dtype=np.uint64), key_idx=[0, 1, 2, 0, 1, 2])
    pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
    aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
    good = np.array([True, False, True, True, False, True])
    seal = b.seal.copy()
    seal[1]["len"] = MAX_RECORD_LEN + 1  # beyond the limit
    seal[4]["key_idx"] = 3               # == the keyset size
    want = filled(b.sealed_bytes)
    R.seal_records(keys, ivs, seal[good], pt, aad, want)
    got = gpu_seal(ks, seal, pt, aad, filled(b.sealed_bytes))
    assert np.array_equal(got, want)  # nothing written for the two, the neighbours as OpenSSL
    full = gpu_seal(ks, b.seal, pt, aad, filled(b.sealed_bytes))
    opn = b.open.copy()
    opn[1]["len"] = MAX_RECORD_LEN + 1
    opn[4]["key_idx"] = 3
    back, ok = gpu_open(ks, opn, full, aad, filled(b.pt_bytes))
    assert ok.tolist() == [1, 0, 1, 1, 0, 1]
    want_back = filled(b.pt_bytes)
    for r in b.seal[good]:
        i, n = int(r["in_off"]), int(r["len"])
        want_back[i:i + n] = pt[i:i + n]
    assert np.array_equal(back, want_back)
    ks.free()


# ---- 8. Poly1305 edge cases


def test_poly1305_rfc_vectors():
    for v in R.load_kat()["poly1305"]:
        key, msg = bytes.fromhex(v["r"] + v["s"]), bytes.fromhex(v["msg"])
        assert pa.chacha_debug_poly1305(key, msg) == bytes.fromhex(v["tag"]), v


def test_poly1305_reduction_edges():
    """One-time keys r = 1 and r = 2 (both survive clamping) and blocks chosen so that the accumulator, as an integer
    before the final reduction, is exactly p - 1, p, p + 1 or 2^130 - 1; s = 2^128 - 1 makes the final add carry out.
    Random data never reaches these carries."""
    p = R.P1305
    cases = []
    for target in (p - 1, p, p + 1, (1 << 130) - 1):
        # r = 1: three full blocks (each m + 2^128) that sum to the target
        x = target - 3 * (1 << 128)
        ms = [x // 2, x - x // 2, 0]
        assert all(0 <= m < 1 << 128 for m in ms) and sum(m + (1 << 128) for m in ms) == target
        cases.append((1, b"".join(m.to_bytes(16, "little") for m in ms)))
        # r = 2: one full block, 2 (m + 2^128) = target (the even targets)
        if target % 2 == 0:
            m = target // 2 - (1 << 128)
            assert 0 <= m < 1 << 128
            cases.append((2, m.to_bytes(16, "little")))
    # r = 2 through a wrap: two blocks whose doubled sum passes 2^130 and lands next to p again
    cases.append((2, ((1 << 128) - 1).to_bytes(16, "little") * 2))
    cases.append((2, ((1 << 128) - 3).to_bytes(16, "little") + ((1 << 128) - 1).to_bytes(16, "little")))
    for r, msg in cases:
        for s in (0, (1 << 128) - 1, 5, (1 << 128) - 5):
            key = r.to_bytes(16, "little") + s.to_bytes(16, "little")
            assert pa.chacha_debug_poly1305(key, msg) == R.py_poly1305(key, msg), (r, s, msg.hex())
    rng = np.random.default_rng(800)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 1000):
        key, msg = rng.bytes(32), rng.bytes(n)
        assert pa.chacha_debug_poly1305(key, msg) == R.py_poly1305(key, msg), n


# ---- 9. header protection


def test_header_protection_masks():
    rng = np.random.default_rng(900)
    keys, ivs = _keys(rng, 16)
    ks = _keyset(keys, ivs)
    n = 256
    base = np.frombuffer(rng.bytes(n * 40 + 64), np.uint8)
    hp = np.zeros(n + 2, HP_DTYPE)
    hp["sample_off"][:n] = np.arange(n) * 40 + rng.integers(0, 24, n)  # any byte offset
    hp["key_idx"][:n] = rng.integers(0, 16, n)
    hp["sample_off"][n:], hp["key_idx"][n:] = 8, (16, 0xffffffff)  # out of range: a zero mask
    d_hp, d_base, d_masks = dev(hp), dev(base), empty(16 * (n + 2) + 16, FILL)
    pa.chacha_hp_mask_batch(ks, d_hp.data_ptr(), n + 2, d_base.data_ptr(), d_masks.data_ptr(), _stream())
    torch.cuda.synchronize()
    masks = d_masks.cpu().numpy()
    for i in range(n):
        o = int(hp["sample_off"][i])
        assert masks[16 * i:16 * i + 16].tobytes() == R.ossl_chacha20(keys[int(hp["key_idx"][i])], base[o:o + 16].tobytes(), bytes(16)), i
    assert not masks[16 * n:16 * (n + 2)].any()
    assert (masks[16 * (n + 2):] == FILL).all()
    c = pa.ChaChaCipher(keys[3])
    assert c.mask(base[:16].tobytes()) == R.ossl_chacha20(keys[3], base[:16].tobytes(), bytes(16))
    ks.free()


# ---- 10. TLS 1.3 framing


def test_tls13_framing():
    rng = np.random.default_rng(1000)
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    cases = [(n, t) for n in (0, 1, 1200, 16384) for t in (23, 22)]
    n = len(cases)
    seal = np.zeros(n, RECORD_DTYPE)
    pin = wire = 0
    for r, (ln, t) in zip(seal, cases):
        r["len"], r["flags"], r["in_off"], r["out_off"] = ln, t, pin, wire
        pin += (ln + 15) // 16 * 16 + 16
        wire += (ln + 22 + 15) // 16 * 16 + 16
    seal["seq"] = rng.integers(0, 2**62, n, dtype=np.uint64)
    payload = np.frombuffer(rng.bytes(pin), np.uint8)
    want = filled(wire)
    for r, (ln, t) in zip(seal, cases):
        hdr = bytes([23, 3, 3, (ln + 17) >> 8, (ln + 17) & 0xff])
        inner = payload[int(r["in_off"]):int(r["in_off"]) + ln].tobytes() + bytes([t])
        rec = hdr + R.ossl_seal(keys[0], R.nonce_for(ivs[0], int(r["seq"])), inner, hdr)
        want[int(r["out_off"]):int(r["out_off"]) + ln + 22] = np.frombuffer(rec, np.uint8)
    d_seal, d_pay, d_wire = dev(seal), dev(payload), dev(filled(wire))
    pa.chacha_seal_tls_records(ks, d_seal.data_ptr(), n, d_pay.data_ptr(), d_wire.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = d_wire.cpu().numpy()
    assert np.array_equal(got, want)

    # three more wire records: a bad outer header, a bad MAC, an all-zero inner plaintext
    def wire_record(inner, seq, hdr0=23):
        hdr = bytes([hdr0, 3, 3, (len(inner) + 16) >> 8, (len(inner) + 16) & 0xff])
        return hdr + R.ossl_seal(keys[0], R.nonce_for(ivs[0], seq), inner, hdr)

    extra = [wire_record(b"hello" + bytes([23]), 77, hdr0=22), wire_record(b"hello" + bytes([23]), 78), wire_record(bytes(9), 79)]
    extra[1] = extra[1][:-1] + bytes([extra[1][-1] ^ 1])
    opn = np.zeros(n + 3, RECORD_DTYPE)
    opn[:n] = seal
    opn["in_off"][:n], opn["out_off"][:n], opn["len"][:n] = seal["out_off"], seal["in_off"], seal["len"] + 1
    win, pout = wire, pin
    for j, rec in enumerate(extra):
        opn[n + j]["in_off"], opn[n + j]["out_off"], opn[n + j]["len"], opn[n + j]["seq"] = win, pout, len(rec) - 21, 77 + j
        win += 64
        pout += 32
    all_wire = np.concatenate([got, np.zeros(3 * 64, np.uint8)])
    for j, rec in enumerate(extra):
        all_wire[wire + 64 * j:wire + 64 * j + len(rec)] = np.frombuffer(rec, np.uint8)
    d_opn, d_in, d_out, d_ok = dev(opn), dev(all_wire), dev(filled(pout + 16)), empty(n + 3, FILL)
    d_res = dev(np.zeros(n + 3, TLS_RESULT_DTYPE))
    pa.chacha_open_tls_records(ks, d_opn.data_ptr(), n + 3, d_in.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(),
                               _stream())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(TLS_RESULT_DTYPE)
    ok, out = d_ok[:n + 3].cpu().numpy(), d_out.cpu().numpy()
    for i, (ln, t) in enumerate(cases):
        empty_handshake = ln == 0 and t == 22  # an empty handshake record is an unexpected message (lib/picotls.c:5960-5968)
        assert int(res[i]["status"]) == (TLS_UNEXPECTED_MESSAGE if empty_handshake else TLS_OK), (ln, t)
        assert int(ok[i]) == (0 if empty_handshake else 1)
        assert (int(res[i]["plain_len"]), int(res[i]["content_type"])) == (ln, t)
        o = int(opn[i]["out_off"])
        assert np.array_equal(out[o:o + ln], payload[o:o + ln])
    assert [int(x) for x in res["status"][n:]] == [TLS_BAD_HEADER, TLS_BAD_MAC, TLS_UNEXPECTED_MESSAGE]
    assert ok[n:].tolist() == [0, 0, 0]
    ks.free()


# ---- 11. per-record helpers and the picotls mirror


def test_per_record_context():
    rng = np.random.default_rng(1100)
    key, iv = rng.bytes(32), rng.bytes(12)
    enc = pa.aead_new_direct(pa.chacha20poly1305, True, key, iv)
    dec = pa.AeadContext(pa.chacha20poly1305, False, key, iv)
    assert enc.get_iv() == iv
    for n, an, seq in ((0, 0, 0), (1, 13, 1), (64, 5, 2**40), (1200, 21, 2**62 - 1), (16384, 5, 7), (70000, 300, 8)):
        pt, aad = rng.bytes(n), rng.bytes(an)
        want = R.ossl_seal(key, R.nonce_for(iv, seq), pt, aad)
        got = enc.encrypt(pt, seq, aad)
        assert got == want, n
        if n <= 1200:
            assert got == R.py_seal(key, R.nonce_for(iv, seq), pt, aad)
        cut = [0, n // 3, n // 3, n - n // 4, n]
        assert enc.encrypt_v([pt[a:b] for a, b in zip(cut, cut[1:])], seq, aad) == want
        assert dec.decrypt(want, seq, aad) == pt
        # a failed decrypt returns None and leaves the output buffer as it was
        out = bytearray([FILL]) * (n + 8)
        bad = bytearray(want)
        bad[len(bad) // 2] ^= 0x10
        assert dec.decrypt(bytes(bad), seq, aad, out=out) is None
        assert dec.decrypt(want, seq + 1, aad, out=out) is None
        assert dec.decrypt(want, seq, aad + b"x", out=out) is None
        assert out == bytearray([FILL]) * (n + 8)
        assert dec.decrypt(want, seq, aad, out=out) == pt and out[n:] == bytearray([FILL]) * 8
    assert dec.decrypt(bytes(15), 0) is None
    # set_iv / xor_iv (ptls_aead_xor_iv): the next records use the new static IV
    iv2 = rng.bytes(12)
    enc.set_iv(iv2)
    assert enc.get_iv() == iv2 and enc.ks.get_iv() == iv2
    assert enc.encrypt(b"abc", 5, b"h") == R.ossl_seal(key, R.nonce_for(iv2, 5), b"abc", b"h")
    mask = rng.bytes(12)
    enc.xor_iv(mask)
    iv3 = bytes(a ^ b for a, b in zip(iv2, mask))
    assert enc.encrypt(b"abc", 5, b"h") == R.ossl_seal(key, R.nonce_for(iv3, 5), b"abc", b"h")
    assert dec.decrypt(enc.encrypt(b"abc", 5, b"h"), 5, b"h") is None  # dec still has the first IV
    dec.xor_iv(bytes(a ^ b for a, b in zip(iv, iv3)))
    assert dec.decrypt(enc.encrypt(b"abc", 5, b"h"), 5, b"h") == b"abc"
    enc.free()
    dec.free()


# ---- 12. the width a launch takes on its own


def test_automatic_width():
    rng = np.random.default_rng(1200)
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    pa.chacha_debug_force(0, 0)
    for ln, width in ((1200, min(WIDTHS)), (16384, WIDEST)):
        b = RecordBatch.build([ln] * 40, 13, seqs=np.arange(40, dtype=np.uint64))
        pa.chacha_debug_counters(reset=True)
        check_batch(ks, keys, ivs, b, rng)
        ran = pa.chacha_debug_counters(reset=True)
        assert ran[width] == 2 and sum(ran.values()) == 2, (ln, ran)
    ks.free()


# ---- 13. one keyset on several streams


def test_claim_slots_on_more_streams_than_slots(forced):
    """One stream more than the keyset has claim slots, each with a batch of its own and no host synchronisation between
    the launches of a round: a slot shared by two launches that are not ordered, or a claim counter not back at zero,
    shows as records skipped or sealed twice."""
    rng = np.random.default_rng(1300)
    nstreams, n = 9, 640  # CHACHA_CLAIM_SLOTS + 1
    keys, ivs = _keys(rng, 3)
    ks = _keyset(keys, ivs)
    forced(min(WIDTHS), 4)  # four workgroups of 64 four-lane groups: each claims several runs of a batch from the counter
    pa.chacha_debug_counters(reset=True)
    streams = [torch.cuda.Stream("cuda:0") for _ in range(nstreams)]
    work = []
    for _ in streams:
        b = RecordBatch.build([int(x) for x in rng.integers(0, 601, n)], 13, seqs=rng.integers(0, 2**62, n, dtype=np.uint64),
                              key_idx=rng.integers(0, 3, n).astype(np.uint32))
        pt = np.frombuffer(rng.bytes(max(b.pt_bytes, 1)), np.uint8)
        aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
        want = filled(b.sealed_bytes)
        R.seal_records(keys, ivs, b.seal, pt, aad, want)
        work.append((b, pt, want, dev(b.seal), dev(b.open), dev(pt), dev(aad)))
    torch.cuda.synchronize()  # the inputs are on the device before any side stream reads them
    sealed = None
    for order in (range(nstreams), reversed(range(nstreams))):
        sealed = [dev(filled(w[0].sealed_bytes)) for w in work]
        torch.cuda.synchronize()
        for i in order:
            b, _, _, d_seal, _, d_pt, d_aad = work[i]
            pa.chacha_seal_batch(ks, d_seal.data_ptr(), n, d_pt.data_ptr(), d_aad.data_ptr(), sealed[i].data_ptr(), streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i, w in enumerate(work):
            assert np.array_equal(sealed[i].cpu().numpy(), w[2]), f"stream {i}"
    backs = [dev(filled(w[0].pt_bytes)) for w in work]
    oks = [empty(n, FILL) for _ in work]
    torch.cuda.synchronize()
    for i in range(nstreams):
        b, _, _, _, d_open, _, d_aad = work[i]
        pa.chacha_open_batch(ks, d_open.data_ptr(), n, sealed[i].data_ptr(), d_aad.data_ptr(), backs[i].data_ptr(), oks[i].data_ptr(),
                             streams[i].cuda_stream)
    torch.cuda.synchronize()
    for i, (b, pt, *_) in enumerate(work):
        assert oks[i][:n].cpu().numpy().tolist() == [1] * n, f"stream {i}"
        assert np.array_equal(backs[i].cpu().numpy(), expect_back(b.seal, pt, b.pt_bytes)), f"stream {i}"
    assert pa.chacha_debug_counters(reset=True)[min(WIDTHS)] == 27  # 2 x 9 seals + 9 opens
    ks.free()


def test_free_and_rekey_right_after_launch_are_ordered():
    """The ChaCha20 counterpart of test_free_right_after_launch_is_ordered, at its shape (a batch still running when the
    host call returns): a rekey and a free made right after a launch are ordered after it on the device.

    Before freed entries were kept out of the stream-ordered pool until their clearing had run (free_after_maint), round
    1's launches sealed every record under round 2's key: the next keyset was handed the block while they still ran."""
    rng = np.random.default_rng(1301)
    n = 20000
    b = RecordBatch.build(np.full(n, 4096), 13, seqs=np.arange(n, dtype=np.uint64))
    pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
    aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
    d_recs, d_pt, d_aad = dev(b.seal), dev(pt), dev(aad)
    side = torch.cuda.Stream("cuda:0")
    outs = []
    for _ in range(3):
        (key,), (iv,) = _keys(rng, 1)
        (key2,), (iv2,) = _keys(rng, 1)
        ks = _keyset([key], [iv])
        d_first, d_second = empty(b.sealed_bytes, FILL), empty(b.sealed_bytes, FILL)
        side.wait_stream(torch.cuda.current_stream())  # the inputs and the filled outputs are ready
        pa.chacha_seal_batch(ks, d_recs.data_ptr(), n, d_pt.data_ptr(), d_aad.data_ptr(), d_first.data_ptr(), side.cuda_stream)
        ks.update([0], key2, iv2)  # immediately, with the batch most likely still running
        pa.chacha_seal_batch(ks, d_recs.data_ptr(), n, d_pt.data_ptr(), d_aad.data_ptr(), d_second.data_ptr(), _stream())
        ks.free()
        outs.append(((key, iv, d_first), (key2, iv2, d_second)))
    torch.cuda.synchronize()
    for r, pair in enumerate(outs):
        for which, (key, iv, d_out) in zip(("launch before the rekey", "launch after the rekey"), pair):
            want = filled(b.sealed_bytes)
            R.seal_records([key], [iv], b.seal, pt, aad, want)
            got = d_out.cpu().numpy()
            bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1)) if got.size == want.size and got.size % n == 0 else [-1]
            assert len(bad) == 0, f"round {r}, {which}: {len(bad)} of {n} records differ from OpenSSL, first {bad[:4]}"
