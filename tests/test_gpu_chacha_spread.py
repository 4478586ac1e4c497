"""ChaCha20-Poly1305 spread launches on the GPU: small unframed batches and per-record calls whose long records are cut
into pieces for groups all over the device. Every comparison is byte-exact against OpenSSL (chacha_ref (a)), a subset
also against the plain-Python restatement (b); whole 0xAA-filled arenas are compared, so stray writes show."""
import numpy as np
import pytest
import torch

import chacha_ref as R
import picotls_amd as pa
from gpu_util import dev, empty
from picotls_amd.records import RecordBatch
from test_chacha_spread_model import EDGE_AADS, EDGE_LENS, EDGE_PARAMS
from test_gpu_chacha import FILL, MAX_RECORD_LEN, WIDEST, _keys, _keyset, _stream, check_batch, expect_back, filled, gpu_open, gpu_seal

pytestmark = pytest.mark.gpu

CLAIM_SLOTS = 8  # CHACHA_CLAIM_SLOTS


@pytest.fixture
def hooks():
    """the spread and force hooks for the test, back to automatic after it"""
    yield pa.chacha_debug_spread
    pa.chacha_debug_spread(0, 0, False)
    pa.chacha_debug_force(0, 0)


def _plan_counts(lens, params):
    plan = pa.chacha_spread_plan(lens, params)
    return sum(len(p) for p in plan), sum(1 for p in plan if p)


def _auto(kind):
    p = pa.chacha_debug_spread_params()
    return {"min_len": p[kind], "piece": p["piece"], "max_pieces": p["max_pieces"]}


# ---- 1. piece edges


@pytest.mark.parametrize("grid_cap", (1, 2, 0))
def test_piece_edges(grid_cap, hooks):
    rng = np.random.default_rng(100 + grid_cap)
    lens = EDGE_LENS
    aads = [EDGE_AADS[i % len(EDGE_AADS)] for i in range(len(lens))]
    b = RecordBatch.build(lens, aads, seqs=rng.integers(0, 2**62, len(lens), dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    hooks(EDGE_PARAMS["piece"], EDGE_PARAMS["min_len"], False)
    pa.chacha_debug_force(0, grid_cap)  # 1: one workgroup loops over all pieces and finishes every record itself
    pa.chacha_debug_spread_counters(reset=True)
    check_batch(ks, keys, ivs, b, rng, py_subset=[0, 9, 10, 13, 18, 24, 27, 35, 36, 38])
    got = pa.chacha_debug_spread_counters(reset=True)
    pieces, nlong = _plan_counts(lens, EDGE_PARAMS)
    assert nlong == 26 and pieces == sum(-(-n // 1024) for n in lens if n >= 2048)
    # one seal and one open
    assert got == {"launches": 2, "pieces": 2 * pieces, "finished": 2 * nlong, "whole": 2 * (len(lens) - nlong)}, got
    ks.free()


# ---- 2. many pieces


def test_many_pieces(hooks):
    rng = np.random.default_rng(200)
    # 201 pieces of 1 KiB: more than loose 26-bit limbs sum without a carry, and than one workgroup has groups; 1 MiB + 77
    # at the piece length the rule gives it
    lens = [200 * 1024 + 77, 1200, 1200, (1 << 20) + 77]
    b = RecordBatch.build(lens, [13, 0, 13, 21], seqs=rng.integers(0, 2**62, len(lens), dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    hooks(1024, 0, False)
    params = dict(_auto("min_batch"), piece=1024)
    pieces, nlong = _plan_counts(lens, params)
    assert nlong >= 2 and len(pa.chacha_spread_plan(lens, params)[0]) == 201
    pa.chacha_debug_spread_counters(reset=True)
    check_batch(ks, keys, ivs, b, rng, py_subset=[1])
    got = pa.chacha_debug_spread_counters(reset=True)
    assert got == {"launches": 2, "pieces": 2 * pieces, "finished": 2 * nlong, "whole": 2 * (len(lens) - nlong)}, got
    ks.free()


# ---- 3. a mixed small batch, odd offsets, out of place and in place


def _mixed_lens(rng):
    lens = [0, 13, 1200, 4096, 16384, 70000, 300000] * 5 + [13, 70000]
    return [int(x) for x in rng.permutation(lens)]


def test_mixed_small_batch():
    rng = np.random.default_rng(300)
    lens = _mixed_lens(rng)
    assert len(lens) == 37
    keys, ivs = _keys(rng, 5)
    ks = _keyset(keys, ivs)
    b = RecordBatch.build_offsets(lens, 13, seqs=rng.integers(0, 2**62, 37, dtype=np.uint64), key_idx=rng.integers(0, 5, 37).astype(np.uint32),
                                  in_base=3, out_base=5, aad_base=1)
    assert any(int(r["in_off"]) % 4 for r in b.seal) and any(int(r["out_off"]) % 4 for r in b.seal)
    pa.chacha_debug_spread_counters(reset=True)
    check_batch(ks, keys, ivs, b, rng, py_subset=[i for i, n in enumerate(lens) if n == 1200][:2])
    pieces, nlong = _plan_counts(lens, _auto("min_batch"))
    got = pa.chacha_debug_spread_counters(reset=True)
    assert got == {"launches": 2, "pieces": 2 * pieces, "finished": 2 * nlong, "whole": 2 * (37 - nlong)}, got
    ks.free()


def test_mixed_small_batch_in_place():
    rng = np.random.default_rng(301)
    lens = _mixed_lens(rng)
    keys, ivs = _keys(rng, 5)
    ks = _keyset(keys, ivs)
    b = RecordBatch.build_offsets(lens, 13, seqs=rng.integers(0, 2**62, 37, dtype=np.uint64), key_idx=rng.integers(0, 5, 37).astype(np.uint32),
                                  out_base=7, aad_base=2, in_place=True)
    recs = b.seal
    assert (recs["in_off"] == recs["out_off"]).all() and any(int(r["in_off"]) % 4 for r in recs)
    aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
    arena = filled(b.sealed_bytes)
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
    pa.chacha_open_batch(ks, d_recs.data_ptr(), len(recs), d_arena.data_ptr(), d_aad.data_ptr(), d_arena.data_ptr(), d_ok.data_ptr(),
                         _stream())
    torch.cuda.synchronize()
    assert d_ok[:len(recs)].cpu().numpy().tolist() == [1] * len(recs)
    restored = want.copy()  # the plaintext back where it was, the tags as the seal left them
    for r in recs:
        o, n = int(r["in_off"]), int(r["len"])
        restored[o:o + n] = arena[o:o + n]
    assert np.array_equal(d_arena.cpu().numpy(), restored), "in-place open"
    ks.free()


# ---- 4. tampering


def test_tampering(hooks):
    rng = np.random.default_rng(400)
    lens = [300000, 1200, 70000, 16384, 5000, 20000]
    b = RecordBatch.build(lens, 13, seqs=rng.integers(0, 2**62, 6, dtype=np.uint64))
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    hooks(1024, 2048, False)  # every record but the second is cut
    _, aad, sealed = check_batch(ks, keys, ivs, b, rng)
    # (kind, record): a bit in the first, a middle and the last piece of a long record, a tag bit, an AAD byte, the seq
    for kind, i in (("first", 0), ("middle", 0), ("last", 0), ("first", 2), ("last", 5), ("tag", 3), ("tag", 0), ("aad", 4),
                    ("aad", 1), ("seq", 2)):
        s, a, recs = sealed.copy(), aad.copy(), b.open.copy()
        o, n, bit = int(recs[i]["in_off"]), int(recs[i]["len"]), 1 << int(rng.integers(0, 8))
        if kind == "aad":
            a[int(recs[i]["aad_off"]) + int(rng.integers(0, 13))] ^= bit
        elif kind == "seq":
            recs[i]["seq"] ^= np.uint64(1 << int(rng.integers(0, 62)))
        else:
            s[o + {"first": 5, "middle": n // 2, "last": n - 1, "tag": n + int(rng.integers(0, 16))}[kind]] ^= bit
        _, ok = gpu_open(ks, recs, s, a, filled(b.pt_bytes))
        assert ok.tolist() == [0 if k == i else 1 for k in range(6)], (kind, i)  # that record rejected, no other
    ks.free()


# ---- 5. rejected descriptors among long records


def test_rejected_descriptors(hooks):
    rng = np.random.default_rng(500)
    keys, ivs = _keys(rng, 3)
    ks = _keyset(keys, ivs)
    b = RecordBatch.build([70000, 20000, 1200, 50000, 30000, 64], 13, seqs=np.arange(6, dtype=np.uint64), key_idx=[0, 1, 2, 0, 1, 2])
    pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
    aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
    good = np.array([True, False, True, False, True, True])
    hooks(1024, 2048, False)
    seal = b.seal.copy()
    seal[1]["len"] = MAX_RECORD_LEN + 1  # beyond the limit
    seal[3]["key_idx"] = 3               # == the keyset size
    want = filled(b.sealed_bytes)
    R.seal_records(keys, ivs, seal[good], pt, aad, want)
    pa.chacha_debug_spread_counters(reset=True)
    got = gpu_seal(ks, seal, pt, aad, filled(b.sealed_bytes))
    assert np.array_equal(got, want)  # nothing written for the two, the others as OpenSSL
    ran = pa.chacha_debug_spread_counters(reset=True)
    assert (ran["launches"], ran["finished"], ran["whole"]) == (1, 2, 4), ran  # the rejected ones are whole items
    full = gpu_seal(ks, b.seal, pt, aad, filled(b.sealed_bytes))
    opn = b.open.copy()
    opn[1]["len"] = MAX_RECORD_LEN + 1
    opn[3]["key_idx"] = 3
    back, ok = gpu_open(ks, opn, full, aad, filled(b.pt_bytes))
    assert ok.tolist() == [1, 0, 1, 0, 1, 1]
    assert np.array_equal(back, expect_back(b.seal[good], pt, b.pt_bytes))
    ks.free()


# ---- 6. state between launches: counters and accumulators back at zero, scratch shared in order


def test_state_between_launches(hooks):
    rng = np.random.default_rng(600)
    keys, ivs = _keys(rng, 2)
    ks = _keyset(keys, ivs)
    hooks(1024, 2048, False)
    batches = []
    for lens in ([5000, 1200, 9000, 3000, 2048], [40000, 64, 2049], [0, 7000, 7000, 7001, 1200, 12345, 4096]):
        b = RecordBatch.build(lens, 13, seqs=rng.integers(0, 2**62, len(lens), dtype=np.uint64),
                              key_idx=rng.integers(0, 2, len(lens)).astype(np.uint32))
        pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
        aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
        want = filled(b.sealed_bytes)
        R.seal_records(keys, ivs, b.seal, pt, aad, want)
        batches.append((b, pt, want, dev(b.seal), dev(b.open), dev(pt), dev(aad)))
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream("cuda:0") for _ in range(CLAIM_SLOTS + 1)]
    # first on one stream, then on one more stream than the keyset has claim slots: three launches back to back on each,
    # no host synchronisation anywhere in a round
    for group in (streams[:1], streams[1:]):
        sealed = [[dev(filled(w[0].sealed_bytes)) for w in batches] for _ in group]
        backs = [[dev(filled(w[0].pt_bytes)) for w in batches] for _ in group]
        oks = [[empty(w[0].n, FILL) for w in batches] for _ in group]
        torch.cuda.synchronize()
        for si, st in enumerate(group):
            for bi, (b, _, _, d_seal, _, d_pt, d_aad) in enumerate(batches):
                pa.chacha_seal_batch(ks, d_seal.data_ptr(), b.n, d_pt.data_ptr(), d_aad.data_ptr(), sealed[si][bi].data_ptr(), st.cuda_stream)
            for bi, (b, _, _, _, d_open, _, d_aad) in enumerate(batches):  # (after the seals of the same stream)
                pa.chacha_open_batch(ks, d_open.data_ptr(), b.n, sealed[si][bi].data_ptr(), d_aad.data_ptr(), backs[si][bi].data_ptr(),
                                     oks[si][bi].data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        for si in range(len(group)):
            for bi, (b, pt, want, *_) in enumerate(batches):
                assert np.array_equal(sealed[si][bi].cpu().numpy(), want), (si, bi)
                assert oks[si][bi][:b.n].cpu().numpy().tolist() == [1] * b.n, (si, bi)
                assert np.array_equal(backs[si][bi].cpu().numpy(), expect_back(b.seal, pt, b.pt_bytes)), (si, bi)
    ks.free()


# ---- 7. the per-record path


def test_per_record_path():
    rng = np.random.default_rng(700)
    key, iv = rng.bytes(32), rng.bytes(12)
    enc = pa.aead_new_direct(pa.chacha20poly1305, True, key, iv)
    dec = pa.AeadContext(pa.chacha20poly1305, False, key, iv)
    params = _auto("min_single")
    assert params["min_len"] > 1
    # (the first length stays on one group whatever the compiled minimum is)
    for n, an, seq in ((params["min_len"] - 1, 13, 3), (4096, 5, 1), (16384, 13, 2**40), (16385, 0, 7), (70000, 300, 8),
                       ((1 << 20) + 5, 21, 2**62 - 1)):
        pt, aad = rng.bytes(n), rng.bytes(an)
        want = R.ossl_seal(key, R.nonce_for(iv, seq), pt, aad)
        pieces, nlong = _plan_counts([n], params)
        assert nlong == (1 if n >= params["min_len"] else 0)
        per_call = {"launches": nlong, "pieces": pieces, "finished": nlong, "whole": 0}
        pa.chacha_debug_spread_counters(reset=True)
        assert enc.encrypt(pt, seq, aad) == want, n
        assert pa.chacha_debug_spread_counters(reset=True) == per_call, n
        cut = [0, n // 3, n // 3, n - n // 4, n]
        assert enc.encrypt_v([pt[a:b] for a, b in zip(cut, cut[1:])], seq, aad) == want
        assert dec.decrypt(want, seq, aad) == pt
        assert pa.chacha_debug_spread_counters(reset=True) == {k: 2 * v for k, v in per_call.items()}, n
        # a failed decrypt returns None and leaves the output buffer as it was
        out = bytearray([FILL]) * (n + 8)
        for at in (0, n // 2, n - 1, n + 3):  # the first, a middle and the last piece, the tag
            bad = bytearray(want)
            bad[at] ^= 0x10
            assert dec.decrypt(bytes(bad), seq, aad, out=out) is None
        assert dec.decrypt(want, seq + 1, aad, out=out) is None
        assert dec.decrypt(want, seq, aad + b"x", out=out) is None
        assert out == bytearray([FILL]) * (n + 8)
        assert dec.decrypt(want, seq, aad, out=out) == pt and out[n:] == bytearray([FILL]) * 8
    enc.free()
    dec.free()


# ---- 8. the thresholds a launch applies on its own


def test_automatic_thresholds(hooks):
    rng = np.random.default_rng(800)
    p = pa.chacha_debug_spread_params()
    keys, ivs = _keys(rng, 1)
    ks = _keyset(keys, ivs)
    hooks(0, 0, False)
    pa.chacha_debug_force(0, 0)

    def run(nrecs, ln):
        b = RecordBatch.build([ln] * nrecs, 13, seqs=np.arange(nrecs, dtype=np.uint64))
        pt = np.frombuffer(rng.bytes(b.pt_bytes), np.uint8)
        aad = np.frombuffer(rng.bytes(b.aad_bytes), np.uint8)
        want = filled(b.sealed_bytes)
        R.seal_records(keys, ivs, b.seal, pt, aad, want)
        pa.chacha_debug_spread_counters(reset=True)
        pa.chacha_debug_counters(reset=True)
        assert np.array_equal(gpu_seal(ks, b.seal, pt, aad, filled(b.sealed_bytes)), want), (nrecs, ln)
        return pa.chacha_debug_spread_counters(reset=True), pa.chacha_debug_counters(reset=True)

    per_rec, _ = _plan_counts([p["min_batch"]], _auto("min_batch"))
    assert per_rec >= 1

    def width(ln):  # the sample rule of the kernels: wide groups from a mean length of 4096
        return WIDEST if ln >= 4096 else min(pa.CHACHA_GROUP_WIDTHS)

    spread, ran = run(p["max_recs"], p["min_batch"])
    assert spread == {"launches": 1, "pieces": p["max_recs"] * per_rec, "finished": p["max_recs"], "whole": 0}, spread
    assert sum(ran.values()) == 1, ran  # a spread launch counts itself once
    spread, ran = run(p["max_recs"], p["min_batch"] - 1)
    assert spread == {"launches": 1, "pieces": 0, "finished": 0, "whole": p["max_recs"]}, spread
    assert ran[width(p["min_batch"] - 1)] == 1 and sum(ran.values()) == 1, ran
    spread, ran = run(p["max_recs"] + 1, p["min_batch"])
    assert spread == {"launches": 0, "pieces": 0, "finished": 0, "whole": 0}, spread
    assert ran[width(p["min_batch"])] == 1 and sum(ran.values()) == 1, ran  # as today
    pa.chacha_debug_force(WIDEST, 0)  # a forced width, the spread hook not forcing: the existing kernel
    spread, ran = run(4, 4 * p["min_batch"])
    assert spread["launches"] == 0 and ran[WIDEST] == 1 and sum(ran.values()) == 1, (spread, ran)
    hooks(0, 0, True)
    spread, ran = run(4, 4 * p["min_batch"])
    assert spread["launches"] == 1 and spread["finished"] == 4 and ran[WIDEST] == 1 and sum(ran.values()) == 1, (spread, ran)
    ks.free()


# ---- 9. the powers of r


def test_powers():
    rng = np.random.default_rng(900)
    clamp = 0x0ffffffc0ffffffc0ffffffc0fffffff
    rs = [int.from_bytes(rng.bytes(16), "little") & clamp, 0, 1, ((1 << 124) - 1) & clamp]
    es = [0, 1, 2, 3] + [1 << k for k in range(27)] + [(1 << k) - 1 for k in range(27)] + [int(x) for x in rng.integers(0, 1 << 26, 32)]
    for r in rs:
        for e in es:
            assert pa.chacha_debug_rpow(r.to_bytes(16, "little"), e) == pow(r, e, R.P1305), (hex(r), e)
