"""A keyset's growing scratch (host/runtime.h Scratch: key grouping, spread pieces, QUIC descriptors) shared between
streams. Every launch on another stream than the scratch's last user waits for that stream's use event, a batch that needs
more regrows the block on its own stream, and a free right after the last launch retires it behind the launches still
running. The launches of a test are queued back to back on their streams with no host synchronisation between them, each
with in and out arenas of its own, and compared once at the end, byte for byte: batches with lib/fusion.c (the `ref`
fixture of the neighbouring tests), packets with tests/quic_aes_ref.py through tests/quic_util.py."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import picotls_amd as pa  # noqa: E402
import quic_aes_ref as Q  # noqa: E402
import quic_util as U  # noqa: E402
from oracle import FusionRef  # noqa: E402
from picotls_amd.records import QUIC_RESULT_DTYPE, RecordBatch  # noqa: E402
from gpu_util import dev, empty  # noqa: E402

pytestmark = pytest.mark.gpu

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))


@pytest.fixture(scope="module")
def ref():
    assert torch.cuda.is_available(), "no GPU visible"
    pa.load_library()
    if not HAVE_REF:
        pytest.skip("oracle/_ref/libfusion_ref.so not shipped")
    return FusionRef()


def _streams(n):
    """n side streams, each behind everything queued so far on the current one (uploads, fills)"""
    streams = [torch.cuda.Stream("cuda:0") for _ in range(n)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    return streams


class Batch:
    """Records on the device with their plaintext and AADs; `nkeys` > 1: every record's key drawn at random"""

    def __init__(self, rng, lens, nkeys=1):
        n = len(lens)
        self.n = n
        self.b = RecordBatch.build(np.asarray(lens), 13, seqs=rng.integers(0, 2**62, n, dtype=np.uint64),
                                   key_idx=rng.integers(0, nkeys, n) if nkeys > 1 else None)
        self.pt = np.frombuffer(rng.bytes(self.b.pt_bytes), np.uint8)
        self.aad = np.frombuffer(rng.bytes(self.b.aad_bytes), np.uint8)
        self.d_seal, self.d_open, self.d_pt, self.d_aad = dev(self.b.seal), dev(self.b.open), dev(self.pt), dev(self.aad)

    def sealed_by_ref(self, ref, keys, ivs, key_size):
        want = np.zeros(self.b.sealed_bytes, np.uint8)
        ref.run_batch(True, keys, ivs, key_size, self.b.seal, self.pt, self.aad, want, nthreads=8)
        return want

    def seal(self, ks, stream):
        """queues the seal on `stream`; its output, zero outside the records"""
        d_out = empty(self.b.sealed_bytes)
        stream.wait_stream(torch.cuda.current_stream())  # (the fill)
        pa.seal_batch(ks, self.d_seal.data_ptr(), self.n, self.d_pt.data_ptr(), self.d_aad.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
        return d_out


def _same_records(got, want, b, what):
    if not np.array_equal(got, want):
        bad = [i for i, r in enumerate(b.seal) if not np.array_equal(got[int(r["out_off"]):int(r["out_off"]) + int(r["len"]) + 16],
                                                                      want[int(r["out_off"]):int(r["out_off"]) + int(r["len"]) + 16])]
        assert False, f"{what}: {len(bad)} of {len(b.seal)} records differ from the reference, first {bad[:8]}"


def _keys(rng, nkeys, key_size):
    return np.frombuffer(rng.bytes(nkeys * key_size), np.uint8), np.frombuffer(rng.bytes(nkeys * 12), np.uint8)


def test_grouping_scratch_regrown_on_other_streams(ref):
    """Ungrouped batches of a 64-key keyset on three streams, sized so that each growth of the grouping scratch happens on
    another stream than its last user's (the fourth adds the balance tiles and bounds), and the two after the largest
    reuse it from a stream that did not allocate it. Then fusion's records of every batch, three of them tampered, are
    opened on the stream after the one that sealed them."""
    rng = np.random.default_rng(9100)
    nkeys = 64
    keys, ivs = _keys(rng, nkeys, 16)
    sizes = [(600, 400), (3000, 400), (9000, 400), (131072, 64), (600, 400), (3000, 400)]
    batches = [Batch(rng, rng.integers(16, hi + 1, n), nkeys) for n, hi in sizes]
    wants = [x.sealed_by_ref(ref, keys, ivs, 16) for x in batches]
    # what the opens read: fusion's records, three per batch tampered (ciphertext, tag, AAD)
    opens = []
    for x, want in zip(batches, wants):
        bad, badaad = want.copy(), x.aad.copy()
        victims = rng.choice(x.n, 3, replace=False)
        for t, v in enumerate(victims):
            r = x.b.open[v]
            if t == 0:
                bad[int(r["in_off"]) + int(rng.integers(0, int(r["len"])))] ^= 1 << int(rng.integers(0, 8))
            elif t == 1:
                bad[int(r["in_off"]) + int(r["len"]) + int(rng.integers(0, 16))] ^= 0x20
            else:
                badaad[int(r["aad_off"]) + int(rng.integers(0, 13))] ^= 2
        expect_ok = np.ones(x.n, np.uint8)
        expect_ok[victims] = 0
        ref_back = np.zeros(x.b.pt_bytes, np.uint8)
        ref.run_batch(False, keys, ivs, 16, x.b.open, bad, badaad, ref_back, ok=np.zeros(x.n, np.uint8), nthreads=8)
        opens.append((dev(bad), dev(badaad), empty(x.b.pt_bytes), empty(x.n, 0xAA), expect_ok, ref_back))
    ks = pa.Keyset(keys, ivs, 16)
    streams = _streams(3)
    sealed = [x.seal(ks, streams[i % 3]) for i, x in enumerate(batches)]
    for i, (x, (d_bad, d_badaad, d_back, d_ok, _, _)) in enumerate(zip(batches, opens)):
        pa.open_batch(ks, x.d_open.data_ptr(), x.n, d_bad.data_ptr(), d_badaad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(),
                      streams[(i + 1) % 3].cuda_stream)
    torch.cuda.synchronize()
    for i, (x, d_out, want, (_, _, d_back, d_ok, expect_ok, ref_back)) in enumerate(zip(batches, sealed, wants, opens)):
        _same_records(d_out.cpu().numpy(), want, x.b, f"seal {i} ({x.n} records)")
        assert np.array_equal(d_ok.cpu().numpy()[:x.n], expect_ok), f"open {i}: ok differs at {np.flatnonzero(d_ok.cpu().numpy()[:x.n] != expect_ok)[:8]}"
        assert np.array_equal(d_back.cpu().numpy(), ref_back), f"open {i} ({x.n} records)"
    ks.free()


def _spread_batches(rng):
    """(3 records: 1 MiB, 600 KiB, 100 B), (40 records, one of 512 KiB: a larger spread scratch)"""
    lens2 = rng.integers(64, 2001, 40)
    lens2[17] = 512 << 10
    return Batch(rng, [1 << 20, 600 << 10, 100]), Batch(rng, lens2)


def test_spread_scratch_regrown_on_another_stream(ref):
    rng = np.random.default_rng(9200)
    keys, ivs = _keys(rng, 1, 32)
    b1, b2 = _spread_batches(rng)
    want1, want2 = b1.sealed_by_ref(ref, keys, ivs, 32), b2.sealed_by_ref(ref, keys, ivs, 32)
    ks = pa.Keyset(keys, ivs, 32)
    pa.debug_counters(reset=True)
    A, B = _streams(2)
    outs = [b1.seal(ks, A), b2.seal(ks, B), b1.seal(ks, A), b2.seal(ks, A)]
    c = pa.debug_counters(reset=True)  # (waits for the device: the one synchronisation)
    assert c["launches"]["spread"] == 4, c
    for i, (x, d_out, want) in enumerate(zip((b1, b2, b1, b2), outs, (want1, want2, want1, want2))):
        _same_records(d_out.cpu().numpy(), want, x.b, f"spread launch {i}")
    ks.free()


def test_quic_descriptor_scratch_regrown_on_another_stream():
    """50 packets on A, then 5,000 on B (the descriptors regrown behind A's batch), then 50 on B; the opens of the three
    reference batches on the other stream each"""
    rng = np.random.default_rng(9300)
    suite = U.Suite(keyset=pa.Keyset, key_size=16, hp_size=16, alt_hp_size=32, seal=pa.seal_quic_packets, open=pa.open_quic_packets,
                    ref=Q, second="oracle", seed=9300)
    K = U.Keys.make(suite, rng, 8)
    jobs = []
    for n in (50, 5000, 50):
        pkts = [U.make_pkt(K, rng, int(rng.integers(0, 8)), int(rng.integers(0, 2**62)), i % 4 + 1, 8, int(rng.integers(20, 1201)),
                           long=i % 9 == 4, phase=i & 1) for i in range(n)]
        clear = [p.header + p.payload for p in pkts]
        in_offs, in_size = U.place([len(c) for c in clear])
        out_offs, out_size = U.place([len(p.packet) for p in pkts])
        back_offs, back_size = U.place([len(c) for c in clear])
        arena_in, want, want_back = U.filled(in_size), U.filled(out_size), U.filled(back_size)
        for c, p, i, o, b in zip(clear, pkts, in_offs, out_offs, back_offs):
            U.put(arena_in, i, c), U.put(want, o, p.packet), U.put(want_back, b, c)
        jobs.append(dict(n=n, want=want, want_back=want_back, want_res=U.want_results(pkts),
                         d_seal=dev(U.seal_recs(pkts, in_offs, out_offs)), d_in=dev(arena_in), d_out=dev(U.filled(out_size)),
                         d_open=dev(U.open_recs(pkts, out_offs, back_offs)), d_pkts=dev(want), d_back=dev(U.filled(back_size)),
                         d_ok=empty(n, U.FILL), d_res=empty(16 * n, U.FILL)))
    ks, hp_ks = K.keysets()
    A, B = _streams(2)
    for j, st in zip(jobs, (A, B, B)):
        pa.seal_quic_packets(ks, hp_ks, j["d_seal"].data_ptr(), j["n"], j["d_in"].data_ptr(), j["d_out"].data_ptr(), st.cuda_stream)
    for j, st in zip(jobs, (B, A, A)):
        pa.open_quic_packets(ks, hp_ks, j["d_open"].data_ptr(), j["n"], j["d_pkts"].data_ptr(), j["d_back"].data_ptr(), j["d_ok"].data_ptr(),
                             j["d_res"].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        assert np.array_equal(j["d_out"].cpu().numpy(), j["want"]), f"seal {i} ({j['n']} packets)"
        assert j["d_ok"].cpu().numpy().tolist() == [1] * j["n"], f"open {i}"
        assert np.array_equal(j["d_back"].cpu().numpy(), j["want_back"]), f"open {i} ({j['n']} packets)"
        assert np.array_equal(j["d_res"].cpu().numpy().view(QUIC_RESULT_DTYPE), j["want_res"]), f"results {i}"
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("kind", ["grouping", "spread"])
def test_free_right_after_a_scratch_launch_and_reuse(ref, kind):
    """A keyset uses its scratch on A and then on B (B waits for A and regrows nothing) and is freed at once; the next
    keyset, made immediately, allocates its scratch on A while those launches most likely still run. Three rounds, as
    the ChaCha20 free-and-rekey test; every output of both keysets is the reference's."""
    rng = np.random.default_rng(9400 + len(kind))
    if kind == "grouping":
        nkeys, key_size = 64, 16
        x, y = (Batch(rng, rng.integers(16, 401, 9000), nkeys) for _ in range(2))
    else:
        nkeys, key_size = 1, 32
        x = y = _spread_batches(rng)[0]
    A, B = _streams(2)
    runs = []
    for _ in range(3):
        k1, k2 = _keys(rng, nkeys, key_size), _keys(rng, nkeys, key_size)
        ks = pa.Keyset(*k1, key_size)
        first, second = x.seal(ks, A), y.seal(ks, B)
        ks.free()  # immediately, with both batches most likely still running
        ks2 = pa.Keyset(*k2, key_size)
        third = x.seal(ks2, A)
        ks2.free()
        runs.append(((x, k1, first), (y, k1, second), (x, k2, third)))
    torch.cuda.synchronize()
    for rnd, launches in enumerate(runs):
        for which, (batch, (keys, ivs), d_out) in zip(("keyset 1 on A", "keyset 1 on B", "keyset 2 on A"), launches):
            _same_records(d_out.cpu().numpy(), batch.sealed_by_ref(ref, keys, ivs, key_size), batch.b, f"round {rnd}, {which}")
