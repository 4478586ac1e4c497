"""The TLS-framed batch calls and seal_batch_hp on the record-per-lane kernel (ptls_mi355x_keyset_set_lane_framed on a
keyset whose schedule is PTLS_MI355X_SCHEDULE_RECORD_PER_LANE; gcm_lane_kernel FRAME 1 and 2) against lib/fusion.c.

Every arena starts as random bytes and is compared whole (footprint_util.assert_arena), so a store one byte outside a
record's wire or plaintext range shows. Every launch is checked through the debug counters: the lane kernel ran, no
chunked, spread, W8, lockstep or span kernel did, and it accepted exactly the records the case means it to. No
comparison has a tolerance."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import far_util as F  # noqa: E402
import picotls_amd as pa  # noqa: E402
from footprint_util import TAIL, assert_arena, packed_case, rand_bytes  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import FusionRef  # noqa: E402
from test_gpu_far_offsets import _far_framed, _tls_case  # noqa: E402
from test_gpu_footprint import OK_FILL, _framed_case, _routed, check  # noqa: E402
from test_gpu_lane import LANE_MAX_LEN, OTHER_KINDS, SCHEDULE, lane_only  # noqa: E402
from test_gpu_tls12 import _tls12_batch, _tls12_expect  # noqa: E402

pytestmark = pytest.mark.gpu

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))
KEY_SIZES = pytest.mark.parametrize("key_size", [16, 32])
VERSIONS = pytest.mark.parametrize("version", [13, 12], ids=["tls13", "tls12"])
# the counter-window edge (the step whose fourth counter is 256 holds text blocks 251..254) and the TLS record limit
EDGE_LENS = list(range(4063, 4113)) + [16383, 16384]


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


def lane_keyset(keys, ivs, key_size, framed=True):
    ks = pa.Keyset(keys, ivs, key_size)
    ks.set_schedule(SCHEDULE)
    ks.set_lane_framed(framed)
    return ks


def no_lane(cnt, phase):
    assert cnt["launches"]["lane"] == 0 and cnt["runs"]["lane_records"] == 0, f"{phase}: {cnt}"
    assert sum(cnt["launches"][k] for k in OTHER_KINDS) >= 1, f"{phase}: {cnt}"


def _packed(base, sizes):
    return base + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ TLS 1.3 cases


class Tls13Case:
    """TLS 1.3 records of ``lens`` payload bytes and inner ``types``: the payloads packed back to back from an odd base
    (the byte behind a payload is the next record's first byte), the wire records back to back from another, the opened
    texts (payload || type) from a third. ``want_wire`` / ``want_plain``: built by ``fill_expected`` over the fills."""

    def __init__(self, rng, lens, types, nkeys, key_size, key_idx):
        self.lens, self.types = np.asarray(lens, np.int64), np.asarray(types, np.int64)
        self.n, self.nkeys, self.key_size = len(lens), nkeys, key_size
        self.keys, self.ivs = rng.bytes(key_size * nkeys), rng.bytes(12 * nkeys)
        self.data = rand_bytes(rng, 7 + int(self.lens.sum()) + TAIL)
        seal = np.zeros(self.n, pa.RECORD_DTYPE)
        seal["len"], seal["flags"], seal["key_idx"] = self.lens, self.types, key_idx
        seal["in_off"], seal["out_off"] = _packed(7, self.lens), _packed(3, self.lens + 22)
        seal["seq"] = rng.integers(0, 2**64, self.n, dtype=np.uint64)
        opn = np.zeros(self.n, pa.RECORD_DTYPE)
        opn["in_off"], opn["len"], opn["seq"], opn["key_idx"] = seal["out_off"], self.lens + 1, seal["seq"], key_idx
        opn["out_off"] = _packed(1, self.lens + 1)
        self.seal, self.open = seal, opn
        self.wire_fill = rand_bytes(rng, 3 + int((self.lens + 22).sum()) + TAIL)
        self.plain_fill = rand_bytes(rng, 1 + int((self.lens + 1).sum()) + TAIL)

    def fill_expected(self, ref, skip=()):
        ksz = self.key_size
        self.want_wire, self.want_plain = self.wire_fill.copy(), self.plain_fill.copy()
        for i in range(self.n):
            if i in skip:
                continue
            k, o, ln, p, t = (int(x) for x in (self.seal["key_idx"][i], self.seal["out_off"][i], self.lens[i],
                                               self.seal["in_off"][i], self.types[i]))
            hdr = bytes([23, 3, 3, (ln + 17) >> 8, (ln + 17) & 0xFF])
            inner = self.data[p:p + ln].tobytes() + bytes([t])
            rec = hdr + ref.seal(self.keys[ksz * k:ksz * k + ksz], self.ivs[12 * k:12 * k + 12], int(self.seal["seq"][i]), hdr, inner)
            self.want_wire[o:o + len(rec)] = np.frombuffer(rec, np.uint8)
            q = int(self.open["out_off"][i])
            self.want_plain[q:q + ln + 1] = np.frombuffer(inner, np.uint8)


def seal_and_open_tls13(c, ks, accepted, rejected=()):
    """Seals case ``c`` over its wire fill and opens the expected wire arena over its plaintext fill, both compared
    whole, with ok bytes, results and their filled tails exact; ``rejected`` records are refused by the kernel."""
    n = c.n
    d_seal, d_in, d_out = dev(c.seal), dev(c.data), dev(c.wire_fill)
    pa.debug_counters(reset=True)
    pa.seal_tls_records(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(lane_only(accepted), "seal")
    assert_arena(d_out.cpu().numpy(), c.want_wire, c.seal["out_off"], c.lens + 22, "wire arena against fusion's records")
    assert np.array_equal(d_in.cpu().numpy(), c.data), "the seal wrote to its payload arena"
    res = np.zeros(n, pa.TLS_RESULT_DTYPE)
    res["plain_len"], res["content_type"] = c.lens, c.types
    res["status"][(c.lens == 0) & (c.types != 23)] = pa.TLS_UNEXPECTED_MESSAGE
    for i in rejected:
        res[i] = (0, 0, pa.TLS_BAD_MAC, 0)
    rfill = rand_bytes(np.random.default_rng(n), 8 * n + TAIL)
    want_res = rfill.copy()
    want_res[:8 * n] = res.view(np.uint8)
    d_open, d_wire, d_plain = dev(c.open), dev(c.want_wire), dev(c.plain_fill)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    pa.open_tls_records(ks, d_open.data_ptr(), n, d_wire.data_ptr(), d_plain.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(lane_only(accepted), "open")
    ok = d_ok.cpu().numpy()
    assert_arena(d_res.cpu().numpy(), want_res, 8 * np.arange(n), np.full(n, 8), "TLS results")
    assert np.array_equal(ok[:n], (res["status"] == pa.TLS_OK).astype(np.uint8))
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"
    assert np.array_equal(d_wire.cpu().numpy(), c.want_wire), "the open wrote to the wire arena"
    assert_arena(d_plain.cpu().numpy(), c.want_plain, c.open["out_off"], c.lens + 1, "opened plaintext arena")


# ------------------------------------------------------------------------------------------------ 1. the interface


def test_the_flag_is_a_second_opt_in_beside_the_schedule():
    """Off on a new keyset; the setter and getter round-trip; it survives a change of schedule; NULL is refused; under
    "auto" it routes nothing to the lane kernel, and the same call under "record_per_lane" gives the same bytes from it."""
    rng = np.random.default_rng(9950)
    lib = pa.load_library()
    c = Tls13Case(rng, rng.integers(0, 200, 300), rng.choice([21, 22, 23], 300), 3, 16, np.arange(300) * 3 // 300)
    ks = pa.Keyset(c.keys, c.ivs, 16)
    assert ks.lane_framed is False and lib.ptls_mi355x_keyset_get_lane_framed(ks.handle) == 0
    ks.set_lane_framed(True)
    assert ks.lane_framed is True and lib.ptls_mi355x_keyset_get_lane_framed(ks.handle) == 1
    ks.set_lane_framed(False)
    assert ks.lane_framed is False
    assert lib.ptls_mi355x_keyset_set_lane_framed(ks.handle, 7) == 0 and ks.lane_framed is True
    ks.set_schedule("auto")
    ks.set_schedule(SCHEDULE)
    assert ks.lane_framed is True
    assert lib.ptls_mi355x_keyset_set_lane_framed(None, 1) == -1
    assert lib.ptls_mi355x_keyset_get_lane_framed(None) == 0
    out = {}
    d_seal, d_in = dev(c.seal), dev(c.data)
    for schedule in ("auto", SCHEDULE):
        ks.set_schedule(schedule)
        d_out = dev(c.wire_fill)
        pa.debug_counters(reset=True)
        pa.seal_tls_records(ks, d_seal.data_ptr(), c.n, d_in.data_ptr(), d_out.data_ptr(), _stream())
        torch.cuda.synchronize()
        _routed(no_lane if schedule == "auto" else lane_only(c.n), schedule)
        out[schedule] = d_out.cpu().numpy()
    assert_arena(out[SCHEDULE], out["auto"], c.seal["out_off"], c.lens + 22, "wire arena against the auto schedule's")
    ks.free()


# ------------------------------------------------------------------------------------------------ 2. TLS 1.3, every length


@KEY_SIZES
def test_tls13_every_length_to_300_with_every_type_and_the_edges(ref, key_size):
    """Payloads of 0..300 bytes x inner types {21, 22, 23}, 4063..4112 bytes (the counter-window edge) and 16,383 and
    16,384, over 5 keys in random order, permuted so that neighbouring lanes differ in length. The text is len + 1
    bytes and a step past the first holds text blocks 4s - 1 .. 4s + 2, so every length to 300 covers: the type byte as
    a block's only byte (0, 16, ...), as a step's first byte (48, 112, ...), as a block's last byte (15, 47, 63, ...),
    and a step whose four blocks are whole by the text length but not by the readable payload (111: 112 text bytes end
    step 1). The byte behind a payload is the next record's first byte, so a kernel that reads it in place of the type
    fails."""
    rng = np.random.default_rng(9960 + key_size)
    lens = np.concatenate([np.repeat(np.arange(301), 3), EDGE_LENS])
    types = np.concatenate([np.tile([21, 22, 23], 301), np.array([21, 22, 23])[np.arange(len(EDGE_LENS)) % 3]])
    assert set((0, 15, 16, 47, 63, 111)) <= set(lens.tolist())
    order = rng.permutation(len(lens))
    c = Tls13Case(rng, lens[order], types[order], 5, key_size, rng.integers(0, 5, len(lens)))
    c.fill_expected(ref)
    ks = lane_keyset(c.keys, c.ivs, key_size)
    seal_and_open_tls13(c, ks, c.n)
    ks.free()


# ------------------------------------------------------------------------------------------------ 3. opens with tampering


@VERSIONS
def test_framed_open_with_tampered_records_and_refused_headers(ref, version):
    """test_gpu_footprint._framed_case: 600 wire records of 0..16,383 payload bytes with a ciphertext, a tag and a header
    bit flipped and two records whose tag verifies under a header the record layer refuses. Results, ok bytes, their
    filled tails, the untouched wire arena and the whole plaintext arena exact, as _framed_open asserts them."""
    rng = np.random.default_rng(9970 + version)
    n = 600
    keys, ivs, key_size, orecs, wire, pfill, want, res, offs, sizes = _framed_case(ref, rng, version, n, True)
    ks = lane_keyset(keys, ivs, key_size)
    rfill = rand_bytes(rng, 8 * n + TAIL)
    d_recs, d_wire, d_out = dev(orecs), dev(wire), dev(pfill)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    opener = pa.open_tls_records if version == 13 else pa.open_tls12_records
    pa.debug_counters(reset=True)
    opener(ks, d_recs.data_ptr(), n, d_wire.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(lane_only(n), "open")
    ok, got_res = d_ok.cpu().numpy(), d_res.cpu().numpy()
    want_res = rfill.copy()
    want_res[:8 * n] = res.view(np.uint8)
    assert_arena(got_res, want_res, 8 * np.arange(n), np.full(n, 8), "TLS results")
    assert np.array_equal(ok[:n], (res["status"] == pa.TLS_OK).astype(np.uint8))
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"
    assert np.array_equal(d_wire.cpu().numpy(), wire), "the open wrote to the wire arena"
    assert_arena(d_out.cpu().numpy(), want, offs, sizes, "opened plaintext arena")
    ks.free()


# ------------------------------------------------------------------------------------------------ 4. TLS 1.2


def _tls12_open_back(ks, recs, lens, wire, arena, routing, rejected=()):
    """opens the TLS 1.2 wire arena ``wire`` back into a random fill: every record but the ``rejected`` restores its
    payload with TLS_OK and type 23, the rejected ones report BAD_MAC and keep the fill"""
    n = len(recs)
    rng = np.random.default_rng(n)
    precs = recs.copy()
    precs["in_off"], precs["out_off"] = recs["out_off"], _packed(1, lens)
    pfill = rand_bytes(rng, 1 + int(lens.sum()) + TAIL)
    want_plain = pfill.copy()
    res = np.zeros(n, pa.TLS_RESULT_DTYPE)
    res["plain_len"], res["content_type"] = lens, 23
    for i in range(n):
        if i in rejected:  # (tls12_check_kernel reports the type byte it finds at the record's start)
            res[i] = (0, int(wire[int(recs["out_off"][i])]), pa.TLS_BAD_MAC, 0)
            continue
        o, p, ln = int(precs["out_off"][i]), int(recs["in_off"][i]) + 8, int(lens[i])
        want_plain[o:o + ln] = arena[p:p + ln]
    rfill = rand_bytes(rng, 8 * n + TAIL)
    want_res = rfill.copy()
    want_res[:8 * n] = res.view(np.uint8)
    d_recs, d_wire, d_plain = dev(precs), dev(wire), dev(pfill)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    pa.debug_counters(reset=True)
    pa.open_tls12_records(ks, d_recs.data_ptr(), n, d_wire.data_ptr(), d_plain.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(routing, "open")
    ok = d_ok.cpu().numpy()
    assert_arena(d_res.cpu().numpy(), want_res, 8 * np.arange(n), np.full(n, 8), "TLS results")
    assert np.array_equal(ok[:n], (res["status"] == pa.TLS_OK).astype(np.uint8))
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"
    assert np.array_equal(d_wire.cpu().numpy(), wire), "the open wrote to the wire arena"
    assert_arena(d_plain.cpu().numpy(), want_plain, precs["out_off"], lens, "opened plaintext arena")


@KEY_SIZES
def test_tls12_seal_every_length_and_open_back(ref, key_size):
    """test_gpu_tls12._tls12_batch with payloads of 0..300 bytes, the counter-edge lengths, 16,383 and 16,384 over 3 keys: every
    wire record equals _tls12_expect (header || explicit nonce || fusion's seal under the record-layer nonce and AAD),
    nothing outside the wire records is written, and every record opens back to its payload with TLS_OK."""
    rng = np.random.default_rng(9980 + key_size)
    lens = rng.permutation(np.array(list(range(301)) + EDGE_LENS))
    n = len(lens)
    keys, ivs, recs, arena = _tls12_batch(rng, lens, 3, key_size)
    fill = rand_bytes(rng, int((lens + 29).sum()) + TAIL)
    want = fill.copy()
    for i in range(n):
        rec = _tls12_expect(ref, keys, ivs, key_size, recs, arena, i)
        assert len(rec) == int(lens[i]) + 29
        want[int(recs["out_off"][i]):int(recs["out_off"][i]) + len(rec)] = np.frombuffer(rec, np.uint8)
    ks = lane_keyset(keys, ivs, key_size)
    d_recs, d_in, d_out = dev(recs), dev(arena), dev(fill)
    pa.debug_counters(reset=True)
    pa.seal_tls12_records(ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(lane_only(n), "seal")
    assert_arena(d_out.cpu().numpy(), want, recs["out_off"], lens + 29, "wire arena against fusion's records")
    assert np.array_equal(d_in.cpu().numpy(), arena), "the seal wrote to its input arena"
    _tls12_open_back(ks, recs, lens, want, arena, lane_only(n))
    ks.free()


# ------------------------------------------------------------------------------------------------ 5. the chunked kernels' bytes


def test_the_wire_arenas_are_the_chunked_kernels():
    """2,000 records of U[0, 2000] payload bytes over 500 keys in random order on one keyset set to the schedule: the
    TLS 1.3 and the TLS 1.2 wire arena sealed with the flag on and with it off, into the same fill, are byte-identical;
    the counters show lane launches in the first arm and none in the second."""
    rng = np.random.default_rng(9990)
    n, nkeys = 2000, 500
    lens = rng.integers(0, 2001, n)
    key_idx = rng.integers(0, nkeys, n)
    c = Tls13Case(rng, lens, rng.choice([21, 22, 23], n), nkeys, 16, key_idx)
    _, _, recs12, arena12 = _tls12_batch(rng, lens, nkeys, 16)
    recs12["key_idx"] = key_idx
    fill12 = rand_bytes(rng, int((lens + 29).sum()) + TAIL)
    ks = lane_keyset(c.keys, c.ivs, 16)
    d13, d_in13, d12, d_in12 = dev(c.seal), dev(c.data), dev(recs12), dev(arena12)
    out = {}
    for framed in (True, False):
        ks.set_lane_framed(framed)
        d_out13, d_out12 = dev(c.wire_fill), dev(fill12)
        for version, call in ((13, lambda: pa.seal_tls_records(ks, d13.data_ptr(), n, d_in13.data_ptr(), d_out13.data_ptr(), _stream())),
                              (12, lambda: pa.seal_tls12_records(ks, d12.data_ptr(), n, d_in12.data_ptr(), d_out12.data_ptr(), _stream()))):
            pa.debug_counters(reset=True)
            call()
            torch.cuda.synchronize()
            cnt = pa.debug_counters(reset=True)
            if framed:
                lane_only(n)(cnt, f"TLS {version}, flag on")
                assert cnt["launches"]["lane"] == 1, cnt
            else:
                no_lane(cnt, f"TLS {version}, flag off")
        out[framed] = d_out13.cpu().numpy(), d_out12.cpu().numpy()
    assert_arena(out[True][0], out[False][0], c.seal["out_off"], lens + 22, "TLS 1.3 wire arena against the chunked kernels'")
    assert_arena(out[True][1], out[False][1], recs12["out_off"], lens + 29, "TLS 1.2 wire arena against the chunked kernels'")
    assert not np.array_equal(out[True][0], c.wire_fill) and not np.array_equal(out[True][1], fill12)
    ks.free()


# ------------------------------------------------------------------------------------------------ 6. batch sizes


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_tls13_batch_sizes_around_a_wave_and_a_tile(ref, n):
    rng = np.random.default_rng(10000 + n)
    c = Tls13Case(rng, rng.integers(0, 500, n), rng.choice([21, 22, 23], n), 7, 16, rng.integers(0, 7, n))
    c.fill_expected(ref)
    ks = lane_keyset(c.keys, c.ivs, 16)
    seal_and_open_tls13(c, ks, n)
    ks.free()


# ------------------------------------------------------------------------------------------------ 7. rejected descriptors


@VERSIONS
def test_framed_descriptors_beyond_the_limits_are_not_written_for(ref, version):
    """len = 65,537, len = 2^30 + 1 and key_idx = nkeys among 700 framed records: their wire ranges keep the fill, an
    open of them gives ok = 0 with status BAD_MAC and writes no plaintext, and their neighbours are exact. (The records
    are laid out with their true, short lengths; the arenas behind the first rejected record are longer than the
    limit, so a kernel that took the descriptor at its word would show in them.)"""
    rng = np.random.default_rng(10100 + version)
    n, nkeys = 700, 4
    lens = rng.integers(0, 400, n)
    key_idx = rng.integers(0, nkeys, n)
    rejected = [17, 64, 301]
    bad_len = {17: LANE_MAX_LEN + 1, 64: (1 << 30) + 1}
    assert int(lens[65:].sum()) > LANE_MAX_LEN + 4096
    if version == 13:
        c = Tls13Case(rng, lens, rng.choice([22, 23], n), nkeys, 16, key_idx)
        c.fill_expected(ref, skip=rejected)
        for d in (c.seal, c.open):
            for i, v in bad_len.items():
                d["len"][i] = v
            d["key_idx"][301] = nkeys
        ks = lane_keyset(c.keys, c.ivs, 16)
        seal_and_open_tls13(c, ks, n - len(rejected), rejected=rejected)
        ks.free()
        return
    keys, ivs, recs, arena = _tls12_batch(rng, lens, nkeys, 16)
    recs["key_idx"] = key_idx
    fill = rand_bytes(rng, int((lens + 29).sum()) + TAIL)
    want = fill.copy()
    for i in range(n):
        if i not in rejected:
            rec = _tls12_expect(ref, keys, ivs, 16, recs, arena, i)
            want[int(recs["out_off"][i]):int(recs["out_off"][i]) + len(rec)] = np.frombuffer(rec, np.uint8)
    for i, v in bad_len.items():
        recs["len"][i] = v
    recs["key_idx"][301] = nkeys
    ks = lane_keyset(keys, ivs, 16)
    d_recs, d_in, d_out = dev(recs), dev(arena), dev(fill)
    pa.debug_counters(reset=True)
    pa.seal_tls12_records(ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(lane_only(n - len(rejected)), "seal")
    assert_arena(d_out.cpu().numpy(), want, recs["out_off"], lens + 29, "wire arena against fusion's records")
    _tls12_open_back(ks, recs, lens, want, arena, lane_only(n - len(rejected)), rejected=rejected)
    ks.free()


# ------------------------------------------------------------------------------------------------ 8. far arenas


@VERSIONS
def test_framed_records_in_arenas_that_straddle_4_gib(ref, version):
    """test_gpu_far_offsets' framed case (300 records of U[0, 3000) payload bytes, the open's wire with an all-zero inner
    plaintext, a refused header under a valid tag and three flipped bits) with every arena straddling 2^32 bytes behind
    the pointer the call is given: the header store, the explicit-nonce load and the type load at in + in_off take
    64-bit offsets."""
    rng = np.random.default_rng(10200 + version)
    t = F.tls_shape(version)
    key_size = 32 if version == 13 else 16
    keys = rand_bytes(rng, 3 * key_size)
    if version == 13:
        ivs = rand_bytes(rng, 3 * 12)
    else:  # the GCM nonce is fixed IV || explicit nonce: fusion's seq is the explicit nonce on a static IV of fixed || 0^64
        ivs = np.concatenate([np.concatenate([rand_bytes(rng, 4), np.zeros(8, np.uint8)]) for _ in range(3)])

    def seal_one(k, seq, aad, text):
        return ref.seal(keys[key_size * k:key_size * (k + 1)].tobytes(), ivs[12 * k:12 * k + 12].tobytes(), seq, aad, text)

    x = _tls_case(t, rng, seal_one, 64)
    ks = lane_keyset(keys, ivs, key_size)
    pa.debug_counters(reset=True)
    sealer, opener = (pa.seal_tls_records, pa.open_tls_records) if version == 13 else (pa.seal_tls12_records, pa.open_tls12_records)
    _far_framed(t, rng, x, ks, sealer, opener, lambda phase: _routed(lane_only(t.n), phase), strict=True)
    ks.free()


# ------------------------------------------------------------------------------------------------ 9. seal_batch_hp


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "in_place"])
def test_seal_batch_hp_is_the_lane_seal_and_a_mask_launch(ref, in_place):
    """The shape of test_gpu_footprint.test_seal_with_header_protection_masks (300 packets of 1185..1215 bytes over 5
    connections, samples 0..3 bytes into the ciphertext) with 20 packets whose sample is their tag (sample_off = out_off
    + len): the sealed arena is fusion's, the masks are ref.seal_with_hp's where the sample lies in the ciphertext and
    the reference's AES-ECB of the tag otherwise, the masks buffer's tail keeps its fill, and the launches are one lane
    seal and no fused one."""
    rng = np.random.default_rng(10300 + in_place)
    n, nkeys = 300, 5
    c = packed_case(rng, rng.integers(1185, 1216, n), rng.integers(8, 30, n), 16, nkeys, in_place)
    s = c.b.seal
    hp_keys = rand_bytes(rng, nkeys * 16)
    sample_in_ct = (4 - rng.integers(1, 5, n)).astype(np.int64)
    on_tag = rng.choice(n, 20, replace=False)
    sample_in_ct[on_tag] = s["len"][on_tag]
    hp = np.zeros(n, dtype=pa.HP_DTYPE)
    hp["sample_off"] = s["out_off"] + sample_in_ct.astype(np.uint64)
    hp["key_idx"] = s["key_idx"]
    hp_ks = pa.Keyset(hp_keys, np.zeros(nkeys * 12, np.uint8), 16)
    mfill = rand_bytes(rng, 16 * n + TAIL)
    d_hp, d_masks = dev(hp), dev(mfill)

    def do_seal(ks, d_recs, n_, d_in, d_aad, d_out):
        ks.set_lane_framed(True)
        pa.seal_batch_hp(ks, d_recs.data_ptr(), n_, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), hp_ks, d_hp.data_ptr(),
                         d_masks.data_ptr(), _stream())

    def routing(cnt, phase):
        lane_only(n)(cnt, phase)
        assert cnt["launches"]["seal_hp"] == 0 and cnt["launches"]["lane"] == 1, f"{phase}: {cnt}"

    check(ref, rng, c, routing, schedule=SCHEDULE, do_seal=do_seal)
    want_masks = mfill.copy()
    for i in range(n):
        k, p, ln, a, al = (int(s[f][i]) for f in ("key_idx", "in_off", "len", "aad_off", "aad_len"))
        hpk = hp_keys[16 * k:16 * k + 16].tobytes()
        tagged = int(sample_in_ct[i]) == ln
        sealed, mask = ref.seal_with_hp(c.keys[16 * k:16 * k + 16].tobytes(), c.ivs[12 * k:12 * k + 12].tobytes(), int(s["seq"][i]),
                                        c.aad[a:a + al].tobytes(), c.src[p:p + ln].tobytes(), hpk, 0 if tagged else int(sample_in_ct[i]))
        if tagged:
            mask = ref.aesecb(hpk, sealed[ln:ln + 16])
        want_masks[16 * i:16 * i + 16] = np.frombuffer(mask, np.uint8)
    assert_arena(d_masks.cpu().numpy(), want_masks, 16 * np.arange(n), np.full(n, 16), "header-protection masks")
    hp_ks.free()
