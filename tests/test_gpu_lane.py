"""The record-per-lane schedule (PTLS_MI355X_SCHEDULE_RECORD_PER_LANE, gcm_lane_kernel) against lib/fusion.c.

Every case is a batch of byte-adjacent records from odd bases (footprint_util.packed_case) in arenas pre-filled with
random bytes, sealed and opened by test_gpu_footprint.check: the whole sealed arena against the arena fusion wrote into,
then fusion's arena opened with three tampered records (one ciphertext bit, one tag bit, one AAD bit) and the whole
plaintext arena, the ok bytes and their tail compared, with no mask and no sampling. Every launch is checked through the
debug counters: the lane kernel ran, no chunked or lockstep kernel did, and it accepted exactly the records the case
means it to."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import far_util as F  # noqa: E402
import picotls_amd as pa  # noqa: E402
from footprint_util import assert_arena, packed_case, rand_bytes  # noqa: E402
from gpu_util import dev, empty  # noqa: E402
from oracle import FusionRef  # noqa: E402
from test_gpu_far_offsets import far_check  # noqa: E402
from test_gpu_footprint import check  # noqa: E402

pytestmark = pytest.mark.gpu

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                       "libfusion_ref.so"))
SCHEDULE = "record_per_lane"
LANE_MAX_LEN = 1 << 16  # PTLS_MI355X_LANE_MAX_LEN
OTHER_KINDS = ("chunked", "spread", "seal_hp", "w8_tree", "w8_serial", "lockstep", "span")
LAYOUTS = pytest.mark.parametrize("in_place", [False, True], ids=["packed", "in_place"])
KEY_SIZES = pytest.mark.parametrize("key_size", [16, 32])


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


def lane_only(accepted):
    """routing for check / far_check: one lane launch that accepted ``accepted`` records, nothing else"""

    def routing(cnt, phase):
        launches = cnt["launches"]
        assert launches["lane"] >= 1 and all(launches[k] == 0 for k in OTHER_KINDS), f"{phase}: {cnt}"
        assert cnt["runs"]["lane_records"] == accepted, f"{phase}: {cnt}"

    return routing


def lane_check(ref, rng, c, rejected=()):
    check(ref, rng, c, lane_only(c.n - len(rejected)), schedule=SCHEDULE, rejected=rejected)


# ------------------------------------------------------------------------------------------------ the interface


def test_the_schedule_is_accepted_by_name_and_by_value():
    ks = pa.Keyset(bytes(16), bytes(12), 16)
    assert pa.Keyset.SCHEDULES[SCHEDULE] == 3
    ks.set_schedule(SCHEDULE)  # (a constant-time keyset, as every keyset is when created: the kernel is constant-time)
    assert ks.constant_time
    lib = pa.load_library()
    assert lib.ptls_mi355x_keyset_set_schedule(ks.handle, 3) == 0
    assert lib.ptls_mi355x_keyset_set_schedule(ks.handle, 7) == -1
    assert lib.ptls_mi355x_keyset_set_schedule(ks.handle, 4) == -1
    ks.free()


# ------------------------------------------------------------------------------------------------ lengths


@LAYOUTS
@KEY_SIZES
def test_every_length_to_300_with_every_aad_kind(ref, key_size, in_place):
    """every length 0..300 x AAD {0, 1, 13, 16, 17, 40} over 5 keys in random order: 1,806 records, eight tiles"""
    rng = np.random.default_rng(9100 + key_size + in_place)
    lens, aads = np.repeat(np.arange(301), 6), np.tile([0, 1, 13, 16, 17, 40], 301)
    order = rng.permutation(len(lens))  # (lanes beside each other hold records of unlike lengths)
    c = packed_case(rng, lens[order], aads[order], key_size, 5, in_place, key_idx=rng.integers(0, 5, len(lens)))
    lane_check(ref, rng, c)


@LAYOUTS
@KEY_SIZES
def test_counter_window_edges_and_the_longest_records(ref, key_size, in_place):
    """4064..4112 bytes: the last counters of the cache's first 256-counter window and the first of the next (the step
    whose fourth counter is 256 holds text blocks 251..254: bytes 4016..4079); 65,520 and 65,536: the sixteenth window
    and the limit itself, beside short records that end long before them."""
    rng = np.random.default_rng(9200 + key_size + in_place)
    lens = np.array(list(range(4064, 4113)) + [65520, 65536, 65535, 65521, 8176, 8177] + [0, 5, 100, 1200])
    aads = np.array([0, 1, 13, 16, 17, 40])[np.arange(len(lens)) % 6]
    order = rng.permutation(len(lens))
    c = packed_case(rng, lens[order], aads[order], key_size, 3, in_place, key_idx=rng.integers(0, 3, len(lens)))
    lane_check(ref, rng, c)


def test_an_aad_of_the_limit_is_accepted(ref):
    """AAD lengths of 64 KiB travel in flags (PTLS_MI355X_RECORD_AAD_LEN): 65,536 bytes of AAD, the limit, seal as
    fusion seals them; the batch reference takes 16-bit AAD lengths, so this record goes through fusion's single call"""
    rng = np.random.default_rng(9250)
    key, iv = rng.bytes(16), rng.bytes(12)
    aad, pt = rand_bytes(rng, LANE_MAX_LEN), rand_bytes(rng, 333)
    recs = np.zeros(1, pa.RECORD_DTYPE)
    recs["in_off"], recs["out_off"], recs["aad_off"], recs["seq"], recs["len"] = 3, 5, 0, 77, 330
    recs["aad_len"], recs["flags"] = 0, 1
    fill = rand_bytes(rng, 512)
    want = fill.copy()
    want[5:5 + 346] = np.frombuffer(ref.seal(key, iv, 77, aad.tobytes(), pt[3:333].tobytes()), np.uint8)
    ks = pa.Keyset(key, iv, 16)
    ks.set_schedule(SCHEDULE)
    d_recs, d_pt, d_aad, d_out = dev(recs), dev(pt), dev(aad), dev(fill)
    pa.debug_counters(reset=True)
    pa.seal_batch(ks, d_recs.data_ptr(), 1, d_pt.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    lane_only(1)(pa.debug_counters(reset=True), "seal")
    assert_arena(d_out.cpu().numpy(), want, [5], [346], "sealed arena against fusion's")
    ks.free()


# ------------------------------------------------------------------------------------------------ rejected descriptors


@LAYOUTS
def test_descriptors_beyond_the_limits_are_not_written_for(ref, in_place):
    """len = 65,537, len = 2^30 + 1, len = 2^32 - 1, an AAD of 65,537 bytes and key_idx = nkeys among 700 records: their
    ranges keep the arena's fill, open gives ok = 0, their neighbours are sealed and opened. (The records are laid out
    with their true, short lengths; the arena behind the first rejected record is longer than the limit.)"""
    rng = np.random.default_rng(9300 + in_place)
    n, nkeys = 700, 4
    c = packed_case(rng, rng.integers(0, 400, n), rng.integers(0, 41, n), 16, nkeys, in_place, key_idx=rng.integers(0, nkeys, n))
    rejected = [17, 64, 255, 256, 301]
    assert c.b.sealed_bytes - int(c.b.seal["out_off"][301]) > LANE_MAX_LEN + 4096
    for d in (c.b.seal, c.b.open):
        d["len"][17], d["len"][64], d["len"][255] = LANE_MAX_LEN + 1, (1 << 30) + 1, 0xFFFFFFFF
        d["aad_len"][256], d["flags"][256] = 1, 1  # 65,537 bytes of AAD
        d["key_idx"][301] = nkeys
    lane_check(ref, rng, c, rejected=rejected)


# ------------------------------------------------------------------------------------------------ keys and batch sizes


@LAYOUTS
@KEY_SIZES
def test_one_key_per_record_in_random_order(ref, key_size, in_place):
    """1,000 records of U[0, 3000] bytes over 1,000 keys, no two records of one key, in no order"""
    rng = np.random.default_rng(9400 + key_size + in_place)
    n = 1000
    c = packed_case(rng, rng.integers(0, 3001, n), rng.integers(0, 41, n), key_size, n, in_place, key_idx=rng.permutation(n))
    lane_check(ref, rng, c)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_around_a_wave_and_a_tile(ref, n):
    rng = np.random.default_rng(9500 + n)
    c = packed_case(rng, rng.integers(1 if n < 3 else 0, 500, n), rng.integers(1, 41, n), 16, 7, False, key_idx=rng.integers(0, 7, n))
    if n >= 3:
        lane_check(ref, rng, c)
        return
    # (the tamper of the shared checker wants three records: a lone record is sealed and opened here)
    ks = pa.Keyset(c.keys, c.ivs, 16)
    ks.set_schedule(SCHEDULE)
    want = c.fill.copy()
    ref.run_batch(True, c.keys, c.ivs, 16, c.b.seal, c.src, c.aad, want)
    d_seal, d_open, d_in, d_aad, d_out = dev(c.b.seal), dev(c.b.open), dev(c.src), dev(c.aad), dev(c.fill)
    pa.debug_counters(reset=True)
    pa.seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    lane_only(n)(pa.debug_counters(reset=True), "seal")
    assert_arena(d_out.cpu().numpy(), want, c.sealed_offs, c.sealed_sizes, "sealed arena against fusion's")
    pfill = rand_bytes(rng, c.b.pt_bytes)
    want_back = pfill.copy()
    ref_ok = np.zeros(n, np.uint8)
    ref.run_batch(False, c.keys, c.ivs, 16, c.b.open, want, c.aad, want_back, ok=ref_ok)
    d_back, d_ok = dev(pfill), empty(n + 64, 0xAA)
    pa.open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), d_aad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    lane_only(n)(pa.debug_counters(reset=True), "open")
    ok = d_ok.cpu().numpy()
    assert ref_ok.all() and (ok[:n] == 1).all() and (ok[n:] == 0xAA).all()
    assert_arena(d_back.cpu().numpy(), want_back, c.plain_offs, c.plain_sizes, "opened arena against fusion's")
    ks.free()


def test_more_tiles_than_workgroups_and_a_ragged_last_wave(ref):
    """256 x CUs + 777 records of 64..200 bytes over 4,096 keys: every workgroup takes a tile, the first four a second
    one (the grid-stride step), the last tile ends inside a wave"""
    rng = np.random.default_rng(9600)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * ncu + 777
    c = packed_case(rng, rng.integers(64, 201, n), rng.choice([0, 13, 17, 21], n), 16, 4096, False, key_idx=rng.integers(0, 4096, n))
    lane_check(ref, rng, c)


# ------------------------------------------------------------------------------------------------ far arenas


def test_arenas_that_straddle_4_gib(ref):
    """300 records sealed from a far arena into a far arena and opened back, each arena straddling 2^32 bytes behind the
    pointer the call is given. The precondition first: every 32-bit image of a shifted offset lies in an alias window
    the test owns and reads back, so an offset narrowed to 32 bits on its way to an access fails an assertion."""
    rng = np.random.default_rng(9700)
    n = 300
    c = packed_case(rng, rng.integers(0, 3000, n), rng.integers(0, 41, n), 32, 40, False, key_idx=rng.integers(0, 40, n))
    for sp in F.batch_spans(c.b.seal, c.b.open, c.b.pt_bytes, c.b.sealed_bytes, False).values():
        lay = F.far_layout(sp.size, 1, spans=sp.span)
        F.check_images(lay, sp.offs, sp.sizes)
        for offs, sizes in sp.parts.values():
            F.check_images(lay, offs, sizes)
    far_check(ref, rng, c, lane_only(n), schedule=SCHEDULE)


# ------------------------------------------------------------------------------------------------ the other schedules


def test_the_sealed_arena_is_the_auto_schedules():
    """5,000 records of U[0, 2000] bytes over 700 keys: the same keyset seals the same batch under "record_per_lane" and
    under "auto" into arenas of the same random fill, byte-identical; both open back"""
    rng = np.random.default_rng(9800)
    n, nkeys = 5000, 700
    c = packed_case(rng, rng.integers(0, 2001, n), rng.integers(0, 41, n), 16, nkeys, False, key_idx=rng.integers(0, nkeys, n))
    ks = pa.Keyset(c.keys, c.ivs, 16)
    d_seal, d_open, d_in, d_aad = dev(c.b.seal), dev(c.b.open), dev(c.src), dev(c.aad)
    out, back = {}, {}
    for schedule in (SCHEDULE, "auto"):
        ks.set_schedule(schedule)
        d_out, d_back, d_ok = dev(c.fill), dev(c.src[::-1].copy()), empty(n, 0xAA)
        pa.debug_counters(reset=True)
        pa.seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
        pa.open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), d_aad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        cnt = pa.debug_counters(reset=True)
        if schedule == SCHEDULE:
            lane_only(2 * n)(cnt, "seal and open")
            assert cnt["launches"]["lane"] == 2, cnt
        else:
            assert cnt["launches"]["lane"] == 0 and cnt["runs"]["lane_records"] == 0 and cnt["launches"]["w8_serial"] >= 2, cnt
        assert (d_ok.cpu().numpy() == 1).all(), schedule
        out[schedule], back[schedule] = d_out.cpu().numpy(), d_back.cpu().numpy()
    assert_arena(out[SCHEDULE], out["auto"], c.sealed_offs, c.sealed_sizes, "sealed arena against the auto schedule's")
    assert_arena(back[SCHEDULE], back["auto"], c.plain_offs, c.plain_sizes, "opened arena against the auto schedule's")
    ks.free()


def test_tls13_framed_batches_keep_the_chunked_kernels(ref):
    """seal_tls_records / open_tls_records on a keyset set to the schedule: the wire arena is header || fusion's seal of
    payload || type for every record and random fill elsewhere, every record opens back, and no lane kernel ran"""
    rng = np.random.default_rng(9900)
    n, nkeys = 300, 3
    lens = rng.integers(0, 2000, n)
    keys, ivs = rng.bytes(16 * nkeys), rng.bytes(12 * nkeys)
    data = rand_bytes(rng, int(lens.sum()) + 7)
    recs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    recs["len"] = lens
    recs["in_off"] = 7 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    recs["out_off"] = 3 + np.concatenate([[0], np.cumsum(lens + 22)[:-1]])
    recs["key_idx"] = np.arange(n) * nkeys // n
    recs["seq"] = rng.integers(0, 2**40, n)
    recs["flags"] = rng.choice([21, 22, 23], n)
    wire_len = 3 + int((lens + 22).sum()) + 64
    fill = rand_bytes(rng, wire_len)
    want = fill.copy()
    for i in range(n):
        k, o, ln, p = int(recs["key_idx"][i]), int(recs["out_off"][i]), int(lens[i]), int(recs["in_off"][i])
        hdr = bytes([23, 3, 3, (ln + 17) >> 8, (ln + 17) & 0xFF])
        rec = hdr + ref.seal(keys[16 * k:16 * k + 16], ivs[12 * k:12 * k + 12], int(recs["seq"][i]), hdr,
                             data[p:p + ln].tobytes() + bytes([int(recs["flags"][i])]))
        want[o:o + len(rec)] = np.frombuffer(rec, np.uint8)
    ks = pa.Keyset(keys, ivs, 16)
    ks.set_schedule(SCHEDULE)
    d_recs, d_in, d_out = dev(recs), dev(data), dev(fill)
    pa.debug_counters(reset=True)
    pa.seal_tls_records(ks, d_recs.data_ptr(), n, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    cnt = pa.debug_counters(reset=True)
    assert cnt["launches"]["lane"] == 0 and cnt["launches"]["w8_serial"] >= 1, cnt
    assert_arena(d_out.cpu().numpy(), want, recs["out_off"], lens + 22, "wire arena against fusion's records")
    orecs = np.zeros(n, dtype=pa.RECORD_DTYPE)
    orecs["in_off"], orecs["len"], orecs["seq"], orecs["key_idx"] = recs["out_off"], lens + 1, recs["seq"], recs["key_idx"]
    orecs["out_off"] = 1 + np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    pfill = rand_bytes(rng, 1 + int((lens + 1).sum()) + 64)
    want_plain = pfill.copy()
    for i in range(n):
        o, ln, p = int(orecs["out_off"][i]), int(lens[i]), int(recs["in_off"][i])
        want_plain[o:o + ln] = data[p:p + ln]
        want_plain[o + ln] = recs["flags"][i]
    d_recs2, d_plain = dev(orecs), dev(pfill)
    d_ok, d_res = empty(n, 0x77), empty(8 * n, 0x77)
    pa.open_tls_records(ks, d_recs2.data_ptr(), n, d_out.data_ptr(), d_plain.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    cnt = pa.debug_counters(reset=True)
    assert cnt["launches"]["lane"] == 0 and cnt["launches"]["w8_serial"] >= 1, cnt
    assert d_ok.cpu().numpy().all()
    res = d_res.cpu().numpy().view(pa.TLS_RESULT_DTYPE)
    assert (res["status"] == pa.TLS_OK).all() and (res["plain_len"] == lens).all() and (res["content_type"] == recs["flags"]).all()
    assert_arena(d_plain.cpu().numpy(), want_plain, orecs["out_off"], lens + 1, "opened arena")
    ks.free()
