"""Every batch call that takes byte offsets, at arena offsets of 2^31 and beyond, at the top of aad_off's range and with
AADs of 64 KiB and more.

include/picotls/mi355x.h gives in_off, out_off and sample_off 64 bits, aad_off a full 32 and the AAD length 32 bits
over aad_len and flags, and every other test's arenas begin at offset 0 and hold a few hundred MB at most. Here each
kernel family runs its smallest shape (those of test_gpu_footprint.py, with its routing assertions on the debug
counters) in arenas that straddle 2^32 bytes behind the pointer the engine is given (tests/far_util.py: a real
allocation of 4 GiB and the arena's size, of which only the arena and the *alias windows* are ever touched by the
host). The arena with its guards is compared byte for byte with the reference's (lib/fusion.c, or OpenSSL for
ChaCha20-Poly1305, both run on the unshifted descriptors and small host arenas), and the alias windows, where every
32-bit misreading of a shifted offset lands, with what they were filled with. test_far_util.py proves on the CPU that
those misreadings stay inside the allocation, so an offset narrowed to 32 bits fails an assertion here and faults
nothing. No comparison has a tolerance.

Two far allocations are alive at the most (input and output, about 8.6 GiB), one of 12.3 GiB in the 3 * 2^32 case; each
is freed and the caching allocator emptied as soon as its call is checked."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import chacha_ref as R  # noqa: E402
import far_util as F  # noqa: E402
import picotls_amd as pa  # noqa: E402
import quic_util as U  # noqa: E402
from far_util import far_arena, shifted  # noqa: E402
from footprint_util import TAIL, PackedCase, assert_arena, packed_case, rand_bytes, tamper  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import FusionRef, GcmOracle  # noqa: E402
from picotls_amd.records import HP_DTYPE, RECORD_DTYPE, TLS_RESULT_DTYPE, RecordBatch  # noqa: E402
from test_chacha_spread_model import EDGE_AADS, EDGE_LENS, EDGE_PARAMS  # noqa: E402
from test_gpu_footprint import HAVE_REF, OK_FILL, _no_w8, _routed, _serial_only  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
WIDTHS = pa.CHACHA_GROUP_WIDTHS


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


@pytest.fixture
def hooks():
    """the ChaCha20 debug hooks back to automatic after the test"""
    yield
    pa.chacha_debug_spread(0, 0, False)
    pa.chacha_debug_force(0, 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _release(*arenas):
    """frees the far allocations (an arena given twice, as in place, once)"""
    for a in {id(a): a for a in arenas if a is not None}.values():
        a.free()


def _ok_tail(d_ok, n, want_ok):
    ok = d_ok.cpu().numpy()
    assert np.array_equal(ok[:n], want_ok), f"ok bytes differ at records {np.flatnonzero(ok[:n] != want_ok)[:8]}"
    assert (ok[n:] == OK_FILL).all(), "ok bytes past the batch were written"


# ------------------------------------------------------------------------------------------------ AES-GCM, unframed


def _seal_batch(ks, recs_ptr, n, in_ptr, aad_ptr, out_ptr, fout):
    pa.seal_batch(ks, recs_ptr, n, in_ptr, aad_ptr, out_ptr, _stream())


def far_check(ref, rng, c, routing, schedule=None, do_seal=_seal_batch, after_seal=None, power=1, both_sides=True):
    """test_gpu_footprint.check with every text arena far: seals case ``c`` from a far input arena into a far output
    arena (in place: one) and compares the far window with fusion's arena and its guards, the alias windows with their
    fill; then opens fusion's arena with three tampered records (a ciphertext, a tag and an AAD bit) from a far input
    into a far output with the same comparisons and the ok bytes exact."""
    b, n = c.b, c.n
    sp = F.batch_spans(b.seal, b.open, b.pt_bytes, b.sealed_bytes, c.in_place)

    def far(arena, which):
        return far_arena(arena, power, spans=sp[which].span, rng=rng, both_sides=both_sides)

    ks = pa.Keyset(c.keys, c.ivs, c.key_size)
    if schedule is not None:
        ks.set_schedule(schedule, allow_variable_time=True)
    want = c.fill.copy()
    ref.run_batch(True, c.keys, c.ivs, c.key_size, b.seal, c.src, c.aad, want, nthreads=8)
    d_aad = dev(c.aad)
    fin = fout = None
    try:
        fin = far(c.src, "seal_in")
        fout = fin if c.in_place else far(c.fill, "sealed")
        d_recs = dev(shifted(b.seal, in_off=fin.D, out_off=fout.D))
        pa.debug_counters(reset=True)
        do_seal(ks, d_recs.data_ptr(), n, fin.ptr, d_aad.data_ptr(), fout.ptr, fout)
        torch.cuda.synchronize()
        _routed(routing, "seal")
        fout.check(want, c.sealed_offs, c.sealed_sizes, "sealed arena against fusion's")
        if not c.in_place:
            fin.check(c.src, b.seal["in_off"], c.lens, "the seal's input arena")
        assert np.array_equal(d_aad.cpu().numpy(), c.aad), "the seal wrote to the AAD arena"
        if after_seal is not None:
            after_seal(fout)
    finally:
        _release(fin, fout)

    bad, badaad, victims, _ = tamper(rng, c, want)
    want_ok = np.ones(n, np.uint8)
    want_ok[victims] = 0
    ref_ok = np.full(n, OK_FILL, np.uint8)
    pfill = bad if c.in_place else rand_bytes(rng, b.pt_bytes)
    ref_back = pfill.copy()
    ref.run_batch(False, c.keys, c.ivs, c.key_size, b.open, bad, badaad, ref_back, ok=ref_ok, nthreads=8)
    assert np.array_equal(ref_ok, want_ok)
    d_badaad, d_ok = dev(badaad), dev(np.full(n + TAIL, OK_FILL, np.uint8))
    fbad = fback = None
    try:
        fbad = far(bad, "sealed")
        fback = fbad if c.in_place else far(pfill, "opened")
        d_recs = dev(shifted(b.open, in_off=fbad.D, out_off=fback.D))
        pa.debug_counters(reset=True)
        pa.open_batch(ks, d_recs.data_ptr(), n, fbad.ptr, d_badaad.data_ptr(), fback.ptr, d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        _routed(routing, "open")
        _ok_tail(d_ok, n, want_ok)
        if c.in_place:
            fback.check(ref_back, c.sealed_offs, c.sealed_sizes, "arena opened in place (a record's last 16 bytes: its tag)")
        else:
            fback.check(ref_back, c.plain_offs, c.plain_sizes, "opened arena against fusion's")
            fbad.check(bad, c.sealed_offs, c.sealed_sizes, "the open's input arena")
    finally:
        _release(fbad, fback)
    ks.free()


def _case(name, rng, in_place):
    s = F.aead_shape(name)
    return s, packed_case(rng, s.lens, s.aads, s.key_size, s.nkeys, in_place, key_idx=s.key_idx)


@LAYOUTS
@pytest.mark.parametrize("name", ["4bit", "lockstep"])
def test_4bit_kernels(ref, name, in_place):
    """255 records of every length 0..254 on the chunked schedule (one key, AES-128) and on the lockstep one (7 keys,
    AES-256): under W8_MIN_RECS records the 4-bit kernels run."""
    rng = np.random.default_rng(8000 + in_place + 2 * (name == "lockstep"))
    s, c = _case(name, rng, in_place)

    def routing(cnt, phase):
        _no_w8(cnt, phase)
        assert (cnt["launches"]["lockstep"] >= 1) == (s.schedule == "lockstep"), f"{phase}: {cnt}"

    far_check(ref, rng, c, routing, schedule=s.schedule)


@LAYOUTS
def test_w8_serial_cut_runs(ref, in_place):
    """2,500 records of the fuzz tests' length mix over 3 keys, AES-256: the W8 serial kernel's cut runs."""
    rng = np.random.default_rng(8010 + in_place)
    far_check(ref, rng, _case("w8_serial", rng, in_place)[1], _serial_only)


@LAYOUTS
def test_w8_serial_whole_runs_in_4_lane_groups(ref, in_place):
    """256 x 130 records of 1100 + U[0, 200) bytes: whole runs in 4-lane groups (the open's line holding)."""
    rng = np.random.default_rng(8020 + in_place)

    def routing(cnt, phase):
        assert cnt["runs"]["w8_g4"] > 0, f"{phase}: {cnt}"

    far_check(ref, rng, _case("w8_g4", rng, in_place)[1], routing)


def _tree_routing(cnt, phase):
    assert cnt["launches"]["w8_tree"] == 1 and cnt["runs"]["w8_tree"] > 0, f"{phase}: {cnt}"


@LAYOUTS
def test_w8_tree_kernel(ref, in_place):
    """256 x 130 records of 8200 + U[0, 200) bytes: the tree kernel, in two far arenas and in place in one."""
    rng = np.random.default_rng(8030 + in_place)
    far_check(ref, rng, _case("w8_tree", rng, in_place)[1], _tree_routing)


def test_w8_tree_kernel_in_place_across_3_times_2_to_the_32(ref):
    """The tree kernel in place in an arena that straddles 3 * 2^32, so that bits 32 and 33 of the offsets are both
    set; the low 32 bits of those offsets land in the alias windows of 0 and of 2^32."""
    rng = np.random.default_rng(8032)
    far_check(ref, rng, _case("w8_tree", rng, True)[1], _tree_routing, power=3)


@LAYOUTS
def test_w8_multi_key_runs(ref, in_place):
    """20,000 records, 17 per connection, of 600 + U[0, 100) bytes: multi-key runs."""
    rng = np.random.default_rng(8040 + in_place)

    def routing(cnt, phase):
        assert cnt["runs"]["w8_mk"] > 0, f"{phase}: {cnt}"

    far_check(ref, rng, _case("w8_mk", rng, in_place)[1], routing)


@LAYOUTS
def test_device_regrouping(ref, in_place):
    """3,000 records over 300 keys in random order, grouped by key on the device: the kernels walk a permutation and the
    ok bytes go through it."""
    rng = np.random.default_rng(8050 + in_place)
    far_check(ref, rng, _case("regroup", rng, in_place)[1], _serial_only)


@LAYOUTS
def test_spread_launch(ref, in_place):
    """600 KiB + 5, 100 and 1 MiB + 1 bytes: the long records in pieces for the spare workgroups. The 1 MiB record lies
    across 2^32, so its pieces lie on both sides (with three records, one of 100 bytes, none lies wholly above)."""
    rng = np.random.default_rng(8060 + in_place)

    def routing(cnt, phase):
        assert cnt["launches"]["spread"] >= 1, f"{phase}: {cnt}"

    far_check(ref, rng, _case("spread", rng, in_place)[1], routing, both_sides=False)


@LAYOUTS
def test_seal_batch_hp_and_hp_mask_batch(ref, in_place):
    """seal_batch_hp on 300 packets of 1185..1215 bytes over 5 keys with sample_off shifted as out_off is, the masks
    against ref.seal_with_hp; then hp_mask_batch reads the same samples from the far sealed arena."""
    rng = np.random.default_rng(8070 + in_place)
    s, c = _case("seal_hp", rng, in_place)
    n, nkeys, rec = c.n, s.nkeys, c.b.seal
    hp_keys = rand_bytes(rng, nkeys * 16)
    sample_in_ct = F.hp_sample_in_ct(n)
    hp_ks = pa.Keyset(hp_keys, np.zeros(nkeys * 12, np.uint8), 16)
    fills = [rand_bytes(rng, 16 * n + TAIL) for _ in range(2)]
    masks = np.zeros(16 * n, np.uint8)
    for i in range(n):
        k, p, ln, a, al = (int(rec[f][i]) for f in ("key_idx", "in_off", "len", "aad_off", "aad_len"))
        _, mask = ref.seal_with_hp(c.keys[16 * k:16 * k + 16].tobytes(), c.ivs[12 * k:12 * k + 12].tobytes(), int(rec["seq"][i]),
                                   c.aad[a:a + al].tobytes(), c.src[p:p + ln].tobytes(), hp_keys[16 * k:16 * k + 16].tobytes(),
                                   int(sample_in_ct[i]))
        masks[16 * i:16 * i + 16] = np.frombuffer(mask, np.uint8)
    held = {}

    def do_seal(ks, recs_ptr, n_, in_ptr, aad_ptr, out_ptr, fout):
        hp = np.zeros(n, HP_DTYPE)
        hp["sample_off"] = rec["out_off"] + sample_in_ct.astype(np.uint64) + np.uint64(fout.D)
        hp["key_idx"] = rec["key_idx"]
        held["hp"], held["masks"] = dev(hp), dev(fills[0])
        pa.seal_batch_hp(ks, recs_ptr, n_, in_ptr, aad_ptr, out_ptr, hp_ks, held["hp"].data_ptr(), held["masks"].data_ptr(), _stream())

    def after_seal(fout):
        for which, d_masks in enumerate((held["masks"], dev(fills[1]))):
            if which == 1:
                pa.hp_mask_batch(hp_ks, held["hp"].data_ptr(), n, fout.ptr, d_masks.data_ptr(), _stream())
                torch.cuda.synchronize()
                fout.check_alias("hp_mask_batch")
            want = fills[which].copy()
            want[:16 * n] = masks
            assert_arena(d_masks.cpu().numpy(), want, 16 * np.arange(n), np.full(n, 16),
                         ("seal_batch_hp", "hp_mask_batch")[which] + " masks")

    def routing(cnt, phase):
        if phase == "seal":
            assert cnt["launches"]["seal_hp"] >= 1, f"{cnt}"

    far_check(ref, rng, c, routing, do_seal=do_seal, after_seal=after_seal)
    hp_ks.free()


# ------------------------------------------------------------------------------------------------ framed TLS records


def _tls_case(t, rng, seal_one, seq_bits):
    """The arenas of F.tls_shape ``t``: the seal's descriptors, payload arena and the wire the reference makes of it
    (over ``wire_fill``); the open's descriptors, a wire with t.special's five records altered, and the plaintext arena
    (over ``pfill``), ok bytes and results that opening it gives. seal_one(key index, seq, aad, text) is the reference's
    ciphertext || tag. Returns a dict."""
    n, v13 = t.n, t.version == 13
    seqs = rng.integers(0, 1 << seq_bits, n, dtype=np.uint64)
    payload = rand_bytes(rng, t.pay_bytes)
    wire_fill, pfill = rand_bytes(rng, t.wire_bytes), rand_bytes(rng, t.text_bytes)

    def pay(i):
        o = int(t.pay_off[i]) + (0 if v13 else 8)
        return payload[o:o + int(t.lens[i])].tobytes()

    def record(i, data, typ, outer=23):
        k, seq, ln = int(t.key_idx[i]), int(seqs[i]), len(data)
        if v13:
            hdr = bytes([outer, 3, 3]) + (ln + 17).to_bytes(2, "big")
            return hdr + seal_one(k, seq, hdr, data + bytes([typ]))
        nonce = payload[int(t.pay_off[i]):int(t.pay_off[i]) + 8].tobytes()
        aad = seq.to_bytes(8, "big") + bytes([typ, 3, 3]) + ln.to_bytes(2, "big")
        return bytes([typ, 3, 3]) + (ln + 24).to_bytes(2, "big") + nonce + seal_one(k, int.from_bytes(nonce, "big"), aad, data)

    seal = np.zeros(n, RECORD_DTYPE)
    seal["in_off"], seal["out_off"], seal["len"], seal["seq"] = t.pay_off, t.wire_off, t.lens, seqs
    seal["key_idx"], seal["flags"] = t.key_idx, t.types
    want_wire = wire_fill.copy()
    for i in range(n):
        rec = record(i, pay(i), int(t.types[i]))
        want_wire[int(t.wire_off[i]):int(t.wire_off[i]) + len(rec)] = np.frombuffer(rec, np.uint8)

    opn = np.zeros(n, RECORD_DTYPE)
    opn["in_off"], opn["out_off"], opn["len"], opn["seq"], opn["key_idx"] = t.wire_off, t.text_off, t.text, seqs, t.key_idx
    wire, back = want_wire.copy(), pfill.copy()
    res = np.zeros(n, TLS_RESULT_DTYPE)
    res["plain_len"], res["content_type"] = t.lens, t.types
    for i in range(n):
        o = int(t.text_off[i])
        back[o:o + int(t.text[i])] = np.frombuffer(pay(i) + (bytes([int(t.types[i])]) if v13 else b""), np.uint8)
    if v13:
        res["status"][(t.lens == 0) & (t.types != 23)] = pa.TLS_UNEXPECTED_MESSAGE
    sp = t.special
    unspecified = [sp["bad_header"], sp["ct"], sp["tag"], sp["hdr"]]  # (where a suite leaves a failed record's output open)

    def put(i, rec):
        wire[int(t.wire_off[i]):int(t.wire_off[i]) + len(rec)] = np.frombuffer(rec, np.uint8)

    def keep_fill(i):
        o = int(t.text_off[i])
        back[o:o + int(t.text[i])] = pfill[o:o + int(t.text[i])]

    def failed(i, status):
        res[i] = (0, 0 if v13 else int(wire[int(t.wire_off[i])]), status, 0)

    if v13:  # an all-zero inner plaintext: it authenticates, is written, and has no content type
        i = sp["zero"]
        put(i, record(i, bytes(int(t.lens[i])), 0))
        back[int(t.text_off[i]):int(t.text_off[i]) + int(t.text[i])] = 0
        res[i] = (0, 0, pa.TLS_UNEXPECTED_MESSAGE, 0)
    # a header the record layer refuses under a tag that verifies: nothing is written
    i = sp["bad_header"]
    if v13:
        put(i, record(i, pay(i), int(t.types[i]), outer=22))
    else:
        wire[int(t.wire_off[i]) + 1] = 2  # (the AAD takes 3, 3 as constants)
    keep_fill(i)
    failed(i, pa.TLS_BAD_HEADER)
    # a ciphertext bit, a tag bit and a header bit (an AAD bit)
    i = sp["ct"]
    at, bit = int(rng.integers(0, int(t.text[i]))), 1 << int(rng.integers(0, 8))
    wire[int(t.wire_off[i]) + t.head + at] ^= bit
    back[int(t.text_off[i]) + at] ^= bit  # (CTR: the plaintext is written all the same)
    failed(i, pa.TLS_BAD_MAC)
    i = sp["tag"]
    wire[int(t.wire_off[i]) + t.head + int(t.text[i]) + int(rng.integers(0, 16))] ^= 0x20
    failed(i, pa.TLS_BAD_MAC)
    i = sp["hdr"]
    wire[int(t.wire_off[i])] ^= 0x04
    if v13:  # (the flipped outer type is a refused header too: the range stays as it was; TLS 1.2 takes any type)
        keep_fill(i)
    failed(i, pa.TLS_BAD_MAC)
    return dict(seal=seal, payload=payload, wire_fill=wire_fill, want_wire=want_wire, open=opn, wire=wire, pfill=pfill, back=back,
                res=res, unspecified=unspecified)


def _far_framed(t, rng, x, ks, sealer, opener, routed, strict):
    """Seals x["payload"] far into a far wire arena and opens x["wire"] far into a far plaintext arena, both compared
    whole. ``routed(phase)`` asserts the kernel family. With ``strict`` a failed record's output is what fusion leaves;
    without, its own output range is left open (include/picotls/mi355x_chacha20.h)."""
    n, sp = t.n, t.spans()
    fin = fout = None
    try:
        fin = far_arena(x["payload"], 1, spans=sp["payload"].span, rng=rng)
        fout = far_arena(x["wire_fill"], 1, spans=sp["wire"].span, rng=rng)
        d_recs = dev(shifted(x["seal"], in_off=fin.D, out_off=fout.D))
        sealer(ks, d_recs.data_ptr(), n, fin.ptr, fout.ptr, _stream())
        torch.cuda.synchronize()
        routed("seal")
        fout.check(x["want_wire"], *sp["wire"].span, "sealed wire against the reference's")
        fin.check(x["payload"], *sp["payload"].span, "the seal's payload arena")
    finally:
        _release(fin, fout)
    rfill = rand_bytes(rng, 8 * n + TAIL)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    fwire = fback = None
    try:
        fwire = far_arena(x["wire"], 1, spans=sp["wire"].span, rng=rng)
        fback = far_arena(x["pfill"], 1, spans=sp["opened"].span, rng=rng)
        d_recs = dev(shifted(x["open"], in_off=fwire.D, out_off=fback.D))
        opener(ks, d_recs.data_ptr(), n, fwire.ptr, fback.ptr, d_ok.data_ptr(), d_res.data_ptr(), _stream())
        torch.cuda.synchronize()
        routed("open")
        want_res = rfill.copy()
        want_res[:8 * n] = x["res"].view(np.uint8)
        assert_arena(d_res.cpu().numpy(), want_res, 8 * np.arange(n), np.full(n, 8), "TLS results")
        _ok_tail(d_ok, n, (x["res"]["status"] == pa.TLS_OK).astype(np.uint8))
        back = x["back"]
        if not strict:
            back, got = back.copy(), fback.arena()
            for i in x["unspecified"]:
                o = int(t.text_off[i])
                back[o:o + int(t.text[i])] = got[o:o + int(t.text[i])]
        fback.check(back, *sp["opened"].span, "opened plaintext arena")
        fwire.check(x["wire"], *sp["wire"].span, "the open's wire arena")
    finally:
        _release(fwire, fback)


@pytest.mark.parametrize("version", [13, 12], ids=["tls13", "tls12"])
def test_framed_tls_records(ref, version):
    """seal_tls_records / open_tls_records (AES-256) and seal_tls12_records / open_tls12_records (AES-128) on 300 records
    of U[0, 3000) payload bytes: wire bytes, ok bytes and results (status, plain_len, content type) exact. The open's
    wire has an all-zero inner plaintext (TLS 1.3) and a header the record layer refuses under a valid tag, so
    tls_unpad_kernel and tls12_check_kernel read out + out_off and in + in_off far, and three records with a ciphertext,
    a tag and a header bit flipped."""
    rng = np.random.default_rng(8100 + version)
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
    ks = pa.Keyset(keys, ivs, key_size)
    pa.debug_counters(reset=True)
    sealer, opener = (pa.seal_tls_records, pa.open_tls_records) if version == 13 else (pa.seal_tls12_records, pa.open_tls12_records)
    _far_framed(t, rng, x, ks, sealer, opener, lambda phase: _routed(_serial_only, phase), strict=True)
    ks.free()


def _chacha_routed(width, launches=1):
    def routed(phase):
        ran = pa.chacha_debug_counters(reset=True)
        print(phase, ran)
        assert ran[width] == launches and sum(ran.values()) == launches, (phase, ran)

    return routed


@pytest.mark.parametrize("width", WIDTHS)
def test_chacha_framed_tls_records(width, hooks):
    """chacha_seal_tls_records / chacha_open_tls_records on the same 300 records, against OpenSSL. A record that fails
    its tag or its header has its own output range left open by the contract; everything else is exact."""
    rng = np.random.default_rng(8120 + width)
    t = F.tls_shape(13)
    keys, ivs = [rng.bytes(32) for _ in range(3)], [rng.bytes(12) for _ in range(3)]

    def seal_one(k, seq, aad, text):
        return R.ossl_seal(keys[k], R.nonce_for(ivs[k], seq), text, aad)

    x = _tls_case(t, rng, seal_one, 62)
    for i in range(0, t.n, 37):  # a subset against the plain-Python restatement too
        o, k, ln = int(t.wire_off[i]), int(t.key_idx[i]), int(t.lens[i])
        hdr = x["want_wire"][o:o + 5].tobytes()
        inner = x["payload"][int(t.pay_off[i]):int(t.pay_off[i]) + ln].tobytes() + bytes([int(t.types[i])])
        assert x["want_wire"][o + 5:o + 22 + ln].tobytes() == R.py_seal(keys[k], R.nonce_for(ivs[k], int(x["seal"]["seq"][i])), inner, hdr)
    ks = pa.ChaChaKeyset(b"".join(keys), b"".join(ivs))
    pa.chacha_debug_force(width, 0)
    pa.chacha_debug_counters(reset=True)
    _far_framed(t, rng, x, ks, pa.chacha_seal_tls_records, pa.chacha_open_tls_records, _chacha_routed(width), strict=False)
    ks.free()


# ------------------------------------------------------------------------------------------------ QUIC packets


def _far_quic(suite, rng, routed):
    """quic_util.every_shape(suite) placed far in both arenas: the seal of the cleartext packets is the reference's
    packets, the open of those restores header || payload with ok all 1 and the reference's results, arenas whole."""
    K, pkts = U.every_shape(suite)
    n, sp = len(pkts), F.quic_spans(pkts)
    ks, hp_ks = K.keysets()
    arena_in, out_fill, back_fill = (rand_bytes(rng, sp[a].size) for a in ("clear", "packets", "opened"))
    want, want_back = out_fill.copy(), back_fill.copy()
    for p, i, o, b in zip(pkts, sp["clear"].offs, sp["packets"].offs, sp["opened"].offs):
        U.put(arena_in, int(i), p.header + p.payload)
        U.put(want, int(o), p.packet)
        U.put(want_back, int(b), p.header + p.payload)
    fin = fout = None
    try:
        fin = far_arena(arena_in, 1, spans=sp["clear"].span, rng=rng)
        fout = far_arena(out_fill, 1, spans=sp["packets"].span, rng=rng)
        d_recs = dev(shifted(U.seal_recs(pkts, sp["clear"].offs, sp["packets"].offs), in_off=fin.D, out_off=fout.D))
        suite.seal(ks, hp_ks, d_recs.data_ptr(), n, fin.ptr, fout.ptr, _stream())
        torch.cuda.synchronize()
        routed("seal")
        fout.check(want, *sp["packets"].span, "sealed packets against the reference's")
        fin.check(arena_in, *sp["clear"].span, "the seal's input arena")
    finally:
        _release(fin, fout)
    rfill = rand_bytes(rng, 16 * n + TAIL)
    d_ok, d_res = dev(np.full(n + TAIL, OK_FILL, np.uint8)), dev(rfill)
    fpk = fback = None
    try:
        fpk = far_arena(want, 1, spans=sp["packets"].span, rng=rng)
        fback = far_arena(back_fill, 1, spans=sp["opened"].span, rng=rng)
        d_recs = dev(shifted(U.open_recs(pkts, sp["packets"].offs, sp["opened"].offs), in_off=fpk.D, out_off=fback.D))
        suite.open(ks, hp_ks, d_recs.data_ptr(), n, fpk.ptr, fback.ptr, d_ok.data_ptr(), d_res.data_ptr(), _stream())
        torch.cuda.synchronize()
        routed("open")
        _ok_tail(d_ok, n, np.ones(n, np.uint8))
        want_res = rfill.copy()
        want_res[:16 * n] = U.want_results(pkts).view(np.uint8)
        assert_arena(d_res.cpu().numpy(), want_res, 16 * np.arange(n), np.full(n, 16), "QUIC results")
        fback.check(want_back, *sp["opened"].span, "opened packets")
        fpk.check(want, *sp["packets"].span, "the open's input arena")
    finally:
        _release(fpk, fback)
    return K, pkts, sp, want, ks, hp_ks


@pytest.mark.parametrize("key_size", [16, 32])
def test_quic_packets(key_size):
    """seal_quic_packets / open_quic_packets on every small shape: the pre-passes read the headers at in + in_off far,
    the batch runs in the W8 serial kernel (above 256 packets), the finish writes the header protection far."""
    from test_gpu_quic_aes import SUITES

    def routed(phase):
        cnt = pa.debug_counters(reset=True)
        print(phase, {kind: {k: int(v) for k, v in d.items() if v} for kind, d in cnt.items()})
        assert cnt["launches"]["w8_serial"] == 1 and cnt["launches"]["w8_tree"] == 0 and cnt["launches"]["chunked"] == 0, (phase, cnt)

    pa.debug_counters(reset=True)
    *_, ks, hp_ks = _far_quic(SUITES[key_size], np.random.default_rng(8200 + key_size), routed)
    ks.free(), hp_ks.free()


@pytest.mark.parametrize("width", WIDTHS)
def test_chacha_quic_packets_and_hp_mask_batch(width, hooks):
    """chacha_seal_quic_packets / chacha_open_quic_packets on every small shape at both forced widths; then
    chacha_hp_mask_batch reads those packets' samples from a far arena."""
    from test_gpu_chacha_quic import S

    rng = np.random.default_rng(8220 + width)
    pa.chacha_debug_force(width, 0)
    pa.chacha_debug_counters(reset=True)
    K, pkts, sp, packets, ks, hp_ks = _far_quic(S, rng, _chacha_routed(width))
    n = len(pkts)
    sample_offs = sp["packets"].parts["sample"][0]
    mfill = rand_bytes(rng, 16 * n + TAIL)
    want = mfill.copy()
    for i, (p, o) in enumerate(zip(pkts, sample_offs)):
        want[16 * i:16 * i + 16] = np.frombuffer(R.ossl_chacha20(K.hps[p.k], packets[int(o):int(o) + 16].tobytes(), bytes(16)), np.uint8)
    fpk = None
    try:
        fpk = far_arena(packets, 1, spans=sp["packets"].span, rng=rng)
        hp = np.zeros(n, HP_DTYPE)
        hp["sample_off"], hp["key_idx"] = sample_offs.astype(np.uint64) + np.uint64(fpk.D), [p.k for p in pkts]
        d_hp, d_masks = dev(hp), dev(mfill)
        pa.chacha_hp_mask_batch(hp_ks, d_hp.data_ptr(), n, fpk.ptr, d_masks.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert_arena(d_masks.cpu().numpy(), want, 16 * np.arange(n), np.full(n, 16), "chacha_hp_mask_batch masks")
        fpk.check(packets, *sp["packets"].span, "chacha_hp_mask_batch's arena")
    finally:
        _release(fpk)
    ks.free(), hp_ks.free()


def test_quiclb_batch():
    """64 connection IDs of every length 7..19, both directions, in_off and out_off far in arenas of their own, against
    the oracle (and fusion where it is shipped)."""
    rng = np.random.default_rng(8300)
    cids, size = F.quiclb_cids()
    sp = F.quiclb_spans()
    key = rng.bytes(16)
    arena, fill = rand_bytes(rng, size), rand_bytes(rng, size)
    want = fill.copy()
    o, fusion = GcmOracle(), FusionRef() if HAVE_REF else None
    for c in cids:
        data = arena[int(c["in_off"]):int(c["in_off"]) + int(c["len"])].tobytes()
        out = o.quiclb(key, data, bool(c["encrypt"]))
        assert fusion is None or fusion.quiclb(key, data, bool(c["encrypt"])) == out
        want[int(c["out_off"]):int(c["out_off"]) + int(c["len"])] = np.frombuffer(out, np.uint8)
    assert {int(c["len"]) for c in cids} == set(range(7, 20)) and {(int(c["len"]), int(c["encrypt"])) for c in cids} >= {
        (ln, e) for ln in range(7, 20) for e in (0, 1)}
    ks = pa.Keyset(key, bytes(12), 16)
    fin = fout = None
    try:
        fin = far_arena(arena, 1, spans=sp["in"].span, rng=rng)
        fout = far_arena(fill, 1, spans=sp["out"].span, rng=rng)
        d_cids = dev(shifted(cids, in_off=fin.D, out_off=fout.D))
        pa.quiclb_batch(ks, d_cids.data_ptr(), len(cids), fin.ptr, fout.ptr, _stream())
        torch.cuda.synchronize()
        fout.check(want, *sp["out"].span, "quiclb output against the oracle's")
        fin.check(arena, *sp["in"].span, "quiclb's input arena")
    finally:
        _release(fin, fout)
    ks.free()


# ------------------------------------------------------------------------------------------------ ChaCha20-Poly1305, unframed


def _chacha_keys(c, nkeys):
    return [c.keys[32 * k:32 * k + 32].tobytes() for k in range(nkeys)], [c.ivs[12 * k:12 * k + 12].tobytes() for k in range(nkeys)]


def chacha_far_check(rng, c, nkeys, routed, py_subset=(), power=1):
    """far_check for the ChaCha20-Poly1305 batch calls, against OpenSSL (records py_subset also against the plain-Python
    restatement). The open's three tampered records get ok = 0; their own output ranges are left open by the contract."""
    b, n = c.b, c.n
    sp = F.batch_spans(b.seal, b.open, b.pt_bytes, b.sealed_bytes, c.in_place)
    keys, ivs = _chacha_keys(c, nkeys)
    want = c.fill.copy()
    R.seal_records(keys, ivs, b.seal, c.src, c.aad, want)
    for i in py_subset:
        r = b.seal[i]
        k, p, o, ln, a, an = (int(r[f]) for f in ("key_idx", "in_off", "out_off", "len", "aad_off", "aad_len"))
        py = R.py_seal(keys[k], R.nonce_for(ivs[k], int(r["seq"])), c.src[p:p + ln].tobytes(), c.aad[a:a + an].tobytes())
        assert want[o:o + ln + 16].tobytes() == py, f"record {i}: OpenSSL and the Python reference differ"
    ks = pa.ChaChaKeyset(c.keys, c.ivs)
    d_aad = dev(c.aad)
    fin = fout = None
    try:
        fin = far_arena(c.src, power, spans=sp["seal_in"].span, rng=rng)
        fout = fin if c.in_place else far_arena(c.fill, power, spans=sp["sealed"].span, rng=rng)
        d_recs = dev(shifted(b.seal, in_off=fin.D, out_off=fout.D))
        pa.chacha_seal_batch(ks, d_recs.data_ptr(), n, fin.ptr, d_aad.data_ptr(), fout.ptr, _stream())
        torch.cuda.synchronize()
        routed("seal")
        fout.check(want, c.sealed_offs, c.sealed_sizes, "sealed arena against OpenSSL's")
        if not c.in_place:
            fin.check(c.src, b.seal["in_off"], c.lens, "the seal's input arena")
    finally:
        _release(fin, fout)

    bad, badaad, victims, _ = tamper(rng, c, want)
    want_ok = np.ones(n, np.uint8)
    want_ok[victims] = 0
    pfill = bad if c.in_place else rand_bytes(rng, b.pt_bytes)
    back = pfill.copy()
    for r in b.seal:  # (in place in_off == out_off: the plaintext back over its ciphertext, the tag kept)
        p, ln = int(r["in_off"]), int(r["len"])
        back[p:p + ln] = c.src[p:p + ln]
    d_badaad, d_ok = dev(badaad), dev(np.full(n + TAIL, OK_FILL, np.uint8))
    fbad = fback = None
    try:
        fbad = far_arena(bad, power, spans=sp["sealed"].span, rng=rng)
        fback = fbad if c.in_place else far_arena(pfill, power, spans=sp["opened"].span, rng=rng)
        d_recs = dev(shifted(b.open, in_off=fbad.D, out_off=fback.D))
        pa.chacha_open_batch(ks, d_recs.data_ptr(), n, fbad.ptr, d_badaad.data_ptr(), fback.ptr, d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        routed("open")
        _ok_tail(d_ok, n, want_ok)
        got = fback.arena()
        for v in victims:
            p, ln = int(b.open["out_off"][v]), int(b.open["len"][v])
            back[p:p + ln] = got[p:p + ln]
        if c.in_place:
            fback.check(back, c.sealed_offs, c.sealed_sizes, "arena opened in place")
        else:
            fback.check(back, c.plain_offs, c.plain_sizes, "opened arena")
            fbad.check(bad, c.sealed_offs, c.sealed_sizes, "the open's input arena")
    finally:
        _release(fbad, fback)
    ks.free()


def _raw_case(rng, recs, pt_bytes, sealed_bytes, aad_bytes, in_place, nkeys=1):
    """A footprint_util.PackedCase of descriptors laid out by hand (``recs``: the seal's)"""
    b = RecordBatch(recs, F.open_of(recs), pt_bytes, sealed_bytes, aad_bytes)
    src = rand_bytes(rng, pt_bytes)
    fill = src if in_place else rand_bytes(rng, sealed_bytes)
    return PackedCase(b, 32, rand_bytes(rng, 32 * nkeys), rand_bytes(rng, 12 * nkeys), src, fill, rand_bytes(rng, aad_bytes), in_place,
                      recs["len"].astype(np.int64))


@pytest.mark.parametrize("width, in_place", [(w, False) for w in WIDTHS] + [(max(WIDTHS), True)])
def test_chacha_forced_widths(width, in_place, hooks):
    """The batch kernels at both forced group widths on test_gpu_chacha's offset batch (80 records, every residue of
    every offset) and records of 1200, 4097 and 16385 bytes; the wide kernel also in place."""
    rng = np.random.default_rng(8400 + width + in_place)
    recs, pt_bytes, sealed_bytes, aad_bytes = F.chacha_offset_recs(in_place)
    recs["seq"] = rng.integers(0, 2**62, len(recs), dtype=np.uint64)
    c = _raw_case(rng, recs, pt_bytes, sealed_bytes, aad_bytes, in_place)
    pa.chacha_debug_force(width, 0)
    pa.chacha_debug_counters(reset=True)
    chacha_far_check(rng, c, 1, _chacha_routed(width), py_subset=list(range(0, 80, 8)) + [80])


def test_chacha_spread_launch(hooks):
    """The spread launch at the piece edges of test_chacha_spread_model (pieces of 1024 bytes from 2048): counters as in
    test_gpu_chacha_spread.test_piece_edges, one launch each for the seal and the open."""
    rng = np.random.default_rng(8450)
    lens = EDGE_LENS
    aads = [EDGE_AADS[i % len(EDGE_AADS)] for i in range(len(lens))]
    b = RecordBatch.build(lens, aads, seqs=rng.integers(0, 2**62, len(lens), dtype=np.uint64))
    c = _raw_case(rng, b.seal, b.pt_bytes, b.sealed_bytes, b.aad_bytes, False)
    plan = pa.chacha_spread_plan(lens, EDGE_PARAMS)
    pieces, nlong = sum(len(p) for p in plan), sum(1 for p in plan if p)
    assert nlong == 26

    def routed(phase):
        got = pa.chacha_debug_spread_counters(reset=True)
        print(phase, got)
        assert got == {"launches": 1, "pieces": pieces, "finished": nlong, "whole": len(lens) - nlong}, (phase, got)

    pa.chacha_debug_spread(EDGE_PARAMS["piece"], EDGE_PARAMS["min_len"], False)
    pa.chacha_debug_force(0, 0)
    pa.chacha_debug_spread_counters(reset=True)
    chacha_far_check(rng, c, 1, routed, py_subset=[0, 9, 10, 13, 18, 24, 27, 35, 36, 38])


# ------------------------------------------------------------------------------------------------ aad_off at its top


def _aad_top_batch(rng, lens):
    """Records of ``lens`` with AADs of 0..40 bytes whose last one ends exactly at byte 2^32 of the AAD arena: the
    descriptors for the reference (aad_off into the small host arena) and for the engine (aad_off below 2^32)."""
    n = len(lens)
    aads = np.arange(n) % 41
    b = RecordBatch.build_offsets(lens, aads, seqs=rng.integers(0, 2**62, n, dtype=np.uint64), in_base=5, out_base=3, aad_base=0)
    top, _ = F.aad_top_offsets(aads)
    assert int(top[-1]) + int(aads[-1]) == 1 << 32
    assert np.array_equal(top.astype(np.int64) - int(top[0]), b.seal["aad_off"].astype(np.int64))
    seal, opn = b.seal.copy(), b.open.copy()
    seal["aad_off"], opn["aad_off"] = top, top
    return b, seal, opn, rand_bytes(rng, int(aads.sum()))


def test_aad_off_top_of_range_aes(ref):
    """300 records (the W8 serial kernel) whose AADs lie in the last bytes below 2^32 of a real AAD arena of 2^32 bytes
    and a guard, aad_off + aad_len == 2^32 for the last: seal bit-exact against fusion, open with ok all 1. An aad_off +
    k that wrapped in 32 bits reads the arena's first 64 KiB, which hold other bytes, and the tag differs."""
    rng = np.random.default_rng(8500)
    n = 300
    b, seal, opn, aad = _aad_top_batch(rng, rng.integers(0, 2000, n))
    keys, ivs = rand_bytes(rng, 32), rand_bytes(rng, 12)
    src, fill, pfill = rand_bytes(rng, b.pt_bytes), rand_bytes(rng, b.sealed_bytes), rand_bytes(rng, b.pt_bytes)
    want, back = fill.copy(), pfill.copy()
    ref.run_batch(True, keys, ivs, 32, b.seal, src, aad, want, nthreads=8)
    ref_ok = np.zeros(n, np.uint8)
    ref.run_batch(False, keys, ivs, 32, b.open, want, aad, back, ok=ref_ok, nthreads=8)
    assert ref_ok.all()
    ks = pa.Keyset(keys, ivs, 32)
    arena = F.AadTopArena(aad, rng)
    try:
        d_seal, d_open, d_in, d_out = dev(seal), dev(opn), dev(src), dev(fill)
        pa.debug_counters(reset=True)
        pa.seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), arena.ptr, d_out.data_ptr(), _stream())
        torch.cuda.synchronize()
        _routed(_serial_only, "seal")
        assert_arena(d_out.cpu().numpy(), want, b.seal["out_off"], b.seal["len"].astype(np.int64) + 16, "sealed arena against fusion's")
        d_back, d_ok = dev(pfill), dev(np.full(n + TAIL, OK_FILL, np.uint8))
        pa.open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), arena.ptr, d_back.data_ptr(), d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        _routed(_serial_only, "open")
        _ok_tail(d_ok, n, np.ones(n, np.uint8))
        assert_arena(d_back.cpu().numpy(), back, b.open["out_off"], b.open["len"], "opened arena against fusion's")
        arena.check_unwritten("seal and open")
    finally:
        arena.free()
    ks.free()


@pytest.mark.parametrize("width", WIDTHS)
def test_aad_off_top_of_range_chacha(width, hooks):
    """The same at both forced ChaCha20-Poly1305 group widths: 100 records, against OpenSSL."""
    rng = np.random.default_rng(8510 + width)
    n = 100
    lens = np.array([0, 1, 63, 64, 65, 255, 1200, 1500, 4097, 333] * 10)
    b, seal, opn, aad = _aad_top_batch(rng, lens)
    key, iv = rng.bytes(32), rng.bytes(12)
    src, fill, pfill = rand_bytes(rng, b.pt_bytes), rand_bytes(rng, b.sealed_bytes), rand_bytes(rng, b.pt_bytes)
    want, back = fill.copy(), pfill.copy()
    R.seal_records([key], [iv], b.seal, src, aad, want)
    for r in b.seal:
        p, ln = int(r["in_off"]), int(r["len"])
        back[p:p + ln] = src[p:p + ln]
    ks = pa.ChaChaKeyset(key, iv)
    pa.chacha_debug_force(width, 0)
    pa.chacha_debug_counters(reset=True)
    arena = F.AadTopArena(aad, rng)
    try:
        d_seal, d_open, d_in, d_out = dev(seal), dev(opn), dev(src), dev(fill)
        pa.chacha_seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), arena.ptr, d_out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert_arena(d_out.cpu().numpy(), want, b.seal["out_off"], b.seal["len"].astype(np.int64) + 16, "sealed arena against OpenSSL's")
        d_back, d_ok = dev(pfill), dev(np.full(n + TAIL, OK_FILL, np.uint8))
        pa.chacha_open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), arena.ptr, d_back.data_ptr(), d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        _chacha_routed(width, 2)("seal and open")
        _ok_tail(d_ok, n, np.ones(n, np.uint8))
        assert_arena(d_back.cpu().numpy(), back, b.open["out_off"], b.open["len"], "opened arena")
        arena.check_unwritten("seal and open")
    finally:
        arena.free()
    ks.free()


# ------------------------------------------------------------------------------------------------ AADs of 64 KiB and more

BIG_AADS = (65535, 65536, 65537, 70001)
HUGE_AAD = (1 << 20) + 5


def _big_aad_recs(rng, cases):
    """Records of (text length, AAD length) in 16-byte slots, the AAD length's bits 16..31 in flags, as
    test_gpu_lifecycle.test_large_aad_batch_via_flags builds them"""
    lens, aads = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    b = RecordBatch.build(lens, 0, seqs=rng.integers(0, 2**62, len(cases), dtype=np.uint64))
    slots = (aads + 15) // 16 * 16
    for recs in (b.seal, b.open):
        recs["aad_off"] = np.concatenate([[0], np.cumsum(slots)[:-1]])
        recs["aad_len"], recs["flags"] = aads & 0xFFFF, aads >> 16
    return b, aads, int(slots.sum())


@pytest.mark.parametrize("path", ["width4", "width16", "spread"])
def test_chacha_large_aad(path, hooks):
    """AADs of 65535, 65536, 65537 and 70,001 bytes over texts of 0, 1200 and 5000 bytes, and one record with an AAD of
    2^20 + 5 bytes, at both forced widths and in a spread launch (texts of 5000 bytes in pieces of 1024): all four
    places that read PTLS_MI355X_RECORD_AAD_LEN. Seal against OpenSSL; an open with one AAD byte beyond offset 65536
    flipped in every record that has one rejects those records and no other."""
    rng = np.random.default_rng(8600 + ["width4", "width16", "spread"].index(path))
    texts = (5000,) if path == "spread" else (0, 1200, 5000)
    cases = [(t, a) for a in BIG_AADS for t in texts] + [(texts[-1] if path == "spread" else 1200, HUGE_AAD)]
    b, aads, aad_bytes = _big_aad_recs(rng, cases)
    n = b.n
    key, iv = rng.bytes(32), rng.bytes(12)
    src, aad = rand_bytes(rng, b.pt_bytes), rand_bytes(rng, aad_bytes)
    fill, pfill = rand_bytes(rng, b.sealed_bytes), rand_bytes(rng, b.pt_bytes)
    want, back = fill.copy(), pfill.copy()
    R.seal_records([key], [iv], b.seal, src, aad, want)  # (reads aad_len | flags << 16)
    for r in b.seal:
        p, ln = int(r["in_off"]), int(r["len"])
        back[p:p + ln] = src[p:p + ln]
    r = b.seal[1]
    assert want[int(r["out_off"]):int(r["out_off"]) + int(r["len"]) + 16].tobytes() == R.py_seal(
        key, R.nonce_for(iv, int(r["seq"])), src[int(r["in_off"]):int(r["in_off"]) + int(r["len"])].tobytes(),
        aad[int(r["aad_off"]):int(r["aad_off"]) + int(aads[1])].tobytes())
    ks = pa.ChaChaKeyset(key, iv)
    if path == "spread":
        pa.chacha_debug_spread(1024, 2048, False)
        pa.chacha_debug_spread_counters(reset=True)
    else:
        pa.chacha_debug_force(int(path[5:]), 0)
        pa.chacha_debug_counters(reset=True)

    def routed(launches):
        if path == "spread":
            got = pa.chacha_debug_spread_counters(reset=True)
            assert got["launches"] == launches and got["finished"] == launches * n and got["whole"] == 0, got
        else:
            _chacha_routed(int(path[5:]), launches)(path)

    d_seal, d_open, d_in, d_aad, d_out = dev(b.seal), dev(b.open), dev(src), dev(aad), dev(fill)
    pa.chacha_seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    routed(1)
    assert_arena(d_out.cpu().numpy(), want, b.seal["out_off"], b.seal["len"].astype(np.int64) + 16, "sealed arena against OpenSSL's")
    badaad = aad.copy()
    victims = np.flatnonzero(aads > 65536)
    for v in victims:  # the AAD's last byte: at offset 65536 or beyond
        badaad[int(b.seal["aad_off"][v]) + int(aads[v]) - 1] ^= 0x01
    for which, (arena, want_ok) in enumerate(((aad, np.ones(n, np.uint8)), (badaad, (aads <= 65536).astype(np.uint8)))):
        d_a, d_back, d_ok = dev(arena), dev(pfill), dev(np.full(n + TAIL, OK_FILL, np.uint8))
        pa.chacha_open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), d_a.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), _stream())
        torch.cuda.synchronize()
        routed(1)
        _ok_tail(d_ok, n, want_ok)
        if which == 0:
            assert_arena(d_back.cpu().numpy(), back, b.open["out_off"], b.open["len"], "opened arena")
    ks.free()


def test_chacha_large_aad_per_record_path():
    """AeadContext.encrypt / decrypt (chacha/host.h splits aadlen into aad_len and flags) with AADs of 70,001 and
    200,000 bytes."""
    rng = np.random.default_rng(8650)
    key, iv = rng.bytes(32), rng.bytes(12)
    enc = pa.aead_new_direct(pa.chacha20poly1305, True, key, iv)
    dec = pa.AeadContext(pa.chacha20poly1305, False, key, iv)
    for ln, an, seq in ((1200, 70001, 5), (0, 70001, 6), (5000, 200000, 2**40), (70000, 200000, 7)):
        pt, aad = rng.bytes(ln), rng.bytes(an)
        want = R.ossl_seal(key, R.nonce_for(iv, seq), pt, aad)
        assert enc.encrypt(pt, seq, aad) == want, (ln, an)
        assert dec.decrypt(want, seq, aad) == pt, (ln, an)
        bad = bytearray(aad)
        bad[an - 1] ^= 0x80
        assert dec.decrypt(want, seq, bytes(bad)) is None, (ln, an)
    enc.free(), dec.free()


def test_chacha_framed_record_flags_high_byte_is_not_aad_length():
    """A framed TLS record's flags is the content type, not AAD length bits: flags = 0x0117 seals as type 0x17 under
    the 5-byte header as AAD, as flags = 0x17 does."""
    rng = np.random.default_rng(8660)
    key, iv = rng.bytes(32), rng.bytes(12)
    recs = np.zeros(2, RECORD_DTYPE)
    recs["len"], recs["flags"], recs["seq"] = (100, 1200), (0x0117, 0x17), (9, 10)
    recs["in_off"], recs["out_off"] = (3, 200), (5, 300)
    payload, fill = rand_bytes(rng, 1500), rand_bytes(rng, 1700)
    want = fill.copy()
    for r in recs:
        p, ln = int(r["in_off"]), int(r["len"])
        hdr = bytes([23, 3, 3]) + (ln + 17).to_bytes(2, "big")
        rec = hdr + R.ossl_seal(key, R.nonce_for(iv, int(r["seq"])), payload[p:p + ln].tobytes() + b"\x17", hdr)
        want[int(r["out_off"]):int(r["out_off"]) + len(rec)] = np.frombuffer(rec, np.uint8)
    ks = pa.ChaChaKeyset(key, iv)
    d_recs, d_in, d_out = dev(recs), dev(payload), dev(fill)
    pa.chacha_seal_tls_records(ks, d_recs.data_ptr(), 2, d_in.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert_arena(d_out.cpu().numpy(), want, recs["out_off"], recs["len"].astype(np.int64) + 22, "sealed wire against OpenSSL's")
    ks.free()


def _w8_big_aad(ref, rng, lens, aads, key_idx, nkeys, routing):
    """A packed batch in which the records with aads >= 65536 carry the length's high bits in flags: sealed against
    fusion (its batch entry reads aad_len alone, so those records are sealed one by one), opened with one of them
    tampered in an AAD byte beyond offset 65536."""
    n = len(lens)
    c = packed_case(rng, lens, aads, 16, nkeys, key_idx=key_idx)
    b = c.b
    big = np.flatnonzero(aads >= 65536)
    for recs in (b.seal, b.open):
        assert np.array_equal(recs["aad_len"], aads & 0xFFFF)
        recs["flags"] = aads >> 16
    want = c.fill.copy()
    small = np.setdiff1d(np.arange(n), big)
    ref.run_batch(True, c.keys, c.ivs, 16, b.seal[small], c.src, c.aad, want, nthreads=8)
    for i in big:
        r = b.seal[i]
        k, p, o, ln, a = (int(r[f]) for f in ("key_idx", "in_off", "out_off", "len", "aad_off"))
        sealed = ref.seal(c.keys[16 * k:16 * k + 16].tobytes(), c.ivs[12 * k:12 * k + 12].tobytes(), int(r["seq"]),
                          c.aad[a:a + int(aads[i])].tobytes(), c.src[p:p + ln].tobytes())
        want[o:o + ln + 16] = np.frombuffer(sealed, np.uint8)
    ks = pa.Keyset(c.keys, c.ivs, 16)
    d_seal, d_open, d_in, d_aad, d_out = dev(b.seal), dev(b.open), dev(c.src), dev(c.aad), dev(c.fill)
    pa.debug_counters(reset=True)
    pa.seal_batch(ks, d_seal.data_ptr(), n, d_in.data_ptr(), d_aad.data_ptr(), d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(routing, "seal")
    assert_arena(d_out.cpu().numpy(), want, c.sealed_offs, c.sealed_sizes, "sealed arena against fusion's")
    victim = int(big[-1])
    badaad = c.aad.copy()
    badaad[int(b.seal["aad_off"][victim]) + int(aads[victim]) - 1] ^= 0x04
    pfill = rand_bytes(rng, b.pt_bytes)
    back = pfill.copy()
    first, total = int(b.seal["in_off"][0]), int(c.lens.sum())  # (byte-adjacent, and the open's output lies as the seal's input)
    back[first:first + total] = c.src[first:first + total]
    want_ok = np.ones(n, np.uint8)
    want_ok[victim] = 0
    d_badaad, d_back, d_ok = dev(badaad), dev(pfill), dev(np.full(n + TAIL, OK_FILL, np.uint8))
    pa.debug_counters(reset=True)
    pa.open_batch(ks, d_open.data_ptr(), n, d_out.data_ptr(), d_badaad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), _stream())
    torch.cuda.synchronize()
    _routed(routing, "open")
    _ok_tail(d_ok, n, want_ok)
    assert_arena(d_back.cpu().numpy(), back, c.plain_offs, c.plain_sizes, "opened arena (the plaintext is written whatever the tag)")
    ks.free()


def test_w8_serial_large_aad(ref):
    """300 records of 1200 bytes, three of them with an AAD of 70,001 bytes: the W8 serial kernel."""
    rng = np.random.default_rng(8700)
    aads = np.full(300, 13)
    aads[[7, 150, 299]] = 70001
    _w8_big_aad(ref, rng, np.full(300, 1200), aads, None, 1, _serial_only)


def test_w8_tree_large_aad(ref):
    """256 x 130 records of 8200 bytes, three of them with an AAD of 70,001 bytes: the tree kernel."""
    rng = np.random.default_rng(8710)
    n = F.WHOLE_RUN_BATCH
    aads = np.full(n, 13)
    aads[[5, n // 2, n - 1]] = 70001
    _w8_big_aad(ref, rng, np.full(n, 8200), aads, None, 1, _tree_routing)


def test_w8_multi_key_large_aad(ref):
    """2,000 records of 650 bytes at 17 per connection, two of them with an AAD of 65,536 bytes: multi-key runs."""
    rng = np.random.default_rng(8720)
    n = 2000
    key_idx = np.arange(n) // 17
    aads = rng.choice([0, 13, 17], n)
    aads[[400, 1603]] = 65536

    def routing(cnt, phase):
        assert cnt["runs"]["w8_mk"] > 0, f"{phase}: {cnt}"

    _w8_big_aad(ref, rng, np.full(n, 650), aads, key_idx, int(key_idx[-1]) + 1, routing)
