"""The far-arena layout of tests/far_util.py, checked without a GPU and without the big allocation, for the descriptor
set of every case of test_gpu_far_offsets.py: the shifted descriptors are the originals plus a multiple of 4096, the
arena straddles its multiple of 2^32 with records on both sides, and every 32-bit misreading of every shifted offset the
descriptors name (text, tag, header, sample) is an address inside the allocation and inside an alias window. That is
what lets the GPU tests tell a narrowed offset by an assertion and not by a fault."""
import numpy as np
import pytest

import far_util as F
from picotls_amd.records import RECORD_DTYPE, RecordBatch

POWERS = (1, 3)


def _aead_cases():
    for name in F.AEAD_SHAPES:
        for in_place in (False, True):
            def spans(name=name, in_place=in_place):
                return F.packed_spans(F.aead_shape(name), in_place)

            yield f"{name}-{'in_place' if in_place else 'packed'}", spans, name != "spread"


def _chacha_cases():
    for in_place in (False, True):
        def spans(in_place=in_place):
            recs, pt_bytes, sealed_bytes, _ = F.chacha_offset_recs(in_place)
            return F.batch_spans(recs, F.open_of(recs), pt_bytes, sealed_bytes, in_place)

        yield f"chacha-widths-{'in_place' if in_place else 'apart'}", spans, True

    def spread():
        from test_chacha_spread_model import EDGE_AADS, EDGE_LENS

        b = RecordBatch.build(EDGE_LENS, [EDGE_AADS[i % len(EDGE_AADS)] for i in range(len(EDGE_LENS))])
        return F.batch_spans(b.seal, b.open, b.pt_bytes, b.sealed_bytes, False)

    yield "chacha-spread", spread, True


def _quic_cases():
    def aes(size):
        from test_gpu_quic_aes import SUITES
        import quic_util as U

        return F.quic_spans(U.every_shape(SUITES[size])[1])

    def chacha():
        from test_gpu_chacha_quic import S
        import quic_util as U

        return F.quic_spans(U.every_shape(S)[1])

    yield "quic-aes128", lambda: aes(16), True
    yield "quic-aes256", lambda: aes(32), True
    yield "quic-chacha20", chacha, True


CASES = [*_aead_cases(), *_chacha_cases(), ("tls13", lambda: F.tls_shape(13).spans(), True),
         ("tls12", lambda: F.tls_shape(12).spans(), True), *_quic_cases(), ("quiclb", F.quiclb_spans, True)]


@pytest.mark.parametrize("name, spans, both_sides", CASES, ids=[c[0] for c in CASES])
def test_every_case_layout(name, spans, both_sides):
    for arena, sp in spans().items():
        for power in POWERS:
            lay = F.far_layout(sp.size, power, spans=sp.span, both_sides=both_sides)
            what = (name, arena, power)
            assert lay.D % 4096 == 0 and lay.h % 4096 == 0 and lay.D + lay.h == power << 32, what
            recs = np.zeros(len(sp.offs), RECORD_DTYPE)
            recs["in_off"], recs["out_off"] = sp.offs, sp.offs
            far = F.shifted(recs, in_off=lay.D, out_off=lay.D)
            assert np.array_equal(far["in_off"] - np.uint64(lay.D), recs["in_off"]), what
            assert np.array_equal(far["out_off"] - np.uint64(lay.D), recs["out_off"]), what
            for f in ("seq", "aad_off", "len", "key_idx", "aad_len", "flags"):
                assert np.array_equal(far[f], recs[f]), what
            assert ((far["in_off"] % 128) == (recs["in_off"] % 128)).all(), what
            # the arena straddles power * 2^32: a record's bytes cross it, records lie wholly below and wholly above
            below, crossing, above = F.split_of(lay.h, sp.span)
            assert crossing >= 1 and (below >= 1 and above >= 1 if both_sides else below + above >= 1), (what, below, crossing, above)
            first, end = sp.offs + lay.D, sp.offs + sp.sizes + lay.D
            assert ((first < power << 32) & (end > power << 32)).sum() == crossing, what
            assert power > 1 or (first >= 1 << 31).all(), what
            # the allocation holds every window, and the windows do not overlap
            wins = lay.alias_windows + [lay.far_window]
            assert wins[0][0] == 0 and wins[-1][1] == lay.alloc_bytes and lay.alloc_bytes == (power << 32) + sp.size + 2 * lay.guard
            assert all(a[1] <= b[0] for a, b in zip(wins, wins[1:])), what
            assert lay.ptr_at + lay.D - lay.guard == lay.far_window[0], what
            F.check_images(lay, sp.offs, sp.sizes)
            for part, (offs, sizes) in sp.parts.items():
                F.check_images(lay, offs, sizes)


def test_images_of_a_narrowed_offset_land_in_the_alias_window():
    """The two mutations the far tests were shown to catch: out_off narrowed to 32 bits at a store. At 2^32 a record at
    or above the boundary is stored into alias window 0 at its own arena offset; at 3 * 2^32 every record is."""
    sp = F.packed_spans(F.aead_shape("4bit"), False)["sealed"]
    for power in POWERS:
        lay = F.far_layout(sp.size, power, spans=sp.span)
        zero_ext, sign_ext = F.images32(sp.offs + lay.D)
        lo0 = lay.alias_windows[0][0] + lay.guard  # where arena offset 0 lies in alias window 0
        above = sp.offs >= lay.h
        assert np.array_equal(lay.ptr_at + zero_ext[above], lo0 + sp.offs[above])
        assert np.array_equal(lay.ptr_at + sign_ext, lo0 + sp.offs)
        if power == 1:  # below 2^32 the low 32 bits are the offset itself
            assert np.array_equal(zero_ext[~above], sp.offs[~above] + lay.D)
        else:
            lo1 = lay.alias_windows[1][0] + lay.guard
            assert np.array_equal(lay.ptr_at + zero_ext[~above], lo1 + sp.offs[~above])


def test_layout_refuses_an_arena_nothing_crosses():
    offs, sizes = np.array([0, 5000]), np.array([100, 100])
    with pytest.raises(AssertionError):
        F.far_layout(8192, 1, spans=(offs, sizes))
    with pytest.raises(AssertionError):  # one record crosses 4096, none lies wholly above
        F.far_layout(8192, 1, spans=(np.array([0, 4000]), np.array([100, 200])))
    assert F.far_layout(8192, 1, spans=(np.array([0, 4000]), np.array([100, 200])), both_sides=False).h == 4096


def test_aad_top_of_range_layout():
    """The AAD arena of the aad_off tests: the last AAD ends exactly at byte 2^32, the others sit just below it, and a
    32-bit aad_off + k that wrapped reads the first 64 KiB of the arena, which the tests fill with other bytes."""
    for n in (100, 300):
        offs, lens = F.aad_top_offsets(np.arange(n) % 41)
        assert int(offs[-1]) + int(lens[-1]) == 1 << 32 and lens[-1] > 0
        assert (offs[1:] == offs[:-1] + lens[:-1]).all() and (offs < 1 << 32).all() and offs.dtype == np.uint32
        ends = offs.astype(np.int64) + lens
        wrapped = ends & 0xFFFFFFFF  # the end of the last AAD, computed in 32 bits
        assert wrapped[-1] == 0 and (ends[:-1] < 1 << 32).all()
        assert int(offs[0]) > F.AAD_ALIAS_BYTES
