"""Arenas at byte offsets of 2^31 and beyond (test_far_util.py on the CPU, test_gpu_far_offsets.py on the GPU).

include/picotls/mi355x.h gives in_off, out_off and sample_off 64 bits. A kernel that narrowed one of them to 32 bits
would pass every test whose arenas start at offset 0 and corrupt memory only for callers with arenas of real size. Here
the arena of a small case is placed ``D`` bytes behind the pointer the engine is given, ``D`` chosen so that the arena
straddles a multiple of 2^32: ``D = power * 2^32 - h``, with ``h`` about half the arena's size and a multiple of 4096.
About half of the records then lie below the boundary and half at or above it, and one record's bytes cross it. ``D``
is a multiple of 4096, so every record keeps its residues mod 16, 64 and 128 and the engine routes it as it does at
offset 0.

The allocation is real and contiguous from ``ptr - h - guard`` to ``ptr + D + size + guard``, so every 32-bit misreading
of a shifted offset (its low 32 bits, zero- or sign-extended) is an address inside memory the test owns: nothing faults,
an assertion fails. Those images fall into the *alias windows*, ``[ptr + j * 2^32 - h - guard, ... + size + 2 * guard)``
for j below ``power``, which are filled with random bytes and must come back as they were; the arena itself with its
guards is the *far window* (the alias window of j == power). Everything between the windows is uninitialised and never
touched by the host.

The layout arithmetic (FarLayout, far_layout, images32, check_images) needs numpy only; FarArena makes the allocation."""
from dataclasses import dataclass

import numpy as np

from footprint_util import assert_arena, rand_bytes

GUARD = 4096
PAGE = 4096


@dataclass(frozen=True)
class FarLayout:
    """Where an arena of ``size`` bytes and its windows lie. ``ptr_at`` and the windows are offsets into the
    allocation; D is the shift of the descriptors' offsets, relative to the pointer the engine is given."""

    size: int
    power: int
    guard: int
    h: int

    @property
    def D(self) -> int:
        return (self.power << 32) - self.h

    @property
    def ptr_at(self) -> int:
        return self.h + self.guard

    @property
    def alloc_bytes(self) -> int:
        return self.ptr_at + self.D + self.size + self.guard

    def window(self, j: int):
        """[begin, end) of the window of boundary j * 2^32 in the allocation: guard || arena image || guard"""
        lo = self.ptr_at + (j << 32) - self.h - self.guard
        return lo, lo + self.size + 2 * self.guard

    @property
    def far_window(self):
        return self.window(self.power)

    @property
    def alias_windows(self):
        return [self.window(j) for j in range(self.power)]


def _spans(spans):
    offs, sizes = (np.asarray(x).astype(np.int64) for x in spans)
    assert offs.shape == sizes.shape and offs.ndim == 1
    return offs, sizes


def split_of(h: int, spans):
    """(records wholly below h, records whose bytes cross h, records wholly at or above h) of the unshifted spans"""
    offs, sizes = _spans(spans)
    ends = offs + sizes
    below, above = (ends <= h) & (sizes > 0), (offs >= h) & (sizes > 0)
    crossing = (offs < h) & (ends > h)
    return int(below.sum()), int(crossing.sum()), int(above.sum())


def far_layout(size: int, power: int = 1, guard: int = GUARD, spans=None, both_sides: bool = True) -> FarLayout:
    """The layout of an arena of ``size`` bytes around power * 2^32. ``spans`` = (offsets, sizes) of the records' byte
    ranges in the arena: h is then the multiple of 4096 nearest size / 2 that a record's bytes cross and that has
    records wholly on each side (a packed arena gives this at the first try), and it is an error if there is none.
    ``both_sides=False`` asks for a record wholly on one side only: the spread launch's three records, of which the
    middle one has 100 bytes, have no such multiple, and there the long record whose pieces lie on both sides is the
    point. Without spans h is size / 2 rounded to 4096."""
    size = int(size)
    assert size > 0 and power >= 1 and guard % PAGE == 0 and guard > 0
    mid = (size // 2 + PAGE // 2) // PAGE * PAGE
    if spans is None:
        return FarLayout(size, power, guard, mid)
    for h in sorted(range(PAGE, size, PAGE), key=lambda x: (abs(x - mid), x)):
        below, crossing, above = split_of(h, spans)
        if crossing and (below and above if both_sides else below or above):
            return FarLayout(size, power, guard, h)
    raise AssertionError(f"no multiple of {PAGE} inside an arena of {size} bytes is crossed by a record with records on both sides")


def shifted(recs: np.ndarray, **shifts) -> np.ndarray:
    """A copy of the descriptors with D added to the named 64-bit offset fields: shifted(recs, in_off=D1, out_off=D2)"""
    out = recs.copy()
    for field, d in shifts.items():
        assert out.dtype[field] == np.dtype("<u8"), field
        out[field] = recs[field] + np.uint64(d)
    return out


def images32(off):
    """The two 32-bit misreadings of a 64-bit offset: its low 32 bits zero-extended and sign-extended"""
    z = np.asarray(off).astype(np.int64) & 0xFFFFFFFF
    return z, np.where(z >= 1 << 31, z - (1 << 32), z)


def check_images(lay: FarLayout, offs, sizes) -> None:
    """For every unshifted byte range [off, off + size) of the arena: shifted by D it lies in the far window, and both
    32-bit images of its shifted offset (of its first byte, of its last byte, and the first byte's image plus the size,
    as a narrowed base with an added lane offset gives) are either the true address or lie in the arena image of an alias
    window; all of them inside the allocation."""
    offs, sizes = _spans((offs, sizes))
    assert (offs >= 0).all() and (offs + sizes <= lay.size).all(), "a range outside the arena"
    far_lo, far_hi = lay.far_window
    true_first = lay.ptr_at + lay.D + offs
    assert (true_first >= far_lo + lay.guard).all() and (true_first + sizes <= far_hi - lay.guard).all()
    last = offs + np.maximum(sizes, 1) - 1
    for byte, add in ((offs, 0), (last, 0), (offs, np.maximum(sizes, 1) - 1)):
        for img in images32(byte + lay.D):
            at = lay.ptr_at + img + add
            true = lay.ptr_at + lay.D + byte + add
            assert (at >= 0).all() and (at < lay.alloc_bytes).all(), "a 32-bit image outside the allocation"
            inside = at == true
            for lo, hi in lay.alias_windows:
                inside |= (at >= lo + lay.guard) & (at < hi - lay.guard)
            assert inside.all(), f"32-bit images outside the alias windows: ranges {np.flatnonzero(~inside)[:8]}"


class FarArena:
    """A device allocation of lay.alloc_bytes with the far window holding guard || host_bytes || guard and every alias
    window random bytes. ``ptr`` is the pointer to give the engine, ``D`` the shift of the offsets."""

    def __init__(self, host_bytes: np.ndarray, lay: FarLayout, rng):
        import torch

        host_bytes = np.ascontiguousarray(host_bytes).view(np.uint8).reshape(-1)
        assert host_bytes.size == lay.size
        self.lay, self.D = lay, lay.D
        self.alloc = torch.empty(lay.alloc_bytes + PAGE, dtype=torch.uint8, device="cuda:0")
        self._skew = -self.alloc.data_ptr() % PAGE  # (the windows on page boundaries, as an arena at offset 0 is)
        self.ptr = self.alloc.data_ptr() + self._skew + lay.ptr_at
        g = lay.guard
        self.far_fill = np.concatenate([rand_bytes(rng, g), host_bytes, rand_bytes(rng, g)])
        self.alias_fill = [rand_bytes(rng, lay.size + 2 * g) for _ in lay.alias_windows]
        for win, fill in zip(lay.alias_windows + [lay.far_window], self.alias_fill + [self.far_fill]):
            self._slice(win).copy_(torch.from_numpy(fill))

    def _slice(self, win):
        return self.alloc[self._skew + win[0]:self._skew + win[1]]

    def arena(self) -> np.ndarray:
        """The arena as it is on the device now"""
        g = self.lay.guard
        return self._slice(self.lay.far_window).cpu().numpy()[g:-g]

    def check(self, want: np.ndarray, offs, sizes, what: str) -> None:
        """Reads both kinds of window back whole: the alias windows are as they were filled, the far window is its guards
        around ``want`` (the reference's arena; offs / sizes name the records in a failure's message)."""
        self.check_alias(what)
        g = self.lay.guard
        got = self._slice(self.lay.far_window).cpu().numpy()
        assert np.array_equal(got[:g], self.far_fill[:g]), f"{what}: the guard below the far arena was written"
        assert np.array_equal(got[-g:], self.far_fill[-g:]), f"{what}: the guard above the far arena was written"
        assert_arena(got[g:-g], np.ascontiguousarray(want).view(np.uint8).reshape(-1), offs, sizes, f"{what} (far window)")

    def check_alias(self, what: str) -> None:
        """Every alias window is as it was filled"""
        g = self.lay.guard
        for j, (win, fill) in enumerate(zip(self.lay.alias_windows, self.alias_fill)):
            got = self._slice(win).cpu().numpy()
            if not np.array_equal(got, fill):
                p = np.flatnonzero(got != fill)
                raise AssertionError(f"{what}: the alias window of {j} * 2^32 (where the 32-bit images of the far offsets lie) was "
                                     f"written: {p.size} bytes, the first at arena offset {int(p[0]) - g}, the last at {int(p[-1]) - g}")

    def free(self) -> None:
        import torch

        self.alloc = None
        torch.cuda.empty_cache()


def far_arena(host_bytes: np.ndarray, shift: int = 1, guard: int = GUARD, spans=None, rng=None, both_sides: bool = True) -> FarArena:
    """``host_bytes`` placed so that it straddles shift * 2^32 bytes behind the pointer the engine gets. The result has
    the allocation (``alloc``), that pointer (``ptr``) and the offset shift (``D``). With ``spans`` (the records' unshifted
    offsets and sizes) the straddle and both-sides conditions are asserted (far_layout)."""
    lay = far_layout(np.asarray(host_bytes).size, shift, guard, spans, both_sides)
    return FarArena(host_bytes, lay, rng if rng is not None else np.random.default_rng(lay.h + shift))


# ------------------------------------------------------------------------------------------------ the cases' shapes
# Numpy only, so that test_far_util.py can check every case's descriptors without a GPU. A case's far arenas are each
# described by a Spans: the arena's size, the records' whole footprints in it (what far_layout's straddle condition is
# asked of) and the byte ranges a descriptor names inside them (text, tag, header, sample).


@dataclass
class Spans:
    size: int
    offs: np.ndarray
    sizes: np.ndarray
    parts: dict

    def __init__(self, size, offs, sizes, **parts):
        self.size, (self.offs, self.sizes) = int(size), _spans((offs, sizes))
        self.parts = {k: _spans(v) for k, v in parts.items()}

    @property
    def span(self):
        return self.offs, self.sizes


@dataclass
class AeadShape:
    """Arguments of footprint_util.packed_case, and the schedule to set"""

    lens: np.ndarray
    aads: np.ndarray
    key_size: int
    nkeys: int = 1
    key_idx: np.ndarray = None
    schedule: str = None


WHOLE_RUN_BATCH = 256 * 130  # (test_gpu_footprint.py: the smallest batches with whole runs)
EXTRA_CHACHA_LENS = (1200, 4097, 16385)


def aead_shape(name: str) -> AeadShape:
    """The smallest shape test_gpu_footprint.py found for each AES-GCM kernel family"""
    rng = np.random.default_rng(7100 + sum(name.encode()))
    if name in ("4bit", "lockstep"):
        nkeys = 1 if name == "4bit" else 7
        return AeadShape(np.arange(255), np.arange(255) % 41, 16 if name == "4bit" else 32, nkeys,
                         np.sort(rng.integers(0, nkeys, 255)) if nkeys > 1 else None, "chunked" if name == "4bit" else "lockstep")
    if name == "w8_serial":
        from test_gpu_fuzz import _lengths

        n = 2500
        return AeadShape(_lengths(rng, n), rng.integers(0, 41, n), 32, 3, np.sort(rng.integers(0, 3, n)))
    if name == "w8_g4":
        n = WHOLE_RUN_BATCH
        return AeadShape(1100 + rng.integers(0, 200, n), rng.choice([0, 13, 17], n), 16)
    if name == "w8_tree":
        n = WHOLE_RUN_BATCH
        return AeadShape(8200 + rng.integers(0, 200, n), np.full(n, 13), 16)
    if name == "w8_mk":
        n = 20000
        key_idx = np.arange(n) // 17
        return AeadShape(600 + rng.integers(0, 100, n), rng.choice([0, 13, 17], n), 16, int(key_idx[-1]) + 1, key_idx)
    if name == "regroup":
        n = 3000
        return AeadShape(rng.integers(0, 5000, n), rng.integers(0, 41, n), 32, 300, rng.integers(0, 300, n))
    if name == "spread":
        return AeadShape(np.array([(600 << 10) + 5, 100, (1 << 20) + 1]), np.array([13, 5, 21]), 32)
    if name == "seal_hp":
        n = 300
        return AeadShape(rng.integers(1185, 1216, n), rng.integers(8, 30, n), 16, 5, np.sort(rng.integers(0, 5, n)))
    raise KeyError(name)


AEAD_SHAPES = ("4bit", "lockstep", "w8_serial", "w8_g4", "w8_tree", "w8_mk", "regroup", "spread", "seal_hp")


def batch_spans(seal: np.ndarray, opn: np.ndarray, pt_bytes: int, sealed_bytes: int, in_place: bool) -> dict:
    """The far arenas of an unframed seal and open: "seal_in" (plaintext), "sealed" (the seal's output, the open's
    input) and "opened". In place all three are the sealed arena."""
    lens = seal["len"].astype(np.int64)
    o = seal["out_off"].astype(np.int64)
    sealed = Spans(sealed_bytes, o, lens + 16, text=(o, lens), tag=(o + lens, np.full(len(lens), 16)))
    if in_place:
        return {"seal_in": sealed, "sealed": sealed, "opened": sealed}
    return {"seal_in": Spans(pt_bytes, seal["in_off"], lens, text=(seal["in_off"], lens)), "sealed": sealed,
            "opened": Spans(pt_bytes, opn["out_off"], lens, text=(opn["out_off"], lens))}


def packed_spans(shape: AeadShape, in_place: bool) -> dict:
    """batch_spans of footprint_util.packed_case(rng, shape.lens, shape.aads, ..., in_place): the offsets follow from the
    lengths alone"""
    from footprint_util import AAD_BASE, IN_BASE, OUT_BASE
    from picotls_amd.records import RecordBatch

    b = RecordBatch.build_offsets(shape.lens, shape.aads, in_base=IN_BASE, out_base=OUT_BASE, aad_base=AAD_BASE, in_place=in_place)
    return batch_spans(b.seal, b.open, b.pt_bytes, b.sealed_bytes, in_place)


def hp_sample_in_ct(n: int) -> np.ndarray:
    """seal_batch_hp's samples: where in its record's ciphertext each starts (QUIC: 4 - pn_len)"""
    return 4 - np.random.default_rng(7190).integers(1, 5, n)


def chacha_offset_recs(in_place: bool = False):
    """test_gpu_chacha._offset_batch() (80 records, every residue mod 16 of in, out and aad offsets) and one record each
    of EXTRA_CHACHA_LENS bytes behind them, as the seal's descriptors; the arena sizes (plaintext, sealed, AAD)"""
    from picotls_amd.records import RECORD_DTYPE
    from test_gpu_chacha import _offset_batch

    base, in_bytes, out_bytes, aad_bytes = _offset_batch()
    recs = np.zeros(len(base) + len(EXTRA_CHACHA_LENS), RECORD_DTYPE)
    recs[:len(base)] = base
    for i, n in enumerate(EXTRA_CHACHA_LENS, len(base)):
        r = recs[i]
        r["len"], r["aad_len"], r["seq"] = n, 13, 1000 + i
        r["in_off"], r["out_off"], r["aad_off"] = in_bytes + 3, out_bytes + 9, aad_bytes + 5
        in_bytes, out_bytes, aad_bytes = in_bytes + 3 + n + 32, out_bytes + 9 + n + 16 + 32, aad_bytes + 5 + 13 + 32
    if in_place:
        recs["in_off"], in_bytes = recs["out_off"], out_bytes
    return recs, in_bytes, out_bytes, aad_bytes


def open_of(seal: np.ndarray) -> np.ndarray:
    opn = seal.copy()
    opn["in_off"], opn["out_off"] = seal["out_off"], seal["in_off"]
    return opn


@dataclass
class TlsShape:
    """n framed records: payloads of U[0, 3000) bytes over three connections, byte-adjacent in every arena from odd bases.
    ``head`` bytes of the wire record lie in front of the ciphertext; ``text`` is the ciphertext's length (TLS 1.3: the
    payload and its inner content type)."""

    version: int
    lens: np.ndarray
    types: np.ndarray
    key_idx: np.ndarray
    head: int
    text: np.ndarray
    pay_off: np.ndarray   # the seal's input: TLS 1.3 the payload, TLS 1.2 explicit nonce || payload
    pay_size: np.ndarray
    wire_off: np.ndarray
    text_off: np.ndarray  # the open's output
    pay_bytes: int
    wire_bytes: int
    text_bytes: int
    special: dict         # record indices: zero (TLS 1.3: all-zero inner plaintext), bad_header, ct, tag, hdr

    @property
    def n(self):
        return len(self.lens)

    def spans(self) -> dict:
        w, t = self.wire_off, self.text
        return {"payload": Spans(self.pay_bytes, self.pay_off, self.pay_size, text=(self.pay_off + (self.pay_size - self.lens), self.lens)),
                "wire": Spans(self.wire_bytes, w, self.head + t + 16, header=(w, np.full(self.n, 5)), text=(w + self.head, t),
                              tag=(w + self.head + t, np.full(self.n, 16))),
                "opened": Spans(self.text_bytes, self.text_off, t, text=(self.text_off, t))}


def tls_shape(version: int, n: int = 300) -> TlsShape:
    rng = np.random.default_rng(7200 + version)
    lens = rng.integers(0, 3000, n)
    types = rng.choice([21, 22, 23], n)
    special = dict(zip(("zero", "bad_header", "ct", "tag", "hdr"), (int(x) for x in rng.choice(n, 5, replace=False))))
    for i in special.values():
        lens[i] = max(int(lens[i]), 40)
    lens[:3] = (0, 1, 2999)  # (an empty record among the others; not one of the special ones, or it is overwritten above)
    for i in special.values():
        lens[i] = max(int(lens[i]), 40)
    head = 5 if version == 13 else 13
    text = lens + 1 if version == 13 else lens
    pay_size = lens if version == 13 else lens + 8

    def packed(base, sizes):
        off = base + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        return off, int(off[-1] + sizes[-1]) + 64

    pay_off, pay_bytes = packed(5, pay_size)
    wire_off, wire_bytes = packed(3, head + text + 16)
    text_off, text_bytes = packed(7, text)
    return TlsShape(version, lens, types, np.arange(n) * 3 // n, head, text, pay_off, pay_size, wire_off, text_off, pay_bytes,
                    wire_bytes, text_bytes, special)


def quic_spans(pkts) -> dict:
    """every packet of a quic_util case placed as quic_util.place does, at rotating residues: the cleartext arena
    (header || payload), the packet arena (+ 16) and the opened arena; the samples' ranges in the packet arena"""
    from quic_util import place

    n = len(pkts)
    clear = np.array([len(p.header) + len(p.payload) for p in pkts])
    hdr = np.array([len(p.header) for p in pkts])
    pn = np.array([p.pn_len for p in pkts])
    in_offs, in_size = place(clear, [(3 * i) % 16 for i in range(n)])
    out_offs, out_size = place(clear + 16, [(5 * i + 1) % 16 for i in range(n)])
    back_offs, back_size = place(clear, [(7 * i + 2) % 16 for i in range(n)])
    in_offs, out_offs, back_offs = (np.asarray(x, np.int64) for x in (in_offs, out_offs, back_offs))
    return {"clear": Spans(in_size, in_offs, clear, header=(in_offs, hdr), text=(in_offs + hdr, clear - hdr)),
            "packets": Spans(out_size, out_offs, clear + 16, header=(out_offs, hdr), text=(out_offs + hdr, clear - hdr),
                             tag=(out_offs + clear, np.full(n, 16)), sample=(out_offs + hdr - pn + 4, np.full(n, 16))),
            "opened": Spans(back_size, back_offs, clear, header=(back_offs, hdr), text=(back_offs + hdr, clear - hdr))}


QUICLB_SLOT = 64


def quiclb_cids():
    """64 connection IDs, every length 7 .. 19 in rotation and both directions, each in a 64-byte slot of its arena at
    an odd offset; the CID in the middle lies across the slot boundary at 4096 bytes, which the arenas straddle 2^32 at"""
    from picotls_amd.records import CID_DTYPE

    n = 64
    cids = np.zeros(n, CID_DTYPE)
    for i in range(n):
        ln = 7 + i % 13
        off = i * 2 * QUICLB_SLOT + (i % 5)
        if i == n // 2:
            off = PAGE - 3
        cids[i] = (off, off + 9 if i != n // 2 else PAGE - 5, 0, ln, (i // 13) & 1, 0)
    size = n * 2 * QUICLB_SLOT
    assert size == 2 * PAGE
    return cids, size


def quiclb_spans() -> dict:
    cids, size = quiclb_cids()
    return {"in": Spans(size, cids["in_off"], cids["len"], text=(cids["in_off"], cids["len"])),
            "out": Spans(size, cids["out_off"], cids["len"], text=(cids["out_off"], cids["len"]))}


# ------------------------------------------------------------------------------------------------ aad_off at its top
AAD_ALIAS_BYTES = 64 << 10


def aad_top_offsets(aad_lens):
    """aad_off of AADs of these lengths packed so that the last one ends exactly at byte 2^32 of the AAD arena (uint32,
    as the descriptor holds them), and the lengths"""
    lens = np.asarray(aad_lens).astype(np.int64)
    assert lens[-1] > 0
    offs = (1 << 32) - int(lens.sum()) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return offs.astype(np.uint32), lens


class AadTopArena:
    """An AAD arena of 2^32 + guard bytes, a real allocation: ``aad`` (the records' AADs back to back) lies in its last
    bytes below 2^32, random bytes around it, and the first AAD_ALIAS_BYTES, where an aad_off + k that wrapped in 32 bits
    reads, hold other random bytes. ``base`` is where aad[0] lies in the arena."""

    def __init__(self, aad: np.ndarray, rng, guard: int = GUARD):
        import torch

        self.base = (1 << 32) - aad.size
        self.alloc = torch.empty((1 << 32) + guard, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.alloc.data_ptr()
        self.alias = rand_bytes(rng, AAD_ALIAS_BYTES)
        self.top = np.concatenate([rand_bytes(rng, guard), aad, rand_bytes(rng, guard)])
        self.alloc[:AAD_ALIAS_BYTES].copy_(torch.from_numpy(self.alias))
        self._top().copy_(torch.from_numpy(self.top))

    def _top(self):
        return self.alloc[(1 << 32) + GUARD - self.top.size:(1 << 32) + GUARD]

    def check_unwritten(self, what: str) -> None:
        assert np.array_equal(self.alloc[:AAD_ALIAS_BYTES].cpu().numpy(), self.alias), f"{what}: the AAD arena's first bytes were written"
        assert np.array_equal(self._top().cpu().numpy(), self.top), f"{what}: the AAD arena's last bytes were written"

    def free(self) -> None:
        import torch

        self.alloc = None
        torch.cuda.empty_cache()
