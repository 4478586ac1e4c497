"""Helpers of the write-footprint tests (test_footprint_ref.py on the CPU, test_gpu_footprint.py on the GPU): batches of
byte-adjacent records (RecordBatch.build_offsets) in arenas pre-filled with random bytes, and a whole-arena comparison
that says where the first differing byte lies."""
from dataclasses import dataclass

import numpy as np

from picotls_amd.records import RecordBatch

IN_BASE, OUT_BASE, AAD_BASE = 5, 3, 1  # odd bases: no record of a packed arena starts on a 16-byte boundary by design
TAIL = 64  # bytes of fill after the n ok bytes / results / masks of a call


def rand_bytes(rng, n: int) -> np.ndarray:
    return np.frombuffer(rng.bytes(max(int(n), 1)), np.uint8).copy()


def span_mask(offs, sizes, total: int) -> np.ndarray:
    """True for the bytes of [offs[i], offs[i] + sizes[i]) (disjoint spans)."""
    d = np.zeros(total + 1, np.int8)  # (disjoint spans: the running sum stays 0 or 1)
    np.add.at(d, np.asarray(offs, np.int64), 1)
    np.add.at(d, np.asarray(offs, np.int64) + np.asarray(sizes, np.int64), -1)
    return np.cumsum(d[:-1], dtype=np.int8) > 0


def locate(pos: int, offs, sizes) -> str:
    """Where byte ``pos`` of an arena lies among the records at ascending ``offs`` of ``sizes`` bytes."""
    offs, sizes = np.asarray(offs, np.int64), np.asarray(sizes, np.int64)
    n = len(offs)
    if n == 0 or pos < int(offs[0]):
        return "before record 0"
    k = int(np.searchsorted(offs, pos, side="right")) - 1
    while k > 0 and sizes[k] == 0 and offs[k - 1] == offs[k]:  # (empty spans share their offset with a neighbour)
        k -= 1
    for j in range(k, min(k + 2, n)):
        if int(offs[j]) <= pos < int(offs[j] + sizes[j]):
            return f"inside record {j} (byte {pos - int(offs[j])} of its {int(sizes[j])})"
    if k == n - 1:
        return f"in the tail, {pos - int(offs[k] + sizes[k])} bytes after record {k}'s end"
    return f"between records {k} and {k + 1}"


def assert_arena(got: np.ndarray, want: np.ndarray, offs, sizes, what: str) -> None:
    """The whole arena, no mask; a failure names the first differing offset and where it lies."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    diff = np.flatnonzero(got != want)
    p = int(diff[0])
    raise AssertionError(f"{what}: {diff.size} bytes differ, the first at offset {p}, {locate(p, offs, sizes)}: got "
                         f"{got[p:p + 16].tobytes().hex()} want {want[p:p + 16].tobytes().hex()}; the last at {int(diff[-1])}, "
                         f"{locate(int(diff[-1]), offs, sizes)}")


@dataclass
class PackedCase:
    """A batch of byte-adjacent records with its keys and arenas. ``src`` is the seal's input arena; ``fill`` the
    random bytes its output arena starts with (in place both are one array: plaintext where the records' texts are,
    random bytes where the tags go and in the tail)."""

    b: RecordBatch
    key_size: int
    keys: np.ndarray
    ivs: np.ndarray
    src: np.ndarray
    fill: np.ndarray
    aad: np.ndarray
    in_place: bool
    lens: np.ndarray  # the records' lengths as laid out (a test may make a descriptor's len invalid afterwards)

    @property
    def n(self):
        return self.b.n

    @property
    def sealed_offs(self):
        return self.b.seal["out_off"].astype(np.int64)

    @property
    def sealed_sizes(self):
        return self.lens + 16

    @property
    def plain_offs(self):
        return self.b.open["out_off"].astype(np.int64)

    @property
    def plain_sizes(self):
        return self.lens


def packed_case(rng, lens, aads, key_size, nkeys=1, in_place=False, key_idx=None) -> PackedCase:
    """Records of ``lens`` / ``aads`` packed byte-adjacent from odd bases, seq from the full 64 bits, ``nkeys`` keys in
    sorted order (or ``key_idx`` as given), every arena random."""
    n = len(lens)
    if key_idx is None and nkeys > 1:
        key_idx = np.sort(rng.integers(0, nkeys, n))
    b = RecordBatch.build_offsets(np.asarray(lens), np.asarray(aads), seqs=rng.integers(0, 2**64, n, dtype=np.uint64),
                                  key_idx=key_idx, in_base=IN_BASE, out_base=OUT_BASE, aad_base=AAD_BASE, in_place=in_place)
    keys, ivs = rand_bytes(rng, nkeys * key_size), rand_bytes(rng, nkeys * 12)
    aad = rand_bytes(rng, b.aad_bytes)
    src = rand_bytes(rng, b.pt_bytes)
    fill = src if in_place else rand_bytes(rng, b.sealed_bytes)
    return PackedCase(b, key_size, keys, ivs, src, fill, aad, in_place, np.asarray(lens, np.int64).copy())


def tamper(rng, case: PackedCase, sealed: np.ndarray, candidates=None):
    """Copies of ``sealed`` and of the AAD arena with three records tampered: one ciphertext bit, one tag bit, one AAD
    bit. Returns (sealed, aad, victims, (offset, mask) of the flipped ciphertext bit relative to its record's text)."""
    s = case.b.seal
    cand = np.arange(case.n) if candidates is None else np.asarray(candidates)
    ct_v = int(rng.choice(cand[s["len"][cand] > 0]))
    rest = cand[cand != ct_v]
    aad_v = int(rng.choice(rest[s["aad_len"][rest] > 0])) if len(rest) else None
    rest = rest[rest != aad_v]
    tag_v = int(rng.choice(rest)) if len(rest) else None
    bad, badaad = sealed.copy(), case.aad.copy()
    at, bit = int(rng.integers(0, int(s["len"][ct_v]))), 1 << int(rng.integers(0, 8))
    bad[int(s["out_off"][ct_v]) + at] ^= bit
    victims = [ct_v]
    if tag_v is not None:
        bad[int(s["out_off"][tag_v]) + int(s["len"][tag_v]) + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        victims.append(tag_v)
    if aad_v is not None:
        badaad[int(s["aad_off"][aad_v]) + int(rng.integers(0, int(s["aad_len"][aad_v])))] ^= 1 << int(rng.integers(0, 8))
        victims.append(aad_v)
    return bad, badaad, victims, (ct_v, at, bit)
