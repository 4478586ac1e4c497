#!/usr/bin/env python3
"""The record-per-lane schedule against the default one on few-packet connections, device-resident, AES-128-GCM.

    python tools/lane_rate.py [--steps 20 --warmup 2 --rounds 5] [--shapes k1,k2,k8,k16,k32,k64,onekey]
                              [--paths batch,quic,tls13,tls12,hp] [--scale 1.0]

Timed the way tools/chacha_rate.py times: inputs already in HBM, the arms interleaved in one process over the same
buffers (`rounds` times each arm in turn runs steps / rounds timed steps), the shader clock inside the batch kernels
(workgroup 0 of every launch, ptls_mi355x_debug_kernel_clock) beside each rate. Seal and open are timed apart
("seal", "open": payload bytes over wall time) and together ("both": one step = seal then open, 2 x payload bytes over
wall time, chacha_rate's metric). GiB/s. Prints one JSON line.

Arms: three keysets of the same keys -- "auto" (the default schedule: the kernels every batch runs today),
"auto_again" (a second such keyset: the spread of two runs of the same code, A/A) and "record_per_lane".

Paths: "batch" = seal_batch / open_batch (13 bytes of AAD a record); "quic" = seal_quic_packets / open_quic_packets
(short headers: first byte, an 8-byte DCID, a packet number of 1..4 bytes; distinct header-protection keys); "tls13" =
seal_tls_records / open_tls_records (inner type 23); "tls12" = seal_tls12_records / open_tls12_records (an 8-byte
explicit nonce in front of each payload); "hp" = seal_batch_hp alone (the batch path's records, one header-protection
sample 0..3 bytes into each ciphertext; "seal" only, rated over the sealed payload bytes). On these three paths the
"record_per_lane" arm also has ptls_mi355x_keyset_set_lane_framed on, without which they keep the default kernels.

Shapes: 1200-byte records over 65,536 keys with 1, 2 and 8 records per key (k1, k2, k8: 65,536 / 131,072 / 524,288
records, a connection's records beside each other, as they arrive); the controls k16, k32, k64 (16, 32 and 64 per key:
where the default schedule overtakes) and onekey (1,048,576 records under one key). --scale multiplies the record counts (and the key counts with them).

Bar, on k1, k2 and k8 (tls13, tls12, hp: on k1 and k2), per path and per direction: record_per_lane > auto x (1 +
spread), spread = |auto - auto_again| / auto of the same run ("bar_met"; the controls are reported, not gated).
Measured: profiles/aesgcm_lane.md.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chacha_rate import in_kernel_mhz  # noqa: E402

NKEYS = 65536
SHAPES = {"k1": (NKEYS, NKEYS), "k2": (2 * NKEYS, NKEYS), "k8": (8 * NKEYS, NKEYS), "k16": (16 * NKEYS, NKEYS), "k32": (32 * NKEYS, NKEYS),
          "k64": (64 * NKEYS, NKEYS), "onekey": (1 << 20, 1)}
GATED = ("k1", "k2", "k8")
FRAMED_PATHS = ("tls13", "tls12", "hp")  # the paths that take the lane kernel only with lane_framed set
FRAMED_GATED = ("k1", "k2")
PATHS = ("batch", "quic") + FRAMED_PATHS
PLEN = 1200
DCID = 8
ARMS = {"auto": "auto", "auto_again": "auto", "record_per_lane": "record_per_lane"}
DIRECTIONS = ("seal", "open", "both")


def run_shape(path: str, name: str, n: int, nkeys: int, steps: int, warmup: int, rounds: int) -> dict:
    import torch

    import picotls_amd as pa
    from picotls_amd.records import HP_DTYPE, QUIC_RESULT_DTYPE, RECORD_DTYPE

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(4242)
    key_idx = (np.arange(n, dtype=np.uint64) * np.uint64(nkeys) // np.uint64(n)).astype(np.uint32)
    keys, ivs, hp_keys = rng.bytes(16 * nkeys), rng.bytes(12 * nkeys), rng.bytes(16 * nkeys)
    arms = {}
    for arm, schedule in ARMS.items():
        arms[arm] = pa.Keyset(keys, ivs, 16)
        arms[arm].set_schedule(schedule)
        arms[arm].set_lane_framed(path in FRAMED_PATHS and schedule == "record_per_lane")
    hp_ks = pa.Keyset(hp_keys, bytes(12 * nkeys), 16)
    pns = rng.integers(0, 2**62, n, dtype=np.uint64)
    pn_len = (np.arange(n) % 4 + 1).astype(np.int64)
    hlen = 1 + DCID + pn_len
    slot = (1 + DCID + 4 + PLEN + 16 + 15) // 16 * 16
    off = np.arange(n, dtype=np.uint64) * np.uint64(slot)

    def recs(**cols):
        r = np.zeros(n, RECORD_DTYPE)
        r["key_idx"] = key_idx
        for k, v in cols.items():
            r[k] = v
        return torch.from_numpy(r.view(np.uint8).copy()).to(dev)

    clear = torch.randint(0, 256, (n, slot), dtype=torch.uint8, device=dev)
    if path == "quic":  # the cleartext packets: header || payload in slots of `slot` bytes
        t_pnl = torch.from_numpy(pn_len).to(dev)
        t_pn = torch.from_numpy(pns.astype(np.int64)).to(dev)
        clear[:, 0] = (0x40 | (t_pnl - 1)).to(torch.uint8)
        for ln in (1, 2, 3, 4):
            rows = torch.nonzero(t_pnl == ln).reshape(-1)
            for i in range(ln):
                clear[rows, 1 + DCID + i] = ((t_pn[rows] >> (8 * (ln - 1 - i))) & 0xff).to(torch.uint8)
        d_seal = recs(in_off=off, out_off=off, seq=pns, len=PLEN, aad_len=hlen)
        d_open = recs(in_off=off, out_off=off, seq=pns, len=pn_len + PLEN + 16, aad_len=hlen - pn_len)
        text_at = back_at = hlen
    elif path == "tls13":  # payloads in the slots; wire records (5 + 1201 + 16 bytes) and opened texts in the same slots
        d_seal = recs(in_off=off, out_off=off, seq=pns, len=PLEN, flags=23)
        d_open = recs(in_off=off, out_off=off, seq=pns, len=PLEN + 1)
        text_at = back_at = np.zeros(n, np.int64)
    elif path == "tls12":  # explicit nonce || payload in the slots; wire records of 13 + 1200 + 16 bytes
        d_seal = recs(in_off=off, out_off=off, seq=pns, len=PLEN, flags=23)
        d_open = recs(in_off=off, out_off=off, seq=pns, len=PLEN)
        text_at, back_at = np.full(n, 8, np.int64), np.zeros(n, np.int64)
    else:  # records in the same slots, 13 bytes of AAD each from an arena of their own
        d_seal = recs(in_off=off, out_off=off, seq=pns, len=PLEN, aad_off=np.arange(n, dtype=np.uint64) * np.uint64(16), aad_len=13)
        d_open = d_seal
        text_at = back_at = np.zeros(n, np.int64)
    clear = clear.reshape(-1)
    d_aad = torch.randint(0, 256, (16 * n,), dtype=torch.uint8, device=dev)
    d_wire = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    d_back = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream(dev).cuda_stream
    if path == "hp":
        hp = np.zeros(n, HP_DTYPE)
        hp["sample_off"], hp["key_idx"] = off + (np.arange(n, dtype=np.uint64) % np.uint64(4)), key_idx
        d_hp = torch.from_numpy(hp.view(np.uint8).copy()).to(dev)
        d_masks = torch.zeros(16 * n, dtype=torch.uint8, device=dev)

    def seal(ks):
        if path == "quic":
            pa.seal_quic_packets(ks, hp_ks, d_seal.data_ptr(), n, clear.data_ptr(), d_wire.data_ptr(), sp)
        elif path == "tls13":
            pa.seal_tls_records(ks, d_seal.data_ptr(), n, clear.data_ptr(), d_wire.data_ptr(), sp)
        elif path == "tls12":
            pa.seal_tls12_records(ks, d_seal.data_ptr(), n, clear.data_ptr(), d_wire.data_ptr(), sp)
        elif path == "hp":
            pa.seal_batch_hp(ks, d_seal.data_ptr(), n, clear.data_ptr(), d_aad.data_ptr(), d_wire.data_ptr(), hp_ks, d_hp.data_ptr(),
                             d_masks.data_ptr(), sp)
        else:
            pa.seal_batch(ks, d_seal.data_ptr(), n, clear.data_ptr(), d_aad.data_ptr(), d_wire.data_ptr(), sp)

    def open_(ks):
        if path == "quic":
            pa.open_quic_packets(ks, hp_ks, d_open.data_ptr(), n, d_wire.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), sp)
        elif path == "tls13":
            pa.open_tls_records(ks, d_open.data_ptr(), n, d_wire.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), sp)
        elif path == "tls12":
            pa.open_tls12_records(ks, d_open.data_ptr(), n, d_wire.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), d_res.data_ptr(), sp)
        else:  # (hp: the timed call is the seal alone; the open here only checks the sealed bytes)
            pa.open_batch(ks, d_open.data_ptr(), n, d_wire.data_ptr(), d_aad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), sp)

    calls = {"seal": lambda ks: seal(ks), "open": lambda ks: open_(ks), "both": lambda ks: (seal(ks), open_(ks))}
    directions = ("seal",) if path == "hp" else DIRECTIONS

    # warm up and check: every arm's sealed arena equals the auto arm's, and every arm's open restores the packets
    out = {"path": path, "shape": name, "records": n, "record_len": PLEN, "keys": nkeys, "payload_bytes": n * PLEN}
    m = min(n, 4096)
    cols = torch.arange(slot, device=dev)[None, :]
    ta = torch.from_numpy(np.asarray(text_at[:m], np.int64)).to(dev)[:, None]
    tb = torch.from_numpy(np.asarray(back_at[:m], np.int64)).to(dev)[:, None]
    body = cols < ta + PLEN if path == "quic" else (cols >= ta) & (cols < ta + PLEN)
    back_body = body if path == "quic" else (cols >= tb) & (cols < tb + PLEN)  # (row-major: the same order of bytes)
    verified, first_wire, first_masks = {}, None, None
    pa.debug_counters(reset=True)
    for arm, ks in arms.items():
        d_wire.zero_(), d_back.zero_(), d_ok.zero_()
        for _ in range(max(warmup, 1)):
            seal(ks), open_(ks)
        torch.cuda.synchronize(dev)
        if first_wire is None:
            first_wire = d_wire.clone()
        same = bool(torch.equal(d_back[:m * slot].reshape(m, slot)[back_body], clear[:m * slot].reshape(m, slot)[body]))
        verified[arm] = bool(d_ok.min().item() == 1) and same and bool(torch.equal(d_wire, first_wire))
        if path == "hp":
            if first_masks is None:
                first_masks = d_masks.clone()
            verified[arm] = verified[arm] and bool(d_masks.any().item()) and bool(torch.equal(d_masks, first_masks))
            d_masks.zero_()
        c = pa.debug_counters(reset=True)
        out.setdefault("launches", {})[arm] = {k: int(v) for k, v in c["launches"].items() if v}
    if path == "quic":
        res = d_res.cpu().numpy().view(QUIC_RESULT_DTYPE)
        verified["results"] = bool(np.array_equal(res["pn"], pns) and (res["status"] == 0).all())
    del first_wire, first_masks
    out["verified"] = verified

    per_round = max(steps // rounds, 1)
    kcap = 8 * per_round + 8
    kclk = torch.zeros(4 * kcap, dtype=torch.int64, device=dev)
    for direction in directions:
        wall = {a: 0.0 for a in arms}
        clocks = {a: [] for a in arms}
        for _ in range(rounds):
            for arm, ks in arms.items():
                pa.debug_kernel_clock(kclk.data_ptr(), kcap)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(per_round):
                    calls[direction](ks)
                torch.cuda.synchronize(dev)
                wall[arm] += time.perf_counter() - t0
                nk = min(pa.debug_kernel_clock_count(), kcap)
                clocks[arm].append(kclk[:4 * nk].cpu().numpy().copy())
        pa.debug_kernel_clock(0, 0)
        d = {}
        passes = 2 if direction == "both" else 1
        for arm in arms:
            k = per_round * rounds
            d[arm] = {"steps": k, "ms_per_step": round(wall[arm] / k * 1e3, 4),
                      "gib_per_s": round(passes * n * PLEN * k / wall[arm] / 2**30, 1),
                      "in_kernel_mhz": in_kernel_mhz(pa, np.concatenate(clocks[arm]))}
        d["aa_spread"] = round(abs(d["auto"]["gib_per_s"] - d["auto_again"]["gib_per_s"]) / d["auto"]["gib_per_s"], 4)
        d["lane_over_auto"] = round(d["record_per_lane"]["gib_per_s"] / d["auto"]["gib_per_s"], 3)
        d["bar_met"] = d["record_per_lane"]["gib_per_s"] > d["auto"]["gib_per_s"] * (1 + d["aa_spread"])
        out[direction] = d
    for ks in arms.values():
        ks.free()
    hp_ks.free()
    del clear, d_wire, d_back, d_ok, d_res, d_aad
    if path == "hp":
        del d_hp, d_masks
    torch.cuda.empty_cache()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--shapes", default="k1,k2,k8,k16,k32,k64,onekey")
    p.add_argument("--paths", default="batch,quic", help="of " + ",".join(PATHS))
    p.add_argument("--scale", type=float, default=1.0, help="record and key counts times this (smaller runs)")
    args = p.parse_args()
    import torch

    import picotls_amd as pa

    assert torch.cuda.is_available(), "needs an MI355X"
    pa.load_library()
    shapes = []
    for path in [s for s in args.paths.split(",") if s]:
        assert path in PATHS, f"unknown path {path!r}"
        for name in [s for s in args.shapes.split(",") if s]:
            n, nkeys = SHAPES[name]
            n, nkeys = max(int(n * args.scale), 4), max(int(nkeys * args.scale), 1) if nkeys > 1 else 1
            shapes.append(run_shape(path, name, n, min(nkeys, n), args.steps, args.warmup, args.rounds))
    gated = [s for s in shapes if s["shape"] in (FRAMED_GATED if s["path"] in FRAMED_PATHS else GATED)]
    print(json.dumps({"tool": "lane_rate", "metric": "GiB/s over payload bytes (seal, open apart; both = seal+open, 2 x payload), device-resident",
                      "shapes": shapes,
                      "bar": "record_per_lane > auto x (1 + A/A spread) on k1, k2, k8 (tls13, tls12, hp: k1, k2): every path and direction",
                      "bar_met": bool(gated) and all(s[d]["bar_met"] for s in gated for d in DIRECTIONS if d in s),
                      "verified": all(all(s["verified"].values()) for s in shapes)}))


if __name__ == "__main__":
    main()
