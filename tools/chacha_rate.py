#!/usr/bin/env python3
"""ChaCha20-Poly1305 against the engine's AES-256-GCM, device-resident seal+open, on the same buffers.

    python tools/chacha_rate.py [--steps 20 --warmup 3 --rounds 5] [--shapes tls16k,quic1200,quic2perkey] [--scale 1.0]

Timed the way bench.py times its headline: one step = seal the whole batch, then open the sealed batch (one call each),
inputs already in HBM; rate = 2 x payload bytes / wall time of the timed steps, in GiB/s. The two arms are interleaved
in one process: `rounds` times, each arm in turn runs steps / rounds timed steps, so that clock and thermal drift meet
both. Beside each rate stands the shader clock inside the kernels over those steps (ptls_mi355x_debug_kernel_clock:
workgroup 0 of every launch reads s_memtime and s_memrealtime at its start and end). The AES-256-GCM arm is the engine's
existing code: the yardstick, not the code under test. Prints one JSON line.

Shapes: 131,072 x 16 KiB under one key; 1,048,576 x 1200 B under one key; 131,072 x 1200 B over 65,536 keys (2 a key).
Also the per-record call latency (host buffers, one record a call) of both suites at 16 B, 1200 B, 16 KiB, 64 KiB and
1 MiB; --latency-libs times that call of several builds of the library against each other instead.

Bar: chacha_over_aes >= 1.0 on every shape ("bar_met"). Measured (profiles/chacha20poly1305.md, builder-box): 1.25 on
the 16 KiB shape, 10.8 on two packets per key, 0.93 (0.92 in earlier runs) on 2^20 x 1200 B under one key: that shape
misses the bar (DESIGN.md 10.3 has the attribution).
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

SHAPES = {
    "tls16k": (131072, 16384, 1),
    "quic1200": (1048576, 1200, 1),
    "quic2perkey": (131072, 1200, 65536),
}


def in_kernel_mhz(pa, k) -> float | None:
    khz = pa.debug_wallclock_khz()
    if len(k) < 4 or khz <= 0:
        return None
    s = np.asarray(k, dtype=np.int64).reshape(-1, 4)
    cyc, ticks = (s[:, 1] - s[:, 0]).astype(np.float64), (s[:, 3] - s[:, 2]).astype(np.float64)
    keep = (ticks > 0) & (cyc > 0)
    if not keep.any():
        return None
    return round(float(cyc[keep].sum() / (ticks[keep].sum() / (khz * 1e3)) / 1e6), 1)


def run_shape(name: str, nrecs: int, rec_len: int, nkeys: int, steps: int, warmup: int, rounds: int) -> dict:
    import torch

    import picotls_amd as pa
    from picotls_amd.records import RecordBatch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2439)
    key_idx = (np.arange(nrecs, dtype=np.uint32) * nkeys // nrecs).astype(np.uint32)  # grouped by connection, as they arrive
    b = RecordBatch.build(np.full(nrecs, rec_len), 13, seqs=rng.integers(0, 2**62, nrecs, dtype=np.uint64), key_idx=key_idx)
    keys, ivs = rng.bytes(32 * nkeys), rng.bytes(12 * nkeys)
    arms = {"chacha20poly1305": (pa.ChaChaKeyset(keys, ivs), pa.chacha_seal_batch, pa.chacha_open_batch),
            "aes256gcm": (pa.Keyset(keys, ivs, 32), pa.seal_batch, pa.open_batch)}
    d_seal = torch.from_numpy(b.seal.view(np.uint8).copy()).to(dev)
    d_open = torch.from_numpy(b.open.view(np.uint8).copy()).to(dev)
    d_aad = torch.randint(0, 256, (max(b.aad_bytes, 1),), dtype=torch.uint8, device=dev)
    d_pt = torch.randint(0, 256, (b.pt_bytes,), dtype=torch.uint8, device=dev)
    d_sealed = torch.zeros(b.sealed_bytes, dtype=torch.uint8, device=dev)
    d_back = torch.zeros(b.pt_bytes, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(b.n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream

    def step(arm):
        ks, seal, open_ = arms[arm]
        seal(ks, d_seal.data_ptr(), b.n, d_pt.data_ptr(), d_aad.data_ptr(), d_sealed.data_ptr(), sp)
        open_(ks, d_open.data_ptr(), b.n, d_sealed.data_ptr(), d_aad.data_ptr(), d_back.data_ptr(), d_ok.data_ptr(), sp)

    out = {"shape": name, "records": nrecs, "record_len": rec_len, "keys": nkeys, "payload_bytes": b.payload_bytes}
    lens = b.seal["len"].astype(np.int64)
    offs = torch.from_numpy(b.seal["in_off"].astype(np.int64)).to(dev)
    same_slots = rec_len % 16 == 0  # whole arenas compare only when no padding lies between the records
    for arm in arms:  # warm up and check the round trip of each arm once
        d_back.zero_(), d_ok.zero_()
        for _ in range(max(warmup, 1)):
            step(arm)
        torch.cuda.synchronize(dev)
        if same_slots:
            same = bool(torch.equal(d_back, d_pt))
        else:
            idx = (offs[:, None] + torch.arange(rec_len, device=dev)[None, :])[:4096].reshape(-1)
            same = bool(torch.equal(d_back[idx], d_pt[idx]))
        out[arm] = {"verified_roundtrip": bool(d_ok.min().item() == 1) and same}
    per_round = max(steps // rounds, 1)
    wall = {a: 0.0 for a in arms}
    clocks = {a: [] for a in arms}
    kcap = 4 * per_round + 8
    kclk = torch.zeros(4 * kcap, dtype=torch.int64, device=dev)
    for _ in range(rounds):
        for arm in arms:
            pa.debug_kernel_clock(kclk.data_ptr(), kcap)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(per_round):
                step(arm)
            torch.cuda.synchronize(dev)
            wall[arm] += time.perf_counter() - t0
            nk = min(pa.debug_kernel_clock_count(), kcap)
            clocks[arm].append(kclk[:4 * nk].cpu().numpy().copy())
    pa.debug_kernel_clock(0, 0)
    for arm in arms:
        n = per_round * rounds
        out[arm].update({"steps": n, "ms_per_step": round(wall[arm] / n * 1e3, 4),
                         "gib_per_s": round(2 * b.payload_bytes * n / wall[arm] / 2**30, 1),
                         "in_kernel_mhz": in_kernel_mhz(pa, np.concatenate(clocks[arm])),
                         "in_kernel_launches": int(sum(len(c) for c in clocks[arm]) // 4)})
    out["chacha_over_aes"] = round(out["chacha20poly1305"]["gib_per_s"] / out["aes256gcm"]["gib_per_s"], 3)
    out["chacha_group_launches"] = pa.chacha_debug_counters(reset=True)
    for ks, _, _ in arms.values():
        ks.free()
    del d_pt, d_sealed, d_back, d_ok, d_seal, d_open, d_aad
    torch.cuda.empty_cache()
    return out


LATENCY_SIZES = (16, 1200, 16384, 65536, 1 << 20)


def per_record_latency_libs(paths: list[str], calls: int = 300, rounds: int = 5, sizes=LATENCY_SIZES) -> dict:
    """ptls_mi355x_chacha_encrypt of several builds of the library (a parent and a new one, or one twice for the noise),
    interleaved in one process: `rounds` times each build in turn makes calls / rounds timed calls; the outputs are
    compared. A path may be lib.so@PIECE:MIN_LEN (ptls_mi355x_chacha_debug_spread before each of its turns)."""
    import ctypes

    rng = np.random.default_rng(7)
    key, iv, aad = rng.bytes(32), rng.bytes(12), b"0123456789abc"
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    bound, arms = {}, []
    for p in paths:
        path, _, spread = p.partition("@")
        if path not in bound:
            lib = ctypes.CDLL(os.path.abspath(path))
            lib.ptls_mi355x_chacha_keyset_new.argtypes, lib.ptls_mi355x_chacha_keyset_new.restype = [vp, vp, sz], vp
            lib.ptls_mi355x_chacha_encrypt.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
            bound[path] = (lib, vp(lib.ptls_mi355x_chacha_keyset_new(key, iv, 1)))
        arms.append((p, *bound[path], tuple(int(x) for x in spread.split(":")) if spread else None))
    res = {p: {} for p in paths}
    for n in sizes:
        pt = rng.bytes(n)
        outs = {p: ctypes.create_string_buffer(n + 16) for p in paths}
        t = {p: [] for p in paths}
        per = max(calls // rounds, 1)
        for rnd in range(rounds + 1):  # (round 0 warms up)
            for p, lib, ks, setting in arms:
                if hasattr(lib, "ptls_mi355x_chacha_debug_spread"):  # (process-wide: a plain path is automatic)
                    assert lib.ptls_mi355x_chacha_debug_spread(*(setting or (0, 0)), 0) == 0
                for i in range(per if rnd else 20):
                    t0 = time.perf_counter()
                    rc = lib.ptls_mi355x_chacha_encrypt(ks, 0, outs[p], pt, n, i, aad, len(aad))
                    dt = time.perf_counter() - t0
                    assert rc == 0
                    if rnd:
                        t[p].append(dt)
        same = all(outs[p].raw == outs[paths[0]].raw for p in paths)
        for p in paths:
            res[p][str(n)] = {"median_us": round(float(np.median(t[p])) * 1e6, 1), "p90_us": round(float(np.percentile(t[p], 90)) * 1e6, 1),
                              "same_output": same}
    return res


def per_record_latency(calls: int = 300) -> dict:
    import picotls_amd as pa

    rng = np.random.default_rng(7)
    key, iv = rng.bytes(32), rng.bytes(12)
    res = {}
    for name, algo in (("chacha20poly1305", pa.chacha20poly1305), ("aes256gcm", pa.aes256gcm)):
        ctx = pa.AeadContext(algo, True, key, iv)
        res[name] = {}
        for n in LATENCY_SIZES:
            pt = rng.bytes(n)
            for _ in range(20):
                ctx.encrypt(pt, 1, b"0123456789abc")
            t = []
            for i in range(calls):
                t0 = time.perf_counter()
                ctx.encrypt(pt, i, b"0123456789abc")
                t.append(time.perf_counter() - t0)
            res[name][str(n)] = {"median_us": round(float(np.median(t)) * 1e6, 1), "p90_us": round(float(np.percentile(t, 90)) * 1e6, 1)}
        ctx.free()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--shapes", default="tls16k,quic1200,quic2perkey")
    p.add_argument("--scale", type=float, default=1.0, help="record counts times this (smaller runs)")
    p.add_argument("--no-latency", action="store_true")
    p.add_argument("--latency-libs", nargs="+", default=None,
                   help="only the per-record ChaCha20-Poly1305 latency of these builds, interleaved (per_record_latency_libs)")
    p.add_argument("--latency-sizes", default="", help="record lengths for --latency-libs, comma separated")
    args = p.parse_args()
    if args.latency_libs:
        sizes = tuple(int(x) for x in args.latency_sizes.split(",")) if args.latency_sizes else LATENCY_SIZES
        print(json.dumps({"tool": "chacha_rate", "per_record_encrypt_latency_libs": per_record_latency_libs(args.latency_libs, sizes=sizes)}))
        return
    import torch

    import picotls_amd as pa

    assert torch.cuda.is_available(), "needs an MI355X"
    pa.load_library()
    pa.chacha_debug_counters(reset=True)
    shapes = []
    for name in [s for s in args.shapes.split(",") if s]:
        nrecs, rec_len, nkeys = SHAPES[name]
        nrecs = max(int(nrecs * args.scale), 1)
        shapes.append(run_shape(name, nrecs, rec_len, min(nkeys, nrecs), max(args.steps, 20) if args.scale >= 1 else args.steps,
                                args.warmup, args.rounds))
    line = {"tool": "chacha_rate", "metric": "seal+open GiB/s over payload bytes, device-resident", "shapes": shapes,
            "bar": "chacha_over_aes >= 1.0 on every shape", "bar_met": all(s["chacha_over_aes"] >= 1.0 for s in shapes),
            "verified": all(s[a]["verified_roundtrip"] for s in shapes for a in ("chacha20poly1305", "aes256gcm"))}
    if not args.no_latency:
        line["per_record_encrypt_latency"] = per_record_latency()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
