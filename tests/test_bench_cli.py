"""bench.py's command line on the CPU: the default legs of a --full run (every BASELINE config, configs[4] included),
the plain run's options, the files of --dump-outputs and when the self-launcher starts ranks (never for N = 1 or inside
torch.distributed.run)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

import bench  # noqa: E402


def test_default_legs_cover_every_baseline_config(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.gpus == 1 and a.workload == "tls16k"
    assert set(a.extra.split(",")) == {"quic1200", "mixed", "mixedrand", "shard1200", "ptlsbench", "quic64k", "tls64k"}
    assert a.e2e is None  # on for N = 1 at full size (main), off with --no-e2e
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-e2e"])
    assert bench.parse().e2e is False


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere"
    for argv in (["--e2e"], ["--steps", "0"]):  # a --full leg asked of a plain run; no timed step to report
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        with pytest.raises(SystemExit):
            bench.parse()
    capsys.readouterr()


def test_block_sums_cover_every_byte_once():
    import torch

    rng = np.random.default_rng(5)
    for n, max_blocks, piece in ((0, 4, 1 << 30), (4095, 4, 1 << 30), (4096, 4, 1 << 30), (5 * 4096 + 17, 1 << 20, 8192),
                                 (5 * 4096 + 17, 4, 1 << 30), (40000, 3, 16384)):
        a = rng.integers(0, 256, n, dtype=np.uint8)
        sums, block = bench._block_sums(torch.from_numpy(a), max_blocks, piece)
        assert block >= 4096 and block & (block - 1) == 0 and len(sums) == (n + block - 1) // block <= max(max_blocks, 0)
        assert sums.dtype == np.float64
        want = [float(a[i:i + block].sum(dtype=np.int64)) for i in range(0, n, block)]
        assert sums.tolist() == want


def test_dump_outputs_files(tmp_path, monkeypatch):
    """dump_outputs on host tensors: the sampled records' bytes, the block sums and the ok bytes are those of the
    arenas, as float32 / float64 .npy files, the same on every call; beyond DUMP_MAX_OK records the ok bytes are sampled."""
    import torch

    from picotls_amd.records import RecordBatch

    rng = np.random.default_rng(6)
    lens = np.concatenate([[0, 1, 15, 16, 17, 16384], rng.integers(0, 3000, 400)])
    b = RecordBatch.build(lens, 13)
    sealed = rng.integers(0, 256, b.sealed_bytes, dtype=np.uint8)
    back = rng.integers(0, 256, b.pt_bytes, dtype=np.uint8)
    ok = rng.integers(0, 2, b.n, dtype=np.uint8)
    t = [torch.from_numpy(x) for x in (sealed, back, ok)]
    info = bench.dump_outputs(str(tmp_path / "a"), 0, b, *t)
    assert info["bytes"] < 64e6 and sorted(os.listdir(tmp_path / "a")) == info["files"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in info["files"]}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    idx = got["sample_index"].astype(np.int64)
    assert idx[0] == 0 and idx[-1] == b.n - 1 and len(np.unique(idx)) == len(idx) > 100
    r = b.seal[idx]
    want_sealed = np.concatenate([sealed[int(o):int(o) + int(n) + 16] for o, n in zip(r["out_off"], r["len"])])
    want_back = np.concatenate([back[int(o):int(o) + int(n)] for o, n in zip(r["in_off"], r["len"])])
    assert np.array_equal(got["sealed_sample"], want_sealed) and np.array_equal(got["opened_sample"], want_back)
    assert np.array_equal(got["ok"], ok)
    sb, ob = (int(x) for x in got["block_bytes"])
    assert got["sealed_blocksum"].sum() == sealed.sum(dtype=np.int64) and len(got["sealed_blocksum"]) == -(-len(sealed) // sb)
    assert got["opened_blocksum"].sum() == back.sum(dtype=np.int64) and len(got["opened_blocksum"]) == -(-len(back) // ob)
    # a second call (and another rank's file names) holds the same arrays
    info1 = bench.dump_outputs(str(tmp_path / "a"), 1, b, *t)
    assert all(f.endswith("_rank1.npy") for f in info1["files"])
    for name, v in got.items():
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}_rank1.npy"), v)
    monkeypatch.setattr(bench, "DUMP_MAX_OK", 100)
    info2 = bench.dump_outputs(str(tmp_path / "b"), 0, b, *t)
    assert "ok.npy" not in info2["files"]
    assert np.array_equal(np.load(tmp_path / "b" / "ok_sample.npy"), ok[idx])
    assert np.load(tmp_path / "b" / "ok_sum.npy").tolist() == [float(ok.sum()), float(b.n)]


def test_self_launch_only_outside_a_launcher(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.self_launch(1) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bench.self_launch(2) is None  # already a rank of torch.distributed.run
