"""CPU tests: bench.py --dump-outputs (bench.dump_outputs / bench.sample_elements) on host tensors standing in for a batch:
whole outputs below the sample size, fixed seeded positions above it, float files within the size limit."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import bench


def _batch(stream_lens, n, nb):
    """Element j of every output holds j (offset by the output's index), so a sample names the positions it took."""
    def ramp(ln, base, dtype):
        return torch.arange(base, base + ln + 16, dtype=torch.int64).to(dtype)
    return SimpleNamespace(stream_lens=list(stream_lens), n=list(n), nb=list(nb),
                           streams=[ramp(ln, 0, torch.int32) for ln in stream_lens],
                           outs=[ramp(ln, 7, torch.int32) for ln in n],
                           status=[torch.zeros(max(b, 1), dtype=torch.int32) for b in nb])


def test_small_outputs_are_dumped_whole(tmp_path):
    b = _batch([5, 3], [11, 4], [2, 1])
    bench.dump_outputs(b, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["block_status.npy", "compressed_sample.npy", "decompressed_sample.npy",
                                            "stream_lengths.npy"]
    lens = np.load(tmp_path / "stream_lengths.npy")
    assert lens.dtype == np.float64 and lens.tolist() == [5.0, 3.0]
    comp = np.load(tmp_path / "compressed_sample.npy")
    assert comp.dtype == np.float32 and comp.tolist() == list(range(5)) + list(range(3))
    assert np.load(tmp_path / "decompressed_sample.npy").tolist() == list(range(7, 18)) + list(range(7, 11))
    status = np.load(tmp_path / "block_status.npy")
    assert status.dtype == np.float32 and status.tolist() == [0.0, 0.0, 0.0]


def test_large_outputs_are_sampled_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    b = _batch([30_000, 20_000], [50_000, 40_000], [2, 2])
    bench.dump_outputs(b, str(tmp_path / "a"))
    bench.dump_outputs(b, str(tmp_path / "b"))
    for name in ("compressed_sample", "decompressed_sample"):
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == (1000,)
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))          # the same positions every run
    # the positions are drawn over the concatenation, in order: container 0's ramp, then container 1's
    comp = np.load(tmp_path / "a" / "compressed_sample.npy")
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, 50_000, size=1000))
    assert np.array_equal(comp, np.where(pos < 30_000, pos, pos - 30_000).astype(np.float32))


def test_ranks_write_their_own_files_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    b = _batch([3000], [4000], [1])
    bench.dump_outputs(b, str(tmp_path), rank=1, world=4)
    assert sorted(os.listdir(tmp_path)) == ["block_status_rank1.npy", "compressed_sample_rank1.npy",
                                            "decompressed_sample_rank1.npy", "stream_lengths_rank1.npy"]
    assert np.load(tmp_path / "compressed_sample_rank1.npy").shape == (250,)           # the budget is shared by the ranks


def test_default_sample_stays_within_64_mb():
    # three float32 samples of DUMP_SAMPLE elements, plus one float64 length per container
    assert 3 * bench.DUMP_SAMPLE * 4 + 8 * 4096 <= 64_000_000
