"""bench.py --dump-outputs: what it writes of a proof stream (float32 / float64 .npy, exact, seeded, bounded).  CPU only:
a host tensor stands in for the device proof buffer."""
import os

import numpy as np
import pytest
import torch

import bench


@pytest.mark.parametrize("total", [3 * (1 << 20) + 12345, 5000, 700])
def test_dump_outputs_are_exact_and_seeded(tmp_path, total):
    proof = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=torch.Generator().manual_seed(total))
    p = proof.numpy()
    bench.dump_outputs(str(tmp_path / "a"), torch, proof, 0x5A494E43)
    bench.dump_outputs(str(tmp_path / "b"), torch, proof, 0x5A494E43)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["proof_block_sums.npy", "proof_head.npy", "proof_sample.npy", "proof_sample_offsets.npy", "proof_tail.npy"]
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(a[n[:-4]], np.load(tmp_path / "b" / n)), n  # same seed, same arrays
        assert a[n[:-4]].dtype in (np.float32, np.float64), n
    edge = min(total, bench.DUMP_EDGE_BYTES)
    assert np.array_equal(a["proof_head"], p[:edge]) and np.array_equal(a["proof_tail"], p[total - edge:])
    offs = a["proof_sample_offsets"].astype(np.int64)
    width = a["proof_sample"].shape[1]
    assert np.all(np.diff(offs) >= width) and offs[-1] + width <= total
    for row, o in zip(a["proof_sample"], offs):
        assert np.array_equal(row, p[o:o + width])
    sums = p.astype(np.int64)
    want = [sums[i:i + bench.DUMP_SUM_BYTES].sum() for i in range(0, total, bench.DUMP_SUM_BYTES)]
    assert np.array_equal(a["proof_block_sums"], np.asarray(want, dtype=np.float64))


def test_dump_of_the_headline_proof_stays_under_64_mb():
    """At 2^24 the proof stream is 1.74 GiB: the dump is bounded by its constants, not by the stream."""
    n_sums = -(-(1_870_000_000) // bench.DUMP_SUM_BYTES)
    size = 4 * (2 * bench.DUMP_EDGE_BYTES + bench.DUMP_BLOCKS * bench.DUMP_BLOCK_BYTES) + 8 * (bench.DUMP_BLOCKS + n_sums)
    assert size <= 64 * 2 ** 20
