"""bench.py --dump-outputs, host side: the sample of the output ciphertexts is fixed, exact (each u64 word as
two 32-bit halves in float64) and bounded in size.  The GPU run of the option is in test_gpu_dist_bench.py."""
import numpy as np

import bench


def test_dump_outputs_exact_fixed_sample(tmp_path):
    rng = np.random.default_rng(1)
    out = rng.integers(0, 2 ** 64, size=(3 * bench.DUMP_ROWS + 5, 17), dtype=np.uint64)
    out[0, 0], out[1, 0] = np.uint64(2 ** 64 - 1), np.uint64(0)
    blocks = [bytes(range(i, i + 16)) for i in range(3)]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, blocks)
    bench.dump_outputs(str(b), out.copy(), blocks)
    names = sorted(p.name for p in a.iterdir())
    assert names == ["ciphertext_hi32.npy", "ciphertext_lo32.npy", "ciphertext_rows.npy", "decrypted_blocks.npy"]
    arrs = {n: np.load(a / n) for n in names}
    for n in names:
        assert arrs[n].dtype == np.float64
        assert np.array_equal(arrs[n], np.load(b / n)), n  # same rows from run to run
    rows = arrs["ciphertext_rows.npy"].astype(np.int64)
    assert rows.shape == (bench.DUMP_ROWS,) and np.all(np.diff(rows) > 0) and rows[-1] < out.shape[0]
    hi, lo = arrs["ciphertext_hi32.npy"].astype(np.uint64), arrs["ciphertext_lo32.npy"].astype(np.uint64)
    assert np.array_equal((hi << np.uint64(32)) | lo, out[rows])
    assert np.array_equal(arrs["decrypted_blocks.npy"], np.array([list(x) for x in blocks], dtype=np.float64))


def test_dump_outputs_small_output_whole(tmp_path):
    out = np.arange(7 * 5, dtype=np.uint64).reshape(7, 5) << np.uint64(40)
    bench.dump_outputs(str(tmp_path), out, [bytes(16)])
    assert np.array_equal(np.load(tmp_path / "ciphertext_rows.npy"), np.arange(7.0))
    hi = np.load(tmp_path / "ciphertext_hi32.npy").astype(np.uint64)
    assert np.array_equal(hi << np.uint64(32), out)


def test_dump_size_bound_at_flagship_shape():
    # params_sqrd_lvl_64 big LWE size 2049 words; 128 blocks x 16 bytes of results
    total = bench.DUMP_ROWS * 8 + 2 * bench.DUMP_ROWS * 2049 * 8 + 128 * 16 * 8
    assert total + 4 * 128 <= 64 * 2 ** 20  # + the four .npy headers
