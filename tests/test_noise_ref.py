"""tests/noise_ref.py against the oracle and against plain arithmetic (CPU; the GPU measurements that use it are
tests/test_gpu_noise.py)."""
import math

import numpy as np
import pytest

import tfhe_aes
from tests import noise_ref as R
from tests.conftest import SEED


@pytest.fixture(scope="module")
def client():
    return tfhe_aes.client_key_from_seed(tfhe_aes.PARAMS_SQRD_LVL_64, SEED)


def test_phases_equal_the_oracle(client, oracle_keys):
    bits = [0, 1, 1, 0, 1, 0, 0, 1]
    fresh = client.encrypt_bits_raw(bits, start_index=11_000_000)
    small = np.stack([oracle_keys.keyswitch(c) for c in fresh])
    assert small.shape == (8, oracle_keys.p["n"] + 1)
    big_ph, small_ph = R.big_phase(client, fresh), R.small_phase(client, small)
    assert [int(x) for x in big_ph] == [oracle_keys.phase(c) for c in fresh]
    assert [int(x) for x in small_ph] == [oracle_keys.small_phase(c) for c in small]
    # and they are phases of the bits: fresh noise is 2^49.6, a keyswitched bit's well below 2^57
    assert np.abs(R.signed_error(big_ph, bits)).max() < 2.0 ** 54
    assert np.abs(R.signed_error(small_ph, bits)).max() < 2.0 ** 60
    with pytest.raises(ValueError):
        R.big_phase(client, small)


def test_signed_error_wraps():
    top = 1 << 63
    phase = np.array([0, 5, 2 ** 64 - 5, top, top + 7, top - 7, top - 1, top, 2 ** 62, 3 * 2 ** 62], dtype=np.uint64)
    bit = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 1], dtype=np.uint64)
    want = [0.0, 5.0, -5.0, 0.0, 7.0, -7.0, 2.0 ** 63, -2.0 ** 63, 2.0 ** 62, 2.0 ** 62]
    assert R.signed_error(phase, bit).tolist() == want
    assert R.signed_error(np.uint64(3), 0).tolist() == 3.0  # scalars broadcast


def test_z_required():
    z = R.z_required()
    assert abs(z - 9.1553) < 1e-3
    assert abs(math.erfc(z / math.sqrt(2.0)) / R.P_ERROR - 1.0) < 1e-9
    # the estimator bounds are the closed forms of their docstrings
    assert R.se_var(200) == 0.1 and R.mean_bound(2.0, 100) == 1.0
    assert R.margin_floor(50) == 0.5 and R.ratio_bound(100) == 2.0 and R.corr_bound(25) == 1.0


def test_modswitch_is_the_oracles_rounding(oracle_mod):
    rng = np.random.default_rng(23)
    words = rng.integers(0, 2 ** 64, 64, dtype=np.uint64)
    step = 1 << 54
    edge = np.array([0, 1, step // 2 - 1, step // 2, step // 2 + 1, step, 3 * step // 2, 2 ** 64 - step // 2 - 1,
                     2 ** 64 - step // 2, 2 ** 64 - 1], dtype=np.uint64)
    words = np.concatenate([words, edge])
    got = R.modswitch(words, 512)
    for w, g in zip(words, got):
        assert int(g) == (oracle_mod.lib().or_pbs_modulus_switch(int(w), 512) << 54) % 2 ** 64, hex(int(w))
        d = (int(g) - int(w)) % 2 ** 64
        assert min(d, 2 ** 64 - d) <= step // 2  # nearest


def test_modswitch_var_against_rounding(client):
    """256 uniformly random small ciphertexts, every word rounded in numpy: the variance of the phase difference
    against the derived term.  A variance of 256 Gaussian samples has relative standard error sqrt(2 / 256); the
    difference is a sum of 339 uniform terms, closer to Gaussian than the bound needs."""
    m = 256
    n = client.params["n"]
    rng = np.random.default_rng(29)
    cts = rng.integers(0, 2 ** 64, (m, n + 1), dtype=np.uint64)
    diff = (R.small_phase(client, R.modswitch(cts, client.params["N"])) - R.small_phase(client, cts))
    diff = diff.view(np.int64).astype(np.float64)
    want = R.modswitch_var(client)
    h = int(client.secrets()[0].sum())
    assert want == (1 + h) * (2.0 ** 54) ** 2 / 12 and n // 3 < h < 2 * n // 3
    ratio = np.mean(diff ** 2) / want  # the rounding error is zero-mean by symmetry up to the tie rule
    assert abs(ratio - 1.0) <= R.N_SE * R.se_var(m), ratio
    assert abs(diff.mean()) <= R.mean_bound(math.sqrt(want), m)


def test_decompose_is_the_oracles(oracle_mod):
    rng = np.random.default_rng(31)
    words = np.concatenate([rng.integers(0, 2 ** 64, 200, dtype=np.uint64),
                            np.array([0, 2 ** 51 - 1, 2 ** 51, 2 ** 63, 2 ** 63 - 2 ** 51, 2 ** 64 - 2 ** 51, 2 ** 64 - 1,
                                      4 << 61, 4 << 58, (4 << 58) | (1 << 61)], dtype=np.uint64)])
    for base_log, levels in ((3, 4), (2, 8), (16, 2)):
        got = R.decompose(words, base_log, levels)
        for w, g in zip(words, got):
            assert g.tolist() == oracle_mod.decompose(int(w), base_log, levels), (hex(int(w)), base_log, levels)
    # the top digit of uniform words is not centred (+B/2 never becomes -B/2), the others are
    top = np.arange(1 << 13, dtype=np.uint64) << np.uint64(51)
    assert R.decompose(top, 3, 4).mean(axis=0).tolist() == [455 / 1024, 0.0, 0.0, 0.0]


def test_keyswitch_offset_against_keyswitched_bits(client, oracle_keys):
    """256 fresh bits through the oracle's keyswitch: the mean of their small-key errors is within 5 sigma / sqrt m
    of the derived offset.  At 256 samples that bound is wider than the offset itself, so this pins the key
    layout and the order of magnitude; the GPU run has the samples that tell the offset from zero."""
    m = 256
    bits = np.random.default_rng(37).integers(0, 2, m).astype(np.uint8)
    fresh = client.encrypt_bits_raw(bits, start_index=11_001_000)
    small = np.stack([oracle_keys.keyswitch(c) for c in fresh])
    err = R.signed_error(R.small_phase(client, small), bits)
    offset = R.keyswitch_offset(client, oracle_keys.raw_server()[0])
    assert 2.0 ** 50 < abs(offset) < 2.0 ** 57  # 0.44 of a sum of 2048 key noises of 2^49.6: about 2^54
    assert abs(err.mean() - offset) <= R.mean_bound(err.std(), m), (err.mean(), offset)


def test_margin_of_a_known_sample(client):
    e = np.array([-3.0, 1.0, 5.0, 1.0]) * 2.0 ** 56  # mean 2^56, variance 8 * 2^112
    want = (2.0 ** 62 - 2.0 ** 56) / math.sqrt(8 * 2.0 ** 112 + R.modswitch_var(client))
    assert R.margin(e, client) == pytest.approx(want, rel=1e-12)
