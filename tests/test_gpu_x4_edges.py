"""br512x4's integer step paths on crafted LWE masks: the rotation amounts e = 0, N and 2N -> 0, the
modulus switch's rounding boundary, steps whose rotated difference and spectra are exactly zero (the whole
wave takes the from_torus_bits fallback of the torus tail), and ordinary ciphertexts beside them, word for
word against the oracle.  Seven small LWEs on br512x4 (TAE_BR_LAT_MAX=0): two full workgroups of three
ciphertexts and one holding a single ciphertext."""
import ctypes as C

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
SMALL = 678


def test_x4_crafted_masks_bit_exact(product_raw, oracle_keys, monkeypatch):
    monkeypatch.setenv("TAE_BR_LAT_MAX", "0")
    monkeypatch.setenv("TAE_PBS_KERNEL", "x4")
    ctx = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    bits = np.array([1, 0, 1], dtype=np.uint8)
    cts = product_raw[0].encrypt_bits_raw(bits, start_index=70_000)
    real = np.stack([oracle_keys.keyswitch(c) for c in cts])
    n = SMALL - 1
    small = np.zeros((7, SMALL), dtype=np.uint64)
    # 0: all-zero mask: every step has e = 0, zero difference, zero spectra, fallback on every wave
    small[0, n] = real[0, n]
    # 1: alternating 0 and 2^63: e = 0 and e = N
    small[1, 1:n:2] = np.uint64(1 << 63)
    small[1, n] = real[1, n]
    # 2: all 2^64 - 1: the modulus switch rounds to 2N, i.e. e = 0
    small[2, :n] = np.uint64((1 << 64) - 1)
    small[2, n] = np.uint64(1 << 62)
    # 3: 2^54 and 2^54 - 2^53: one rotation unit and its rounding boundary
    small[3, 0:n:2] = np.uint64(1 << 54)
    small[3, 1:n:2] = np.uint64((1 << 54) - (1 << 53))
    small[3, n] = real[2, n]
    # 4, 5: real keyswitched ciphertexts whose first 16 mask words are zero; 6: one untouched
    small[4] = real[0]
    small[5] = real[1]
    small[4, :16] = 0
    small[5, :16] = 0
    small[6] = real[2]
    out = np.zeros((7, BIG), dtype=np.uint64)
    N.check(N.lib().tae_stage_pbs_shift_boolean(ctx._h, small.ctypes.data_as(C.c_void_p), 7, 1,
                                                out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
    for i in range(7):
        assert np.array_equal(out[i], oracle_keys.homomorphic_shift_boolean(small[i], 1)), i
