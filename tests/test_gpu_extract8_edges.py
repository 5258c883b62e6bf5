"""Engine::extract_bits of the 8-bit model (lwe_shl -> keyswitch -> PBS(body_add 2^62, out_add alpha, LUT -alpha) ->
lwe_sub, seven times) on every row, on the rounding boundaries of the extracted bit and across the kernel
selections of Engine::bootstrap, word for word against the oracle's extract_bits.  test_edge_inputs.py pins that
the trivial rows sit on the boundary."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import aes_128
from tests import edge_inputs as E

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
VALUES = [0x00, 0x01, 0x80, 0xFF, 0xB5, 0x7F, 0xAA]


def _oracle_rows(oracle_keys8, ints):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(oracle_keys8.extract_bits, ints))


@pytest.fixture(scope="module")
def seven(product_raw8, oracle_keys8):
    """The seven ints and the oracle's eight bits of each, computed once."""
    ints = product_raw8[0].encrypt_ints_raw(VALUES, start_index=610)
    return ints, _oracle_rows(oracle_keys8, ints)


def test_extract_bits_every_row(gpu_context8, product_raw8, seven):
    ints, refs = seven
    out = gpu_context8.extract_bits_from_ciphertext_raw(ints)
    for i, v in enumerate(VALUES):
        assert np.array_equal(out[i], refs[i]), hex(v)
        assert aes_128.bits_to_u8(product_raw8[0].decrypt_bits_raw(out[i])) == v


def test_extract_bits_trivial_ints_on_the_boundaries(gpu_context8, oracle_keys8):
    """Zero-mask ints with the body v 2^56, just below the rounding boundary of bit 0, on it (the tie) and one below
    v 2^56, for v = 0x00, 0xFF and 0x80: twelve rows in one call, every output row against the oracle."""
    ints = np.concatenate([E.extract_tie_ints(oracle_keys8.K, v) for v in E.EXTRACT_TIE_VALUES])
    out = gpu_context8.extract_bits_from_ciphertext_raw(ints)
    for i, ref in enumerate(_oracle_rows(oracle_keys8, ints)):
        assert np.array_equal(out[i], ref), (hex(E.EXTRACT_TIE_VALUES[i // 4]), i % 4)


@pytest.mark.parametrize("lat", ["default", "TAE_B1K_LAT=0"])
def test_extract_bits_batch_across_kernel_selections(gpu_context8, product_raw8, seven, lat):
    """B = CUs + 1: all seven PBS launches of the chain leave br1024lat for the two-per-workgroup kernel, whose last
    workgroup holds one ciphertext; again on a context built with TAE_B1K_LAT=0.  Every row against the oracle's
    rows of its int."""
    import torch
    ints, refs = seven
    B = torch.cuda.get_device_properties(0).multi_processor_count + 1
    ctx = gpu_context8
    if lat != "default":
        old = os.environ.get("TAE_B1K_LAT")
        os.environ["TAE_B1K_LAT"] = "0"
        try:
            ctx = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_WOPPBS_8BIT, product_raw8[1], device=0)
        finally:
            if old is None:
                del os.environ["TAE_B1K_LAT"]
            else:
                os.environ["TAE_B1K_LAT"] = old
    out = ctx.extract_bits_from_ciphertext_raw(np.resize(ints, (B, ints.shape[1])))
    for i in range(B):
        assert np.array_equal(out[i], refs[i % len(VALUES)]), i
