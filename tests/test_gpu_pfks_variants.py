"""Every K-layout PFKS GEMM kernel compiled into the library (TAE_PFKS_GEMM: the present gemm_g6 "g6", its
16x16x64-MFMA form "s16", the 8-wave 96 x 128 wave tiles "w32" / "w16") gives the same GGSW words.

Inputs are real outputs of the PBS stage (keyswitch + homomorphic_shift_boolean of fresh encryptions, run once
on the GPU and shared), so the digits have their real distribution: about 4.3 M lower-level digits at
B = 2085, a few dozen of which are +32768 and take the clamp fix-up by themselves.  Row 0 is also crafted:
coefficients whose lower-level residue is exactly half the base (+32768 with the upper digit's low bit clear,
-32768 with a carry otherwise), so the fix-up runs at B = 1 too.

Each variant is compared word for word with the gemm_g6 path over the whole batch, and both with the oracle's
private functional keyswitch on the rows where the tiling can go wrong (first and last row, both sides of every
384-row tile edge, the crafted row, a row with a clamped digit) for the first and the last of the k + 1 keys.
Which kernel ran is read from the engine (Context.last_pfks_kernel), not inferred.
"""
import ctypes as C
import os

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N

pytestmark = pytest.mark.gpu

K = 4 * 512
BIG = K + 1
SMALL = 678
VARIANTS = ("g6", "s16", "w32", "w16")
DEFAULT = "w16"  # what a context without the switch launches
B_AUTO = 2048 + 37  # the smallest batch the engine sends to the K layout by itself, ragged last M tile


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _lower_digits(big):
    """The lower-level (finest) base-2^16 digit of every coefficient, by the closest-representable signed
    decomposition with 2 levels (round to 32 bits, balanced digits, finest first): a residue of exactly 0x8000
    stays +32768 when bit 15 of the part above it is clear, and becomes -32768 with a carry otherwise."""
    s = ((big >> np.uint64(31)) + np.uint64(1)) >> np.uint64(1)
    res, up = s & np.uint64(0xFFFF), s >> np.uint64(16)
    carry = (((res - np.uint64(1)) | up) & res) >> np.uint64(15)
    return res.astype(np.int64) - (carry.astype(np.int64) << 16)


def _context(product_raw, switch):
    os.environ["TAE_PFKS_GEMM"] = switch
    try:
        return tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    finally:
        del os.environ["TAE_PFKS_GEMM"]


@pytest.fixture(scope="module")
def pbs_outputs(product_raw, gpu_context):
    """B_AUTO real PBS outputs; row 0 crafted onto the clamp boundary."""
    client = product_raw[0]
    bits = np.random.default_rng(11).integers(0, 2, size=B_AUTO).astype(np.uint8)
    cts = client.encrypt_bits_raw(bits, start_index=90_000)
    small = np.zeros((B_AUTO, SMALL), dtype=np.uint64)
    N.check(N.lib().tae_stage_keyswitch(gpu_context._h, _vp(cts), B_AUTO, _vp(small), N.TAE_MEM_HOST))
    big = np.zeros((B_AUTO, BIG), dtype=np.uint64)
    N.check(N.lib().tae_stage_pbs_shift_boolean(gpu_context._h, _vp(small), B_AUTO, 1, _vp(big), N.TAE_MEM_HOST))
    # residue exactly half the base: bits 47..32 = 0x8000, nothing below; the upper digit keeps its value
    for i in range(0, BIG, 7):
        big[0, i] = (big[0, i] & np.uint64(0xFFFF_0000_0000_0000)) | np.uint64(0x0000_8000_0000_0000)
    return big


@pytest.fixture(scope="module")
def clamp_rows(pbs_outputs):
    """Real rows with a lower digit of +32768 (the clamped value).  2085 x 2049 lower digits hit it about 32
    times (2^-17 each); none at all has probability e^-32."""
    hits = (_lower_digits(pbs_outputs) == 32768).sum(axis=1)
    assert hits[0] > 100, "the crafted row has too few +32768 lower digits"
    natural = [int(b) for b in np.nonzero(hits)[0] if b]
    print(f"clamped lower digits: crafted row {hits[0]}, {int(hits[1:].sum())} in {len(natural)} real rows")
    assert natural, "no real PBS output has a +32768 lower digit"
    return natural


def _run(ctx, big, want):
    out = np.zeros((len(big), 5, 5 * 512), dtype=np.uint64)
    N.check(N.lib().tae_stage_pfks_ggsw(ctx._h, _vp(big), len(big), 1, _vp(out), N.TAE_MEM_HOST))
    assert ctx.last_pfks_kernel() == want
    return out


@pytest.fixture(scope="module")
def reference_outputs(product_raw, pbs_outputs):
    """gemm_g6<6, 4, true> on every batch size, computed once."""
    forced, auto = _context(product_raw, "g6:all"), _context(product_raw, "g6")
    big = pbs_outputs
    return {1: _run(forced, big[:1], "g6"), 385: _run(forced, big[:385], "g6"), B_AUTO: _run(auto, big, "g6")}


def _edge_rows(B, extra=()):
    rows = {0, B - 1}
    for edge in range(384, B, 384):
        rows |= {edge - 1, edge}
    return sorted(rows | {r for r in extra if r < B})


def test_small_batches_take_the_row_layout_without_the_switch(gpu_context, pbs_outputs):
    """Without ":all" (and without TAE_PFKS_LAYOUT) a batch below 2048 stays on the row-limb GEMM, from
    2048 on the K layout runs by itself, on the default kernel."""
    _run(gpu_context, pbs_outputs[:385], "rows")
    _run(gpu_context, pbs_outputs[:2048], os.environ.get("TAE_PFKS_GEMM", DEFAULT).split(":")[0])


def test_reference_kernel_equals_oracle(reference_outputs, oracle_keys, pbs_outputs, clamp_rows):
    for B, out in reference_outputs.items():
        for i in _edge_rows(B, clamp_rows[:1]):
            for q in (0, 4):
                assert np.array_equal(out[i, q], oracle_keys.pfks(q, pbs_outputs[i])), (B, i, q)


@pytest.mark.parametrize("variant", VARIANTS[1:])
def test_variant_equals_reference_and_oracle(product_raw, reference_outputs, oracle_keys, pbs_outputs, clamp_rows,
                                             variant):
    big = pbs_outputs
    forced, auto = _context(product_raw, variant + ":all"), _context(product_raw, variant)
    for B, ctx in ((1, forced), (385, forced), (B_AUTO, auto)):
        out = _run(ctx, big[:B], variant)
        ref = reference_outputs[B]
        bad = np.argwhere((out != ref).any(axis=2))
        assert bad.size == 0, (variant, B, "first differing (row, key):", bad[:4].tolist(), "of", len(bad))
        for i in _edge_rows(B, clamp_rows[:1])[:3] + [B - 1]:
            assert np.array_equal(out[i, 4], oracle_keys.pfks(4, big[i])), (variant, B, i)


def test_switch_rejects_unknown_names(product_raw):
    with pytest.raises(tfhe_aes.TaeError):
        _context(product_raw, "w64")
