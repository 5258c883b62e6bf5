"""Vertical packing and the GGSW forward transform on crafted inputs (tests/edge_inputs.py), word for word
against the oracle, on params_sqrd_lvl_64 (br512x4<1, false, 13>, three outputs per workgroup) and the 8-bit
set (br1024's vertical-packing instantiation, two per workgroup).

The other tests feed these stages one real GGSW or the GGSWs of one real byte.  Here the GGSWs are noiseless
trivial ones of the bits of 0x00 (all-zero spectra: every CMux step adds exact zeros, the from_torus_bits
fallback of the torus tail), 0xFF and 0xA7, three groups in one call, with output counts that leave ragged
workgroups; the LUTs are a 0 / 2^63 table (differences of exactly 2^63: tie digits, tail inputs +-1/2) and a
mix of 2^62 and random words; and the forward transform gets the u64 -> f64 rounding ties and the sign
boundary.  GGSWs of 0 and 1 turn a difference of 2^63 into +1/2 only (the decomposer's top digit is never
negative, edge_inputs.py); groups with the trivial GGSW of -1 among their selectors reach -1/2, the i64
saturation of the torus conversion.
"""
import ctypes as C

import numpy as np
import pytest

from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests import edge_inputs as E

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1
BYTES = (0x00, 0xFF, 0xA7)
N_OUT = {"lvl64": (1, 5, 24), "8bit": (1, 3, 8)}
CASES = [(w, n) for w in ("lvl64", "8bit") for n in N_OUT[w]]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


_SETS = {}


def _set(request, which):
    """(context, oracle keys, spectra of the trivial GGSWs of 0, 1 and -1 by value) of a set, built on first
    use"""
    if which not in _SETS:
        sfx = "" if which == "lvl64" else "8"
        ctx, ok = request.getfixturevalue("gpu_context" + sfx), request.getfixturevalue("oracle_keys" + sfx)
        _SETS[which] = ctx, ok, {b: ok.ggsw_to_fourier(E.trivial_ggsw(ok.p, b)) for b in (0, 1, -1)}
    return _SETS[which]


def _vertical_packing(ctx, ok, gf, groups, n_in, lut, n_out):
    gfd = np.ascontiguousarray(gf).view(np.float64)
    lut = np.ascontiguousarray(lut, dtype=np.uint64)
    out = np.zeros((groups, n_out, ok.K + 1), dtype=np.uint64)
    N.check(N.lib().tae_stage_vertical_packing(ctx._h, _vp(gfd), groups, n_in, _vp(lut), n_out, _vp(out),
                                               N.TAE_MEM_HOST))
    return out


def _check(ctx, ok, spec, bit_rows, lut, n_out):
    """One call over len(bit_rows) groups; every output against oracle.vertical_packing.  Returns the outputs."""
    Np, n_in = ok.p["N"], len(bit_rows[0])
    groups = [np.concatenate([spec[b] for b in bits]) for bits in bit_rows]
    out = _vertical_packing(ctx, ok, np.concatenate(groups), len(groups), n_in, lut, n_out)
    for g, gf in enumerate(groups):
        for j in range(n_out):
            ref = ok.vertical_packing(lut[j * Np:(j + 1) * Np], gf, n_in)
            assert np.array_equal(out[g, j], ref), (g, j)
    return out


def _mixed_lut(rng, n_out, Np):
    """Output j: the constant 2^62 (j % 3 == 0), random words (1), or both alternating in runs of eight (2)."""
    lut = E.random_words(rng, (n_out, Np))
    for j in range(n_out):
        if j % 3 == 0:
            lut[j] = np.uint64(1 << 62)
        elif j % 3 == 2:
            lut[j, (np.arange(Np) // 8) % 2 == 0] = np.uint64(1 << 62)
    return lut.reshape(-1)


@pytest.mark.parametrize("which,n_out", CASES)
def test_vertical_packing_trivial_ggsws_sbox_lut(request, oracle_mod, which, n_out):
    """8 -> n_out with the 0 / 2^63 table of the S-box (its low n_out bits, three copies for 24): bit exact,
    and the outputs (zero masks: the body is the phase) decode to the S-box of each byte."""
    ctx, ok, spec = _set(request, which)
    f = lambda v: (aes_128.SBOX[v] * 0x10101) & ((1 << n_out) - 1)
    lut = oracle_mod.generate_lut(ok.p["N"], 8, n_out, f)
    out = _check(ctx, ok, spec, [aes_128.u8_to_bits(b) for b in BYTES], lut, n_out)
    for g, byte in enumerate(BYTES):
        assert not out[g, :, :-1].any()
        got = [((int(out[g, j, -1]) + (1 << 62)) & MASK) >> 63 for j in range(n_out)]
        assert got == [(f(byte) >> (n_out - 1 - j)) & 1 for j in range(n_out)], hex(byte)


@pytest.mark.parametrize("which,n_out", CASES)
def test_vertical_packing_trivial_ggsws_mixed_lut(request, which, n_out):
    ctx, ok, spec = _set(request, which)
    lut = _mixed_lut(np.random.default_rng(n_out), n_out, ok.p["N"])
    _check(ctx, ok, spec, [aes_128.u8_to_bits(b) for b in BYTES], lut, n_out)


NEGATED = ([-1] * 8, [-1, 1, 0, -1, 1, 1, 0, -1], [1, -1] * 4)


@pytest.mark.parametrize("which,n_out", CASES)
def test_vertical_packing_negated_ggsws(request, oracle_mod, which, n_out):
    """Selectors from {0, 1, -1}: a CMux with the GGSW of -1 subtracts the rotated difference, so the 0 / 2^63
    table's differences of 2^63 arrive at the torus tail as exactly -1/2 (test_edge_inputs.py pins that on
    the oracle).  Both LUTs, every output against the oracle."""
    ctx, ok, spec = _set(request, which)
    f = lambda v: (aes_128.SBOX[v] * 0x10101) & ((1 << n_out) - 1)
    for lut in (oracle_mod.generate_lut(ok.p["N"], 8, n_out, f),
                _mixed_lut(np.random.default_rng(100 + n_out), n_out, ok.p["N"])):
        _check(ctx, ok, spec, NEGATED, lut, n_out)


@pytest.mark.parametrize("which", ["lvl64", "8bit"])
def test_vertical_packing_saturation_on_the_fast_path(request, which):
    """The saturation inside torus_add_fast itself: one input, masked_ggsw(-1), 24 first_step_lut polynomials.
    The one CMux gives every lane a full-size value (no wave reaches the fallback) and, for most of the
    polynomials, exactly -1/2 at coefficient 0, the one the output extracts (both pinned on the oracle by
    test_edge_inputs.py::test_first_step_luts_reach_the_saturation_on_the_fast_path).  Two groups: the masked
    GGSW and the trivial GGSW of -1."""
    ctx, ok, spec = _set(request, which)
    Np = ok.p["N"]
    rng = np.random.default_rng(E.FIRST_STEP_SEED)
    lut = np.concatenate([E.first_step_lut(Np, rng) for _ in range(E.FIRST_STEP_LUTS)])
    groups = [ok.ggsw_to_fourier(E.masked_ggsw(ok.p, -1)), spec[-1]]
    out = _vertical_packing(ctx, ok, np.concatenate(groups), 2, 1, lut, E.FIRST_STEP_LUTS)
    for g, gf in enumerate(groups):
        for j in range(E.FIRST_STEP_LUTS):
            assert np.array_equal(out[g, j], ok.vertical_packing(lut[j * Np:(j + 1) * Np], gf, 1)), (g, j)


@pytest.mark.parametrize("which", ["lvl64", "8bit"])
@pytest.mark.parametrize("n_in", ["one", "log2N"])
def test_vertical_packing_input_counts(request, which, n_in):
    """n_in = 1 and n_in = log2 N (the largest count that needs no CMux tree), two outputs (a ragged workgroup
    of br512x4), the selector bits all zero, all one and mixed."""
    ctx, ok, spec = _set(request, which)
    n = 1 if n_in == "one" else E.log2_exact(ok.p["N"])
    rows = [[0] * n, [1] * n, [(0x2A7 >> (n - 1 - i)) & 1 for i in range(n)]]
    _check(ctx, ok, spec, rows, _mixed_lut(np.random.default_rng(n), 2, ok.p["N"]), 2)


@pytest.mark.parametrize("which", ["lvl64", "8bit"])
def test_ggsw_fourier_edge_words(request, which):
    """Three GGSWs in one call (N = 512: 75 polynomials, a ragged last block of the transform kernel): the
    trivial GGSWs of 0 and 1 and one made of the u64 -> f64 edge words; bit patterns equal the oracle's."""
    ctx, ok, _ = _set(request, which)
    ggsws = [E.trivial_ggsw(ok.p, 0), E.trivial_ggsw(ok.p, 1), E.crafted_ggsw(ok.p)]
    ref = np.concatenate([ok.ggsw_to_fourier(g) for g in ggsws])
    inp = np.concatenate(ggsws)
    out = np.zeros(ref.size * 2, dtype=np.float64)
    N.check(N.lib().tae_stage_ggsw_fourier(ctx._h, _vp(inp), 3, _vp(out), N.TAE_MEM_HOST))
    assert np.array_equal(out.view(np.uint64), ref.view(np.float64).view(np.uint64))
