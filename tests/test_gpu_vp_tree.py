"""Vertical packing of LUTs wider than one polynomial (n_in > log2 N: Engine::vertical_packing_tree) on crafted
inputs, word for word against the oracle, on params_sqrd_lvl_64 (N = 512) and the 8-bit set (N = 1024).

This path alone runs vp_leaves_kernel, cmux_tree_kernel, the generic vp_kernel<N> and the generic
ext_product_step<N> (decomp_digit, the plain from_torus tail, the radix transform, the ct1 form of the CMux):
every set has a specialised vertical-packing kernel for n_in <= log2 N, which test_gpu_vp_edges.py covers.

One tae_stage_vertical_packing call (host memory: the entry point stages the [n_out][N << tree] LUT) runs three
groups whose selectors differ in the tree bits, so the group stride of the tree levels, the GGSW group index and,
from depth 2, both ping-pong buffers take part; n_out = 3 makes the output index ragged.  The GGSWs are noiseless
trivial ones of 0, 1 and -1 (tests/edge_inputs.py): all-zero spectra add exact zeros, and with the 0 / 2^63 table
a leaf difference is 0 or exactly 2^63, i.e. the decomposer's tie digit and a tail input of +1/2 under the GGSW
of 1 and -1/2 (the i64 saturation of from_torus) under -1; test_edge_inputs.py pins those on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from tfhe_aes import _native as N
from tests import edge_inputs as E

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1
CASES = [(w, t, n) for w in ("lvl64", "8bit") for t in E.TREE_DEPTHS for n in E.TREE_N_OUT]


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


def _check(ctx, ok, spec, rows, lut, n_out):
    """One call over len(rows) groups; every output against oracle.vertical_packing.  Returns the outputs."""
    n_in = len(rows[0])
    small = ok.p["N"] << (n_in - E.log2_exact(ok.p["N"]))
    lut = np.ascontiguousarray(lut, dtype=np.uint64)
    assert lut.size == n_out * small
    groups = [np.concatenate([spec[b] for b in row]) for row in rows]
    gfd = np.ascontiguousarray(np.concatenate(groups)).view(np.float64)
    out = np.zeros((len(groups), n_out, ok.K + 1), dtype=np.uint64)
    N.check(N.lib().tae_stage_vertical_packing(ctx._h, _vp(gfd), len(groups), n_in, _vp(lut), n_out, _vp(out),
                                               N.TAE_MEM_HOST))
    for g, gf in enumerate(groups):
        for j in range(n_out):
            ref = ok.vertical_packing(lut[j * small:(j + 1) * small], gf, n_in)
            assert np.array_equal(out[g, j], ref), (g, j)
    return out


@pytest.mark.parametrize("which,tree,n_out", CASES)
def test_tree_trivial_selectors_bit_lut(request, oracle_mod, which, tree, n_out):
    """The 0 / 2^63 table of a hash of the selector: bit exact, and the outputs (zero masks: the body is the
    phase) decode to f(selector), selectors MSB first with the first `tree` GGSWs choosing the polynomial."""
    ctx, ok, spec = _set(request, which)
    n_in = E.log2_exact(ok.p["N"]) + tree
    f = E.tree_lut_fn(n_out)
    rows = E.tree_selector_rows(n_in)
    out = _check(ctx, ok, spec, rows, oracle_mod.generate_lut(ok.p["N"], n_in, n_out, f), n_out)
    for g, row in enumerate(rows):
        assert not out[g, :, :-1].any()
        got = [((int(out[g, j, -1]) + (1 << 62)) & MASK) >> 63 for j in range(n_out)]
        assert got == [(f(E.selector_value(row)) >> (n_out - 1 - j)) & 1 for j in range(n_out)], row


@pytest.mark.parametrize("which,tree,n_out", CASES)
def test_tree_trivial_selectors_mixed_lut(request, which, tree, n_out):
    """Pairwise different polynomials (2^62, random words, runs of both): a leaf, pair, output or group mix-up
    changes the result."""
    ctx, ok, spec = _set(request, which)
    n_in = E.log2_exact(ok.p["N"]) + tree
    _check(ctx, ok, spec, E.tree_selector_rows(n_in), E.tree_mixed_lut(n_out, ok.p["N"], tree, 10 * tree + n_out),
           n_out)


@pytest.mark.parametrize("which,tree,n_out", CASES)
def test_tree_negated_selectors(request, oracle_mod, which, tree, n_out):
    """Selectors from {0, 1, -1}, -1 at tree positions too: with the 0 / 2^63 table the leaf differences of
    exactly 2^63 reach the plain from_torus tail as +1/2 and as -1/2.  Both LUTs, every output against the
    oracle."""
    ctx, ok, spec = _set(request, which)
    n_in = E.log2_exact(ok.p["N"]) + tree
    for lut in (oracle_mod.generate_lut(ok.p["N"], n_in, n_out, E.tree_lut_fn(n_out)),
                E.tree_mixed_lut(n_out, ok.p["N"], tree, 100 + 10 * tree + n_out)):
        _check(ctx, ok, spec, E.tree_negated_rows(n_in), lut, n_out)


def test_tree_depth_6_grid_stride_leaves(request):
    """n_in = 16 at N = 1024: a 64-polynomial base, the shape of the 16 -> 8 LUT.  The leaf array has
    2 x 64 x 3072 words, more than the 1024 x 256 threads of vp_leaves_kernel, so its grid-stride loop goes
    round; six tree levels alternate the ping-pong buffers three times.  Two groups (a {0, 1} and a
    {0, 1, -1} selector), the mixed LUT."""
    ctx, ok, spec = _set(request, "8bit")
    assert ok.p["N"] == 1024
    n_in = 10 + E.DEEP_TREE
    assert E.DEEP_N_OUT * (1 << E.DEEP_TREE) * (ok.p["k"] + 1) * 1024 > 1024 * 256
    rows = [E.tree_selector_rows(n_in)[2], E.tree_negated_rows(n_in)[1]]
    _check(ctx, ok, spec, rows, E.tree_mixed_lut(E.DEEP_N_OUT, 1024, E.DEEP_TREE, 6), E.DEEP_N_OUT)


@pytest.mark.parametrize("n_in,n_out", [(0, 1), (10, 0), ("deep", 1)])
def test_stage_vertical_packing_argument_errors(gpu_context, n_in, n_out):
    """n_in = 0, n_out = 0 and a tree deeper than the entry point's cap (log2 N + 16 inputs) are TAE_E_ARG,
    decided before anything is staged: the buffers here are far too small for any of the calls."""
    if n_in == "deep":
        n_in = 9 + 17
    buf = np.zeros(16, dtype=np.uint64)
    rc = N.lib().tae_stage_vertical_packing(gpu_context._h, _vp(buf.view(np.float64)), 1, n_in, _vp(buf), n_out,
                                            _vp(buf), N.TAE_MEM_HOST)
    assert rc == N.TAE_E_ARG
