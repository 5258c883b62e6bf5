"""The crafted keyswitch inputs of tests/edge_inputs.py sit on the edges they are built for (CPU only).
test_gpu_ks_edges.py compares the integer keyswitch kernels (ksgemm.hpp, keyswitch_kernel, pfks_kernel) with the
oracle on these inputs; this file pins the inputs themselves: the decomposer edge words against oracle.decompose,
the limb models against the definitions the kernels implement, and the saturating rows against the accumulator
bounds that ksgemm.hpp states, computed here from get_params."""
import os
import re
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tests import edge_inputs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
PIDS = {"lvl_1": tfhe_aes.PARAMS_SQRD_LVL_1, "lvl_4": tfhe_aes.PARAMS_SQRD_LVL_4, "lvl_64": tfhe_aes.PARAMS_SQRD_LVL_64,
        "lvl_256": tfhe_aes.PARAMS_SQRD_LVL_256, "8bit": tfhe_aes.PARAMS_WOPPBS_8BIT,
        "shortint_1bit": tfhe_aes.PARAMS_SHORTINT_1BIT}
MFMA_PFKS = ("lvl_4", "lvl_64", "lvl_256", "8bit")  # the sets whose PFKS runs on the int8 GEMMs


def _p(name):
    return tfhe_aes.get_params(PIDS[name])


def test_ks_shapes_are_those_of_the_parameter_sets():
    shapes = set()
    for name in PIDS:
        p = _p(name)
        shapes |= {(p["ks_b"], p["ks_l"]), (p["pfks_b"], p["pfks_l"])}
    assert shapes == set(E.KS_SHAPES)


@pytest.mark.parametrize("B,L", E.KS_SHAPES)
def test_edge_words_decompose_as_named(oracle_mod, B, L):
    words, named = E.decomposer_edge_words(B, L), E.edge_word_digits(B, L)
    assert list(words) == list(named)
    for name, x in words.items():
        assert 0 <= x <= MASK
        assert oracle_mod.decompose(x, B, L) == named[name], (name, hex(x))
    half = 1 << (B - 1)
    seen = {d for digits in named.values() for d in digits}
    assert {0, 1, half, -half + 1, -1} <= seen and (L == 1 or -half in seen)
    # the tie is exact: one less rounds down, and the word is half a unit of the last level
    assert words["tie"] * 2 == 1 << (64 - B * L) and words["tie_below"] == words["tie"] - 1
    # the numpy model used by the GPU test's assertions and by the searches below is the oracle's decomposition
    row = np.concatenate([E.edge_row(B, L, 64), E.random_words(np.random.default_rng(B * 10 + L), 4000)])
    model = E.digits_np(row, B, L)
    for x, d in zip(row.tolist(), model.tolist()):
        assert oracle_mod.decompose(x, B, L) == d, hex(x)


def test_limb_chain_words_recombine():
    words = E.limb_chain_words()
    assert len(words) == 13 and len(set(words)) == 13
    for w in words:
        for sh in (0, 8, 16, 24):
            v = (w << sh) & MASK
            limbs = E.key_limbs_np(np.uint64(v)).tolist()
            assert all(-128 <= b <= 127 for b in limbs)
            assert sum(b << (8 * j) for j, b in enumerate(limbs)) & MASK == v, (hex(w), sh)
    assert E.key_limbs_np(np.uint64(0x7F7F7F7F7F7F7F80)).tolist() == [-128] * 8
    assert E.key_limbs_np(np.uint64(0x7F7F7F7F7F7F7F7F)).tolist() == [127] * 8
    assert E.key_limbs_np(np.uint64(MASK)).tolist() == [-1] + [0] * 7  # the carry runs through all eight bytes
    assert E.key_limbs_np(np.uint64(0x8080808080808080)).tolist() == [-128] + [-127] * 7
    # the saturating word keeps -128 from the shifted position up
    for m in (1, 2):
        assert E.key_limbs_np(np.uint64((E.SATURATING_WORD << (8 * m)) & MASK)).tolist() == [0] * m + [-128] * (8 - m)


def test_pattern_key_period_divides_no_stride():
    period = len(E.limb_chain_words())
    assert period == 13
    for name in PIDS:
        p = _p(name)
        glwe, K = (p["k"] + 1) * p["N"], p["k"] * p["N"]
        strides = [p["n"] + 1, glwe, (K + 1) * p["pfks_l"] * glwe]
        assert all(s % period for s in strides), (name, strides)
        assert max(p["ks_l"], p["pfks_l"]) < period
        key = E.pattern_key(3 * (p["n"] + 1)).reshape(3, p["n"] + 1)
        assert (key[0] != key[1]).all() and (key[1] != key[2]).all() and (key[0, :-1] != key[0, 1:]).all()


def test_kslots_mirror_equals_the_compiled_plan(tmp_path):
    """kslots_plan restates kslots_build in numpy; the native test prints the plan the kernels use."""
    exe = str(tmp_path / "kslots_test")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "kslots_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, "1000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = 0
    for line in r.stdout.splitlines():
        m = re.match(r"2\^(\d+) x (\d+)( \(no clamp\))?: S = (\d+), limbs/level(.*)", line)
        if not m:
            continue
        plan = E.kslots_plan(int(m.group(1)), int(m.group(2)), allow_clamp=not m.group(3))
        levels = re.findall(r" (\d+) \(c = (-?\d+)(, clamped)?\)", m.group(5))
        assert plan["S"] == int(m.group(4)), line
        assert [(n, c, bool(cl)) for n, c, cl in
                zip(plan["nlimb"], plan["off"], plan["clamp"])] == [(int(n), int(c), bool(cl)) for n, c, cl in levels], line
        seen += 1
    assert seen == 4


# ---- saturating rows against the accumulator bounds of ksgemm.hpp --------------------------------------------
def _saturated_maximum(B, L, model, n_coef):
    """Largest |partial sum| of a row of saturating_coefficient against a column of saturating_key."""
    x = E.saturating_coefficient(B, L, model)
    row = np.full(n_coef, x, dtype=np.uint64)
    sums = E.modelled_partial_sums(row, E.saturating_key(n_coef * L), B, L, model)
    return x, int(np.abs(sums).max())


@pytest.mark.parametrize("name", MFMA_PFKS)
def test_saturating_row_reaches_the_k_layout_bound(name):
    """K layout (prep_digits_kl / prep_key_kl / gemm_g6<.., true> / gemm_g7): ksgemm.hpp bounds every i32 sum by
    128 * 128 * S * (K + 1).  By hand: base 2^16 x 2 (S = 4, offsets 129 and, on the clamped level, 128) stores the
    digits -32767 and -32768 of the coefficient 0x8000800000000000 as -32896 = (-128, -128) twice: every slot at
    -128, the bound itself, on the key limbs j >= 1 (limb 0 of a pre-shifted key row is zero).  Base 2^12 x 3
    (S = 6) holds digits up to 2048 in two bytes, so the upper limb stays within +-8 and the best digit
    -1920 = (-128, -7) gives 135 / 256 = 0.527."""
    p = _p(name)
    B, L, n_coef = p["pfks_b"], p["pfks_l"], p["k"] * p["N"] + 1
    bound = 128 * 128 * E.kslots_plan(B, L)["S"] * n_coef
    x, got = _saturated_maximum(B, L, "kslots", n_coef)
    print(f"{name} K layout: coefficient {x:#018x}, modelled max |sum| {got} = {got / bound:.4f} of {bound}")
    assert bound < 1 << 31 and got < 1 << 31
    assert 2 * got >= bound
    assert got <= bound


@pytest.mark.parametrize("name", MFMA_PFKS)
def test_saturating_row_reaches_the_row_layout_bound(name):
    """Row layout (prep_digits3<6> + gemm_g6<6, 4>): limb rows of 6 bits, bound 2^(LB-1) * 128 * Kd with LB = 6 and
    Kd = (K + 1) pfks_l.  The lowest limb row reaches -32 in every column: the bound itself."""
    p = _p(name)
    B, L, n_coef = p["pfks_b"], p["pfks_l"], p["k"] * p["N"] + 1
    bound = (1 << 5) * 128 * n_coef * L
    x, got = _saturated_maximum(B, L, "rows6", n_coef)
    print(f"{name} row layout: coefficient {x:#018x}, modelled max |sum| {got} = {got / bound:.4f} of {bound}")
    assert bound < 1 << 31 and got < 1 << 31
    assert 2 * got >= bound
    assert got <= bound


@pytest.mark.parametrize("name,which", [(n, "ks") for n in ("lvl_4", "lvl_64", "lvl_256", "8bit", "shortint_1bit")]
                         + [("shortint_1bit", "pks")])
def test_saturating_row_of_the_byte_digit_gemm(name, which):
    """prep_digits<1, 8> + gemm<1, 8> (LWE keyswitch; packing keyswitch of shortint_1bit): one byte per digit, so
    the header's bound is 2^(LB-1) * 128 * Kd with LB = 8.  No input reaches half of it, and the bar is not lowered
    for convenience but because none can: a digit of base 2^b is at most 2^(b-1) (b = 2, 3 or 6 here), not the 2^7
    a byte could hold, so no ciphertext produces more than 2^(b-1) * 128 * Kd = 2^(b-8) of the header's bound
    (2^-5 at base 2^3).  Neighbouring levels cannot both hold +2^(b-1) (the carry rule turns the lower one into
    -2^(b-1)), so the search alternates 2^(b-1) and 2^(b-1) - 1.  The saturating row must reach at least half of
    that digit-range ceiling, and the header's bound must hold."""
    p = _p(name)
    B, L = (p["ks_b"], p["ks_l"]) if which == "ks" else (p["pfks_b"], p["pfks_l"])
    n_coef = p["k"] * p["N"] if which == "ks" else p["n"]
    header = (1 << 7) * 128 * n_coef * L
    ceiling = (1 << (B - 1)) * 128 * n_coef * L  # = header >> (8 - B)
    x, got = _saturated_maximum(B, L, "bytes", n_coef)
    print(f"{name} {which}: coefficient {x:#018x}, modelled max |sum| {got} = {got / ceiling:.4f} of the digit-range "
          f"ceiling {ceiling} = {got / header:.5f} of {header}")
    assert header < 1 << 31 and got < 1 << 31
    assert ceiling << (8 - B) == header
    assert 2 * got >= ceiling and got <= ceiling


def test_random_rows_sit_far_below_the_bounds():
    """What the suite had before: uniform keys and coefficients give sums of about 2^20 (the reason for the
    crafted keys)."""
    p = _p("lvl_64")
    n_coef = p["k"] * p["N"] + 1
    rng = np.random.default_rng(5)
    sums = E.modelled_partial_sums(E.random_words(rng, n_coef), E.random_words(rng, n_coef * 2), 16, 2, "kslots")
    assert int(np.abs(sums).max()) < 1 << 23
