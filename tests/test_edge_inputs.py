"""The crafted inputs of tests/edge_inputs.py really sit on the edges they are built for (CPU oracle only).
test_gpu_br_edges.py and test_gpu_vp_edges.py compare kernels with the oracle on these inputs; if a later
change to the builders moved them off the edges those tests would still pass, and this file would not."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_inputs as E

MASK = (1 << 64) - 1


@pytest.mark.parametrize("N,B", [(512, 12), (512, 6), (1024, 7)])
@pytest.mark.parametrize("transform", ["fft", "lf"])
def test_tie_digits_round_trip_hits_the_saturation(oracle_mod, N, B, transform):
    """One row of an external product with a noiseless GGSW of 1: digits +-2^(B-1) (the decomposition's tie)
    with random signs, times the gadget 2^(64-B) at coefficient 0, through the oracle's own transforms the way
    ext_product_add runs them (forward of the digits, product with the key spectrum -- rescaled by conj(E2)
    for the fused-twiddle transform, as lf_rescale does --, backward with the torus conversion).  The exact
    product is +-2^63 per coefficient: +1/2 of the torus converts to 2^63, -1/2 saturates to 2^63 - 1, and
    rounding moves the rest off by a few units.  Both exact values must occur."""
    rng = np.random.default_rng(N + B)
    digits = (rng.integers(0, 2, N).astype(np.int64) * 2 - 1) * np.int64(1 << (B - 1))
    gadget = np.zeros(N, dtype=np.uint64)
    gadget[0] = np.uint64(1 << (64 - B))
    key = oracle_mod.FFT(N).fwd_torus(gadget)
    if transform == "fft":
        t = oracle_mod.FFT(N)
    else:
        t = oracle_mod.LfTransform(N)
        key = key * t.conj_e2()
    out = t.add_bwd_torus(t.fwd_int(digits) * key, np.zeros(N, dtype=np.uint64))
    # every word within rounding of 2^63 (= -2^63) ...
    assert int((out - np.uint64((1 << 63) - (1 << 20))).max()) < 1 << 21, "round trip left the neighbourhood of 2^63"
    # ... and both exact conversions occur
    assert np.count_nonzero(out == np.uint64(1 << 63)) >= 1
    assert np.count_nonzero(out == np.uint64((1 << 63) - 1)) >= 1


@pytest.mark.parametrize("N,B", [(512, 12), (512, 6), (1024, 7)])
@pytest.mark.parametrize("m", [1, -1])
def test_top_digit_is_never_negative_so_the_key_needs_minus_one(oracle_mod, N, B, m):
    """What a difference of exactly 2^63 becomes in one blind-rotation step under a noiseless GGSW of m: the
    decomposer's top digit is +2^(B-1), never -2^(B-1), so m = 1 gives tail inputs of +1/2 (2^63, no
    saturation) and only m = -1 gives -1/2 (the saturated 2^63 - 1).  This is why key_pattern holds -1."""
    assert oracle_mod.decompose(1 << 63, B, 2)[0] == 1 << (B - 1)
    rng = np.random.default_rng(N + B + m)
    digits = rng.integers(0, 2, N).astype(np.int64) * np.int64(1 << (B - 1))  # 0 or the tie, as a real step
    gadget = np.zeros(N, dtype=np.uint64)
    gadget[0] = np.uint64((m << (64 - B)) & MASK)
    t = oracle_mod.LfTransform(N)
    key = oracle_mod.FFT(N).fwd_torus(gadget) * t.conj_e2()
    out = t.add_bwd_torus(t.fwd_int(digits) * key, np.zeros(N, dtype=np.uint64))
    hit, other = ((1 << 63), (1 << 63) - 1) if m == 1 else ((1 << 63) - 1, (1 << 63))
    assert np.count_nonzero(out == np.uint64(hit)) >= 1
    assert np.count_nonzero(out == np.uint64(other)) == 0


@pytest.mark.parametrize("m", [1, -1])
def test_vertical_packing_cmux_reaches_the_saturation(noiseless, m):
    """One CMux of the vertical packing (add_external_product_assign with the circuit bootstrap's levels)
    with the trivial GGSW of m on a difference of 0 / 2^63, the S-box table's: m = -1 yields words equal to
    2^63 - 1, m = 1 words equal to 2^63."""
    p, keys = noiseless
    k, N = p["k"], p["N"]
    diff = np.zeros((k + 1) * N, dtype=np.uint64)
    diff[k * N:] = np.random.default_rng(3).integers(0, 2, N).astype(np.uint64) << np.uint64(63)
    out = keys.external_product_add(keys.ggsw_to_fourier(E.trivial_ggsw(p, m)), p["cbs_l"], p["cbs_b"], diff,
                                    np.zeros((k + 1) * N, dtype=np.uint64))
    assert not out[:k * N].any()
    hit = (1 << 63) if m == 1 else (1 << 63) - 1
    assert np.count_nonzero(out[k * N:] == np.uint64(hit)) >= 1


def test_first_step_luts_reach_the_saturation_on_the_fast_path(noiseless):
    """A one-input vertical packing with masked_ggsw(-1) on the first_step_lut polynomials the GPU test uses:
    no word of the CMux's output, mask polynomials included, is small enough (|x| < 2^-12) for torus_add_fast
    to refuse, so no wave goes to the fallback; and for at least half of the polynomials the tail input at
    coefficient 0 is exactly -1/2: the extracted body is p[0] + 2^63 - 1."""
    p, keys = noiseless
    k, N = p["k"], p["N"]
    gf = keys.ggsw_to_fourier(E.masked_ggsw(p, -1))
    rng = np.random.default_rng(E.FIRST_STEP_SEED)
    hits = 0
    for _ in range(E.FIRST_STEP_LUTS):
        lut = E.first_step_lut(N, rng)
        diff = np.zeros((k + 1) * N, dtype=np.uint64)
        diff[k * N:] = np.concatenate([lut[1:], np.uint64(0) - lut[:1]]) - lut  # X^-1 p - p
        assert int(diff[k * N]) == 1 << 63
        out = keys.external_product_add(gf, p["cbs_l"], p["cbs_b"], diff, np.zeros((k + 1) * N, dtype=np.uint64))
        assert int(np.minimum(out, np.uint64(0) - out).min()) >= 1 << 52
        hits += int(keys.vertical_packing(lut, gf, 1)[-1]) == (int(lut[0]) + (1 << 63) - 1) & MASK
    assert hits >= E.FIRST_STEP_LUTS // 2, hits


@pytest.fixture(scope="module", params=["lvl64", "8bit"])
def noiseless(request, oracle_mod):
    """(params, oracle keys) of a set under (zero ksk, noiseless bsk, zero pfpksk): a bootstrap reads the bsk
    alone."""
    pid = oracle_mod.PARAMS_SQRD_LVL_64 if request.param == "lvl64" else oracle_mod.PARAMS_WOPPBS_8BIT
    p = oracle_mod.params(pid)
    L = oracle_mod.lib()
    pp = oracle_mod._Params()
    assert L.or_params_get(pid, C.byref(pp)) == 0
    ksk = np.zeros(L.or_ksk_len(C.byref(pp)), dtype=np.uint64)
    pf = np.zeros(L.or_pfpksk_len(C.byref(pp)), dtype=np.uint64)
    bsk = E.noiseless_bsk(p, E.key_pattern(p["n"]))
    assert bsk.size == L.or_bsk_len(C.byref(pp))
    return p, oracle_mod.Keys(pid, None, raw=(ksk, bsk, pf))


def test_key_pattern_has_runs_of_every_value():
    s = E.key_pattern(677)
    assert set(s.tolist()) == {0, 1, MASK}
    runs = np.diff(np.flatnonzero(s[1:] != s[:-1]))
    assert runs.min() >= 3  # runs, not isolated values: whole steps of exact zeros follow each other


def test_noiseless_bootstrap_stays_on_the_boundary(noiseless):
    """Keys.bootstrap under the noiseless key with the constant-2^62 LUT: the mask polynomials stay exactly
    zero (they take the fallback of the torus tail at every step) and the body ends within 2^32 of +-2^62,
    i.e. every step's differences were 0 or +-2^63 up to rounding."""
    p, keys = noiseless
    rng = np.random.default_rng(5)
    real = E.random_words(rng, (3, p["n"] + 1))
    rows = E.crafted_small(p["n"], p["N"], real, 0)
    lut = E.const_lut_glwe(p, 1 << 62)
    for i in (1, 3, 6, 9):
        out = keys.bootstrap(rows[i], lut)
        assert not out[:-1].any(), i
        body = int(out[-1])
        assert min((body - (1 << 62)) & MASK, ((1 << 62) - body) & MASK,
                   (body + (1 << 62)) & MASK, (-(1 << 62) - body) & MASK) < 1 << 32, (i, hex(body))


@pytest.mark.parametrize("n,N", [(677, 512), (785, 1024)])
@pytest.mark.parametrize("body_add", [0, 1 << 62])
def test_crafted_rows_rotation_amounts(oracle_mod, n, N, body_add):
    """or_pbs_modulus_switch of the crafted rows gives exactly what crafted_small's docstring promises."""
    ms = lambda x: int(oracle_mod.lib().or_pbs_modulus_switch(int(x) & MASK, N))
    real = E.random_words(np.random.default_rng(n), (3, n + 1))
    real[:, 0] |= np.uint64(1 << 60)  # keep the test's own 'real' masks away from zero
    rows = E.crafted_small(n, N, real, body_add)
    assert rows.shape == (E.CRAFTED_ROWS, n + 1) and rows.dtype == np.uint64
    u = E.rotation_unit(N)
    assert not rows[0, :n].any()
    assert [ms(x) for x in rows[1, :n]] == [0, N] * (n // 2) + [0] * (n % 2)
    assert all(ms(x) == 2 * N and x != 0 for x in rows[2, :n])
    assert all(ms(x) == 1 for x in rows[3, :n])
    assert int(rows[3, 0]) == u and int(rows[3, 1]) == u // 2
    assert ms(u // 2 - 1) == 0 and ms(u + u // 2 - 1) == 1 and ms(u + u // 2) == 2  # the boundaries themselves
    for r, src in ((4, 0), (5, 1)):
        assert not rows[r, :16].any() and np.array_equal(rows[r, 16:], real[src, 16:])
    assert np.array_equal(rows[6], real[2])
    for r, src, want in ((7, 0, 2 * N), (8, 1, 0), (9, 2, N)):
        assert np.array_equal(rows[r, :n], real[src, :n])
        assert ms(int(rows[r, n]) + body_add) == want, r
    assert (int(rows[7, n]) + body_add) & MASK == MASK
    assert (int(rows[8, n]) + body_add) & MASK == 0
    assert (int(rows[9, n]) + body_add) & MASK == 1 << 63


def test_trivial_ggsw_selects_through_vertical_packing(oracle_mod, noiseless):
    """Vertical packing over the trivial GGSWs of a byte's bits returns LUT entry `byte` (within rounding of
    0 / 2^63 for a generate_lut table), and all-zero spectra return entry 0 untouched."""
    from tfhe_aes import aes_128
    p, keys = noiseless
    N = p["N"]
    lut = oracle_mod.generate_lut(N, 8, 8, lambda v: aes_128.SBOX[v])
    spec = {b: keys.ggsw_to_fourier(E.trivial_ggsw(p, b)) for b in (0, 1)}
    assert not spec[0].any()
    for byte in (0x00, 0xFF, 0xA7):
        gf = np.concatenate([spec[b] for b in aes_128.u8_to_bits(byte)])
        outs = [keys.vertical_packing(lut[j * N:(j + 1) * N], gf, 8) for j in range(8)]
        assert all(not o[:-1].any() for o in outs)
        bodies = [int(o[-1]) for o in outs]
        assert all(min(b, (b - (1 << 63)) & MASK, ((1 << 63) - b) & MASK, (-b) & MASK) < 1 << 16 for b in bodies)
        assert aes_128.bits_to_u8([((b + (1 << 62)) & MASK) >> 63 for b in bodies]) == aes_128.SBOX[byte]
        if byte == 0:
            assert bodies == [int(lut[j * N]) for j in range(8)]


# ---- the CMux tree of wide LUTs (test_gpu_vp_tree.py) ----
def _tree_shapes(N):
    return [(t, n) for t in E.TREE_DEPTHS for n in E.TREE_N_OUT] + ([(E.DEEP_TREE, E.DEEP_N_OUT)] if N == 1024 else [])


@pytest.mark.parametrize("tree", E.TREE_DEPTHS)
def test_tree_selection_order(oracle_mod, noiseless, tree):
    """Under trivial selectors from {0, 1}, oracle.vertical_packing over a 2^tree-polynomial LUT has a zero mask
    and decodes to f(selector): selectors MSB first, the first `tree` GGSWs choosing the polynomial."""
    p, keys = noiseless
    N, n_out = p["N"], 3
    n_in = E.log2_exact(N) + tree
    small = N << tree
    f = E.tree_lut_fn(n_out)
    lut = oracle_mod.generate_lut(N, n_in, n_out, f)
    assert lut.size == n_out * small
    spec = {b: keys.ggsw_to_fourier(E.trivial_ggsw(p, b)) for b in (0, 1)}
    rows = E.tree_selector_rows(n_in)
    assert len({tuple(r[:tree]) for r in rows}) == (3 if tree > 1 else 2)  # the groups differ in the tree bits
    if tree > 1:  # and one of them reads differently backwards: the order of the tree's GGSWs matters
        assert any(r[:tree] != r[:tree][::-1] for r in rows)
    for row in rows:
        gf = np.concatenate([spec[b] for b in row])
        outs = [keys.vertical_packing(lut[j * small:(j + 1) * small], gf, n_in) for j in range(n_out)]
        assert all(not o[:-1].any() for o in outs)
        got = [((int(o[-1]) + (1 << 62)) & MASK) >> 63 for o in outs]
        v = E.selector_value(row)
        assert got == [(f(v) >> (n_out - 1 - j)) & 1 for j in range(n_out)], row
        # the polynomial is chosen by the leading bits alone: entry v sits in polynomial v >> log2 N
        assert int(lut[(v >> E.log2_exact(N)) * N + (v & (N - 1))]) == (((f(v) >> (n_out - 1)) & 1) << 63)


@pytest.mark.parametrize("N", [512, 1024])
@pytest.mark.parametrize("tree", E.TREE_DEPTHS)
@pytest.mark.parametrize("n_out", E.TREE_N_OUT)
def test_tree_negated_rows_reach_the_edge(oracle_mod, N, tree, n_out):
    """The 0 / 2^63 table under the negated rows.  Every group's leaf-level selector (position tree - 1) is 1 or
    -1 and both occur among the groups; the leaf-level nodes of every group and output combine polynomial pairs
    (2i, 2i + 1), and at least one of those differences has a coefficient of exactly 2^63 (every other one is 0):
    the tie digit, times the gadget of 1 or -1 a tail input of +1/2 or -1/2.  One level up the exact CMux values
    are 0 / 2^63 again (2^63 = -2^63), so the same holds for the upper levels up to the transform's rounding."""
    n_in = E.log2_exact(N) + tree
    rows = E.tree_negated_rows(n_in)
    assert all(set(r) <= {0, 1, -1} for r in rows)
    assert {r[tree - 1] for r in rows} == {1, -1}
    assert any(-1 in r[:tree] for r in rows) and any(-1 in r[tree:] for r in rows)
    assert tree == 1 or any(r[:tree] != r[:tree][::-1] for r in rows)
    lut = oracle_mod.generate_lut(N, n_in, n_out, E.tree_lut_fn(n_out)).reshape(n_out, 1 << tree, N)
    assert np.isin(lut, [0, 1 << 63]).all()
    for row in rows:            # the leaves are shared; the selector decides what a difference of 2^63 becomes
        assert row[tree - 1] in (1, -1)
        for j in range(n_out):
            diff = lut[j, 1::2] - lut[j, 0::2]
            assert np.isin(diff, [0, 1 << 63]).all()
            assert (diff == np.uint64(1 << 63)).any(), (row, j)


@pytest.mark.parametrize("N", [512, 1024])
def test_tree_mixed_lut_polynomials_differ(N):
    """Every polynomial of every output of the mixed LUT is different from every other, at every shape the GPU
    tests use, and the constant 2^62, full-size random words and runs of both are all present."""
    for tree, n_out in _tree_shapes(N):
        lut = E.tree_mixed_lut(n_out, N, tree, 7).reshape(n_out << tree, N)
        assert len({row.tobytes() for row in lut}) == len(lut), (tree, n_out)
        assert (lut[1] == np.uint64(1 << 62)).all()
        assert (lut[0] >> np.uint64(60)).max() == 15 and len(np.unique(lut[0])) > N // 2
        if len(lut) > 2:  # depth 1 with one output has two polynomials only
            runs = lut[2]
            assert (runs[:8] == np.uint64(1 << 62)).all() and not (runs[8:16] == np.uint64(1 << 62)).any()


# ---- shortint_1bit: the noiseless set, test-vector windows, packing sum (test_gpu_s1_edges.py) ----
S1_SEED = bytes(range(32))


@pytest.fixture(scope="module")
def s1_real(oracle_mod):
    """The real shortint_1bit keys: the oracle with its client key, and the raw server arrays."""
    ok = oracle_mod.S1Keys(S1_SEED, threads=8)
    return ok, ok.raw_server()


@pytest.fixture(scope="module")
def s1_noiseless(oracle_mod, s1_real):
    """(oracle on (real ksk, noiseless bsk, real packing key), the twelve input rows, the key pattern)."""
    ok, raw = s1_real
    p = ok.p
    s = E.key_pattern(p["n"])
    nl = oracle_mod.S1Keys(None, raw=(raw[0], E.noiseless_bsk(p, s), raw[2]))
    real = ok.s1_encrypt([0, 1, 1], S1_SEED, 150)
    rows = np.concatenate([E.crafted_small(p["n"], p["N"], real, 0),
                           E.random_words(np.random.default_rng(105), (2, p["n"] + 1))])
    return nl, rows, s


def test_monomial_mul_np_matches_the_exact_product(oracle_mod):
    """monomial_mul_np (the rotation of tv_from_polys_np and pack_np) against the oracle's exact negacyclic
    product with the monomial, for shifts on both sides of every wrap."""
    N = 512
    p = E.random_words(np.random.default_rng(12), N)
    for e in (0, 1, N // 4, N - 1, N, N + 1, 2 * N - 1, 2 * N, -1, -N):
        mono = np.zeros(N, dtype=np.int64)
        mono[e % N] = 1 if (e % (2 * N)) < N else -1
        assert np.array_equal(E.monomial_mul_np(p, e), oracle_mod.negacyclic_mul_exact(p, mono)), e


def test_s1_noiseless_steps_reach_the_tie_at_base_2_6(oracle_mod, s1_noiseless):
    """A CMux step on the accumulator the blind rotation starts from, computed exactly (an exact rotation of the
    constant 2^62), for the first 22 rotating steps of every row: the rotated difference X^a acc - acc holds words of
    exactly 2^63 and nothing else but zeros, the
    decomposition of 2^63 at 7 levels of 2^6 is [32, 0, ...] (the tie 2^(B-1)), and over the rows those steps meet
    key entries 1, -1 and 0; the 0 entry's GGSW is all zero, so that step adds exact zeros."""
    nl, rows, s = s1_noiseless
    p = nl.p
    n, N, B, lv = p["n"], p["N"], p["pbs_b"], p["pbs_l"]
    assert (lv, B) == (7, 6)
    assert oracle_mod.decompose(1 << 63, B, lv) == [1 << (B - 1)] + [0] * (lv - 1) == [32, 0, 0, 0, 0, 0, 0]
    ms = lambda x: int(oracle_mod.lib().or_pbs_modulus_switch(int(x) & MASK, N))
    bsk = E.noiseless_bsk(p, s).reshape(n, -1)
    assert not bsk[s == 0].any() and bsk[s != 0].any(axis=1).all()
    met = set()
    for r, row in enumerate(rows):
        acc = E.monomial_mul_np(np.full(N, 1 << 62, dtype=np.uint64), -ms(row[n]))
        steps = [i for i in range(n) if ms(row[i]) % (2 * N)]
        if r in (0, 2):  # the all-zero mask and the mask that rounds to 2N rotate nowhere
            assert not steps
            continue
        # every rotating step of the row on the accumulator it would meet first
        for i in steps[:22]:
            diff = E.monomial_mul_np(acc, ms(row[i])) - acc
            assert np.isin(diff, [0, 1 << 63]).all() and (diff == np.uint64(1 << 63)).any(), (r, i)
            met.add(int(s[i]))
    assert met == {0, 1, MASK}


def test_s1_noiseless_bootstrap_stays_on_the_boundary(s1_noiseless):
    """S1Keys.bootstrap_big (the blind rotation alone) under the noiseless key: with the constant-2^62 vector the
    mask stays exactly zero and the body ends within 2^32 of +-2^62 (every step's differences were 0 or +-2^63 up to
    rounding); with the constant-2^63 vector every difference is 2^64 = 0, every step adds exact zeros and the
    output is exactly 2^63.  The two outputs differ in the body alone: where the tie was taken."""
    nl, rows, _ = s1_noiseless
    tvs = E.noiseless_test_vectors(nl.p, np.random.default_rng(106))
    for i in (1, 3, 6, 9, 10, 11):
        out = nl.bootstrap_big(rows[i], tvs["const 2^62"])
        assert not out[:-1].any(), i
        body = int(out[-1])
        assert min((body - (1 << 62)) & MASK, ((1 << 62) - body) & MASK,
                   (body + (1 << 62)) & MASK, (-(1 << 62) - body) & MASK) < 1 << 32, (i, hex(body))
        flat = nl.bootstrap_big(rows[i], tvs["const 2^63"])
        assert not flat[:-1].any() and int(flat[-1]) == 1 << 63, i


def test_tv_window_polys_closed_form():
    """tv_from_polys_np on the window-edge pairs: a single coefficient gives single_coefficient_tv (each output
    coefficient is +-2^63 or +-(2^64 - 1) by the window of its shift), all ones against all 2^63 gives
    sum of signs times the window counts, and each of the seven positions puts another output coefficient on each
    window edge."""
    N = 512
    pairs = E.tv_window_polys(N)
    assert [name for name, _, _ in pairs] == [f"single {q}" for q in E.TV_WINDOW_POSITIONS(N)] + ["ones / 2^63", "random"]
    v0, v1 = E.TV_WINDOW_VALUES
    for pos, (_, p0, p1) in zip(E.TV_WINDOW_POSITIONS(N), pairs):
        assert np.count_nonzero(p0) == np.count_nonzero(p1) == 1 and int(p0[pos]) == v0 and int(p1[pos]) == v1
        tv = E.tv_from_polys_np(p0, p1)
        assert np.array_equal(tv, E.single_coefficient_tv(N, pos, v0, v1)), pos
        # the four window edges: shifts N/4 - 1 | N/4 and 3N/4 - 1 | 3N/4
        for i, v in ((N // 4 - 1, v0), (N // 4, v1), (3 * N // 4 - 1, v1), (3 * N // 4, v0), (0, v0), (N - 1, v0)):
            t = (pos + i) % N
            assert int(tv[t]) == (v if pos + i < N else (-v) & MASK), (pos, i)
    _, ones, halves = pairs[-2]
    tv = E.tv_from_polys_np(ones, halves)
    # coefficient t: shifts i <= t count +1, the others -1; N/2 shifts take 2^63 each (an even count: 0 mod 2^64)
    for t in (0, 1, N // 4 - 1, N // 4, 3 * N // 4 - 1, 3 * N // 4, N - 1):
        plus = sum(1 for i in range(N) if not (N // 4 <= i < 3 * N // 4) and i <= t)
        assert int(tv[t]) == (2 * plus - N // 2) & MASK, t
    _, r0, r1 = pairs[-1]
    ref = np.zeros(N, dtype=np.uint64)
    for t in range(0, N, 37):  # the definition, coefficient by coefficient, in Python integers
        acc = 0
        for i in range(N):
            src = r1 if N // 4 <= i < 3 * N // 4 else r0
            acc += int(src[t - i]) if t >= i else -int(src[t - i + N])
        assert int(E.tv_from_polys_np(r0, r1)[t]) == acc & MASK, t


def test_tv_and_pack_references_equal_the_oracle(s1_real):
    """tv_from_polys_np and pack_np on the oracle's packing keyswitches of real ciphertexts equal S1Keys.tv_from_cts
    and S1Keys.pack (the reference's add-then-rotate loops) under the real key."""
    ok, _ = s1_real
    N = ok.p["N"]
    cts = ok.s1_encrypt([1, 0, 1, 1, 0], S1_SEED, 900)
    P = np.stack([ok.pks(c) for c in cts]).reshape(len(cts), -1, N)
    for a, b in ((0, 1), (2, 3), (4, 4)):
        assert np.array_equal(E.tv_from_polys_np(P[a], P[b]).reshape(-1), ok.tv_from_cts(cts[a], cts[b])), (a, b)
    for count in (1, 2, 5):
        assert np.array_equal(E.pack_np(P[:count]).reshape(-1), ok.pack(cts[:count])), count


def test_asymmetric_tables():
    """The function tables of the selector-tree tests: no permutation or complement of the input bits fixes
    them; parity (the table the existing tests use most) is fixed by every permutation."""
    for nbits in (4, 8):
        for seed in (0, 1):
            tab = E.asymmetric_table(nbits, seed)
            assert len(tab) == 1 << nbits and set(tab) == {0, 1} and E.is_asymmetric_table(tab, nbits)
    assert E.asymmetric_table(8, 0) != E.asymmetric_table(8, 1)
    assert not E.is_asymmetric_table([bin(v).count("1") % 2 for v in range(16)], 4)
    assert not E.is_asymmetric_table([1, 0, 0, 1, 0, 1, 1, 0], 3)
    assert not E.is_asymmetric_table([bin(v).count("1") % 2 for v in range(256)], 8)


# ---- extract_bits of the 8-bit model (test_gpu_extract8_edges.py) ----
def test_extract_bits_tie_rows_are_on_the_edge(oracle_keys8):
    """Trivial ints (zero mask) with the body on either side of the rounding boundary of bit 0: the shift to the
    MSB and the keyswitch of a zero mask give the trivial small LWE of body << 7, i.e. v 2^63 + 2^62 - 128 below the
    boundary and v 2^63 + 2^62 on it, which decode to v & 1 and to its complement: the extracted bits differ."""
    n = oracle_keys8.p["n"]
    for v in (0x00, 0xFF, 0x80):
        rows = E.extract_tie_ints(oracle_keys8.K, v)
        below, tie = (oracle_keys8.extract_bits(rows[i]) for i in (1, 2))
        for out, body in ((below, rows[1, -1]), (tie, rows[2, -1])):
            assert not out[7, :n].any() and int(out[7, n]) == (int(body) << 7) & MASK
        assert int(tie[7, n]) - int(below[7, n]) == 128
        bit = lambda row: ((int(row[n]) + (1 << 62)) & MASK) >> 63
        assert bit(below[7]) == v & 1 and bit(tie[7]) == 1 - (v & 1)
        assert list(oracle_keys8.decrypt_small_bits(below[7:])) == [v & 1]
        assert list(oracle_keys8.decrypt_small_bits(tie[7:])) == [1 - (v & 1)]
