"""The shortint_1bit model (Engine::s1_*, br512x4::br_kernel<7, true, 6>) on crafted inputs and shape edges, word for
word against the oracle, against plain numpy references (tests/edge_inputs.py) or against the composition of stage
calls that are themselves pinned here.  Everything is integer-exact: no tolerance anywhere.

  * the noiseless bootstrapping key at 7 levels of 2^6 (the tie 32, tail inputs of +-1/2, the i64 saturation, exact
    zeros), B = 13 = 3 + 3 + 3 + 3 + 1, n_tv = 1 and 3;
  * lut_mod shapes: lut_mod == B, a lut_mod that wraps inside a workgroup of three, n_tv > B, n_tv = 3 with B = 4;
  * s1_tv_kernel: the zero packing key turns an LWE into the trivial GLWE of its body, so the window edges
    [0, N/4) u [3N/4, N) / [N/4, 3N/4) are read off the output; the pattern key gives dense polynomials, compared
    with N explicit rotations (tv_from_polys_np) and with the oracle, 9 pairs (45 workgroups) in one call;
  * s1_pack_kernel + the packing GEMM: count = 1, 2, TM - 1, TM, TM + 1, 511, 512, and the refused 0 and 513;
  * the selector tree for 1, 2 and 4 bits against the oracle, for 8 and 3 bits with two functions and several
    groups against the composition gather -> bootstrap -> test vectors; chunked runs with a ragged last chunk;
  * the AES layer and the key schedule at L = 641 against the composition of those stages and numpy u64 sums.

test_edge_inputs.py pins, on the CPU, that the inputs are on those edges and that the numpy references equal the
oracle's loops.
"""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tfhe_aes import shortint_1bit as S
from tests import edge_inputs as E
from tests.conftest import ROOT, SEED

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
P5 = tfhe_aes.PARAMS_SHORTINT_1BIT
U64 = np.uint64
A1 = aes_128.Shortint1BitSboxPbsAesEncrypt


def _ksgemm_tm() -> int:
    with open(os.path.join(ROOT, "tfhe-aes-2_amd", "csrc", "ksgemm.hpp")) as fh:
        return int(re.search(r"constexpr int TM = (\d+)", fh.read()).group(1))


TM = _ksgemm_tm()


class _Env:
    """Set environment variables, then restore them."""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class S1Set:
    """One key generation of set 5; the crafted key sets (noiseless bsk; pattern and zero keyswitch keys with a zero
    bsk), one oracle and one context per key set, made on first use and kept for the module."""

    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.ck, real = tfhe_aes.generate_keys_raw(P5, SEED, threads=THREADS)
        self.p = tfhe_aes.get_params(P5)
        self.n, self.Np, self.L = self.p["n"], self.p["N"], self.p["n"] + 1
        self.glwe = (self.p["k"] + 1) * self.p["N"]
        self._raw = {"real": real}
        self._ok, self._ctx, self._pks = {}, {}, {}

    def raw(self, key):
        if key not in self._raw:
            ksk, bsk, pk = self._raw["real"]
            if key == "noiseless":
                self._raw[key] = (ksk, E.noiseless_bsk(self.p, E.key_pattern(self.n)), pk)
            else:
                make = {"pattern": E.pattern_key, "zero": E.zero_key}[key]
                if "zero_bsk" not in self._raw:
                    self._raw["zero_bsk"] = np.zeros(len(bsk), dtype=U64)
                self._raw[key] = (make(len(ksk)), self._raw["zero_bsk"], make(len(pk)))
        return self._raw[key]

    def ok(self, key):
        if key not in self._ok:
            self._ok[key] = self.oracle_mod.S1Keys(None, raw=self.raw(key))
        return self._ok[key]

    def ctx(self, key):
        if key not in self._ctx:
            self._ctx[key] = tfhe_aes.context_from_raw(P5, self.raw(key), device=0)
        return self._ctx[key]

    def pks(self, key, row):
        """S1Keys.pks of one row [(k+1)][N], once per (key, row)."""
        k = (key, row.tobytes())
        if k not in self._pks:
            self._pks[k] = self.ok(key).pks(row).reshape(-1, self.Np)
        return self._pks[k]

    def keyswitch_rows(self, count, start):
        """Rows cycling through the decomposer edge row, the saturating row and real ciphertexts."""
        p = self.p
        rows = self.ck.encrypt_bits_raw(np.arange(count) & 1, start_index=start)
        rows[0::3] = E.edge_row(p["pfks_b"], p["pfks_l"], self.L)
        rows[1::3] = U64(E.saturating_coefficient(p["pfks_b"], p["pfks_l"], "bytes"))
        return rows


@pytest.fixture(scope="module")
def s1(oracle_mod):
    return S1Set(oracle_mod)


class BootRefs:
    """S1Keys.bootstrap per distinct (row, test vector), on a thread pool (ctypes drops the GIL)."""

    def __init__(self, ok):
        self.ok, self.cache = ok, {}

    def get(self, pairs):
        keys = [(r.tobytes(), t.tobytes()) for r, t in pairs]
        todo = {k: p for k, p in zip(keys, pairs) if k not in self.cache}
        if todo:
            with ThreadPoolExecutor(THREADS) as ex:
                for k, ref in zip(todo, ex.map(lambda p: self.ok.bootstrap(p[0], p[1]), todo.values())):
                    self.cache[k] = ref
        return [self.cache[k] for k in keys]


def _check_bootstrap(ctx, refs, rows, tvs, what):
    out = S.bootstrap_raw(ctx, rows, tvs)
    ref = refs.get([(rows[b], tvs[b % len(tvs)]) for b in range(len(rows))])
    for b in range(len(rows)):
        assert np.array_equal(out[b], ref[b]), (what, b)


# ---- br512x4<7, true, 6> ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(s1):
    real = s1.ck.encrypt_bits_raw([0, 1, 1], start_index=150)
    return E.crafted_small(s1.n, s1.Np, real, 0)


@pytest.fixture(scope="module")
def noiseless(s1, crafted):
    rng = np.random.default_rng(105)
    rows = np.concatenate([crafted, E.random_words(rng, (2, s1.L))])
    return rows, E.noiseless_test_vectors(s1.p, rng), BootRefs(s1.ok("noiseless"))


@pytest.mark.parametrize("which", ["const 2^62", "const 2^63", "random", "all three"])
def test_noiseless_key_s1(s1, noiseless, which):
    """(real ksk, noiseless bsk, real packing key): thirteen ciphertexts (the twelve rows, the first repeated; the
    last workgroup holds one) with one test vector, then with all three in one call (ciphertext b takes b % 3)."""
    rows, tvs, refs = noiseless
    batch = np.resize(rows, (13, s1.L))
    t = np.stack(list(tvs.values())) if which == "all three" else tvs[which][None]
    _check_bootstrap(s1.ctx("noiseless"), refs, batch, t, which)


@pytest.fixture(scope="module")
def real_refs(s1):
    rng = np.random.default_rng(107)
    ok = s1.ok("real")
    tvs = [ok.tv_from_fn(1, 0), ok.tv_from_fn(0, 1), ok.tv_from_fn(1, 1)] + [E.random_words(rng, s1.glwe) for _ in range(4)]
    return np.stack(tvs), BootRefs(ok)


@pytest.mark.parametrize("B,n_tv", [(7, 7), (7, 5), (2, 4), (4, 3)])
def test_lut_mod_shapes(s1, crafted, real_refs, B, n_tv):
    """Per-ciphertext test vectors under the real key on the crafted rows: lut_mod == B (the shape of every inner
    tree level), a lut_mod that wraps inside a workgroup of three (ciphertexts 3, 4, 5 take vectors 3, 4, 0), more
    vectors than ciphertexts, and three vectors over a batch of four."""
    tvs, refs = real_refs
    _check_bootstrap(s1.ctx("real"), refs, np.resize(crafted, (B, s1.L)), tvs[:n_tv], (B, n_tv))


# ---- s1_tv_kernel ------------------------------------------------------------------------------------------------
def test_tv_window_edges_zero_key(s1):
    """Under the zero packing key the packing keyswitch of an LWE is the trivial GLWE with the LWE's body at
    coefficient 0 of the body polynomial, whatever its mask: the test vector's body holds b0 on
    [0, N/4) u [3N/4, N) and b1 on [N/4, 3N/4) (shift i moves coefficient 0 to i, never across the wrap), and its
    masks are zero.  Bodies 2^63, 2^64 - 1, 1 and a random word, every ordered pair of them."""
    rng = np.random.default_rng(108)
    bodies = [1 << 63, E.MASK64, 1, int(E.random_words(rng, 1)[0])]
    pairs = [(a, b) for a in bodies for b in bodies]
    ct0, ct1 = E.random_words(rng, (len(pairs), s1.L)), E.random_words(rng, (len(pairs), s1.L))
    ct0[:, -1] = np.array([a for a, _ in pairs], dtype=U64)
    ct1[:, -1] = np.array([b for _, b in pairs], dtype=U64)
    tv = S.test_vectors_from_ciphertexts(s1.ctx("zero"), ct0, ct1).reshape(len(pairs), -1, s1.Np)
    Np = s1.Np
    for i, (a, b) in enumerate(pairs):
        assert not tv[i, :-1].any(), i
        want = np.full(Np, a, dtype=U64)
        want[Np // 4:3 * Np // 4] = U64(b)
        assert np.array_equal(tv[i, -1], want), (i, hex(a), hex(b))


def test_tv_dense_polynomials_pattern_key(s1):
    """Under the pattern key every polynomial of a packing keyswitch is dense: 9 pairs in one call (45 workgroups;
    polynomial c = 0 of pair 0 and c = k of pair 8 included) of the decomposer edge row, the saturating row and
    real ciphertexts equal N explicit rotations of the oracle's keyswitches (tv_from_polys_np) and the oracle's own
    add-then-rotate loops (S1Keys.tv_from_cts)."""
    pool = s1.keyswitch_rows(6, 340_000)
    a, b = pool[np.arange(9) % 6], pool[(2 * np.arange(9) + 1) % 6]
    tv = S.test_vectors_from_ciphertexts(s1.ctx("pattern"), a, b)
    ok = s1.ok("pattern")
    for i in range(9):
        want = E.tv_from_polys_np(s1.pks("pattern", a[i]), s1.pks("pattern", b[i])).reshape(-1)
        assert np.array_equal(tv[i], want), i
        assert np.array_equal(tv[i], ok.tv_from_cts(a[i], b[i])), i


# ---- s1_pack_kernel + the packing keyswitch GEMM -----------------------------------------------------------------
PACK_COUNTS = (1, 2, TM - 1, TM, TM + 1, 511, 512)


@pytest.mark.parametrize("key", ["pattern", "real"])
def test_packing_keyswitch_counts(s1, key):
    """count = 1, 2, TM - 1, TM, TM + 1, 511, 512 with TM = 128 (ksgemm::TM, the GEMM's row tile, against the 2560
    key columns): the rotate-and-add of count keyswitched GLWEs equals pack_np of the oracle's keyswitches, and up
    to three ciphertexts S1Keys.pack itself."""
    assert TM == 128
    rows = s1.keyswitch_rows(512, 350_000)
    ctx, ok = s1.ctx(key), s1.ok(key)
    P = np.stack([s1.pks(key, r) for r in rows])
    for count in PACK_COUNTS:
        got = S.packing_keyswitch(ctx, rows[:count])
        assert np.array_equal(got, E.pack_np(P[:count]).reshape(-1)), (key, count)
        if count <= 3:
            assert np.array_equal(got, ok.pack(rows[:count])), (key, count)


def test_packing_keyswitch_zero_key_and_refused_counts(s1):
    """Zero key, count = N = 512: body coefficient j is the body of ciphertext j and the masks are zero.  count = 0
    and count = 513 are refused on the host with TAE_E_ARG, and the next call on the context is still right."""
    rows = E.random_words(np.random.default_rng(109), (513, s1.L))
    ctx = s1.ctx("zero")
    want = np.zeros(s1.glwe, dtype=U64)
    want[-s1.Np:] = rows[:512, -1]
    assert np.array_equal(S.packing_keyswitch(ctx, rows[:512]), want)
    for bad in (rows[:0], rows):
        with pytest.raises(tfhe_aes.TaeError) as e:
            S.packing_keyswitch(ctx, bad)
        assert e.value.code == N.TAE_E_ARG
        assert np.array_equal(S.packing_keyswitch(ctx, rows[:512]), want)


# ---- the selector tree -------------------------------------------------------------------------------------------
def _mvs(tables, nbits):
    return [S.MultivariateTestVector(nbits, t) for t in tables]


def compose_tree(s1, ctx, bits, tables):
    """calculate_multivariate_function as stage calls: per level, gather the selector bit of each row's group in
    numpy, bootstrap with the level's vectors (one per row from level 1 on), pair the results into the next
    level's vectors.  bits [G][nbits][L] -> [G][n_fn][L]."""
    G, nbits, _ = bits.shape
    n_fn, V = len(tables), 1 << (nbits - 1)
    ok = s1.ok("real")
    tvs = np.stack([ok.tv_from_fn(t[2 * v], t[2 * v + 1]) for t in tables for v in range(V)])
    for sel in range(nbits - 1, -1, -1):
        B = G * n_fn * V
        rows = bits[np.arange(B) // (n_fn * V), sel]
        out = S.bootstrap_raw(ctx, rows, tvs)
        if V == 1:
            return out.reshape(G, n_fn, -1)
        tvs = S.test_vectors_from_ciphertexts(ctx, out[0::2], out[1::2])
        V //= 2


def _group_bits(s1, values, nbits, start):
    flat = [(v >> (nbits - 1 - i)) & 1 for v in values for i in range(nbits)]
    return s1.ck.encrypt_bits_raw(flat, start_index=start).reshape(len(values), nbits, -1)


@pytest.mark.parametrize("nbits,tables,values", [(1, ([0, 1], [1, 0]), (0, 1)),
                                                 (2, ([0, 0, 1, 0], [0, 1, 1, 1]), (0b01, 0b10))])
def test_selector_tree_small_against_the_oracle(s1, nbits, tables, values):
    """nbits = 1 (one bootstrap, no packing level) and 2, one group per call, against S1Keys.multivariate."""
    ctx, ok = s1.ctx("real"), s1.ok("real")
    bits = _group_bits(s1, values, nbits, 360_000 + 16 * nbits)
    cases = [(g, t) for g in range(len(values)) for t in tables]
    with ThreadPoolExecutor(THREADS) as ex:
        refs = list(ex.map(lambda c: ok.multivariate(bits[c[0]], c[1]), cases))
    for (g, t), ref in zip(cases, refs):
        got = S.calculate_multivariate_function_raw(ctx, bits[g][None], _mvs([t], nbits))[0, 0]
        assert np.array_equal(got, ref), (nbits, values[g], t)
        assert s1.ck.decrypt_bits_raw(got[None])[0] == t[values[g]]


def test_selector_tree_4_bits_asymmetric_against_the_oracle(s1):
    """nbits = 4, one group, a table that no permutation or complement of the bits fixes, on an input whose bits
    read differently backwards: 15 oracle bootstraps."""
    table, value = E.asymmetric_table(4), 0b0010
    bits = _group_bits(s1, [value], 4, 361_000)
    got = S.calculate_multivariate_function_raw(s1.ctx("real"), bits, _mvs([table], 4))[0, 0]
    assert np.array_equal(got, s1.ok("real").multivariate(bits[0], table))
    assert s1.ck.decrypt_bits_raw(got[None])[0] == table[value]


@pytest.mark.parametrize("nbits,G", [(8, 3), (3, 4)])
def test_selector_tree_against_the_stage_composition(s1, nbits, G):
    """Two functions over G groups, word for word the composition of the stage calls pinned above (gather in numpy,
    bootstrap_raw with n_tv = batch, test_vectors_from_ciphertexts).  8 bits: asymmetric tables, 768 rows at the
    first level; 3 bits: G = 4."""
    tables = [E.asymmetric_table(nbits, 0), E.asymmetric_table(nbits, 1)] if nbits > 3 else \
        [[1, 0, 0, 1, 0, 1, 1, 0], [0, 0, 0, 1, 0, 1, 1, 1]]
    values = [(0xB5 * (g + 1) + g) & ((1 << nbits) - 1) for g in range(G)]
    bits = _group_bits(s1, values, nbits, 362_000 + 100 * nbits)
    ctx = s1.ctx("real")
    got = S.calculate_multivariate_function_raw(ctx, bits, _mvs(tables, nbits))
    assert np.array_equal(got, compose_tree(s1, ctx, bits, tables))
    if nbits == 3:  # at 8 bits the testing parameters' noise may flip a decryption
        for g, v in enumerate(values):
            assert [s1.ck.decrypt_bits_raw(got[g, f][None])[0] for f in range(2)] == [t[v] for t in tables]


def test_chunk_edges(s1):
    """n_fn = 2, nbits = 3 (8 rows per group), G = 5 with TAE_S1_ROWS = 16 (chunks of 2, 2 and 1 groups), 1 (a budget
    below one group: one group per chunk) and 100000 (one chunk): the three outputs are word for word equal, and
    equal the stage composition.  TAE_S1_ROWS = 0 and = x raise when the call runs."""
    tables = [[1, 0, 0, 1, 0, 1, 1, 0], [0, 0, 0, 1, 0, 1, 1, 1]]
    values = [0b011, 0b110, 0b101, 0b000, 0b111]
    bits = _group_bits(s1, values, 3, 363_000)
    outs = {}
    for rows in ("16", "1", "100000"):
        with _Env(TAE_S1_ROWS=rows):
            ctx = tfhe_aes.context_from_raw(P5, s1.raw("real"), device=0)
            outs[rows] = S.calculate_multivariate_function_raw(ctx, bits, _mvs(tables, 3))
            del ctx
    assert np.array_equal(outs["16"], outs["100000"]) and np.array_equal(outs["1"], outs["100000"])
    assert np.array_equal(outs["100000"], compose_tree(s1, s1.ctx("real"), bits, tables))
    for bad in ("0", "x"):
        with _Env(TAE_S1_ROWS=bad):
            with pytest.raises(tfhe_aes.TaeError):
                S.calculate_multivariate_function_raw(s1.ctx("real"), bits, _mvs(tables, 3))
    assert np.array_equal(S.calculate_multivariate_function_raw(s1.ctx("real"), bits, _mvs(tables, 3)), outs["16"])


# ---- the AES layer at L = 641 ------------------------------------------------------------------------------------
KEY, IV = bytes.fromhex("76b8e0ada0f13d90405d6ae55386bd28"), bytes.fromhex("bdd219b8a08ded1a")
SBOX_TABLES = [[(aes_128.SBOX[x] >> (7 - f)) & 1 for x in range(256)] for f in range(8)]


def _sub_bytes(ctx, state):
    """[n_bytes * 8][L] -> [n_bytes][8][L]: the eight S-box bit functions of every byte."""
    return S.calculate_multivariate_function_raw(ctx, state.reshape(-1, 8, state.shape[-1]), _mvs(SBOX_TABLES, 8))


def _shift_rows(sb):
    """[16][8][L] -> [16][8][L]: byte 4c + row comes from byte 4((c + row) % 4) + row."""
    return sb[[4 * ((c + row) % 4) + row for c in range(4) for row in range(4)]]


def test_aes_rounds_against_the_stage_composition(s1, oracle_mod):
    """aes_round0_kernel, aes8_mix_kernel and aes_final_kernel at L = n + 1 = 641: one block, rounds = 1 and 2, word
    for word the composition round 0 = rk0 + block, SubBytes = the multivariate call with the eight S-box bit
    tables over 16 groups, middle layer = ShiftRows + the oracle's mix_column_terms + round key in numpy u64, final
    step = ShiftRows + rk10.  (Two rounds need not decrypt to AES with the testing parameters; words only.)"""
    ctx, L = s1.ctx("real"), s1.L
    ek = b"".join(aes_128.key_schedule_plain(KEY))
    rk = s1.ck.encrypt_bits_raw([b for byte in ek for b in aes_128.u8_to_bits(byte)], start_index=10_000)
    block = s1.ck.encrypt_bits_raw(aes_128.blocks_to_bits(aes_128.counter_blocks(IV, 1)), start_index=20_000)
    rk = rk.reshape(11, 16, 8, L)
    sb1 = _sub_bytes(ctx, rk[0].reshape(128, L) + block)
    want1 = _shift_rows(sb1) + rk[10]
    got1 = A1.encrypt_blocks_raw(ctx, rk.reshape(-1, L), block.reshape(1, 128, L), rounds=1)
    assert np.array_equal(got1[0], want1.reshape(128, L))
    terms = oracle_mod.mix_column_terms()
    cols = _shift_rows(sb1).reshape(4, 32, L)  # [column][byte-major bit][L]
    mixed = np.zeros_like(cols)
    for o in range(32):
        for i in range(32):
            for _ in range(int(terms[o, i])):
                mixed[:, o] += cols[:, i]
    state1 = mixed.reshape(16, 8, L) + rk[1]
    want2 = _shift_rows(_sub_bytes(ctx, state1.reshape(128, L))) + rk[10]
    got2 = A1.encrypt_blocks_raw(ctx, rk.reshape(-1, L), block.reshape(1, 128, L), rounds=2)
    assert np.array_equal(got2[0], want2.reshape(128, L))


def test_key_schedule_first_words_against_the_stage_composition(s1):
    """Words 4..7 of the FHE key schedule at L = 641: w4 = w0 + SubWord(RotWord(w3)) + Rcon (the model's trivial bit:
    2^62 on the body), w5..w7 = w(i-4) + w(i-1) on the words before their bootstrap, then one identity-vector
    bootstrap per bit of the four words."""
    ctx, L = s1.ctx("real"), s1.L
    kb = s1.ck.encrypt_bits_raw([b for byte in KEY for b in aes_128.u8_to_bits(byte)], start_index=30_000)
    w = kb.reshape(4, 4, 8, L)  # [word][byte][bit][L]
    rot = w[3][[1, 2, 3, 0]]
    w4 = w[0] + _sub_bytes(ctx, rot.reshape(32, L))
    w4[0, :, L - 1] += np.array(aes_128.u8_to_bits(0x01), dtype=U64) << U64(62)
    w5 = w[1] + w4
    w6 = w[2] + w5
    w7 = w[3] + w6
    pre = np.stack([w4, w5, w6, w7]).reshape(128, L)
    want = S.bootstrap_raw(ctx, pre, s1.ok("real").tv_from_fn(0, 1)[None])
    got = A1.key_schedule_raw(ctx, kb)
    assert np.array_equal(got[:128], kb)
    assert np.array_equal(got[128:256], want)
