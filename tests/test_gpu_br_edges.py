"""Every blind-rotation kernel on crafted inputs (tests/edge_inputs.py), word for word against the oracle.

Real ciphertexts under real keys give the torus tail of a CMux step (torus_add_fast* + the wave-uniform
from_torus_bits fallback, fft_device.hpp) inputs that are in effect uniform: the fallback, the i64 saturation
and the refused high dword 0x80000000 then never occur.  Here they occur at every step:

  * crafted masks under the real key (rotation amounts 0, N, 2N, the rounding boundary, zeroed mask words,
    bodies that switch to 0, N and 2N) on every kernel selection of Engine::bootstrap;
  * a noiseless bootstrapping key (trivial GGSWs of a fixed pattern of 0, 1 and -1) handed to both the
    product and the oracle: mask polynomials stay exactly zero (fallback) while the body takes the fast
    path, and with the constant-2^62 LUT every non-zero difference is 2^63: the top digit is the tie
    2^(B-1), the tail input +1/2 under a GGSW of 1 and -1/2, the i64 saturation, under a GGSW of -1;
  * tae_stage_bootstrap (generic LUT GLWE, nothing added to the body) under both keys.

test_edge_inputs.py pins, on the CPU oracle, that the inputs are on those edges.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import shortint_1bit as S
from tests import edge_inputs as E
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
P64 = tfhe_aes.PARAMS_SQRD_LVL_64
P8 = tfhe_aes.PARAMS_WOPPBS_8BIT
SHIFT_ADD = 1 << 62  # homomorphic_shift_boolean adds 2^62 to the body before the modulus switch

# kernel selections (environment read by context_from_raw; every variable is set, then restored)
LVL64_KERNELS = {
    "br512lat": {"TAE_BR_LAT_MAX": "256", "TAE_PBS_KERNEL": "x4"},
    "br512x4": {"TAE_BR_LAT_MAX": "0", "TAE_PBS_KERNEL": "x4"},
    "br512p16": {"TAE_BR_LAT_MAX": "0", "TAE_PBS_KERNEL": "p16"},
}


def _b1k(lat="1", pair="1", occ2="0", wide="1"):
    return {"TAE_B1K_LAT": lat, "TAE_B1K_PAIR": pair, "TAE_B1K_OCC2": occ2, "TAE_B1K_WIDE": wide}


# name -> (environment, batch size): the batch sizes of test_pbs8_kernel_variants_bit_exact (256 CUs)
B1K_KERNELS = {
    "br1024lat": (_b1k(), 10),
    "br1024_one_paired": (_b1k(lat="0"), 10),
    "br1024_one_unpaired": (_b1k(lat="0", pair="0"), 10),
    "br1024_two": (_b1k(), 513),
    "br1024_occ2": (_b1k(occ2="1"), 513),
    "br1024w": (_b1k(), 1027),
    "br1024_two_1027": (_b1k(wide="0"), 1027),
}
# the noiseless-key runs: every kernel source once, a one-per-workgroup and a batched form per set
B1K_NOISELESS = ["br1024lat", "br1024_one_paired", "br1024_two", "br1024w"]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _context(pid, keys, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tfhe_aes.context_from_raw(pid, keys, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _shift(ctx, small, level, big_len):
    small = np.ascontiguousarray(small)
    out = np.zeros((len(small), big_len), dtype=np.uint64)
    N.check(N.lib().tae_stage_pbs_shift_boolean(ctx._h, _vp(small), len(small), level, _vp(out), N.TAE_MEM_HOST))
    return out


def _bootstrap(ctx, small, lut_glwe, big_len):
    small = np.ascontiguousarray(small)
    out = np.zeros((len(small), big_len), dtype=np.uint64)
    N.check(N.lib().tae_stage_bootstrap(ctx._h, _vp(small), len(small), _vp(lut_glwe), _vp(out), N.TAE_MEM_HOST))
    return out


class Refs:
    """Oracle results, computed once per distinct input row on a thread pool (ctypes drops the GIL) and
    shared by the parametrisations that run the same rows through different kernels."""

    def __init__(self, fn):
        self.fn, self.cache = fn, {}

    def get(self, rows):
        keys = [r.tobytes() for r in rows]
        todo = {k: r for k, r in zip(keys, rows) if k not in self.cache}
        if todo:
            with ThreadPoolExecutor(THREADS) as ex:
                for k, ref in zip(todo, ex.map(self.fn, todo.values())):
                    self.cache[k] = ref
        return [self.cache[k] for k in keys]


def _assert_rows(out, rows, refs, idx, what):
    for i, ref in zip(idx, refs.get([rows[i] for i in idx])):
        assert np.array_equal(out[i], ref), (what, i)


# ---- crafted masks under the real key ----------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted64(product_raw, oracle_keys):
    cts = product_raw[0].encrypt_bits_raw(np.array([1, 0, 1], dtype=np.uint8), start_index=71_000)
    real = np.stack([oracle_keys.keyswitch(c) for c in cts])
    rows = E.crafted_small(677, 512, real, SHIFT_ADD)
    return real, rows, Refs(lambda r: oracle_keys.homomorphic_shift_boolean(r, 1))


@pytest.mark.parametrize("kernel", list(LVL64_KERNELS))
def test_crafted_masks_lvl64(product_raw, crafted64, kernel):
    """params_sqrd_lvl_64: br512lat (ten workgroups of one), br512x4 (3 + 3 + 3 + 1), br512p16 (five of two)."""
    _, rows, refs = crafted64
    ctx = _context(P64, product_raw[1], LVL64_KERNELS[kernel])
    out = _shift(ctx, rows, 1, 4 * 512 + 1)
    _assert_rows(out, rows, refs, range(len(rows)), kernel)
    del ctx


@pytest.fixture(scope="module")
def crafted8(product_raw8, oracle_keys8):
    """1027 real small LWEs of the 8-bit set, the ten crafted rows built from the first three, and the level-2
    references."""
    bits = np.random.default_rng(1027).integers(0, 2, size=1027).astype(np.uint8)
    pool = product_raw8[0].encrypt_bits_raw(bits, start_index=910_000)
    rows = E.crafted_small(785, 1024, pool[:3], SHIFT_ADD)
    return pool, rows, Refs(lambda r: oracle_keys8.homomorphic_shift_boolean(r, 2))


def _place_crafted(pool, rows, B):
    """A batch of B: real ciphertexts with the crafted rows at the start, across a workgroup boundary (from
    index 101 on: the workgroups of two or four that hold 100..103 and 108..111 mix crafted and real
    ciphertexts) and at the end (the ragged last workgroup holds crafted rows only).  Returns the batch and
    the indices to compare: every crafted row, the first and the last real one."""
    n = len(rows)
    if B == n:
        return rows.copy(), list(range(n))
    batch = pool[:B].copy()
    starts = (0, 101, B - n)
    for s in starts:
        batch[s:s + n] = rows
    idx = [i for s in starts for i in range(s, s + n)] + [n, B - n - 1]
    return batch, sorted(idx)


@pytest.mark.parametrize("kernel", list(B1K_KERNELS))
def test_crafted_masks_8bit(product_raw8, crafted8, kernel):
    """The 8-bit set at CBS level 2 on every N = 1024 selection of Engine::bootstrap."""
    pool, rows, refs = crafted8
    env, B = B1K_KERNELS[kernel]
    ctx = _context(P8, product_raw8[1], env)
    batch, idx = _place_crafted(pool, rows, B)
    out = _shift(ctx, batch, 2, 2 * 1024 + 1)
    _assert_rows(out, batch, refs, idx, kernel)
    del ctx


@pytest.mark.parametrize("pid", [tfhe_aes.PARAMS_SQRD_LVL_1, tfhe_aes.PARAMS_SQRD_LVL_4,
                                 tfhe_aes.PARAMS_SQRD_LVL_256])
def test_crafted_masks_other_n1024_sets(pid, oracle_mod):
    """br1024's lvl_1, lvl_4 (2 x 2^15) and lvl_256 (4 x 2^9) instantiations, one ciphertext per workgroup."""
    ck, keys = tfhe_aes.generate_keys_raw(pid, SEED, threads=THREADS)
    ctx = tfhe_aes.context_from_raw(pid, keys, device=0)
    ok = oracle_mod.Keys(pid, None, raw=keys)
    p = tfhe_aes.get_params(pid)
    cts = ck.encrypt_bits_raw([1, 0, 1], start_index=91)
    real = np.stack([ok.keyswitch(c) for c in cts])
    rows = E.crafted_small(p["n"], p["N"], real, SHIFT_ADD)
    out = _shift(ctx, rows, 1, p["k"] * p["N"] + 1)
    _assert_rows(out, rows, Refs(lambda r: ok.homomorphic_shift_boolean(r, 1)), range(len(rows)), pid)
    del ctx


def test_crafted_masks_shortint1(oracle_mod):
    """br512x4<7, true, 6> through tae_s1_bootstrap: ten crafted ciphertexts (3 + 3 + 3 + 1), two test vectors
    (ciphertext b takes tvs[b % 2]: the lut_mod = 2 path), against FheContext::bootstrap of the oracle."""
    P5 = tfhe_aes.PARAMS_SHORTINT_1BIT
    ck, keys = tfhe_aes.generate_keys_raw(P5, SEED, threads=THREADS)
    ctx = tfhe_aes.context_from_raw(P5, keys, device=0)
    ok = oracle_mod.S1Keys(None, raw=keys)
    real = ck.encrypt_bits_raw([0, 1, 1], start_index=150)
    rows = E.crafted_small(ok.p["n"], ok.p["N"], real, 0)
    tvs = np.stack([ok.tv_from_fn(1, 0), ok.tv_from_fn(0, 1)])
    out = S.bootstrap_raw(ctx, rows, tvs)
    with ThreadPoolExecutor(THREADS) as ex:
        ref = list(ex.map(lambda b: ok.bootstrap(rows[b], tvs[b % 2]), range(len(rows))))
    for b in range(len(rows)):
        assert np.array_equal(out[b], ref[b]), b
    del ctx


# ---- tae_stage_bootstrap under the real key ------------------------------------------------------------
@pytest.mark.parametrize("which", ["lvl64", "8bit"])
def test_stage_bootstrap_random_lut_real_key(request, which):
    """tae_stage_bootstrap (body_add = out_add = 0) with a random LUT GLWE, mask and body, on the crafted
    rows built for body_add = 0, on the default contexts (br512lat / br1024lat)."""
    if which == "lvl64":
        ctx, ok = request.getfixturevalue("gpu_context"), request.getfixturevalue("oracle_keys")
        cts = request.getfixturevalue("product_raw")[0].encrypt_bits_raw([0, 1, 1], start_index=72_000)
        real = np.stack([ok.keyswitch(c) for c in cts])
    else:
        ctx, ok = request.getfixturevalue("gpu_context8"), request.getfixturevalue("oracle_keys8")
        real = request.getfixturevalue("product_raw8")[0].encrypt_bits_raw([0, 1, 1], start_index=920_000)
    p = ok.p
    rows = E.crafted_small(p["n"], p["N"], real, 0)
    lut = E.random_words(np.random.default_rng(64), (p["k"] + 1) * p["N"])
    out = _bootstrap(ctx, rows, lut, ok.K + 1)
    _assert_rows(out, rows, Refs(lambda r: ok.bootstrap(r, lut)), range(len(rows)), which)


# ---- noiseless bootstrapping key -----------------------------------------------------------------------
NOISELESS_ROWS = 12


class Noiseless:
    """(real ksk, noiseless bsk, real pfpksk) for one set, the oracle built from the same arrays, twelve input
    rows (the ten crafted ones and two random) and the three LUT GLWEs of tae_stage_bootstrap."""

    def __init__(self, oracle_mod, pid, raw, real):
        self.pid = pid
        p = self.p = oracle_mod.params(pid)
        self.raw = (raw[0], E.noiseless_bsk(p, E.key_pattern(p["n"])), raw[2])
        self.ok = oracle_mod.Keys(pid, None, raw=self.raw)
        self.big = p["k"] * p["N"] + 1
        rng = np.random.default_rng(pid + 100)
        self.rows = np.concatenate([E.crafted_small(p["n"], p["N"], real, SHIFT_ADD),
                                    E.random_words(rng, (NOISELESS_ROWS - E.CRAFTED_ROWS, p["n"] + 1))])
        self.luts = {"const 2^62": E.const_lut_glwe(p, 1 << 62), "const 2^63": E.const_lut_glwe(p, 1 << 63),
                     "random": E.random_words(rng, (p["k"] + 1) * p["N"])}
        self.shift_refs = {lv: Refs(lambda r, lv=lv: self.ok.homomorphic_shift_boolean(r, lv)) for lv in (1, 2)}
        self.lut_refs = {name: Refs(lambda r, lut=lut: self.ok.bootstrap(r, lut)) for name, lut in self.luts.items()}

    def check(self, ctx, B, level, what):
        """(a) pbs_shift_boolean and (b) the three generic LUTs on a batch of B made of the twelve rows
        repeated; every output row against the oracle."""
        batch = np.resize(self.rows, (B, self.rows.shape[1]))
        ref = self.shift_refs[level].get(self.rows)
        out = _shift(ctx, batch, level, self.big)
        for i in range(B):
            assert np.array_equal(out[i], ref[i % NOISELESS_ROWS]), (what, "shift_boolean", i)
        for name, lut in self.luts.items():
            ref = self.lut_refs[name].get(self.rows)
            out = _bootstrap(ctx, batch, lut, self.big)
            for i in range(B):
                assert np.array_equal(out[i], ref[i % NOISELESS_ROWS]), (what, name, i)


@pytest.fixture(scope="module")
def noiseless64(oracle_mod, product_raw, crafted64):
    return Noiseless(oracle_mod, P64, product_raw[1], crafted64[0])


@pytest.fixture(scope="module")
def noiseless8(oracle_mod, product_raw8, crafted8):
    return Noiseless(oracle_mod, P8, product_raw8[1], crafted8[0][:3])


@pytest.mark.parametrize("kernel", list(LVL64_KERNELS))
def test_noiseless_key_lvl64(noiseless64, kernel):
    """Thirteen ciphertexts per kernel: the last workgroup of br512x4 (three each) and of br512p16 (two each)
    holds one."""
    ctx = _context(P64, noiseless64.raw, LVL64_KERNELS[kernel])
    noiseless64.check(ctx, NOISELESS_ROWS + 1, 1, kernel)
    del ctx


@pytest.mark.parametrize("kernel", B1K_NOISELESS)
def test_noiseless_key_8bit(noiseless8, kernel):
    env, B = B1K_KERNELS[kernel]
    ctx = _context(P8, noiseless8.raw, env)
    noiseless8.check(ctx, max(B, NOISELESS_ROWS), 2, kernel)
    del ctx
