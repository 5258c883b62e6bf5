"""Every integer keyswitch kernel on crafted keys and crafted inputs (tests/edge_inputs.py), word for word against
the oracle's u64 loops (Keys.keyswitch, Keys.pfks, S1Keys.pack) built with raw= on the same key arrays.

Real keys are uniform words: the i32 accumulators of the int8 GEMMs (ksgemm.hpp) then stay near 2^20 and key limb
carry chains stay short.  Here

  * pattern_key: thirteen words with long limb carry chains, repeated with a period that divides no stride of any
    key layout -- an index mix-up, a dropped limb carry or a wrong pre-shift (prep_key_kl) changes words;
  * saturating_key (every limb -128) against rows of saturating_coefficient: the accumulators reach the bounds the
    header derives (test_ks_edge_inputs.py pins the modelled maxima) -- a narrower accumulator or another K split
    changes words;
  * decomposer_edge_words in row 0 of every batch: ties, wraps, residues of exactly half the base with and without
    the carry, the carry through every level, both ends of the top level (and the clamp tie of the K layout);
  * rows on both sides of the tile edges (127 / 128 of the byte-digit and the row-layout GEMM, 383 / 384 of the K
    layout), body-only rows (the ragged last N tile holds the body column of the LWE keyswitch), one-row batches.

The bootstrapping key of a crafted context is all zeros; no test here bootstraps.  Tests are ordered by parameter
set: the `sets` fixture holds the keys, oracles and shared contexts of one set at a time.
test_ks_edge_inputs.py pins, on the CPU, that the inputs are on those edges.
"""
import ctypes as C
import os

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tests import edge_inputs as E
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
PIDS = {"lvl_1": tfhe_aes.PARAMS_SQRD_LVL_1, "lvl_4": tfhe_aes.PARAMS_SQRD_LVL_4, "lvl_64": tfhe_aes.PARAMS_SQRD_LVL_64,
        "lvl_256": tfhe_aes.PARAMS_SQRD_LVL_256, "8bit": tfhe_aes.PARAMS_WOPPBS_8BIT,
        "shortint_1bit": tfhe_aes.PARAMS_SHORTINT_1BIT}
SESSION_SETS = {"lvl_64": ("product_raw", "oracle_keys", "gpu_context"),
                "8bit": ("product_raw8", "oracle_keys8", "gpu_context8")}
VARIANTS = ("g6", "s16", "w32", "w16")
DEFAULT = "w16"  # the K-layout kernel of a context without TAE_PFKS_GEMM
ROWS = {"TAE_PFKS_LAYOUT": "rows"}
KL = {"TAE_PFKS_LAYOUT": "k"}
BODIES = (0, 1 << 63, E.MASK64)
U64 = np.uint64


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


class KeySet:
    """One parameter set: the client key and the real server keys, the crafted keys, one oracle per key, and the
    contexts that several tests share (the session's default context; one TAE_PFKS_LAYOUT=rows context per key)."""

    def __init__(self, oracle_mod, name, client, real, real_oracle=None, session_ctx=None):
        self.oracle_mod, self.name, self.pid, self.client = oracle_mod, name, PIDS[name], client
        self.p = tfhe_aes.get_params(self.pid)
        self.K = self.p["k"] * self.p["N"]
        self.glwe = (self.p["k"] + 1) * self.p["N"]
        self._raw = {"real": real}
        self._oracle = {"real": real_oracle} if real_oracle is not None else {}
        self._rows_ctx, self._session_ctx, self._pfks_ref = {}, session_ctx, {}

    def raw(self, key):
        if key not in self._raw:
            ksk, bsk, pfpksk = self._raw["real"]
            make = {"pattern": E.pattern_key, "saturating": E.saturating_key}[key]
            self._raw[key] = (make(len(ksk)), np.zeros(len(bsk), dtype=U64), make(len(pfpksk)))
        return self._raw[key]

    def oracle(self, key):
        if key not in self._oracle:
            if self.name == "shortint_1bit":
                self._oracle[key] = self.oracle_mod.S1Keys(None, raw=self.raw(key))
            else:
                self._oracle[key] = self.oracle_mod.Keys(self.pid, None, raw=self.raw(key))
        return self._oracle[key]

    def context(self, key, rows=False):
        """The context the keyswitch tests run on: the session's for the real key (where the session has one),
        otherwise, and with rows=True always, one built with TAE_PFKS_LAYOUT=rows and kept for the set."""
        if key == "real" and not rows and self._session_ctx is not None:
            return self._session_ctx
        if key not in self._rows_ctx:
            self._rows_ctx[key] = _context(self.pid, self.raw(key), ROWS)
        return self._rows_ctx[key]

    def new_context(self, key, env):
        return _context(self.pid, self.raw(key), env)

    def pfks_ref(self, key, q, row):
        """Keys.pfks of one row, computed once per (key, q, row)."""
        k = (key, q, row.tobytes())
        if k not in self._pfks_ref:
            self._pfks_ref[k] = self.oracle(key).pfks(q, row)
        return self._pfks_ref[k]

    def release(self):
        self._rows_ctx.clear()
        self._oracle.clear()
        self._raw.clear()
        self._pfks_ref.clear()


@pytest.fixture(scope="module")
def sets(request, oracle_mod):
    class Sets:
        current = None

        def get(self, name):
            if self.current is not None and self.current.name == name:
                return self.current
            if self.current is not None:
                self.current.release()
            if name in SESSION_SETS:
                raw, ok, ctx = (request.getfixturevalue(f) for f in SESSION_SETS[name])
                self.current = KeySet(oracle_mod, name, raw[0], raw[1], ok, ctx)
            else:
                client, keys = tfhe_aes.generate_keys_raw(PIDS[name], SEED, threads=THREADS)
                self.current = KeySet(oracle_mod, name, client, keys)
            return self.current

    s = Sets()
    yield s
    if s.current is not None:
        s.current.release()


# ---- inputs ----------------------------------------------------------------------------------------------------
def crafted_batch(B, n_words, base_log, levels, limb_model, filler, sat_row, body_row):
    """[B][n_words] made of `filler` (real ciphertexts or random words) with
      row 0         decomposer_edge_words repeated (body included);
      rows 2, 3, 4  only the last word (the body) non-zero: 0, 2^63, 2^64 - 1 (B > 4);
      sat_row       saturating_coefficient(limb_model) in every word;
      body_row      only the body non-zero: 2^63.
    Returns the batch and the rows to compare: those, and the untouched row 1."""
    batch = np.ascontiguousarray(filler[:B], dtype=U64).copy()
    assert batch.shape == (B, n_words)
    batch[0] = E.edge_row(base_log, levels, n_words)
    idx = [0]
    if B > 4:
        for r, body in zip((2, 3, 4), BODIES):
            batch[r] = 0
            batch[r, -1] = U64(body)
        batch[sat_row] = U64(E.saturating_coefficient(base_log, levels, limb_model))
        batch[body_row] = 0
        batch[body_row, -1] = U64(1 << 63)
        idx += [1, 2, 3, 4, sat_row, body_row]
    return batch, sorted(set(idx))


def real_big_lwes(s, B, start_index):
    """B real ciphertexts under the big key [B][K+1]."""
    if s.name == "8bit":
        cts = s.client.encrypt_ints_raw(np.arange(B) & 0xFF, start_index=start_index)
    else:
        cts = s.client.encrypt_bits_raw(np.arange(B) & 1, start_index=start_index)
    assert cts.shape == (B, s.K + 1)
    return cts


def _keyswitch(ctx, s, batch):
    out = np.full((len(batch), s.p["n"] + 1), 0x5A5A, dtype=U64)
    N.check(N.lib().tae_stage_keyswitch(ctx._h, _vp(batch), len(batch), _vp(out), N.TAE_MEM_HOST))
    return out


def _pfks(ctx, s, batch, level, want, poison=0):
    """tae_stage_pfks_ggsw: [B][cbs_l][k+1][(k+1)N]; which kernel ran is read from the engine."""
    out = np.full((len(batch), s.p["cbs_l"], s.p["k"] + 1, s.glwe), poison, dtype=U64)
    N.check(N.lib().tae_stage_pfks_ggsw(ctx._h, _vp(batch), len(batch), level, _vp(out), N.TAE_MEM_HOST))
    assert ctx.last_pfks_kernel() == want
    return out


# ---- a. LWE keyswitch ------------------------------------------------------------------------------------------
KS_ROWS = {"real": None, "pattern": (0, 2, 3, 4, 127, 128), "saturating": (0, 127)}


def check_keyswitch(s, key):
    """B = 129 (two m-tiles of gemm<1, 8>; n + 1 columns are 43 n-tiles for lvl_64, two tile groups, the second 11
    wide; nine 16-ciphertext groups of keyswitch_kernel, the last of one) and B = 1."""
    p = s.p
    batch, idx = crafted_batch(129, s.K + 1, p["ks_b"], p["ks_l"], "bytes", real_big_lwes(s, 129, 310_000), 127, 128)
    ctx, ok = s.context(key), s.oracle(key)
    out = _keyswitch(ctx, s, batch)
    for i in KS_ROWS[key] or idx:
        assert np.array_equal(out[i], ok.keyswitch(batch[i])), (s.name, key, i)
    for i in (0, 127):
        one = _keyswitch(ctx, s, batch[i:i + 1])
        assert np.array_equal(one[0], out[i]), (s.name, key, "B = 1", i)


# ---- c. PFKS, row layout -----------------------------------------------------------------------------------------
def pfks_filler(s, B):
    """Random words: what PBS outputs are to the PFKS."""
    return E.random_words(np.random.default_rng(1000 + s.pid), (B, s.K + 1))


def check_pfks_rows(s, key):
    """prep_digits3<6> + gemm_g6<6, 4> at B = 129: a full 128-ciphertext tile and a tile of one."""
    p = s.p
    batch, idx = crafted_batch(129, s.K + 1, p["pfks_b"], p["pfks_l"], "rows6", pfks_filler(s, 129), 127, 128)
    out = _pfks(s.context(key, rows=True), s, batch, 1, "rows")
    for i in (0, 127) if key == "saturating" else idx:
        for q in (0, p["k"]):
            assert np.array_equal(out[i, 0, q], s.pfks_ref(key, q, batch[i])), (s.name, key, i, q)


# ---- d. PFKS, K layout -------------------------------------------------------------------------------------------
def k_batch(s):
    """385 rows: a full 384-ciphertext tile and a tile of one; row 383 saturating, row 384 body-only."""
    p = s.p
    return crafted_batch(385, s.K + 1, p["pfks_b"], p["pfks_l"], "kslots", pfks_filler(s, 385), 383, 384)


def check_pfks_k(s, key, env, want, one_row=False):
    p = s.p
    batch, _ = k_batch(s)
    if E.kslots_plan(p["pfks_b"], p["pfks_l"])["clamp"][-1]:
        # the clamp tie sits in row 0: lower digits of +2^(B-1), which prep_digits_kl stores as -2^(B-1) and
        # pfks_clamp_fixup repairs
        lower = E.digits_np(batch[0], p["pfks_b"], p["pfks_l"])[:, -1]
        assert int((lower == 1 << (p["pfks_b"] - 1)).sum()) >= 100
    ctx = s.new_context(key, env)
    out = _pfks(ctx, s, batch, 1, want)
    for i in (0, 383, 384):
        for q in (0, p["k"]):
            assert np.array_equal(out[i, 0, q], s.pfks_ref(key, q, batch[i])), (s.name, key, want, i, q)
    if one_row:
        one = _pfks(ctx, s, batch[:1], 1, want)
        assert np.array_equal(one[0], out[0]), (s.name, key, want, "B = 1")
    del ctx


# ======== params_sqrd_lvl_64 ========
@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_keyswitch_lvl64(sets, key):
    check_keyswitch(sets.get("lvl_64"), key)


@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_pfks_rows_lvl64(sets, key):
    check_pfks_rows(sets.get("lvl_64"), key)


@pytest.mark.parametrize("key", ["pattern", "saturating"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_pfks_k_lvl64(sets, variant, key):
    """Every K-layout GEMM at B = 385 and B = 1 under the crafted keys (test_gpu_pfks_variants.py has the real
    key): under saturating_key row 383 drives every accumulator of key limbs 1..7 to 128 * 128 * 4 * 2049."""
    check_pfks_k(sets.get("lvl_64"), key, {"TAE_PFKS_GEMM": variant + ":all"}, variant, one_row=True)


def test_scratch_reuse_lvl64(sets):
    """d_digits_ is one scratch buffer for three layouts (row-major digits of the keyswitch, row-pair interleaved
    rows of Kp = 4224 and of Kp = 8320 for the two PFKS layouts) and zero_pad re-runs per call: a call's result must
    not depend on what used the buffer before.  On one context: PFKS B = 2085 (K layout), PFKS B = 5 (rows),
    keyswitch B = 129, PFKS B = 5, keyswitch B = 1; each equals the same call made first on a fresh context."""
    s = sets.get("lvl_64")
    rng = np.random.default_rng(2085)
    big = E.random_words(rng, (2085, s.K + 1))
    small5, ks129, ks1 = big[100:105], big[200:329], big[400:401]
    env = {"TAE_PFKS_GEMM": "w16"}

    def fresh(fn):
        ctx = s.new_context("real", env)
        out = fn(ctx)
        del ctx
        return out

    calls = [("pfks 2085", lambda c: _pfks(c, s, big, 1, "w16")),
             ("pfks 5", lambda c: _pfks(c, s, small5, 1, "rows")),
             ("keyswitch 129", lambda c: _keyswitch(c, s, ks129)),
             ("pfks 5 again", lambda c: _pfks(c, s, small5, 1, "rows")),
             ("keyswitch 1", lambda c: _keyswitch(c, s, ks1))]
    ctx = s.new_context("real", env)
    first = {}
    for name, fn in calls:
        got = fn(ctx)
        ref_name = name.replace(" again", "")
        if ref_name not in first:
            first[ref_name] = got if name == "pfks 2085" else fresh(fn)  # the first call on ctx is itself fresh
        assert np.array_equal(got, first[ref_name]), name
    del ctx
    # the fresh results are the right ones
    ok = s.oracle("real")
    assert np.array_equal(first["pfks 2085"][2084, 0, 4], s.pfks_ref("real", 4, big[2084]))
    assert np.array_equal(first["pfks 5"][4, 0, 0], s.pfks_ref("real", 0, small5[4]))
    assert np.array_equal(first["keyswitch 129"][128], ok.keyswitch(ks129[128]))
    assert np.array_equal(first["keyswitch 1"][0], ok.keyswitch(ks1[0]))


# ======== params_sqrd_lvl_4 ========
@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_pfks_rows_lvl4(sets, key):
    check_pfks_rows(sets.get("lvl_4"), key)


@pytest.mark.parametrize("key", ["real", "pattern"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_pfks_k_lvl4(sets, variant, key):
    """N = 1024, k = 2: 9216 key columns, base 2^16 with the clamped lower level, on every K-layout GEMM."""
    check_pfks_k(sets.get("lvl_4"), key, {"TAE_PFKS_GEMM": variant + ":all"}, variant)


# ======== params_sqrd_lvl_256 ========
@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_keyswitch_lvl256(sets, key):
    """ks 6 x 2^2."""
    check_keyswitch(sets.get("lvl_256"), key)


@pytest.mark.parametrize("key", ["real", "pattern"])
@pytest.mark.parametrize("kernel", ["g6", "default"])
def test_pfks_k_lvl256(sets, kernel, key):
    """pfks 3 x 2^12: six slots per coefficient, no offset and no clamp."""
    env, want = ({"TAE_PFKS_GEMM": "g6:all"}, "g6") if kernel == "g6" else (KL, DEFAULT)
    check_pfks_k(sets.get("lvl_256"), key, env, want)


# ======== the 8-bit set ========
@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_keyswitch_8bit(sets, key):
    """ks 8 x 2^2: Kd = 16384."""
    check_keyswitch(sets.get("8bit"), key)


@pytest.mark.parametrize("level", [2, 4])
def test_pfks_k_8bit_upper_levels(sets, level):
    """The only set with cbs_l > 1: dst = ggsw + (level - 1) ncols and out_stride = cbs_l ncols are shared by the
    GEMM epilogue and nothing else here (no clamp at base 2^12).  The named level's rows equal the oracle's; the
    host path hands back zeros for the levels the stage does not write, whatever the caller's array held."""
    s = sets.get("8bit")
    p = s.p
    batch = pfks_filler(s, 3)
    batch[0] = E.edge_row(p["pfks_b"], p["pfks_l"], s.K + 1)
    batch[1] = U64(E.saturating_coefficient(p["pfks_b"], p["pfks_l"], "kslots"))
    ctx = s.new_context("real", KL)
    out = _pfks(ctx, s, batch, level, DEFAULT, poison=0x5A5A)
    for i in range(3):
        for q in range(p["k"] + 1):
            assert np.array_equal(out[i, level - 1, q], s.pfks_ref("real", q, batch[i])), (level, i, q)
    assert not out[:, [l for l in range(p["cbs_l"]) if l != level - 1]].any()
    del ctx


# ======== params_sqrd_lvl_1: the scalar u64 kernels ========
@pytest.mark.parametrize("key", ["real", "pattern", "saturating"])
def test_keyswitch_lvl1_scalar(sets, key):
    """keyswitch_kernel: nine groups of KS_CT = 16 ciphertexts, the last holding one."""
    check_keyswitch(sets.get("lvl_1"), key)


@pytest.mark.parametrize("key", ["real", "pattern"])
def test_pfks_lvl1_scalar(sets, key):
    """pfks_kernel at base 2^24, one level: five ciphertexts in a PF_CT = 32 group, row 0 the edge words."""
    s = sets.get("lvl_1")
    p = s.p
    batch = pfks_filler(s, 5)
    batch[0] = E.edge_row(p["pfks_b"], p["pfks_l"], s.K + 1)
    out = _pfks(s.context(key), s, batch, 1, "u64")
    for i in range(5):
        for q in range(p["k"] + 1):
            assert np.array_equal(out[i, 0, q], s.pfks_ref(key, q, batch[i])), (key, i, q)


# ======== b. shortint_1bit: the packing keyswitch ========
@pytest.mark.parametrize("key", ["real", "pattern"])
def test_packing_keyswitch_shortint1(sets, key):
    """tae_s1_packing_keyswitch = gemm<1, 8> with the packing key (kd over n x pfks_l, 2560 columns, the body at
    column kN), then the rotate-and-add of S1Keys.pack: count = 1 (the edge row; the saturating row) and 3."""
    from tfhe_aes import shortint_1bit as S
    s = sets.get("shortint_1bit")
    p = s.p
    real = s.client.encrypt_bits_raw([1], start_index=330_000)
    edge = E.edge_row(p["pfks_b"], p["pfks_l"], p["n"] + 1)
    sat = np.full(p["n"] + 1, E.saturating_coefficient(p["pfks_b"], p["pfks_l"], "bytes"), dtype=U64)
    ctx, ok = s.context(key), s.oracle(key)
    for cts in (edge[None], sat[None], np.stack([edge, sat, real[0]])):
        assert np.array_equal(S.packing_keyswitch(ctx, cts), ok.pack(cts)), (key, len(cts))
