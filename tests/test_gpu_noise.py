"""Measured noise: every level of the squared-noise bookkeeping against the margin of the next bootstrap
(params_sqrd_lvl_64, 1-bit model, gal-mul driver).

The parity tests pin the kernels to the oracle word for word, and the noise tests replay the bookkeeping against
itself.  Neither measures a phase error.  Here the client's secret keys give the exact phase of every ciphertext
(tests/noise_ref.py), big-key and after tae_stage_keyswitch, at each construction the DESIGN.md 5.7 - 5.16 tables
assign a level to.  Sums are formed in numpy u64 (the linear kernels are pinned word for word elsewhere) over
outputs of the public entry points.  Per sample point, with m its number of independent samples (where one group
feeds several samples through different output indices, the number of distinct groups):

  1. zero mean, at fresh bits and bootstrap outputs: |mean| <= 5 sigma / sqrt m;
  2. margin at the input of the next bootstrap, on the small-key errors:
     (2^62 - |mean|) / sqrt(var + modswitch_var) * (1 - 5 / sqrt(2 m)) >= z_required() = 9.155, the two-sided
     Gaussian quantile of the reference's p_error 5.42101086e-20; and no sample at or beyond 2^62;
  3. levels are conservative: with the unit U = var_big(8 -> 24 output) / 8 (the reference's rule,
     shortint_woppbs_1bit.rs:322-325), a point of level l has var_big <= l U (1 + 10 / sqrt m);
  4. independence where fresh ids are handed out: var(sum) / sum var(parts) <= 1 + 10 / sqrt m, the parts'
     variances estimated per output index in the same run; for the GCM product also the correlation of the parts
     of a chunk that share an operand nibble (hence their GGSWs), |rho| <= 5 / sqrt m_pairs;
  5. the level-64 sums, refreshed, decrypt to the XOR of their plaintext bits.

No threshold comes from the product's output except U, which is the bookkeeping's own definition of its unit.
Each test prints its points (run with -s):
  noise: name level m log2(std_big) log2(std_small) mean_big/sigma mean_small/sigma margin var/(l U) ratio
(`ratio` is the independence ratio of 4, `-` where the point is no sum).

The small-key mean is not zero and is not meant to be: the keyswitch adds one constant per key set,
noise_ref.keyswitch_offset(), about -0.12 sigma here.  It enters a bootstrap input once whatever the number of
summed terms, so it cannot grow with a row's weight; margin() charges it, and where 1 is asserted the small-key
mean must equal the derived offset within the same 5 sigma / sqrt m.  Encryption indices 12 000 000 ... are
used by no other test.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests import gcm_ref as G
from tests import noise_ref as R

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
SMALL = 677 + 1
N_GROUPS = 512
AT_FRESH, AT_FWD, AT_INV, AT_GCM = 12_000_000, 12_100_000, 12_200_000, 12_300_000


def f_fwd24(x):
    """The gal-mul driver's SubBytes table: SBOX times 1, 2, 3."""
    s = aes_128.SBOX[x]
    return (aes_128.gf_256_mul(s, 1) << 16) | (aes_128.gf_256_mul(s, 2) << 8) | aes_128.gf_256_mul(s, 3)


def f_inv32(x):
    """The inverse cipher's table: InvSbox times 14, 11, 13, 9 (tests/test_gpu_decrypt.py)."""
    y = aes_128.INV_SBOX[x]
    return (aes_128.gf_mul(y, 14) << 24) | (aes_128.gf_mul(y, 11) << 16) | (aes_128.gf_mul(y, 13) << 8) | aes_128.gf_mul(y, 9)


def _msb_bits(values, width):
    """[n] integers -> [n][width] bits, most significant first (the order of u8_to_bits and of a table's outputs)."""
    v = np.asarray(values, dtype=np.uint64)[:, None]
    return ((v >> np.arange(width - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def _keyswitch(ctx, cts):
    cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, BIG)
    out = np.zeros((cts.shape[0], SMALL), dtype=np.uint64)
    N.check(N.lib().tae_stage_keyswitch(ctx._h, cts.ctypes.data_as(C.c_void_p), cts.shape[0],
                                        out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
    return out


def _errors(ctx, client, cts, bits):
    """Signed phase errors of [n][BIG] ciphertexts of `bits`: under the big key, and under the small key after
    the keyswitch (what the next bootstrap's modulus switch sees)."""
    cts = cts.reshape(-1, BIG)
    bits = np.asarray(bits).ravel()
    return (R.signed_error(R.big_phase(client, cts), bits),
            R.signed_error(R.small_phase(client, _keyswitch(ctx, cts)), bits))


def _refresh(ctx, lut_id, cts):
    return ctx.circuit_bootstrap_raw(cts.reshape(-1, 1, BIG), lut_id).reshape(-1, BIG)


def _check(client, name, level, m, eb, es, unit, zero_mean=None, ratio=None):
    """Print the point's line, then assert 2 and 3, 1 where asked (zero_mean = the keyswitch's derived offset,
    which is what the small-key mean must then be) and 4 where a ratio is given.  `level` is one number or one per
    sample; var/(l U) and the ratio are then means of squares of normalised errors."""
    level = np.broadcast_to(np.asarray(level, dtype=np.float64), eb.shape)
    std_b, std_s = eb.std(), es.std()
    mean_sig = eb.mean() / std_b
    margin = R.margin(es, client)
    uniform = level.min() == level.max()
    lvl = eb.var() / (level[0] * unit) if uniform else np.mean(eb ** 2 / (level * unit))
    tag = ("%d" % level[0]) if uniform else "%d..%d" % (level.min(), level.max())
    print("noise: %-28s %-6s %5d %6.2f %6.2f %+6.3f %+6.3f %6.2f %7.4f %s"
          % (name, tag, m, math.log2(std_b), math.log2(std_s), mean_sig, es.mean() / std_s, margin, lvl,
             "-" if ratio is None else "%.4f" % ratio))
    if zero_mean is not None:
        assert abs(eb.mean()) <= R.mean_bound(std_b, m), (name, "big-key mean", mean_sig)
        assert abs(es.mean() - zero_mean) <= R.mean_bound(std_s, m), (name, "small-key mean", es.mean(), zero_mean)
    assert np.abs(es).max() < R.HALF_GAP and np.abs(eb).max() < R.HALF_GAP, (name, "a sample beyond 2^62")
    assert margin * R.margin_floor(m) >= R.z_required(), (name, "margin", margin, m)
    assert lvl <= R.ratio_bound(m), (name, "var_big / (level U)", lvl)
    if ratio is not None:
        assert ratio <= R.ratio_bound(m), (name, "var(sum) / sum var(parts)", ratio)
    return margin


# ---- sample points (module scope: each is made once) ----------------------------------------------------------
@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def ks_offset(client, product_raw):
    return R.keyswitch_offset(client, product_raw[1][0])


@pytest.fixture(scope="module")
def lut_id(gpu_context):
    return gpu_context.generate_lookup_table(1, 1, lambda v: v)


@pytest.fixture(scope="module")
def fresh(gpu_context, client):
    """(a) 4096 fresh random bits: bits, ciphertexts, errors."""
    bits = np.random.default_rng(101).integers(0, 2, 4096).astype(np.uint8)
    cts = client.encrypt_bits_raw(bits, start_index=AT_FRESH)
    return bits, cts, _errors(gpu_context, client, cts, bits)


def _table_point(ctx, client, f, n_out, seed, start):
    data = np.random.default_rng(seed).integers(0, 256, N_GROUPS)
    cts = client.encrypt_bits_raw(_msb_bits(data, 8).ravel(), start_index=start).reshape(N_GROUPS, 8, BIG)
    out = ctx.circuit_bootstrap_raw(cts, ctx.generate_lookup_table(8, n_out, f))
    bits = _msb_bits([f(int(x)) for x in data], n_out)
    eb, es = _errors(ctx, client, out, bits)
    return bits, out, (eb.reshape(N_GROUPS, n_out), es.reshape(N_GROUPS, n_out))


@pytest.fixture(scope="module")
def fwd(gpu_context, client):
    """(b) 512 groups of the 8 -> 24 table on fresh random bytes: bits [512][24], outputs, errors [512][24]."""
    return _table_point(gpu_context, client, f_fwd24, 24, 102, AT_FWD)


@pytest.fixture(scope="module")
def inv(gpu_context, client):
    """(c) the same for the 8 -> 32 inverse table."""
    return _table_point(gpu_context, client, f_inv32, 32, 103, AT_INV)


@pytest.fixture(scope="module")
def unit(fwd):
    """U: an 8-input circuit bootstrap's output is at level 8 by the reference's rule."""
    return fwd[2][0].var() / 8.0


@pytest.fixture(scope="module")
def refreshed(gpu_context, client, lut_id, fresh):
    """(d) the identity bootstrap of the 4096 fresh bits."""
    bits, cts, _ = fresh
    out = _refresh(gpu_context, lut_id, cts)
    return bits, out, _errors(gpu_context, client, out, bits)


@pytest.fixture(scope="module")
def cap(gpu_context, client, fwd):
    """(e) 64 sets of 8 groups, summed per output index: 1536 sums at level 64."""
    bits, out, _ = fwd
    sums = out.reshape(N_GROUPS // 8, 8, 24, BIG).sum(axis=1, dtype=np.uint64).reshape(-1, BIG)
    sbits = (bits.reshape(N_GROUPS // 8, 8, 24).sum(axis=1) & 1).astype(np.uint8).ravel()
    return sbits, sums, _errors(gpu_context, client, sums, sbits)


def _table_lines(client, name, pt, unit, n_out, ks_offset):
    """Assertions 1 - 3 for a table's outputs: pooled with m = the number of groups, and per output index."""
    _, _, (eb, es) = pt
    _check(client, name, 8, N_GROUPS, eb.ravel(), es.ravel(), unit, zero_mean=ks_offset)
    worst_mean = worst_var = 0.0
    for j in range(n_out):
        worst_mean = max(worst_mean, abs(eb[:, j].mean()) / eb[:, j].std())
        worst_var = max(worst_var, eb[:, j].var() / (8 * unit))
        assert abs(eb[:, j].mean()) <= R.mean_bound(eb[:, j].std(), N_GROUPS), (name, j, "big-key mean")
        assert abs(es[:, j].mean() - ks_offset) <= R.mean_bound(es[:, j].std(), N_GROUPS), (name, j, "small-key mean")
        assert eb[:, j].var() <= 8 * unit * R.ratio_bound(N_GROUPS), (name, j, "var_big / 8 U")
    rho = np.corrcoef(eb.T)[np.triu_indices(n_out, 1)]
    same = np.abs(rho) > 0.999  # equal table columns give the same ciphertext twice
    print("noise:   per output index: max |mean|/sigma %.3f (bound %.3f), max var/(8 U) %.3f; inside one group:"
          " %d of %d pairs identical, the rest mean rho %+.4f, max |rho| %.3f (not asserted: no plan sums two outputs"
          " of one group)" % (worst_mean, R.N_SE / math.sqrt(N_GROUPS), worst_var, same.sum(), rho.size,
                             rho[~same].mean(), np.abs(rho[~same]).max()))


# ---- the tests ------------------------------------------------------------------------------------------------
def test_fresh_bits(client, fresh, unit, ks_offset):
    _, _, (eb, es) = fresh
    print("\nnoise: U = var_big(8 -> 24 output) / 8 = 2^%.2f (std 2^%.2f); modulus switch std 2^%.2f; z_required %.4f"
          % (math.log2(unit), math.log2(unit) / 2, math.log2(R.modswitch_var(client)) / 2, R.z_required()))
    print("noise: keyswitch offset (derived from the key) %+.4e = %+.3f sigma of a keyswitched fresh bit"
          % (ks_offset, ks_offset / es.std()))
    _check(client, "a fresh bit", 1, eb.size, eb, es, unit, zero_mean=ks_offset)


def test_forward_table_outputs(client, fwd, unit, ks_offset):
    print()
    _table_lines(client, "b 8->24 output", fwd, unit, 24, ks_offset)


def test_inverse_table_outputs(client, inv, unit, ks_offset):
    print()
    _table_lines(client, "c 8->32 output", inv, unit, 32, ks_offset)


def test_identity_refresh_of_fresh_bits(client, refreshed, unit, ks_offset):
    print()
    _, _, (eb, es) = refreshed
    _check(client, "d refresh of fresh bits", 1, eb.size, eb, es, unit, zero_mean=ks_offset)


def test_cap_sums_of_eight_groups(client, fwd, cap, unit):
    """(e), the binding case.  Each group feeds 24 sums through its 24 output indices: m = 512 groups."""
    print()
    _, _, (eb, es) = cap
    var_j = fwd[2][0].var(axis=0)  # per output index, over the 512 groups
    z = eb.reshape(-1, 24) / np.sqrt(8 * var_j)
    margin = _check(client, "e sum of 8 groups", 64, N_GROUPS, eb, es, unit, ratio=z.var())
    print("noise:   headroom at level 64: margin / z_required = %.3f in std" % (margin / R.z_required()))


def test_refresh_of_cap_sums_decrypts(gpu_context, client, lut_id, cap, unit, ks_offset):
    """(d) on level-64 inputs and 5: 1024 of the level-64 sums through the identity bootstrap."""
    print()
    sbits, sums, _ = cap
    out = _refresh(gpu_context, lut_id, sums[:1024])
    assert np.array_equal(client.decrypt_bits_raw(out), sbits[:1024])
    eb, es = _errors(gpu_context, client, out, sbits[:1024])
    _check(client, "d refresh of level-64 sums", 1, 1024, eb, es, unit, zero_mean=ks_offset)


def _mix_sums(gpu_context, client, pt, fresh, unit, name, out_index):
    """(f) per column of four groups, row r, bit b: the four terms out[4 c + (r + j) % 4][out_index(j, b)] plus one
    fresh bit, 4096 sums at level 4 * 8 + 1.  An output enters at most two sums of its column; m = 512 groups."""
    bits, out, (eb_t, _) = pt
    kbits, kcts, (eb_k, _) = fresh
    c, r, b = np.meshgrid(np.arange(N_GROUPS // 4), np.arange(4), np.arange(8), indexing="ij")
    c, r, b = c.ravel(), r.ravel(), b.ravel()
    sums, sbits, expect = kcts.copy(), kbits.copy(), np.full(c.size, eb_k.var())
    var_j = eb_t.var(axis=0)
    for j in range(4):
        g, o = 4 * c + ((r + j) & 3), out_index(j, b)
        sums += out[g, o]
        sbits ^= bits[g, o]
        expect += var_j[o]
    eb, es = _errors(gpu_context, client, sums, sbits)
    _check(client, name, 33, N_GROUPS, eb, es, unit, ratio=np.var(eb / np.sqrt(expect)))


def test_mixcolumns_sums_forward(gpu_context, client, fwd, fresh, unit):
    print()  # 2 s(r) + 3 s(r+1) + s(r+2) + s(r+3) + key bit: outputs 8 + b, 16 + b, b, b of the 24
    _mix_sums(gpu_context, client, fwd, fresh, unit, "f MixColumns sum, 8->24", lambda j, b: (8, 16, 0, 0)[j] + b)


def test_mixcolumns_sums_inverse(gpu_context, client, inv, fresh, unit):
    print()  # 14 s(r) + 11 s(r+1) + 13 s(r+2) + 9 s(r+3) + key bit: outputs 8 j + b of the 32
    _mix_sums(gpu_context, client, inv, fresh, unit, "f InvMixColumns sum, 8->32", lambda j, b: 8 * j + b)


@pytest.fixture(scope="module")
def gcm(gpu_context, client, lut_id):
    """(g) two GF(2^128) products of fresh random operands through the public composition of
    tests/test_gpu_gcm.py::_product_np; errors only are kept.  Per product: the 7168 partial bits (big key), the
    1135 chunk sums, their refreshes and the 128 reduced sums."""
    chunks, _, reduce, _ = G.product_plan()
    lut = gpu_context.generate_lookup_table(8, 7, G.nibble_product)
    src = np.array([G.pair_sources(g) for g in range(1024)])
    keep = {k: [] for k in ("part_eb", "chunk_eb", "chunk_es", "fresh_eb", "fresh_es", "red_eb", "red_es")}
    for p in range(2):
        obits = np.random.default_rng(104 + p).integers(0, 2, 256).astype(np.uint8)
        ops = client.encrypt_bits_raw(obits, start_index=AT_GCM + 1000 * p)
        parts = gpu_context.circuit_bootstrap_raw(ops[src], lut).reshape(1024 * 7, BIG)
        values = (obits[src].astype(np.uint64) << np.arange(7, -1, -1, dtype=np.uint64)).sum(axis=1)
        pbits = _msb_bits([G.nibble_product(int(v)) for v in values], 7).ravel()
        keep["part_eb"].append(R.signed_error(R.big_phase(client, parts), pbits))
        csum = G.sum_rows(parts, chunks)
        del parts
        cbits = np.array([pbits[c].sum() & 1 for c in chunks], dtype=np.uint8)
        again = _refresh(gpu_context, lut_id, csum)
        rbits = np.array([cbits[row].sum() & 1 for row in reduce], dtype=np.uint8)
        for name, cts, bits in (("chunk", csum, cbits), ("fresh", again, cbits),
                                ("red", G.sum_rows(again, reduce), rbits)):
            eb, es = _errors(gpu_context, client, cts, bits)
            keep[name + "_eb"].append(eb)
            keep[name + "_es"].append(es)
    return {k: np.stack(v) for k, v in keep.items()}


def test_gcm_product_chunks(client, gcm, unit):
    """Chunk sums at levels 8 ... 56 from groups that share operand nibbles.  2 x 1135 sums from 2 x 1024 groups,
    each group feeding up to 7 chunks through its 7 outputs: m = 2048 pooled, the chunk count per level."""
    print()
    chunks = G.product_plan()[0]
    part = gcm["part_eb"].reshape(2, 1024, 7)
    std_d = np.sqrt(part.reshape(-1, 7).var(axis=0))  # per output index over the 2048 groups
    z_part = (part / std_d).reshape(2, -1)
    print("noise: %-28s %-6s %5d %6.2f      - %+6.3f      -      - %7.4f -"
          % ("g 8->7 partial bit", "8", 2048, math.log2(part.std()), part.mean() / part.std(), part.var() / (8 * unit)))
    length = np.array([len(c) for c in chunks])
    d_of = [np.array(c) % 7 for c in chunks]
    expect = np.array([(std_d[d] ** 2).sum() for d in d_of])
    eb, es = gcm["chunk_eb"], gcm["chunk_es"]
    _check(client, "g chunk sums, all", np.tile(8.0 * length, 2), 2048, eb.ravel(), es.ravel(), unit,
           ratio=np.var(eb / np.sqrt(expect)))
    for n in range(1, 8):
        at = length == n
        _check(client, "g chunk sums of %d" % n, 8 * n, 2 * int(at.sum()), eb[:, at].ravel(), es[:, at].ravel(), unit,
               ratio=np.var(eb[:, at] / np.sqrt(expect[at])))
    # parts of one chunk that share a's nibble (the same I) or b's (the same J): the same keyswitched inputs
    for which, key in (("a", lambda g: g >> 5), ("b", lambda g: g & 31)):
        pairs = np.array([(c[i], c[j]) for c in chunks for i in range(len(c)) for j in range(i + 1, len(c))
                          if key(c[i] // 7) == key(c[j] // 7)])
        prod = z_part[:, pairs[:, 0]] * z_part[:, pairs[:, 1]]
        rho, m_pairs = prod.mean(), prod.size
        print("noise:   parts of a chunk sharing the nibble of %s: rho %+.4f over %d pairs (bound %.4f)"
              % (which, rho, m_pairs, R.corr_bound(m_pairs)))
        assert abs(rho) <= R.corr_bound(m_pairs), (which, rho)


def test_gcm_product_refreshed_and_reduced(client, gcm, unit, ks_offset):
    print()
    _check(client, "d refresh of chunk sums", 1, gcm["fresh_eb"].size, gcm["fresh_eb"].ravel(), gcm["fresh_es"].ravel(),
           unit, zero_mean=ks_offset)
    length = np.array([len(row) for row in G.product_plan()[2]], dtype=np.float64)
    assert length.max() == 34
    eb, es = gcm["red_eb"], gcm["red_es"]
    _check(client, "g reduced sums", np.tile(length, 2), eb.size, eb.ravel(), es.ravel(), unit,
           ratio=np.var(eb / np.sqrt(length * gcm["fresh_eb"].var())))


def test_sums_of_refreshed_bits_at_the_caps(gpu_context, client, refreshed, fwd, fresh, unit):
    """(h) the tag row's first chunk, 55 refreshed bits + one 8 -> 24 output + one fresh bit = 64 (the outputs are
    indices 0 and 1 of the 512 groups: m = 512), and 64 refreshed bits (later chunks, XTS-style mask rows)."""
    print()
    rbits, rcts, (eb_r, _) = refreshed
    rng = np.random.default_rng(106)
    first, later = np.zeros((1024, BIG), dtype=np.uint64), np.zeros((1024, BIG), dtype=np.uint64)
    fbits, lbits = np.zeros(1024, dtype=np.uint8), np.zeros(1024, dtype=np.uint8)
    for i in range(1024):
        pick = rng.choice(4096, 56, replace=False)
        g, o = i % N_GROUPS, i // N_GROUPS
        first[i] = rcts[pick[:55]].sum(axis=0, dtype=np.uint64) + fwd[1][g, o] + fresh[1][pick[55]]
        fbits[i] = (rbits[pick[:55]].sum() + fwd[0][g, o] + fresh[0][pick[55]]) & 1
        pick = rng.choice(4096, 64, replace=False)
        later[i] = rcts[pick].sum(axis=0, dtype=np.uint64)
        lbits[i] = rbits[pick].sum() & 1
    eb, es = _errors(gpu_context, client, first, fbits)
    expect = 55 * eb_r.var() + fwd[2][0][:, :2].var(axis=0)[np.arange(1024) // N_GROUPS] + fresh[2][0].var()
    _check(client, "h 55 refreshed + E(J0) bit", 64, N_GROUPS, eb, es, unit, ratio=np.var(eb / np.sqrt(expect)))
    eb, es = _errors(gpu_context, client, later, lbits)
    _check(client, "h 64 refreshed", 64, 1024, eb, es, unit, ratio=eb.var() / (64 * eb_r.var()))
