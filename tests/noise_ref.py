"""Exact reference arithmetic for the measured-noise tests (tests/test_noise_ref.py on the CPU,
tests/test_gpu_noise.py on the GPU).  Plain numpy and Python integers; the only product call
is ClientKey.secrets().

Where the thresholds come from, and nothing else enters them:
  - P_ERROR, the failure probability the reference's parameters were optimised for;
  - 2^62, the distance from a boolean phase bit * 2^63 (+ 2^62 after homomorphic_shift_boolean's shift) to the
    two sign boundaries of the bootstrap's test vector;
  - modswitch_var(), the rounding of the blind rotation's modulus switch, derived below;
  - the reference's "times the number of selector bits" rule for a circuit bootstrap's output level
    (shortint_woppbs_1bit.rs:322-325), which defines the unit of the bookkeeping;
  - 5 standard errors of the estimator in question (N_SE).
"""
import math

import numpy as np

# ./optimizer --min-precision 1 --max-precision 1 --p-error 5.42101086e-20 --ciphertext-modulus-log 64 --wop-pbs
# (the reference's src/tfhe/shortint_woppbs_1bit/parameters.rs:114, the optimiser line of params_sqrd_lvl_64)
P_ERROR = 5.42101086e-20
HALF_GAP = 2.0 ** 62
N_SE = 5.0


def _keys(ck):
    lwe, glwe = ck.secrets()
    return np.ascontiguousarray(lwe, dtype=np.uint64), np.ascontiguousarray(glwe, dtype=np.uint64)


def _phase(cts, key):
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    if cts.ndim != 2 or cts.shape[1] != key.size + 1:
        raise ValueError("ciphertexts must be [n][%d]" % (key.size + 1))
    out = np.empty(cts.shape[0], dtype=np.uint64)
    for at in range(0, cts.shape[0], 512):  # u64 products and sums wrap mod 2^64, which is the torus
        blk = cts[at:at + 512]
        out[at:at + 512] = blk[:, -1] - (blk[:, :-1] * key).sum(axis=1, dtype=np.uint64)
    return out


def big_phase(ck, cts):
    """body - <mask, s> mod 2^64 of big-key ciphertexts [n][K+1]; the GLWE key is the flat [k N] array that
    tae_decrypt_bits_raw reads (polynomial p's coefficient j at p N + j)."""
    return _phase(cts, _keys(ck)[1])


def small_phase(ck, cts):
    """The same for small-key ciphertexts [n][n_lwe+1] (after the keyswitch)."""
    return _phase(cts, _keys(ck)[0])


def signed_error(phase, bit):
    """The centred residue of phase - bit * 2^63 in [-2^63, 2^63) as float64 (the conversion drops at most 2^10)."""
    phase = np.asarray(phase, dtype=np.uint64)
    bit = np.asarray(bit, dtype=np.uint64)
    return (phase - (bit << np.uint64(63))).view(np.int64).astype(np.float64)


def z_required():
    """z with erfc(z / sqrt 2) = P_ERROR: the two-sided Gaussian quantile of the reference's target (9.1553)."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > P_ERROR:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def modswitch(words, poly_size):
    """The blind rotation's modulus switch of u64 words, back on the 2^64 scale: round to nearest onto 2N values
    (ties up), as the oracle's or_pbs_modulus_switch does for every mask word and for the body
    (x >> (64 - log 2N - 1), + its low bit, >> 1)."""
    log2n = int(poly_size).bit_length()  # log2(2N) for a power of two N
    w = np.asarray(words, dtype=np.uint64) >> np.uint64(64 - log2n - 1)
    w = (w + (w & np.uint64(1))) >> np.uint64(1)
    return w << np.uint64(64 - log2n)


def modswitch_var(ck):
    """Variance the modulus switch adds to the phase the blind rotation acts on: (1 + h) (2^64 / 2N)^2 / 12.

    The oracle's or_bootstrap switches the body and each mask word with or_pbs_modulus_switch, which is
    round-to-nearest onto 2N (checked in tests/test_noise_ref.py against that function).  A rounded word is off
    by a value uniform on an interval of 2^64 / 2N, variance (2^64 / 2N)^2 / 12; the phase takes the body's
    and, through the binary secret, those of the h mask words whose key bit is 1."""
    lwe, _ = _keys(ck)
    if np.any(lwe > 1):
        raise ValueError("the derivation is for a binary small secret")
    h = int(lwe.sum())
    step = 2.0 ** 64 / (2 * ck.params["N"])
    return (1 + h) * step * step / 12.0


def margin(errors_small, ck):
    """(2^62 - |mean|) / sqrt(var + modswitch_var): the decision boundary's distance in standard deviations of
    what the next bootstrap sees."""
    e = np.asarray(errors_small, dtype=np.float64)
    return (HALF_GAP - abs(e.mean())) / math.sqrt(e.var() + modswitch_var(ck))


def decompose(words, base_log, levels):
    """The keyswitch's balanced signed decomposition (tfhe-rs SignedDecomposer, the oracle's or_decompose):
    [n] u64 -> [n][levels] int64 digits in [-B/2, B/2], the most significant level first."""
    w = np.asarray(words, dtype=np.uint64)
    drop = 64 - base_log * levels
    state = w >> np.uint64(drop - 1)
    state = (state + (state & np.uint64(1))) >> np.uint64(1)  # closest representable; a carry past 2^64 falls off
    out = np.zeros(w.shape + (levels,), dtype=np.int64)
    for lev in range(levels - 1, -1, -1):
        res = state & np.uint64((1 << base_log) - 1)
        state = state >> np.uint64(base_log)
        carry = (((res - np.uint64(1)) | state) & res) >> np.uint64(base_log - 1)
        state = state + carry
        out[..., lev] = res.astype(np.int64) - (carry.astype(np.int64) << base_log)
    return out


def keyswitch_offset(ck, ksk):
    """The constant the keyswitch adds to every phase under one key set: - sum_l E[d_l] sum_i e_(i,l).

    The keyswitch subtracts sum d_(i,l) KSK[i][l] for the digits d of the K mask words; row (i, l) encrypts
    s_i 2^(64 - b (l+1)) with a noise e_(i,l) that is fixed once the key is made.  Digits of uniform mask words
    are zero-mean at every level but the most significant: there +B/2 and -B/2 are the same residue, no level
    above takes a carry, and the decomposer always answers +B/2, so E[d_1] = 455/1024 for B = 8 and four levels.
    That leaves - E[d_1] sum_i e_(i,1), of the order 2^54 against a keyswitched bit's 2^57.4.  It enters once per
    bootstrap input, never once per summed term (sums are taken under the big key), and margin() charges it as |mean|.
    E[d_l] is exact: the digits depend on the top b L + 1 bits only, which are enumerated."""
    p = ck.params
    n, big, lev, b = p["n"], p["k"] * p["N"], p["ks_l"], p["ks_b"]
    rows = np.ascontiguousarray(ksk, dtype=np.uint64).reshape(big * lev, n + 1)
    _, glwe = _keys(ck)
    weight = np.array([64 - b * (j + 1) for j in range(lev)], dtype=np.uint64)
    e = (_phase(rows, _keys(ck)[0]).reshape(big, lev) - (glwe[:, None] << weight)).view(np.int64).astype(np.float64)
    top = np.arange(1 << (b * lev + 1), dtype=np.uint64) << np.uint64(64 - b * lev - 1)
    mean_digit = decompose(top, b, lev).mean(axis=0)
    return float(-(mean_digit * e.sum(axis=0)).sum())


# ---- estimator tolerances: N_SE standard errors, Gaussian samples, m of them independent -----------------------
def se_var(m):
    """Relative standard error of a variance estimated from m samples: sqrt(2 / m)."""
    return math.sqrt(2.0 / m)


def mean_bound(std, m):
    """|mean| of m zero-mean samples stays below this: N_SE sigma / sqrt m."""
    return N_SE * std / math.sqrt(m)


def margin_floor(m):
    """A margin divides by an estimated std (relative standard error 1 / sqrt(2 m)): the factor by which the
    estimate is lowered before it is compared with z_required()."""
    return 1.0 - N_SE / math.sqrt(2.0 * m)


def ratio_bound(m):
    """A ratio of two variances of m samples each has standard error 2 / sqrt m: the ratio of two equal
    variances stays below 1 + N_SE * 2 / sqrt m."""
    return 1.0 + N_SE * 2.0 / math.sqrt(m)


def corr_bound(m_pairs):
    """A correlation coefficient of m independent pairs has standard error 1 / sqrt m."""
    return N_SE / math.sqrt(m_pairs)
