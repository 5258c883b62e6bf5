"""Crafted inputs that put the blind rotations and the vertical packing on the edges of their integer
paths (shared by test_gpu_br_edges.py, test_gpu_vp_edges.py and test_edge_inputs.py, which pins the edges
themselves on the CPU oracle).

Every value here is an ordinary torus word or key word.  The edges aimed at:
  - rotation amounts e = 0, N and 2N (= 0 mod 2N) of the PBS modulus switch, and its rounding boundary;
  - CMux steps whose rotated difference is exactly zero: the inverse transform returns exact zeros, the one
    input the branch-free torus tail (torus_add_fast*, fft_device.hpp) refuses, so the whole wave goes to the
    from_torus_bits fallback;
  - under a noiseless bootstrapping key (a trivial GGSW of a fixed pattern of 0, 1 and -1 per LWE key
    element) and a LUT whose body is the constant 2^62: differences of exactly 2^63 (= -2^63), i.e. top
    digits on the tie 2^(B-1) and tail inputs of +-1/2, whose negative side is the i64 saturation of
    from_torus (2^63 - 1, not 2^63).

Why the key holds -1 as well: the signed decomposer never emits -2^(B-1) at its top level (decompose(2^63) is
[+2^(B-1), 0, ...]), so a GGSW of 0 or 1 turns a difference of 2^63 into a tail input of +1/2 only, and the
saturation is not reached.  A GGSW of -1 multiplies the same digit by -2^(64-B): the tail input is -1/2.

The second half of the file holds the crafted keys and inputs of the integer keyswitches (test_gpu_ks_edges.py,
pinned by test_ks_edge_inputs.py); see the comment there.  The last part holds the selector rows and LUTs of the
vertical packing's CMux tree (test_gpu_vp_tree.py, pinned by test_edge_inputs.py).
"""
import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1


def log2_exact(x: int) -> int:
    assert x > 0 and x & (x - 1) == 0
    return x.bit_length() - 1


def rotation_unit(N: int) -> int:
    """The torus distance of one rotation step of the PBS modulus switch: 2^64 / 2N."""
    return 1 << (64 - log2_exact(2 * N))


CRAFTED_ROWS = 10


def crafted_small(n: int, N: int, real: np.ndarray, body_add: int) -> np.ndarray:
    """Ten small LWEs [10][n+1] for a blind rotation over polynomials of size N whose kernel adds body_add
    to the body before the modulus switch.  `real` holds at least three ordinary ciphertexts [>=3][n+1].
    With u = rotation_unit(N), the rotation amounts (or_pbs_modulus_switch) are:

      row 0  all-zero mask (every step skipped or e = 0: zero difference, zero spectra), body of real[0]
      row 1  mask alternating 0 and 2^63: e = 0 and e = N; body of real[1]
      row 2  mask all 2^64 - 1: rounds to e = 2N, i.e. 0 mod 2N, with a non-zero mask word; body 2^62
      row 3  mask alternating u and u - u/2: e = 1 for both, the second exactly on the rounding boundary
             (u/2 - 1 gives e = 0); body of real[2]
      row 4  real[0] with its first 16 mask words zeroed
      row 5  real[1] with its first 16 mask words zeroed
      row 6  real[2] untouched
      row 7  mask of real[0], body + body_add == 2^64 - 1: the body's rotation rounds to 2N
      row 8  mask of real[1], body + body_add == 0:    rotation 0
      row 9  mask of real[2], body + body_add == 2^63: rotation N
    """
    real = np.asarray(real, dtype=U64)
    assert real.ndim == 2 and real.shape[0] >= 3 and real.shape[1] == n + 1
    u = rotation_unit(N)
    rows = np.zeros((CRAFTED_ROWS, n + 1), dtype=U64)
    rows[0, n] = real[0, n]
    rows[1, 1:n:2] = U64(1 << 63)
    rows[1, n] = real[1, n]
    rows[2, :n] = U64(MASK64)
    rows[2, n] = U64(1 << 62)
    rows[3, 0:n:2] = U64(u)
    rows[3, 1:n:2] = U64(u - u // 2)
    rows[3, n] = real[2, n]
    rows[4] = real[0]
    rows[5] = real[1]
    rows[4, :16] = 0
    rows[5, :16] = 0
    rows[6] = real[2]
    rows[7] = real[0]
    rows[8] = real[1]
    rows[9] = real[2]
    rows[7, n] = U64((MASK64 - body_add) & MASK64)
    rows[8, n] = U64((0 - body_add) & MASK64)
    rows[9, n] = U64(((1 << 63) - body_add) & MASK64)
    return rows


def key_pattern(n: int) -> np.ndarray:
    """The fixed LWE 'key' of noiseless_bsk: runs of four ones, three zeros and four times -1 (2^64 - 1)."""
    r = np.arange(n) % 11
    return np.where(r < 4, U64(1), np.where(r < 7, U64(0), U64(MASK64))).astype(U64)


def _gadget_rows(levels: int, base_log: int, k: int, N: int, m: int) -> np.ndarray:
    """m (0, 1 or -1) times the gadget matrix, [levels][k+1][(k+1)N]: row (l, q) holds
    m << (64 - base_log (l+1)), mod 2^64, at coefficient 0 of polynomial q (a GGSW of m with zero masks and
    zero noise, valid under any key)."""
    assert m in (0, 1, -1)
    g = np.zeros((levels, k + 1, (k + 1) * N), dtype=U64)
    for l in range(levels):
        for q in range(k + 1):
            g[l, q, q * N] = U64((m << (64 - base_log * (l + 1))) & MASK64)
    return g


def noiseless_bsk(params: dict, s: np.ndarray) -> np.ndarray:
    """A bootstrapping key [n][pbs_l][k+1][(k+1)N] (flattened) whose entry i is the noiseless trivial GGSW of
    s[i], s[i] in {0, 1, 2^64 - 1}.  An s[i] = 0 entry is all zero: that CMux step adds exact zeros to every
    polynomial.  Under this key the mask polynomials of an accumulator that starts with a zero mask stay
    exactly zero."""
    n, k, N = params["n"], params["k"], params["N"]
    s = np.asarray(s, dtype=U64)
    assert len(s) == n and np.isin(s, [0, 1, MASK64]).all()
    bsk = np.zeros((n, params["pbs_l"], k + 1, (k + 1) * N), dtype=U64)
    for m, word in ((1, 1), (-1, MASK64)):
        bsk[s == U64(word)] = _gadget_rows(params["pbs_l"], params["pbs_b"], k, N, m)
    return bsk.reshape(-1)


def trivial_ggsw(params: dict, bit: int) -> np.ndarray:
    """The circuit bootstrap's GGSW layout [cbs_l][k+1][(k+1)N] (flattened) holding the noiseless trivial
    GGSW of `bit`; bit = 0 is all zero, bit = -1 is the negated gadget (see the module docstring)."""
    return _gadget_rows(params["cbs_l"], params["cbs_b"], params["k"], params["N"], int(bit)).reshape(-1)


def masked_ggsw(params: dict, bit: int) -> np.ndarray:
    """trivial_ggsw(bit) with a non-zero word at coefficient 0 of the mask polynomials of the top level's body
    row (still an ordinary GGSW: an encryption of `bit` under the all-zero key).  An accumulator with a zero
    mask gets non-zero mask polynomials from it, while its body is computed as under trivial_ggsw.  The word
    is 2^(63-B) + a small odd number, so that a top digit of 2^(B-2) .. 2^(B-1) times it is 2^61 .. 2^62: on the
    differences of first_step_lut every lane of the torus tail holds a full-size value and none takes the
    wave to the fallback."""
    k, N, B = params["k"], params["N"], params["cbs_b"]
    g = _gadget_rows(params["cbs_l"], B, k, N, int(bit))
    for q in range(k):
        g[0, k, q * N] = U64((1 << (63 - B)) + 12345 + 2 * q)
    return g.reshape(-1)


# the polynomials of the fast-path saturation case: test_gpu_vp_edges.py runs them, test_edge_inputs.py pins them
FIRST_STEP_SEED, FIRST_STEP_LUTS = 77, 24


def first_step_lut(N: int, rng) -> np.ndarray:
    """LUT polynomial p whose first vertical-packing difference X^-1 p - p is exactly 2^63 at coefficient 0
    (the coefficient the sample extraction of a one-input vertical packing returns) and a full-size random
    word everywhere else: under masked_ggsw(-1) the tail input at coefficient 0 is -1/2 up to the transform's
    rounding, which differs from one random polynomial to the next, and no lane holds a small value."""
    d = (random_words(rng, N) & U64((1 << 62) - 1)) | U64(1 << 62)  # in [2^62, 2^63): no small digit sums
    d[0] = U64(1 << 63)
    p = np.zeros(N, dtype=U64)
    p[1:] = np.cumsum(d[:-1], dtype=U64)  # p[j+1] = p[j] + d[j]; the wrap's difference -p[0] - p[N-1] is what it is
    return p


def const_lut_glwe(params: dict, value: int) -> np.ndarray:
    """Accumulator GLWE [(k+1)N] with a zero mask and the body polynomial constant `value`."""
    k, N = params["k"], params["N"]
    g = np.zeros((k + 1) * N, dtype=U64)
    g[k * N:] = U64(value)
    return g


def random_words(rng, shape) -> np.ndarray:
    return rng.integers(0, 1 << 63, size=shape, dtype=U64) * U64(2) + rng.integers(0, 2, size=shape, dtype=U64)


# u64 -> f64 conversion edges of the forward torus transform: zero, the sign boundary 2^63 and its
# neighbours, all ones, and words that sit on or next to round-to-even ties of the 53-bit significand
GGSW_EDGE_WORDS = np.array([0, 1 << 63, (1 << 63) - 1, MASK64, (1 << 53) + 1, (1 << 63) + (1 << 10),
                            (1 << 63) - (1 << 9)], dtype=U64)


def crafted_ggsw(params: dict) -> np.ndarray:
    """A GGSW-shaped array [cbs_l (k+1) (k+1) N] made of GGSW_EDGE_WORDS, repeated."""
    k, N = params["k"], params["N"]
    return np.resize(GGSW_EDGE_WORDS, params["cbs_l"] * (k + 1) * (k + 1) * N).copy()


# ---- integer keyswitches (ksgemm.hpp): crafted keys, decomposer edges, saturating rows ------------------------
# Shared by test_gpu_ks_edges.py (GPU against the oracle's u64 loops) and test_ks_edge_inputs.py (CPU pins).
# A keyswitch is out = body - sum_kd d[kd] KEY[kd][col] mod 2^64.  The int8 GEMMs split d into signed limbs and
# KEY into 8 balanced byte limbs and rely on every i32 partial sum being exact; under a real (uniform) key those
# sums are random walks far below the design bounds, and key limb carry chains stay short.  The keys below are
# plain u64 arrays in the layouts of the KSK [K][ks_l][n+1] and the PFPKSK [k+1][K+1][pfks_l][(k+1)N]
# ([n][pfks_l][(k+1)N] for the shortint_1bit packing key); they decrypt nothing and need not.

# the (base_log, levels) of every integer keyswitch of the six parameter sets: (ks_b, ks_l) and (pfks_b, pfks_l)
KS_SHAPES = ((3, 4), (2, 6), (2, 8), (6, 2), (24, 1), (16, 2), (12, 3))

_LIMB_CHAIN_WORDS = (
    0x7F7F7F7F7F7F7F80,  # every balanced limb -128, a carry out of every byte
    0x7F7F7F7F7F7F7F7F,  # every limb +127
    0x8080808080808080,  # limb 0 = -128, then (0x80 + 1) = -127 with a carry, all the way up
    0xFFFFFFFFFFFFFFFF,  # limb 0 = -1, every other limb 0: the carry chain that wraps mod 2^64
    0x8000000000000000,  # only limb 7, at -128 (its carry is the one dropped mod 2^64)
    0x0000000000000080,  # limb 0 = -128, limb 1 = +1
    0x00000000000000FF,  # limb 0 = -1, limb 1 = +1
    0x0100000000000000,  # only limb 7, at +1: shifted out by any pre-shift
    0,
    1,
    0x9E3779B97F4A7C15,  # three full-size words (fixed; any would do)
    0xC2B2AE3D27D4EB4F,
    0x165667B19E3779F9,
)


def limb_chain_words() -> list:
    """Thirteen fixed u64 key words aimed at key_limbs (ksgemm.hpp) and at prep_key_kl's pre-shift v << 8 limb:
    the carry chains above, zero, one and three full-size words."""
    return list(_LIMB_CHAIN_WORDS)


def pattern_key(length: int) -> np.ndarray:
    """limb_chain_words() repeated to `length` (np.resize).  The period is 13, a prime that divides none of the
    strides of the key layouts: n + 1 = 672, 680, 678, 666, 786, 641 of the keyswitch keys, glwe_len = 2560 and 3072 of the
    (packing) functional keys, and the (K+1) pfks_l glwe_len blocks of the k + 1 functional keys
    (test_ks_edge_inputs.py checks this from get_params).  Key row r = (i, l) therefore starts at phase
    r * stride mod 13 with stride invertible mod 13: any 13 consecutive rows are 13 different rotations of the
    list, so neighbouring columns, the ks_l / pfks_l <= 8 levels of one coefficient, neighbouring coefficients
    and the k + 1 functional keys all differ, and an index mix-up between any of them changes the result."""
    return np.resize(np.array(_LIMB_CHAIN_WORDS, dtype=U64), length).copy()


SATURATING_WORD = 0x7F7F7F7F7F7F7F80


def saturating_key(length: int) -> np.ndarray:
    """Every word 0x7F7F7F7F7F7F7F80: all eight balanced limbs are -128, and v << 8, v << 16 (what prep_key_kl
    feeds the K-layout GEMM) keep -128 from the shifted position up, with zeros below."""
    return np.full(length, SATURATING_WORD, dtype=U64)


def digits_np(x, base_log: int, levels: int) -> np.ndarray:
    """numpy model of the closest-representable signed decomposition (tfhe-rs SignedDecomposer; oracle.decompose
    is the reference, test_ks_edge_inputs.py pins this model on it): int64 [..., levels], index 0 the most
    significant level."""
    x = np.asarray(x, dtype=U64)
    nrb = 64 - base_log * levels
    s = x >> U64(nrb - 1)
    s = (s + (s & U64(1))) >> U64(1)
    mask = U64((1 << base_log) - 1)
    out = np.zeros(x.shape + (levels,), dtype=np.int64)
    with np.errstate(over="ignore"):  # res - 1 wraps on purpose
        for lev in range(levels, 0, -1):
            res = s & mask
            s = s >> U64(base_log)
            carry = (((res - U64(1)) | s) & res) >> U64(base_log - 1)
            s = s + carry
            out[..., lev - 1] = res.astype(np.int64) - (carry.astype(np.int64) << base_log)
    return out


def compose_digits(digits, base_log: int) -> int:
    """sum_l d_l 2^(64 - base_log (l + 1)) mod 2^64, digits most significant first."""
    return sum(int(d) << (64 - base_log * (l + 1)) for l, d in enumerate(digits)) & MASK64


def decomposer_edge_words(base_log: int, levels: int) -> dict:
    """Coefficients on the edges of the closest-representable signed decomposition with `levels` levels of base
    B = 2^base_log, as {name: word}.  half = B / 2, w_l = 2^(64 - base_log l) is the weight of level l (1 = most
    significant), u = w_levels the weight of the last one.  Digits are listed most significant first:

      zero             0                                  all digits 0
      all_ones         2^64 - 1                           rounds up and wraps: all digits 0
      top_bit          2^63                               [+half, 0, ..]: the top level's upper end (it has no -half)
      tie_below        u/2 - 1                            just under the rounding tie: all digits 0
      tie              u/2                                the exact tie rounds up: [0, .., 0, 1]
      tie_above        u/2 + 1                            [0, .., 0, 1]
      half_keep_l      half w_l            (l >= 2)       residue exactly half at level l and the residue above it
                                                          below half (its top bit, the one the carry rule reads,
                                                          clear): digit l stays +half, every other digit 0
      half_carry_l     half (w_(l-1) + w_l)  (l >= 2)     the same residue with that bit set: digit l is -half, and
                                                          the carry makes the residue above half + 1, i.e. digit
                                                          l-1 = -half + 1 with a carry of its own (digit l-2 = 1;
                                                          dropped when l-1 is the top level)
      ripple           half (w_1 + .. + w_L)              a carry out of every level:
                                                          [-half + 1, .., -half + 1, -half] (two neighbouring levels
                                                          can never both hold +half or both -half)
      wrap_minus_unit  2^64 - u                           raw digits all B - 1: [0, .., 0, -1], the carry runs up
                                                          through every level and off the top
      top_min          (half + 1) w_1                     the top level's lower end: [-half + 1, 0, ..]
      top_max_low_min  half w_1 + (half + 1) w_L  (L >= 2)  the top level's upper end over a negative last digit:
                                                          [+half, 0, .., 0, 1, -half + 1] (L > 2: the carry stops at
                                                          level L-1); with L = 2 it reaches the top level:
                                                          [-half + 1, -half + 1]

    With levels = 1 the per-level entries do not exist and ripple = top_bit.  Built from the
    definition; edge_word_digits gives the digits named here, and test_ks_edge_inputs.py holds oracle.decompose
    against them."""
    B, L = base_log, levels
    half = 1 << (B - 1)
    w = lambda l: 1 << (64 - B * l)
    u = w(L)
    words = {"zero": 0, "all_ones": MASK64, "top_bit": 1 << 63, "tie_below": u // 2 - 1, "tie": u // 2,
             "tie_above": u // 2 + 1}
    for l in range(2, L + 1):
        words[f"half_keep_{l}"] = half * w(l)
        words[f"half_carry_{l}"] = half * (w(l - 1) + w(l))
    words["ripple"] = (half * sum(w(l) for l in range(1, L + 1))) & MASK64
    words["wrap_minus_unit"] = (1 << 64) - u
    words["top_min"] = ((half + 1) * w(1)) & MASK64
    if L >= 2:
        words["top_max_low_min"] = (half * w(1) + (half + 1) * w(L)) & MASK64
    return words


def edge_word_digits(base_log: int, levels: int) -> dict:
    """{name: digits, most significant first} as the docstring of decomposer_edge_words names them."""
    L, half = levels, 1 << (base_log - 1)
    unit = lambda l, v: [v if i == l else 0 for i in range(1, L + 1)]
    d = {"zero": [0] * L, "all_ones": [0] * L, "top_bit": unit(1, half), "tie_below": [0] * L, "tie": unit(L, 1),
         "tie_above": unit(L, 1)}
    for l in range(2, L + 1):
        d[f"half_keep_{l}"] = unit(l, half)
        d[f"half_carry_{l}"] = [{l: -half, l - 1: -half + 1, l - 2: 1}.get(i, 0) for i in range(1, L + 1)]
    d["ripple"] = [-half + 1] * (L - 1) + [-half] if L > 1 else [half]
    d["wrap_minus_unit"] = unit(L, -1)
    d["top_min"] = unit(1, -half + 1)
    if L > 2:
        d["top_max_low_min"] = [half] + [0] * (L - 3) + [1, -half + 1]
    elif L == 2:
        d["top_max_low_min"] = [-half + 1, -half + 1]
    return d


def edge_row(base_log: int, levels: int, length: int) -> np.ndarray:
    """decomposer_edge_words repeated to `length` words."""
    return np.resize(np.array(list(decomposer_edge_words(base_log, levels).values()), dtype=U64), length).copy()


# -- limb models of the three int8 operand layouts --
def key_limbs_np(words) -> np.ndarray:
    """Balanced signed byte limbs of u64 words (ksgemm.hpp key_limbs): int64 [..., 8], least significant first,
    sum_j limb_j 256^j = word mod 2^64."""
    k = np.asarray(words, dtype=U64).copy()
    out = np.zeros(k.shape + (8,), dtype=np.int64)
    with np.errstate(over="ignore"):  # mod 2^64
        for j in range(8):
            s = (k & U64(0xFF)).astype(np.uint8).astype(np.int8).astype(np.int64)
            out[..., j] = s
            k = (k - s.astype(U64)) >> U64(8)
    return out


def balanced_limbs(d, bits: int, n: int) -> np.ndarray:
    """n balanced signed limbs of `bits` bits of int64 digits, least significant first, the last taking the rest
    (prep_digits / prep_digits3 / kl_next_limb): int64 [..., n]."""
    d = np.asarray(d, dtype=np.int64).copy()
    out = np.zeros(d.shape + (n,), dtype=np.int64)
    for m in range(n - 1):
        limb = ((d + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))
        out[..., m] = limb
        d = (d - limb) >> bits
    out[..., n - 1] = d
    return out


def _kslots_fit(lo: int, hi: int):
    """kslots.hpp kslots_fit: the fewest byte limbs n and the offset c that hold the digits [lo, hi]."""
    for n in range(1, 5):
        span = (256 ** n - 1) // 255
        mn, mx = -128 * span, 127 * span
        c = max(hi - mx, 0)
        if lo - c >= mn:
            return n, c
    return None


def kslots_plan(base_log: int, levels: int, allow_clamp: bool = True) -> dict:
    """numpy-side mirror of kslots.hpp kslots_build (test_ks_edge_inputs.py holds it against what
    tests/native/kslots_test.cpp prints for the compiled plan): per level the limb count, the digit offset and
    whether +half is stored as -half; S the slots per coefficient."""
    half = 1 << (base_log - 1)
    nlimb, off, clamp = [], [], []
    for l in range(levels):
        lo, hi = (-half + 1 if l == 0 else -half), half
        n, c = _kslots_fit(lo, hi)
        cl = False
        if allow_clamp and l > 0:
            alt = _kslots_fit(lo, hi - 1)
            if alt and alt[0] < n:
                (n, c), cl = alt, True
        nlimb.append(n)
        off.append(c)
        clamp.append(cl)
    assert sum(nlimb) <= 8
    return {"S": sum(nlimb), "nlimb": nlimb, "off": off, "clamp": clamp}


LIMB_MODELS = ("bytes", "rows6", "kslots")


def digit_limbs(digits, level: int, base_log: int, levels: int, limb_model: str) -> np.ndarray:
    """The signed limbs the GEMM's A operand holds for level `level` (0 = most significant) digits, int64 [..., n]:
      bytes   the digit itself, one byte (prep_digits<1, 8>: the LWE and the packing keyswitch)
      rows6   three balanced 6-bit limbs (prep_digits3<6>: the PFKS row layout, one GEMM row per limb)
      kslots  the level's byte limbs of (digit - offset), +half stored as -half on a clamped level
              (prep_digits_kl: the PFKS K layout)"""
    d = np.asarray(digits, dtype=np.int64)
    if limb_model == "bytes":
        return d[..., None]
    if limb_model == "rows6":
        return balanced_limbs(d, 6, 3)
    assert limb_model == "kslots"
    plan, half = kslots_plan(base_log, levels), 1 << (base_log - 1)
    if plan["clamp"][level]:
        d = np.where(d == half, -half, d)
    return balanced_limbs(d - plan["off"][level], 8, plan["nlimb"][level])


def saturating_coefficient(base_log: int, levels: int, limb_model: str) -> int:
    """The coefficient whose digit limbs have the largest sum of absolute values under `limb_model`, found by
    search: every digit of every level's range is split by digit_limbs, the two best digits per level and sign
    are combined, and the best combination that the decomposer really produces (digits_np of the composed word
    gives the same digits back) wins.  Limbs of one sign are preferred (and decide ties): against a constant key
    the partial sum of a GEMM column is the signed sum of the limbs."""
    import itertools
    half = 1 << (base_log - 1)
    best = None
    for sign in (-1, 1):
        cands = []
        for l in range(levels):
            d = np.arange(-half + 1 if l == 0 else -half, half + 1, dtype=np.int64)
            limbs = digit_limbs(d, l, base_log, levels, limb_model)
            score = np.where((limbs * sign >= 0).all(axis=-1), np.abs(limbs).sum(axis=-1), -1)
            order = np.argsort(-score, kind="stable")[:2]
            cands.append([(int(d[i]), int(score[i])) for i in order if score[i] >= 0])
        for combo in sorted(itertools.product(*cands), key=lambda c: -sum(s for _, s in c)):
            digits = [d for d, _ in combo]
            x = compose_digits(digits, base_log)
            if digits_np(U64(x), base_log, levels).tolist() == digits:
                total = sum(s for _, s in combo)
                if best is None or total > best[0]:
                    best = (total, x)
                break
    assert best is not None
    return best[1]


def modelled_partial_sums(row, key_col, base_log: int, levels: int, limb_model: str) -> np.ndarray:
    """int64 model of the i32 accumulators of one output (one ciphertext row against one key column): `row` holds
    the n_coef input coefficients, key_col the u64 key words [n_coef][levels] of that column.  Returns the partial
    sums the GEMM forms before its epilogue: [8] (bytes), [3][8] (rows6: one per digit-limb row) or [8] (kslots),
    the last axis the key limb j."""
    dig = digits_np(row, base_log, levels)                       # [n_coef][levels]
    key_col = np.asarray(key_col, dtype=U64).reshape(len(dig), levels)
    if limb_model == "kslots":
        plan = kslots_plan(base_log, levels)
        acc = np.zeros(8, dtype=np.int64)
        for l in range(levels):
            limbs = digit_limbs(dig[:, l], l, base_log, levels, limb_model)  # [n_coef][nlimb]
            for m in range(plan["nlimb"][l]):
                acc += limbs[:, m] @ key_limbs_np(key_col[:, l] << U64(8 * m))  # the pre-shifted key row
        return acc
    kl = key_limbs_np(key_col)                                   # [n_coef][levels][8]
    acc = 0
    for l in range(levels):
        acc = acc + np.einsum("im,ij->mj", digit_limbs(dig[:, l], l, base_log, levels, limb_model), kl[:, l])
    return acc[0] if limb_model == "bytes" else acc


# ---- vertical packing of LUTs wider than one polynomial (the CMux tree) -----------------------------------------
# Shared by test_gpu_vp_tree.py (GPU against oracle.vertical_packing) and test_edge_inputs.py (CPU pins).  With
# n_in = log2 N + tree inputs a LUT output holds 2^tree polynomials; the first `tree` GGSWs (the selector's most
# significant bits) choose the polynomial through a tree of CMuxes, the rest rotate it.  Selector rows are lists
# of n_in values from {0, 1, -1}, MSB first, standing for the trivial GGSWs of those values.

TREE_DEPTHS = (1, 2, 3)
TREE_N_OUT = (1, 3)
# (tree, n_out) of the 16 -> n LUT shape of the N = 1024 sets: a 64-polynomial base
DEEP_TREE, DEEP_N_OUT = 6, 2

# the leading (tree) entries of the mixed rows read differently backwards from depth 2 on, so that a tree that
# takes its GGSWs in the wrong order selects another polynomial (test_edge_inputs.py checks it)
_MIXED_BITS = (1, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0)
_NEGATED_CYCLES = ((-1,), (-1, 1, 1, 0, 1, 1, 0, -1), (1, -1))


def tree_lut_fn(n_out: int):
    """f(selector) of the 0 / 2^63 tables: a fixed multiplicative hash, so that the bits of neighbouring entries,
    and with them neighbouring polynomials of one output, differ."""
    return lambda v: (((v + 1) * 0x9E3779B1 & 0xFFFFFFFF) >> 15) & ((1 << n_out) - 1)


def tree_selector_rows(n_in: int) -> list:
    """Three rows of {0, 1}: all zero, all one and a fixed word whose leading (tree) bits are 1, 0, 0, 1, 0, 1."""
    assert n_in <= len(_MIXED_BITS)
    return [[0] * n_in, [1] * n_in, list(_MIXED_BITS[:n_in])]


def tree_negated_rows(n_in: int) -> list:
    """Three rows of {0, 1, -1} with -1 at tree positions too.  For every depth in TREE_DEPTHS the selector of the
    leaf level (position tree - 1) is non-zero in every row, and both 1 and -1 occur there among the rows: a leaf
    difference of 2^63 becomes a tail input of +1/2 in one group and of -1/2 in another."""
    return [[c[i % len(c)] for i in range(n_in)] for c in _NEGATED_CYCLES]


def selector_value(row) -> int:
    """The LUT entry a row of {0, 1} selects (MSB first)."""
    v = 0
    for b in row:
        assert b in (0, 1)
        v = 2 * v + b
    return v


def tree_mixed_lut(n_out: int, N: int, tree: int, seed: int) -> np.ndarray:
    """[n_out][2^tree][N] (flattened): polynomial 1 of output 0 is the constant 2^62; of the others, numbered
    q = j 2^tree + i, those with q % 3 == 2 alternate 2^62 and random words in runs of eight and the rest are random
    full-size words.  Every polynomial is seeded by (seed, j, i), so all of them differ, and a leaf, pair, output
    or group mix-up changes the result."""
    cnt = 1 << tree
    lut = np.zeros((n_out, cnt, N), dtype=U64)
    for j in range(n_out):
        for i in range(cnt):
            q = j * cnt + i
            lut[j, i] = random_words(np.random.default_rng([seed, j, i]), N)
            if q == 1:
                lut[j, i] = U64(1 << 62)
            elif q % 3 == 2:
                lut[j, i, (np.arange(N) // 8) % 2 == 0] = U64(1 << 62)
    return lut.reshape(-1)


# ---- shortint_1bit: the noiseless set, the test-vector windows and the packing sum --------------------------------
# Shared by test_gpu_s1_edges.py (GPU against the oracle and against these references) and test_edge_inputs.py (CPU
# pins).  The blind rotation of the set is br512x4<7, true, 6>: 7 levels of 2^6, 22 discarded bits, a test vector per
# ciphertext.

def zero_key(length: int) -> np.ndarray:
    """An all-zero key array: under it a (packing) keyswitch returns the trivial ciphertext of the input's body."""
    return np.zeros(length, dtype=U64)


def noiseless_test_vectors(params: dict, rng) -> dict:
    """The three test vectors of the noiseless-key runs, {name: GLWE [(k+1)N]}: zero mask with the body constant
    2^62 (every non-zero rotated difference is exactly 2^63: the top digit is the tie 2^(B-1)), zero mask with the
    body constant 2^63 (every rotated difference is 2^64 = 0: exact zeros at every step) and random words."""
    return {"const 2^62": const_lut_glwe(params, 1 << 62), "const 2^63": const_lut_glwe(params, 1 << 63),
            "random": random_words(rng, (params["k"] + 1) * params["N"])}


def monomial_mul_np(p, e: int) -> np.ndarray:
    """X^e p mod X^N + 1 along the last axis (N its length, any integer e), wrapping u64."""
    p = np.asarray(p, dtype=U64)
    N = p.shape[-1]
    e %= 2 * N
    if e >= N:
        p, e = U64(0) - p, e - N
    return p.copy() if e == 0 else np.concatenate([U64(0) - p[..., N - e:], p[..., :N - e]], axis=-1)


TV_WINDOW_POSITIONS = lambda N: (0, 1, N // 4 - 1, N // 4, 3 * N // 4 - 1, 3 * N // 4, N - 1)
TV_WINDOW_VALUES = (1 << 63, MASK64)  # of P0 and of P1


def tv_window_polys(N: int) -> list:
    """Polynomial pairs [(name, P0 [N], P1 [N])] on the window edges of test_vector_from_ciphertexts: a single
    non-zero coefficient at each of the positions 0, 1, N/4 - 1, N/4, 3N/4 - 1, 3N/4 and N - 1, 2^63 in P0 and
    2^64 - 1 in P1 (single_coefficient_tv gives the closed form); all ones against all 2^63; one random pair."""
    pairs = []
    for pos in TV_WINDOW_POSITIONS(N):
        p0, p1 = np.zeros(N, dtype=U64), np.zeros(N, dtype=U64)
        p0[pos], p1[pos] = U64(TV_WINDOW_VALUES[0]), U64(TV_WINDOW_VALUES[1])
        pairs.append((f"single {pos}", p0, p1))
    pairs.append(("ones / 2^63", np.ones(N, dtype=U64), np.full(N, 1 << 63, dtype=U64)))
    rng = np.random.default_rng(N + 4)
    pairs.append(("random", random_words(rng, N), random_words(rng, N)))
    return pairs


def single_coefficient_tv(N: int, pos: int, v0: int, v1: int) -> np.ndarray:
    """The test vector of P0 = v0 X^pos, P1 = v1 X^pos in closed form: shift i moves the coefficient to
    t = pos + i mod N, negated when it wraps, and takes v1 for N/4 <= i < 3N/4 and v0 otherwise."""
    tv = np.zeros(N, dtype=U64)
    for t in range(N):
        i = (t - pos) % N
        v = v1 if N // 4 <= i < 3 * N // 4 else v0
        tv[t] = U64(v if t >= pos else (-v) & MASK64)
    return tv


def tv_from_polys_np(P0, P1) -> np.ndarray:
    """test_vector_from_ciphertexts on the packing keyswitches P0, P1 ([..., N], the last axis a polynomial):
    sum_{i < N} X^i (P1 if N/4 <= i < 3N/4 else P0), negacyclic, wrapping u64, as N explicit rotations (the
    device kernel takes windows of prefix sums instead)."""
    P0, P1 = np.asarray(P0, dtype=U64), np.asarray(P1, dtype=U64)
    assert P0.shape == P1.shape
    N = P0.shape[-1]
    acc = np.zeros_like(P0)
    for i in range(N):
        acc += monomial_mul_np(P1 if N // 4 <= i < 3 * N // 4 else P0, i)
    return acc


def pack_np(pks_rows) -> np.ndarray:
    """The packing sum sum_j X^j P_j over the keyswitched GLWEs pks_rows [count][..., N], as explicit rotations."""
    rows = np.asarray(pks_rows, dtype=U64)
    assert 1 <= len(rows) <= rows.shape[-1]
    acc = np.zeros_like(rows[0])
    for j, p in enumerate(rows):
        acc += monomial_mul_np(p, j)
    return acc


def asymmetric_table(nbits: int, seed: int = 0) -> list:
    """A 0 / 1 function table of nbits inputs (index MSB first) that no permutation of the input bits combined
    with complementing any of them leaves unchanged (is_asymmetric_table checks it): a selector tree that
    gathers its bits in another order, or reads a selector inverted, computes another function."""
    rng = np.random.default_rng([nbits, seed])
    while True:
        tab = rng.integers(0, 2, 1 << nbits).tolist()
        if is_asymmetric_table(tab, nbits):
            return tab


def is_asymmetric_table(tab, nbits: int) -> bool:
    """Up to four bits by trying every permutation and complement.  Above that by a sufficient condition: with
    c_i(b) the number of ones of the table among the indices whose bit i is b, a symmetry that sends bit i to bit
    j complemented by f needs c_j(b ^ f) = c_i(b); so if the unordered pairs {c_i(0), c_i(1)} all differ no bit
    can move, and if c_i(0) != c_i(1) for every i none can be complemented."""
    import itertools
    idx = np.arange(1 << nbits)
    bits = [(idx >> (nbits - 1 - i)) & 1 for i in range(nbits)]  # bit i, MSB first
    t = np.asarray(tab)
    if nbits > 4:
        sig = [(int(t[b == 0].sum()), int(t[b == 1].sum())) for b in bits]
        return all(c0 != c1 for c0, c1 in sig) and len({frozenset(s) for s in sig}) == nbits
    for perm in itertools.permutations(range(nbits)):
        for flip in range(1 << nbits):
            if flip == 0 and perm == tuple(range(nbits)):
                continue
            j = sum((bits[perm[i]] ^ ((flip >> i) & 1)) << (nbits - 1 - i) for i in range(nbits))
            if np.array_equal(t[j], t):
                return False
    return True


# ---- extract_bits of the 8-bit model: trivial ints on the bit boundaries (test_gpu_extract8_edges.py) ------------
EXTRACT_TIE_VALUES = (0x00, 0xFF, 0x80)


def extract_tie_ints(K: int, v: int, delta_log: int = 56) -> np.ndarray:
    """Four big-key LWEs [4][K+1] with a zero mask and the bodies v 2^56, v 2^56 + 2^55 - 1 (just below the
    rounding boundary of bit 0), v 2^56 + 2^55 (on it) and v 2^56 - 1 (every bit below the message set)."""
    half = 1 << (delta_log - 1)
    rows = np.zeros((4, K + 1), dtype=U64)
    for r, d in enumerate((0, half - 1, half, -1)):
        rows[r, K] = U64(((v << delta_log) + d) & MASK64)
    return rows
