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
