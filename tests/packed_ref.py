"""numpy restatements of the packed-I/O maps of csrc/glwe_pack.hpp for params_sqrd_lvl_64 (N = 512, k = 4), shared
by the CPU and GPU tests of the packed ciphertext I/O: the sample extraction of coefficient j, the multiplication
by X^j, the sum over the oracle's private functional keyswitch, and the phase of a GLWE under the binary key."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U64 = np.uint64
PN, PK = 512, 4
K = PK * PN
BIG = K + 1
GLWE = (PK + 1) * PN


def extract_np(glwes, count):
    """a[pN + i] = A_p[j - i] (i <= j), -A_p[N + j - i] (i > j), b = B[j], for bit b at coefficient j = b % N of GLWE
    b // N: [G][(k+1)N] -> [count][K+1]."""
    out = np.zeros((count, BIG), dtype=U64)
    i = np.arange(PN)
    for b in range(count):
        g, j = divmod(b, PN)
        polys = glwes[g].reshape(PK + 1, PN)
        vals = polys[:PK, np.where(i <= j, j - i, PN + j - i)]
        out[b, :K] = np.where(i <= j, vals, U64(0) - vals).reshape(-1)
        out[b, K] = polys[PK, j]
    return out


def rotate_np(glwe, j):
    """X^j times every polynomial of a GLWE: coefficient c is P[c - j] (c >= j), -P[N + c - j] (c < j)."""
    polys = np.roll(glwe.reshape(PK + 1, PN), j, axis=1)
    polys[:, :j] = U64(0) - polys[:, :j]
    return polys.reshape(-1)


def oracle_pfks_rows(ok, rows):
    """Keys.pfks(k, row) of every row, threads over the rows (the oracle call is a pure function of its key)."""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda r: ok.pfks(PK, r), rows))


def oracle_pack(ok, rows):
    """sum_j X^j Keys.pfks(k, rows[j]) for up to N rows: one packed GLWE."""
    assert 1 <= len(rows) <= PN
    acc = np.zeros(GLWE, dtype=U64)
    for j, g in enumerate(oracle_pfks_rows(ok, rows)):
        acc += rotate_np(g, j)
    return acc


def glwe_phase_np(glwe, glwe_sk):
    """B - sum_p A_p S_p (mod X^N + 1, mod 2^64) of one GLWE under the binary key [k N]: [N] uint64."""
    c, i = np.meshgrid(np.arange(PN), np.arange(PN), indexing="ij")
    src, neg = (c - i) % PN, i > c
    polys = glwe.reshape(PK + 1, PN)
    phase = polys[PK].copy()
    for p in range(PK):
        terms = polys[p][src]
        terms = np.where(neg, U64(0) - terms, terms)
        phase -= (terms * glwe_sk[p * PN:(p + 1) * PN].astype(U64)[None, :]).sum(axis=1, dtype=U64)
    return phase


def signed(x):
    """uint64 torus words as centred int64."""
    return np.asarray(x, dtype=U64).view(np.int64)
