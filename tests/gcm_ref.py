"""The tests' own restatement of the GCM plans of DESIGN.md 5.14, from a byte-wise "times x" alone: the field in
GCM's bit-reflected order, the squaring rows, the product's chunk and reduction rows, the power schedule and a
frame's tag rows.  Shared by tests/test_aes_gcm.py (CPU) and tests/test_gpu_gcm.py (numpy u64 sums)."""
from functools import lru_cache

import numpy as np

KEY1 = bytes(16)
H1 = bytes.fromhex("66e94bd4ef8a2c3b884cfa59ca342b2e")  # test case 2: E_0(0^128)
KEY3 = bytes.fromhex("feffe9928665731c6d6a8f9467308308")
IV3 = bytes.fromhex("cafebabefacedbaddecaf888")
PT3 = bytes.fromhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a72"
                    "1c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b391aafd255")
AAD4 = bytes.fromhex("feedfacedeadbeeffeedfacedeadbeefabaddad2")
TAG3 = bytes.fromhex("4d5c2af327cd64a62cf35abd2ba6fab4")
TAG4 = bytes.fromhex("5bc94fbc3221a5db94fae95ae7121a47")


def times_x(b: bytes) -> bytes:
    """A right shift of the 128-bit string, 0xE1 into byte 0 on carry out."""
    out, carry = bytearray(16), 0
    for i in range(16):
        out[i] = (b[i] >> 1) | (carry << 7)
        carry = b[i] & 1
    if carry:
        out[0] ^= 0xE1
    return bytes(out)


def coefs(b: bytes):
    """Coefficient k = bit k from the MSB of byte 0."""
    return [(b[k >> 3] >> (7 - (k & 7))) & 1 for k in range(128)]


def from_coefs(c) -> bytes:
    out = bytearray(16)
    for k in range(128):
        out[k >> 3] |= (int(c[k]) & 1) << (7 - (k & 7))
    return bytes(out)


def mul(x: bytes, y: bytes) -> bytes:
    """SP 800-38D algorithm 1 with the byte-wise times_x."""
    z, v = bytearray(16), y
    for bit in coefs(x):
        if bit:
            z = bytearray(a ^ b for a, b in zip(z, v))
        v = times_x(v)
    return bytes(z)


ONE = bytes([0x80]) + bytes(15)


@lru_cache(maxsize=None)
def x_pows():
    """x^0 .. x^254, reduced."""
    out, v = [], ONE
    for _ in range(255):
        out.append(v)
        v = times_x(v)
    return out


@lru_cache(maxsize=None)
def square_rows():
    """rows[r] = the operand bits i with x^(2 i) mod p containing x^r."""
    xp = x_pows()
    return [[i for i in range(128) if coefs(xp[2 * i])[r]] for r in range(128)]


def nibble_product(v: int) -> int:
    """The 8 -> 7 table: a's nibble in the high four input bits, b's in the low four, the first bit of a nibble the
    lowest coefficient; coefficient d of the carry-less product at bit 6 - d."""
    r = 0
    for p in range(4):
        for q in range(4):
            if (v >> (7 - p)) & 1 and (v >> (3 - q)) & 1:
                r ^= 1 << (6 - (p + q))
    return r


@lru_cache(maxsize=None)
def product_plan():
    """(chunks, chunk_t, reduce): chunks[c] lists partial bits 7 g + d, g = 32 I + J ascending, at most 7 per chunk,
    per unreduced coefficient t = 4 I + 4 J + d; reduce[r] lists the chunks of every t with x^t mod p containing x^r."""
    chunks, chunk_t, per_t = [], [], []
    for t in range(255):
        parts = [7 * g + (t - 4 * (g >> 5) - 4 * (g & 31)) for g in range(1024)
                 if 0 <= t - 4 * (g >> 5) - 4 * (g & 31) < 7]
        per_t.append(len(parts))
        for at in range(0, len(parts), 7):
            chunks.append(parts[at:at + 7])
            chunk_t.append(t)
    xp = [coefs(v) for v in x_pows()]
    reduce = [[c for c, t in enumerate(chunk_t) if xp[t][r]] for r in range(128)]
    return chunks, chunk_t, reduce, per_t


def pair_sources(g: int):
    """The 8 operand bits of group g among a[0..128) b[0..128)."""
    return [4 * (g >> 5) + p for p in range(4)] + [128 + 4 * (g & 31) + q for q in range(4)]


def power_schedule(n: int):
    """[(squares, products)] per generation: an even power is the square of k / 2, an odd one H^(k-1) H."""
    gen = {1: 0}
    for k in range(2, n + 1):
        gen[k] = 1 + (gen[k - 1] if k & 1 else gen[k // 2])
    out = [([], []) for _ in range(max(gen.values()))]
    for k in range(2, n + 1):
        out[gen[k] - 1][k & 1].append(k)
    return out


def hashed_blocks(aad: bytes, c: bytes):
    buf = (aad + bytes(-len(aad) % 16) + c + bytes(-len(c) % 16) + (8 * len(aad)).to_bytes(8, "big")
           + (8 * len(c)).to_bytes(8, "big"))
    return [buf[i:i + 16] for i in range(0, len(buf), 16)]


def tag_rows(aad: bytes, c: bytes, tag_len: int):
    """rows[r] = the table bits 128 (k - 1) + i with coefficient r of X_(m+1-k) x^i set, ascending (k, i)."""
    xs = hashed_blocks(aad, c)
    m = len(xs)
    rows = [[] for _ in range(8 * tag_len)]
    for k in range(1, m + 1):
        col = xs[m - k]
        for i in range(128):
            cf = coefs(col)
            for r in range(8 * tag_len):
                if cf[r]:
                    rows[r].append(128 * (k - 1) + i)
            col = times_x(col)
    return rows


def row_chunks(row, first=55, later=64):
    """Greedy chunks of a row's sources: the first has room for 55 next to the E(J0) bit, later ones for 64."""
    out, at, room = [], 0, first
    while True:
        out.append(row[at:at + room])
        at += room
        room = later
        if at >= len(row):
            return out


def sum_rows(sources: np.ndarray, rows) -> np.ndarray:
    """LWE row sums in u64: sources [n][L] -> [len(rows)][L]."""
    out = np.zeros((len(rows), sources.shape[-1]), dtype=np.uint64)
    for r, row in enumerate(rows):
        if len(row):
            out[r] = sources[np.asarray(row, dtype=np.int64)].sum(axis=0, dtype=np.uint64)
    return out
