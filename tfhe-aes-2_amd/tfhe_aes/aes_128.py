"""AES-128 over the 1-bit WoP-PBS model -- Python mirror of the reference's `aes_128` module.

Reference:
  src/aes_128.rs                       Block/Key, SBOX, RC, ROUNDS, gf_256_mul (with its quirk)
  src/aes_128/plain.rs                 plain AES with a `rounds` parameter (test oracle)
  src/aes_128/fhe.rs:16-38             trait Aes128Encrypt {encrypt_block, encrypt_block_for_rounds, key_schedule}
  src/aes_128/fhe/fhe_encryption.rs    client-side bytes <-> Byte<Bit>
  src/aes_128/fhe/fhe_impls/shortint_woppbs_1bit.rs:131-151  ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
  src/util.rs:33-42                    MSB-first bit order
The FHE round function runs on the GPU through the C-ABI (tae_aes_*).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _native as N
from ._native import check, lib
from .tfhe import BitCt, ClientKey, Cleartext, FheContext, PackedBits, _handles
from .tfhe import _flatten_bits as _flat_bits

ROUNDS = 10

SBOX = [
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
    0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
    0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
    0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
    0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
    0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
    0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
    0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
    0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
    0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
    0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
    0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
    0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
    0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
    0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
    0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16,
]
RC = [0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36]


def gf_256_mul(a: int, b: int) -> int:
    """aes_128.rs:42-56, including `if high_bit != 0x80 { a ^= 0x1b }`."""
    res = 0
    for _ in range(8):
        if b & 1:
            res ^= a
        high = a & 0x80
        a = (a << 1) & 0xFF
        if high != 0x80:
            a ^= 0x1B
        b >>= 1
    return res


# ---------------------------------------------------------------- util.rs:33-42 ----
def u8_to_bits(byte: int) -> List[int]:
    return [1 if byte & (0x80 >> i) else 0 for i in range(8)]


def bits_to_u8(bits: Sequence[int]) -> int:
    return sum((int(b) & 1) << (7 - i) for i, b in enumerate(bits))


# ---------------------------------------------------------------- plain.rs ----
def key_schedule_plain(key: bytes) -> List[bytes]:
    """plain::key_schedule (plain.rs:106-132): 44 words of 4 bytes."""
    w = [bytes(key[4 * i:4 * i + 4]) for i in range(4)]
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[t[1]] ^ RC[i // 4], SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
        w.append(bytes(a ^ b for a, b in zip(w[i - 4], t)))
    return w


def encrypt_block_plain(expanded_key: Sequence[bytes], block: bytes, rounds: int = ROUNDS) -> bytes:
    """plain::encrypt_block (plain.rs:75-103); the last round always uses words 40..44."""
    rk = b"".join(expanded_key)
    s = [block[i] ^ rk[i] for i in range(16)]
    for r in range(1, rounds + 1):
        last = r == rounds
        s = [SBOX[x] for x in s]
        t = [s[4 * ((c + row) % 4) + row] for c in range(4) for row in range(4)]
        if not last:
            m = []
            for c in range(4):
                col = t[4 * c:4 * c + 4]
                m += [gf_256_mul(col[i], 2) ^ col[(i + 3) % 4] ^ col[(i + 2) % 4] ^ gf_256_mul(col[(i + 1) % 4], 3)
                      for i in range(4)]
            t = m
        k = rk[160:176] if last else rk[16 * r:16 * r + 16]
        s = [t[i] ^ k[i] for i in range(16)]
    return bytes(s)


def expand_key_and_encrypt_blocks(key: bytes, blocks: Sequence[bytes], rounds: int) -> List[bytes]:
    ek = key_schedule_plain(key)
    return [encrypt_block_plain(ek, b, rounds) for b in blocks]


# ---------------------------------------------------------------- FIPS-197 5.3 (no reference counterpart) ----
def gf_mul(a: int, b: int) -> int:
    """The true product in GF(2^8) modulo 0x11b (gf_256_mul above carries the reference's quirk, which
    cancels only inside the forward MixColumns)."""
    res = 0
    for _ in range(8):
        if b & 1:
            res ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return res


INV_SBOX = [0] * 256
for _x, _y in enumerate(SBOX):
    INV_SBOX[_y] = _x
INV_MIX = (14, 11, 13, 9)  # InvMixColumns: out(row) = 14 s(row) ^ 11 s(row+1) ^ 13 s(row+2) ^ 9 s(row+3)


def _inv_mix_columns(t: Sequence[int]) -> List[int]:
    return [gf_mul(t[4 * c + row], 14) ^ gf_mul(t[4 * c + (row + 1) % 4], 11) ^ gf_mul(t[4 * c + (row + 2) % 4], 13)
            ^ gf_mul(t[4 * c + (row + 3) % 4], 9) for c in range(4) for row in range(4)]


def decrypt_key_plain(expanded_key: Sequence[bytes]) -> List[bytes]:
    """The decryption key of FIPS-197 5.3.5, 44 words: words 0..3 and 40..43 are the expanded key's, words
    4r..4r+3 (r = 1..9) are InvMixColumns(rk[r])."""
    rk = b"".join(expanded_key)
    dk = bytearray(rk)
    for r in range(1, 10):
        dk[16 * r:16 * r + 16] = bytes(_inv_mix_columns(rk[16 * r:16 * r + 16]))
    return [bytes(dk[4 * i:4 * i + 4]) for i in range(44)]


def decrypt_block_plain(expanded_key: Sequence[bytes], block: bytes, rounds: int = ROUNDS) -> bytes:
    """The straightforward inverse cipher (FIPS-197 5.3, figure 12) with the ENCRYPTION key: inverts
    encrypt_block_plain(expanded_key, ., rounds), which uses round keys 0, 1..rounds-1 and 10."""
    rk = b"".join(expanded_key)
    s = [block[i] ^ rk[160 + i] for i in range(16)]
    for r in range(rounds - 1, -1, -1):
        s = [s[4 * ((c - row) % 4) + row] for c in range(4) for row in range(4)]  # InvShiftRows
        s = [INV_SBOX[x] for x in s]
        s = [s[i] ^ rk[16 * r + i] for i in range(16)]
        if r:
            s = _inv_mix_columns(s)
    return bytes(s)


def cbc_encrypt_plain(key: bytes, iv: bytes, data: bytes) -> bytes:
    """Plain AES-128-CBC of whole blocks (no padding)."""
    if len(iv) != 16 or len(data) % 16:
        raise ValueError("iv must be 16 bytes and data whole 16-byte blocks")
    ek, prev, out = key_schedule_plain(key), bytes(iv), []
    for i in range(0, len(data), 16):
        prev = encrypt_block_plain(ek, bytes(a ^ b for a, b in zip(data[i:i + 16], prev)))
        out.append(prev)
    return b"".join(out)


def cbc_decrypt_plain(key: bytes, iv: bytes, data: bytes) -> bytes:
    """P_i = Dec(C_i) ^ C_{i-1}, C_{-1} = iv."""
    if len(iv) != 16 or len(data) % 16:
        raise ValueError("iv must be 16 bytes and data whole 16-byte blocks")
    ek, prev, out = key_schedule_plain(key), bytes(iv), []
    for i in range(0, len(data), 16):
        c = bytes(data[i:i + 16])
        out.append(bytes(a ^ b for a, b in zip(decrypt_block_plain(ek, c), prev)))
        prev = c
    return b"".join(out)


# ---------------------------------------------------------------- fhe_encryption.rs ----
def encrypt_byte(client_key: ClientKey, byte: int) -> List[BitCt]:
    return [client_key.encrypt(Cleartext(b)) for b in u8_to_bits(byte)]


def encrypt_byte_array(client_key: ClientKey, array: bytes) -> List[List[BitCt]]:
    return [encrypt_byte(client_key, b) for b in array]


def encrypt_word_array(client_key: ClientKey, words: Sequence[bytes]) -> List[List[List[BitCt]]]:
    return [encrypt_byte_array(client_key, w) for w in words]


def decrypt_byte(client_key: ClientKey, byte: Sequence[BitCt]) -> int:
    return bits_to_u8([client_key.decrypt(b).value for b in byte])


def decrypt_byte_array(client_key: ClientKey, array) -> bytes:
    return bytes(decrypt_byte(client_key, b) for b in array)


def encrypt_byte_array_packed(client_key: ClientKey, array: bytes, start_index=None) -> PackedBits:
    """encrypt_byte_array as one packed upload: 8 bits per byte, MSB first, 64 bytes per GLWE.  FheContext.unpack
    turns it into the [len][8] bits that encrypt_byte_array returns."""
    bits = [b for byte in bytes(array) for b in u8_to_bits(byte)]
    return client_key.encrypt_packed(bits, start_index, group=8)


def decrypt_byte_array_packed(client_key: ClientKey, packed: PackedBits) -> bytes:
    """The bytes of a packed upload or of FheContext.pack of [len][8] bits (MSB first)."""
    if packed.count % 8:
        raise ValueError("a packed byte array holds a multiple of 8 bits")
    bits = client_key.decrypt_packed(packed)
    return bytes(bits_to_u8(bits[i:i + 8]) for i in range(0, packed.count, 8))


# ---------------------------------------------------------------- Aes128Encrypt ----
class ShortintWoppbs1BitSboxGalMulPbsAesEncrypt:
    """fhe_impls/shortint_woppbs_1bit.rs:131-151 -- SBOX + GF x{1,2,3} by one 8->24 WoP-PBS
    (fhe_sbox_gal_mul_pbs.rs:84-191).  Every entry point runs batched on the device."""

    _C = "tae_aes_"  # C-ABI entry points of this driver: <prefix>encrypt_blocks[_raw], <prefix>key_schedule[_raw]

    @classmethod
    def _fn(cls, name: str):
        return getattr(lib(), cls._C + name)

    @classmethod
    def encrypt_block(cls, ctx: FheContext, expanded_key, block):
        return cls.encrypt_block_for_rounds(ctx, expanded_key, block, ROUNDS)

    @classmethod
    def encrypt_block_for_rounds(cls, ctx: FheContext, expanded_key, block, rounds: int):
        """expanded_key: [44][4][8] BitCt (nested or flat); block: [16][8] BitCt -> [16][8]."""
        return cls.encrypt_blocks(ctx, expanded_key, [block], rounds)[0]

    @classmethod
    def encrypt_blocks(cls, ctx: FheContext, expanded_key, blocks, rounds: int = ROUNDS):
        """Batched extension: all blocks' SBOXes of a round go to the GPU as one batch."""
        ek = _flat_bits(expanded_key)
        flat = _flat_bits(blocks)
        nb = len(flat) // 128
        outs = (C.c_void_p * (128 * nb))()
        check(cls._fn("encrypt_blocks")(ctx._h, _handles(ek), _handles(flat), nb, rounds, outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[b * 128 + 8 * i:b * 128 + 8 * i + 8] for i in range(16)] for b in range(nb)]

    @classmethod
    def key_schedule(cls, ctx: FheContext, key):
        """key_schedule (fhe_sbox_gal_mul_pbs.rs:134-164 / fhe_sbox_pbs.rs:123-171): [16][8] BitCt -> [44][4][8]."""
        kb = _flat_bits(key)
        outs = (C.c_void_p * (44 * 32))()
        check(cls._fn("key_schedule")(ctx._h, _handles(kb), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[w * 32 + 8 * b:w * 32 + 8 * b + 8] for b in range(4)] for w in range(44)]

    @classmethod
    def encrypt_blocks_raw(cls, ctx: FheContext, rk: np.ndarray, blocks: np.ndarray, rounds: int = ROUNDS) -> np.ndarray:
        """Host arrays: rk [1408][L], blocks [n][128][L] -> [n][128][L] (L = ctx.lwe_size)."""
        rk = np.ascontiguousarray(rk, dtype=np.uint64)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
        nb = blocks.shape[0]
        out = np.zeros_like(blocks)
        check(cls._fn("encrypt_blocks_raw")(ctx._h, rk.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p),
                                            nb, rounds, out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
        return out

    @classmethod
    def encrypt_blocks_device(cls, ctx: FheContext, d_rk: int, d_blocks: int, nb: int, rounds: int, d_out: int):
        """Device pointers (ints), inputs resident in HBM."""
        check(cls._fn("encrypt_blocks_raw")(ctx._h, C.c_void_p(d_rk), C.c_void_p(d_blocks), nb, rounds,
                                            C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @classmethod
    def key_schedule_raw(cls, ctx: FheContext, key: np.ndarray) -> np.ndarray:
        """Host arrays: fresh key bits [128][L] -> expanded [1408][L] (L = ctx.lwe_size)."""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        out = np.zeros((44 * 32, ctx.lwe_size), dtype=np.uint64)
        check(cls._fn("key_schedule_raw")(ctx._h, key.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                          N.TAE_MEM_HOST))
        return out

    # ---- AES-128-CTR with public counters: transciphering (main.rs:108-128) ----
    # Counter block i is iv || be64(first_counter + i); the iv and the counters are public, so no counter
    # ciphertexts are made or uploaded, and round 1 is bootstrapped once per distinct (position, byte) pair.
    # The entry points are the same for every driver class (tae_aes_ctr_*; the C-ABI dispatches on the model).
    @staticmethod
    def ctr_keystream_raw(ctx: FheContext, rk: np.ndarray, iv: bytes, first_counter: int, n_blocks: int,
                          rounds: int = ROUNDS) -> np.ndarray:
        """Host arrays: rk [1408][L] -> keystream blocks [n_blocks][128][L], equal word for word to
        encrypt_blocks_raw on trivial encryptions of the counter blocks."""
        rk = np.ascontiguousarray(rk, dtype=np.uint64)
        out = np.zeros((n_blocks, 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aes_ctr_keystream_raw(ctx._h, rk.ctypes.data_as(C.c_void_p), _iv8(iv), first_counter,
                                              n_blocks, rounds, out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ctr_keystream_device(ctx: FheContext, d_rk: int, iv: bytes, first_counter: int, n_blocks: int, rounds: int,
                             d_out: int):
        """Device pointers (ints) for rk and the output [n_blocks][128][L]; iv is host bytes."""
        check(lib().tae_aes_ctr_keystream_raw(ctx._h, C.c_void_p(d_rk), _iv8(iv), first_counter, n_blocks, rounds,
                                              C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def ctr_transcipher_raw(ctx: FheContext, rk: np.ndarray, iv: bytes, first_counter: int, data: bytes) -> np.ndarray:
        """data: AES-128-CTR ciphertext bytes -> [len][8][L] FHE encryptions of the plaintext bits (10 rounds)."""
        rk = np.ascontiguousarray(rk, dtype=np.uint64)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.zeros((len(buf), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aes_ctr_transcipher_raw(ctx._h, rk.ctypes.data_as(C.c_void_p), _iv8(iv), first_counter,
                                                buf.ctypes.data_as(C.c_void_p), len(buf),
                                                out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ctr_transcipher(ctx: FheContext, expanded_key, iv: bytes, first_counter: int, data: bytes):
        """expanded_key: [44][4][8] BitCt (nested or flat) -> [len][8] BitCt of the plaintext bits."""
        ek = _flat_bits(expanded_key)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        outs = (C.c_void_p * (8 * len(buf)))()
        check(lib().tae_aes_ctr_transcipher(ctx._h, _handles(ek), _iv8(iv), first_counter,
                                            buf.ctypes.data_as(C.c_void_p), len(buf), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [bits[8 * i:8 * i + 8] for i in range(len(buf))]

    # ---- inverse cipher and CBC transciphering (FIPS-197 5.3; the reference has no decryption) ----
    # InvSubBytes and InvMixColumns' multiples {14, 11, 13, 9} in one 8 -> 32 WoP-PBS per byte and middle round,
    # 8 -> 8 for the last: `rounds` circuit bootstraps per block, as encryption.  This driver on the 1-bit
    # model only: the other driver classes raise TaeError (TAE_E_PARAM), as the C-ABI does for their models.
    _INVERSE = True

    @classmethod
    def _require_inverse(cls):
        if not cls._INVERSE:
            raise N.TaeError(N.TAE_E_PARAM, "the inverse cipher belongs to the gal-mul driver on the 1-bit model")

    @classmethod
    def decrypt_key(cls, ctx: FheContext, expanded_key):
        """[44][4][8] BitCt -> the decryption key [44][4][8]: words 4..39 = InvMixColumns of the round keys,
        derived on the device with fresh noise; words 0..3 and 40..43 are the expanded key's."""
        cls._require_inverse()
        ek = _flat_bits(expanded_key)
        outs = (C.c_void_p * (44 * 32))()
        check(lib().tae_aes_decrypt_key(ctx._h, _handles(ek), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[w * 32 + 8 * b:w * 32 + 8 * b + 8] for b in range(4)] for w in range(44)]

    @classmethod
    def decrypt_block(cls, ctx: FheContext, dk, block):
        return cls.decrypt_block_for_rounds(ctx, dk, block, ROUNDS)

    @classmethod
    def decrypt_block_for_rounds(cls, ctx: FheContext, dk, block, rounds: int):
        """dk: decrypt_key's output; block [16][8] BitCt -> [16][8]; inverts encrypt_block_for_rounds(rounds)."""
        return cls.decrypt_blocks(ctx, dk, [block], rounds)[0]

    @classmethod
    def decrypt_blocks(cls, ctx: FheContext, dk, blocks, rounds: int = ROUNDS):
        cls._require_inverse()
        key = _flat_bits(dk)
        flat = _flat_bits(blocks)
        nb = len(flat) // 128
        outs = (C.c_void_p * (128 * nb))()
        check(lib().tae_aes_decrypt_blocks(ctx._h, _handles(key), _handles(flat), nb, rounds, outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[b * 128 + 8 * i:b * 128 + 8 * i + 8] for i in range(16)] for b in range(nb)]

    @classmethod
    def decrypt_key_raw(cls, ctx: FheContext, rk: np.ndarray) -> np.ndarray:
        """Host arrays: expanded key [1408][L] -> decryption key [1408][L]."""
        cls._require_inverse()
        rk = np.ascontiguousarray(rk, dtype=np.uint64)
        out = np.zeros((44 * 32, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aes_decrypt_key_raw(ctx._h, rk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                            N.TAE_MEM_HOST))
        return out

    @classmethod
    def decrypt_blocks_raw(cls, ctx: FheContext, dk: np.ndarray, blocks: np.ndarray, rounds: int = ROUNDS) -> np.ndarray:
        """Host arrays: dk [1408][L], blocks [n][128][L] -> [n][128][L]."""
        cls._require_inverse()
        dk = np.ascontiguousarray(dk, dtype=np.uint64)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
        out = np.zeros_like(blocks)
        check(lib().tae_aes_decrypt_blocks_raw(ctx._h, dk.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p),
                                               blocks.shape[0], rounds, out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
        return out

    @classmethod
    def decrypt_blocks_device(cls, ctx: FheContext, d_dk: int, d_blocks: int, nb: int, rounds: int, d_out: int):
        """Device pointers (ints), inputs resident in HBM."""
        cls._require_inverse()
        check(lib().tae_aes_decrypt_blocks_raw(ctx._h, C.c_void_p(d_dk), C.c_void_p(d_blocks), nb, rounds,
                                               C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @classmethod
    def cbc_transcipher(cls, ctx: FheContext, dk, iv: bytes, data: bytes):
        """dk: decrypt_key's output; data: AES-128-CBC ciphertext bytes (whole blocks) -> [len][8] BitCt of
        the plaintext bits, padding included."""
        cls._require_inverse()
        key = _flat_bits(dk)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        outs = (C.c_void_p * (8 * len(buf)))()
        check(lib().tae_aes_cbc_transcipher(ctx._h, _handles(key), _iv16(iv), buf.ctypes.data_as(C.c_void_p), len(buf),
                                            outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [bits[8 * i:8 * i + 8] for i in range(len(buf))]

    @classmethod
    def cbc_transcipher_raw(cls, ctx: FheContext, dk: np.ndarray, iv: bytes, data: bytes) -> np.ndarray:
        """Host arrays: dk [1408][L] -> [len][8][L] FHE encryptions of the plaintext bits (10 rounds)."""
        cls._require_inverse()
        dk = np.ascontiguousarray(dk, dtype=np.uint64)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.zeros((len(buf), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aes_cbc_transcipher_raw(ctx._h, dk.ctypes.data_as(C.c_void_p), _iv16(iv),
                                                buf.ctypes.data_as(C.c_void_p), len(buf),
                                                out.ctypes.data_as(C.c_void_p), N.TAE_MEM_HOST))
        return out

    @classmethod
    def cbc_transcipher_device(cls, ctx: FheContext, d_dk: int, iv: bytes, data: bytes, d_out: int):
        """Device pointers (ints) for dk and the output [len][8][L]; iv and data are host bytes."""
        cls._require_inverse()
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().tae_aes_cbc_transcipher_raw(ctx._h, C.c_void_p(d_dk), _iv16(iv), buf.ctypes.data_as(C.c_void_p),
                                                len(buf), C.c_void_p(d_out), N.TAE_MEM_DEVICE))


class ShortintWoppbs1BitSboxPbsAesEncrypt(ShortintWoppbs1BitSboxGalMulPbsAesEncrypt):
    """fhe_impls/shortint_woppbs_1bit.rs:47-81: the generic fhe_sbox_pbs driver (fhe_sbox_pbs.rs:22-171) over
    the 1-bit model -- SubBytes = Byte::sbox_substitute (one 8 -> 8 circuit bootstrap per byte, all bytes of
    all blocks in one batched device call), MixColumns = gf_256_mul by BitCt XORs (:33-73), key_schedule with
    Byte::bootstrap_assign = one 1 -> 1 identity circuit bootstrap per bit.

    The reference ships this combination with its tests #[ignore]d ("does not work since cipher text noise
    is not independent in calculations", :160-176): gf_256_mul keeps reducing its multiplicand after the
    last multiplier bit and XORs a bit into a ciphertext that already holds it, so the first MixColumns
    raises NoiseNotIndependent (before any device work; tae_aes_noise_schedule_check restates it), exactly
    where the reference panics.  A 1-round run (no MixColumns) and the key schedule run on the device.
    """

    _C = "tae_aes_sbox_pbs_"
    _INVERSE = False  # decrypt_* / cbc_* raise TAE_E_PARAM here and in the two subclasses


class ShortintWoppbs8BitSboxPbsAesEncrypt(ShortintWoppbs1BitSboxPbsAesEncrypt):
    """fhe_impls/shortint_woppbs_8bit.rs:44-64 -- the fhe_sbox_pbs driver over the 8-bit model.

    Same API; use a context of param set PARAMS_WOPPBS_8BIT (bits are small-key LWEs [n+1]).  SubBytes is
    Byte::bootstrap_with_lut (CBS-VP of the 8 bits into one 8-bit int, then extract_bits), MixColumns is
    leveled (gf_256_mul by bit shifts/XORs, fhe_sbox_pbs.rs:33-73).  The C-ABI dispatches on the model.
    """


class Shortint1BitSboxPbsAesEncrypt(ShortintWoppbs1BitSboxPbsAesEncrypt):
    """fhe_impls/shortint_1bit.rs:52-72 -- the fhe_sbox_pbs driver over the shortint_1bit model.

    Same API; use a context of param set PARAMS_SHORTINT_1BIT (bits are shortint ciphertexts under the small
    key [n+1]).  ByteT::sbox_substitute is 8 multivariate functions of the byte (one selector tree per output
    bit, :32-50), bootstrap_assign one PBS per bit with the identity test vector (:18-30); XOR is unchecked
    addition, so nothing raises.  The reference #[ignore]s its AES tests with these testing parameters ("tests
    fail currently due to too big noise accumulation", :79-102): decryptions of whole rounds may be wrong, as
    there.  The C-ABI dispatches on the model.
    """


def noise_schedule_check(param_set: int, driver: int, rounds: int) -> None:
    """The round function's noise bookkeeping for fresh inputs, without a context or device: raises the
    error the reference panics with (NoiseNotIndependent / NoiseTooBig), else returns None."""
    check(lib().tae_aes_noise_schedule_check(param_set, driver, rounds))


def decrypt_noise_schedule_check(param_set: int, rounds: int) -> None:
    """The inverse cipher's noise bookkeeping for fresh inputs (the decryption-key derivation, then `rounds`
    rounds with the derived key), without a context or device."""
    check(lib().tae_aes_decrypt_noise_schedule_check(param_set, rounds))


def _iv16(iv: bytes) -> bytes:
    iv = bytes(iv)
    if len(iv) != 16:
        raise ValueError("iv must be 16 bytes")
    return iv


def _iv8(iv: bytes) -> bytes:
    iv = bytes(iv)
    if len(iv) != 8:
        raise ValueError("iv must be 8 bytes")
    return iv


def counter_blocks(iv: bytes, count: int, *, first: int = 1) -> List[bytes]:
    """main.rs:108-115: block = iv (8 bytes) || ctr as u64 big-endian, ctr = first..first + count - 1
    (the reference counts from 1)."""
    return [bytes(iv) + c.to_bytes(8, "big") for c in range(first, first + count)]


def ctr_plan(iv: bytes, first_counter: int, n_blocks: int) -> int:
    """Number of round-1 SBOX groups the counter-mode entry points bootstrap for this range: one per
    distinct (byte position, byte value) of the counter blocks (8 for the iv + the distinct values of
    each counter byte).  Host only; a range that wraps past 2^64 - 1 raises TaeError (TAE_E_ARG)."""
    n = C.c_size_t(0)
    check(lib().tae_aes_ctr_plan(_iv8(iv), first_counter, n_blocks, C.byref(n)))
    return n.value


def ctr_xor_plain(key: bytes, iv: bytes, first_counter: int, data: bytes) -> bytes:
    """Plain AES-128-CTR (main.rs:117-128): data xor the keystream of counters first_counter.. ; encrypts
    and decrypts."""
    ek = key_schedule_plain(key)
    nb = (len(data) + 15) // 16
    ks = b"".join(encrypt_block_plain(ek, b) for b in counter_blocks(_iv8(iv), nb, first=first_counter))
    return bytes(d ^ k for d, k in zip(data, ks))


def blocks_to_bits(blocks: Sequence[bytes]) -> np.ndarray:
    return np.array([[b for byte in blk for b in u8_to_bits(byte)] for blk in blocks], dtype=np.uint8)


def bits_to_blocks(bits: np.ndarray) -> List[bytes]:
    bits = np.asarray(bits).reshape(-1, 16, 8)
    return [bytes(bits_to_u8(byte) for byte in blk) for blk in bits]
