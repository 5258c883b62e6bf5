"""AES-128 / 192 / 256 over the 1-bit WoP-PBS model: key expansion on the device, cipher, counter mode, inverse
cipher and CBC for every key size of FIPS-197 (section 5.2 and figure 11; the reference is AES-128 only).

A key of Nk = 4 / 6 / 8 words expands to W = 4 (Nr + 1) = 44 / 52 / 60 words for Nr = Nk + 6 = 10 / 12 / 14
rounds.  Ciphertext layouts, bit order and the `rounds` convention are those of `aes_128`: a run of `rounds`
rounds uses round keys 0, 1..rounds-1 and Nr.  The FHE side runs on the GPU through the C-ABI (tae_aesx_*),
gal-mul driver on the 1-bit parameter sets; the other models raise TaeError (TAE_E_PARAM) for 192 and 256.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from ._native import check, lib
from .aes_128 import (INV_SBOX, RC, SBOX, _flat_bits, _inv_mix_columns, _iv8, _iv16, counter_blocks, gf_256_mul)
from .tfhe import BitCt, FheContext, _handles

KEY_BITS = (128, 192, 256)


def _key_bits_of_words(words: int) -> int:
    if words not in (44, 52, 60):
        raise N.TaeError(N.TAE_E_ARG, f"an expanded key has 44, 52 or 60 words, not {words}")
    return 32 * (words // 4 - 7)


def rounds(key) -> int:
    """Nr of a key: 16 / 24 / 32 bytes, or an expanded key of 44 / 52 / 60 words -> 10 / 12 / 14."""
    n = len(key)
    if isinstance(key, (bytes, bytearray)) and n in (16, 24, 32):
        return n // 4 + 6
    return _key_bits_of_words(n) // 32 + 6


def expanded_words(key_bits: int) -> int:
    n = C.c_size_t(0)
    check(lib().tae_aesx_expanded_words(key_bits, C.byref(n)))
    return n.value


# ---------------------------------------------------------------- plain, FIPS-197 5.1 - 5.3 ----
def key_schedule_plain(key: bytes) -> List[bytes]:
    """FIPS-197 5.2: 16 / 24 / 32 key bytes -> 44 / 52 / 60 words of 4 bytes."""
    if len(key) not in (16, 24, 32):
        raise ValueError("key must be 16, 24 or 32 bytes")
    nk = len(key) // 4
    w = [bytes(key[4 * i:4 * i + 4]) for i in range(nk)]
    for i in range(nk, 4 * (nk + 7)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ RC[i // nk], SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
        elif nk == 8 and i % 8 == 4:
            t = [SBOX[x] for x in t]
        w.append(bytes(a ^ b for a, b in zip(w[i - nk], t)))
    return w


def encrypt_block_plain(expanded_key: Sequence[bytes], block: bytes, rounds: Optional[int] = None) -> bytes:
    """aes_128.encrypt_block_plain for any key size; the last round always uses round key Nr."""
    nr = len(expanded_key) // 4 - 1
    rounds = nr if rounds is None else rounds
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
        k = rk[16 * nr:16 * nr + 16] if last else rk[16 * r:16 * r + 16]
        s = [t[i] ^ k[i] for i in range(16)]
    return bytes(s)


def decrypt_key_plain(expanded_key: Sequence[bytes]) -> List[bytes]:
    """The decryption key of FIPS-197 5.3.5: words 0..3 and 4Nr..4Nr+3 are the expanded key's, words 4r..4r+3
    (r = 1..Nr-1) are InvMixColumns(rk[r])."""
    nr = len(expanded_key) // 4 - 1
    rk = b"".join(expanded_key)
    dk = bytearray(rk)
    for r in range(1, nr):
        dk[16 * r:16 * r + 16] = bytes(_inv_mix_columns(rk[16 * r:16 * r + 16]))
    return [bytes(dk[4 * i:4 * i + 4]) for i in range(len(expanded_key))]


def decrypt_block_plain(expanded_key: Sequence[bytes], block: bytes, rounds: Optional[int] = None) -> bytes:
    """The inverse cipher (FIPS-197 5.3) with the ENCRYPTION key: inverts encrypt_block_plain(., ., rounds)."""
    nr = len(expanded_key) // 4 - 1
    rounds = nr if rounds is None else rounds
    rk = b"".join(expanded_key)
    s = [block[i] ^ rk[16 * nr + i] for i in range(16)]
    for r in range(rounds - 1, -1, -1):
        s = [s[4 * ((c - row) % 4) + row] for c in range(4) for row in range(4)]  # InvShiftRows
        s = [INV_SBOX[x] for x in s]
        s = [s[i] ^ rk[16 * r + i] for i in range(16)]
        if r:
            s = _inv_mix_columns(s)
    return bytes(s)


def ctr_xor_plain(key: bytes, iv: bytes, first_counter: int, data: bytes) -> bytes:
    """Plain AES-CTR with the counter blocks of aes_128.counter_blocks; encrypts and decrypts."""
    ek = key_schedule_plain(key)
    nb = (len(data) + 15) // 16
    ks = b"".join(encrypt_block_plain(ek, b) for b in counter_blocks(_iv8(iv), nb, first=first_counter))
    return bytes(d ^ k for d, k in zip(data, ks))


def cbc_encrypt_plain(key: bytes, iv: bytes, data: bytes) -> bytes:
    """Plain AES-CBC of whole blocks (no padding)."""
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


def _xts_tweak16(tweak) -> bytes:
    """16 tweak bytes, or a data-unit number (little-endian, IEEE 1619)."""
    if isinstance(tweak, int):
        return tweak.to_bytes(16, "little")
    tweak = bytes(tweak)
    if len(tweak) != 16:
        raise ValueError("an XTS tweak is 16 bytes or a data-unit number")
    return tweak


def xts_alpha(t: bytes) -> bytes:
    """IEEE 1619: multiplication by alpha, the byte-wise left shift with carry; 0x87 into byte 0 on carry out."""
    out, carry = bytearray(16), 0
    for i in range(16):
        out[i] = ((t[i] << 1) & 0xff) | carry
        carry = t[i] >> 7
    if carry:
        out[0] ^= 0x87
    return bytes(out)


def _xts_plain(key1: bytes, key2: bytes, tweak16, data: bytes, first_block: int, block_fn) -> bytes:
    if len(key1) != len(key2) or len(key1) not in (16, 24, 32):
        raise ValueError("XTS keys are two keys of one size: 16 or 32 bytes in IEEE 1619, 24 as for the other modes")
    if not data or len(data) % 16:
        raise ValueError("data must be a positive number of whole 16-byte blocks (no ciphertext stealing)")
    ek1, ek2 = key_schedule_plain(key1), key_schedule_plain(key2)
    mask = encrypt_block_plain(ek2, _xts_tweak16(tweak16))
    for _ in range(first_block):
        mask = xts_alpha(mask)
    out = []
    for i in range(0, len(data), 16):
        x = block_fn(ek1, bytes(a ^ b for a, b in zip(data[i:i + 16], mask)))
        out.append(bytes(a ^ b for a, b in zip(x, mask)))
        mask = xts_alpha(mask)
    return b"".join(out)


def xts_encrypt_plain(key1: bytes, key2: bytes, tweak16, data: bytes, first_block: int = 0) -> bytes:
    """Plain XTS-AES of whole blocks: C_j = Enc_K1(P_j ^ M_j) ^ M_j, M_j = alpha^j Enc_K2(tweak).  `data` starts at
    block `first_block` of the data unit; tweak16 is 16 bytes or the unit number."""
    return _xts_plain(key1, key2, tweak16, data, first_block, encrypt_block_plain)


def xts_decrypt_plain(key1: bytes, key2: bytes, tweak16, data: bytes, first_block: int = 0) -> bytes:
    """P_j = Dec_K1(C_j ^ M_j) ^ M_j."""
    return _xts_plain(key1, key2, tweak16, data, first_block, decrypt_block_plain)


def xts_row_weight(block_index: int) -> int:
    """w(j): the largest row weight of the GF(2) matrix of alpha^j, the noise^2 of block j's mask."""
    w = C.c_int(0)
    check(lib().tae_aesx_xts_row_weight(block_index, C.byref(w)))
    return w.value


def xts_noise_schedule_check(param_set: int, key_bits: int, rounds: int, max_block_index: int) -> None:
    """The noise bookkeeping of XTS decryption for fresh keys, without a context or device: both key expansions,
    the decryption key, the refreshed tweak and block `max_block_index` of a unit."""
    check(lib().tae_aesx_xts_noise_schedule_check(param_set, key_bits, rounds, max_block_index))


def _xts_units(units):
    """[(tweak, data) | (tweak, data, first_block)] -> a tae_xts_unit array, the buffers it points into and the
    total length."""
    arr = (N.TaeXtsUnit * max(len(units), 1))()
    keep, total = [], 0
    for i, u in enumerate(units):
        tweak, data = u[0], u[1]
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        keep.append(buf)
        arr[i].tweak[:] = list(_xts_tweak16(tweak))
        arr[i].first_block = u[2] if len(u) > 2 else 0
        arr[i].data = buf.ctypes.data if len(buf) else None
        arr[i].len = len(buf)
        total += len(buf)
    return arr, keep, total


# ---------------------------------------------------------------- plain CCM, RFC 3610 ----
def _ccm_blocks_plain(nonce: bytes, aad: bytes, payload: bytes, tag_len: int):
    """RFC 3610 section 2: (L, the MAC blocks B_0 .., the counter blocks A_0 ..) of a frame."""
    nonce, aad, payload = bytes(nonce), bytes(aad), bytes(payload)
    if not 7 <= len(nonce) <= 13:
        raise ValueError("a CCM nonce is 7..13 bytes")
    if tag_len not in (4, 6, 8, 10, 12, 14, 16):
        raise ValueError("a CCM tag is 4, 6 .. 16 bytes")
    if len(aad) >= 0xFF00:
        raise ValueError("associated data of 0xFF00 bytes or more is not supported")
    ell = 15 - len(nonce)
    if len(payload) >> (8 * ell):
        raise ValueError("the payload length does not fit the nonce's length field")
    flags = (64 if aad else 0) | (8 * ((tag_len - 2) // 2)) | (ell - 1)
    mac = bytes([flags]) + nonce + len(payload).to_bytes(ell, "big")
    if aad:
        enc = len(aad).to_bytes(2, "big") + aad
        mac += enc + bytes(-len(enc) % 16)
    mac += payload + bytes(-len(payload) % 16)
    n_blk = (len(payload) + 15) // 16
    ctr = [bytes([ell - 1]) + nonce + i.to_bytes(ell, "big") for i in range(n_blk + 1)]
    return ell, [mac[i:i + 16] for i in range(0, len(mac), 16)], ctr


def ccm_mac_plain(key: bytes, nonce: bytes, aad: bytes, payload: bytes, tag_len: int,
                  rounds: Optional[int] = None) -> bytes:
    """The CBC-MAC of a frame before it is masked with S_0: the first tag_len bytes of X_last."""
    ek = key_schedule_plain(key)
    _, mac, _ = _ccm_blocks_plain(nonce, aad, payload, tag_len)
    x = bytes(16)
    for b in mac:
        x = encrypt_block_plain(ek, bytes(p ^ q for p, q in zip(x, b)), rounds)
    return x[:tag_len]


def ccm_encrypt_plain(key: bytes, nonce: bytes, aad: bytes, plaintext: bytes, tag_len: int,
                      rounds: Optional[int] = None) -> bytes:
    """Plain AES-CCM: the encrypted payload followed by the encrypted tag U = T ^ S_0."""
    ek = key_schedule_plain(key)
    _, _, ctr = _ccm_blocks_plain(nonce, aad, plaintext, tag_len)
    ks = [encrypt_block_plain(ek, a, rounds) for a in ctr]
    tag = ccm_mac_plain(key, nonce, aad, plaintext, tag_len, rounds)
    body = bytes(p ^ k for p, k in zip(plaintext, b"".join(ks[1:])))
    return body + bytes(t ^ k for t, k in zip(tag, ks[0]))


def ccm_decrypt_plain(key: bytes, nonce: bytes, aad: bytes, data: bytes, tag_len: int,
                      rounds: Optional[int] = None):
    """data = encrypted payload || encrypted tag -> (payload, tag difference): what the server computes under FHE.
    The frame is authentic iff the tag_len difference bytes are zero; the payload is returned either way."""
    data = bytes(data)
    if len(data) < tag_len:
        raise ValueError("data is shorter than the tag")
    body, u = data[:len(data) - tag_len], data[len(data) - tag_len:]
    ek = key_schedule_plain(key)
    _, _, ctr = _ccm_blocks_plain(nonce, aad, body, tag_len)
    ks = [encrypt_block_plain(ek, a, rounds) for a in ctr]
    payload = bytes(c ^ k for c, k in zip(body, b"".join(ks[1:])))
    tag = ccm_mac_plain(key, nonce, aad, payload, tag_len, rounds)
    return payload, bytes(t ^ k ^ r for t, k, r in zip(tag, ks[0], u))


def _bytes_ptr(b: bytes):
    """(array, pointer or None) of host bytes; the array keeps the pointer alive."""
    buf = np.frombuffer(bytes(b), dtype=np.uint8)
    return buf, (C.c_void_p(buf.ctypes.data) if len(buf) else None)


def ccm_format(nonce: bytes, aad: bytes, payload_len: int, tag_len: int):
    """The library's frame layout (tae_aesx_ccm_format): (ctr [n_ctr][16], mac [n_mac][16], src [n_mac][16]) with
    A_0 .. in ctr, the public bytes of B_0 .. in mac (0 where a payload byte goes) and src = -1 for a public byte,
    else the index of the payload byte.  Refusals are TAE_E_PARAM."""
    nb, _ = _bytes_ptr(nonce)
    ab, a_ptr = _bytes_ptr(aad)
    n_ctr, n_mac = C.c_size_t(0), C.c_size_t(0)
    check(lib().tae_aesx_ccm_format(_p(nb), len(nb), tag_len, a_ptr, len(ab), payload_len, C.byref(n_ctr),
                                    C.byref(n_mac), None, None, None))
    ctr = np.zeros((n_ctr.value, 16), dtype=np.uint8)
    mac = np.zeros((n_mac.value, 16), dtype=np.uint8)
    src = np.zeros((n_mac.value, 16), dtype=np.int64)
    check(lib().tae_aesx_ccm_format(_p(nb), len(nb), tag_len, a_ptr, len(ab), payload_len, C.byref(n_ctr),
                                    C.byref(n_mac), _p(ctr), _p(mac), _p(src)))
    return ctr, mac, src


def ccm_noise_schedule_check(param_set: int, key_bits: int, rounds: int) -> None:
    """The noise bookkeeping of CCM decryption for a fresh key, without a context or device."""
    check(lib().tae_aesx_ccm_noise_schedule_check(param_set, key_bits, rounds))


def ccm_tag_ok(client_key, tag_diff) -> bool:
    """The client's check: decrypts the tag-difference bits ([tag_len][8] BitCt, a raw array [tag_len][8][L] or
    FheContext.pack of either) and accepts iff all are zero."""
    from .tfhe import PackedBits
    if isinstance(tag_diff, PackedBits):
        bits = client_key.decrypt_packed(tag_diff)
    elif isinstance(tag_diff, np.ndarray):
        bits = client_key.decrypt_bits_raw(tag_diff.reshape(-1, tag_diff.shape[-1]))
    else:
        bits = [client_key.decrypt(b).value for b in _flat_bits(tag_diff)]
    return not any(int(b) for b in bits)


# ---------------------------------------------------------------- plain GCM, SP 800-38D ----
GCM_TAG_LENGTHS = (4, 8, 12, 13, 14, 15, 16)


def gf128_mul_plain(x: bytes, y: bytes) -> bytes:
    """SP 800-38D algorithm 1 on 16-byte blocks: the coefficient of x^k is bit k from the MSB of byte 0."""
    xi, v, z = int.from_bytes(x, "big"), int.from_bytes(y, "big"), 0
    for i in range(128):
        if (xi >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120 if v & 1 else 0)
    return z.to_bytes(16, "big")


def _gcm_hashed_blocks(aad: bytes, ciphertext: bytes) -> List[bytes]:
    buf = (aad + bytes(-len(aad) % 16) + ciphertext + bytes(-len(ciphertext) % 16)
           + (8 * len(aad)).to_bytes(8, "big") + (8 * len(ciphertext)).to_bytes(8, "big"))
    return [buf[i:i + 16] for i in range(0, len(buf), 16)]


def ghash_plain(h: bytes, aad: bytes, ciphertext: bytes) -> bytes:
    """GHASH_H over the padded AAD, the padded ciphertext and the length block: Y_i = (Y_{i-1} ^ X_i) H."""
    y = bytes(16)
    for x in _gcm_hashed_blocks(bytes(aad), bytes(ciphertext)):
        y = gf128_mul_plain(bytes(a ^ b for a, b in zip(y, x)), h)
    return y


def _gcm_check_plain(iv: bytes, tag_len: int) -> None:
    if len(iv) != 12:
        raise ValueError("only 12-byte GCM IVs are supported")
    if tag_len not in GCM_TAG_LENGTHS:
        raise ValueError("a GCM tag is 4, 8 or 12 .. 16 bytes")


def _gcm_counter_block(iv: bytes, i: int) -> bytes:
    """The cipher input of payload block i: the low 32 bits wrap modulo 2^32 and never carry into the IV."""
    return iv + ((2 + i) & 0xFFFFFFFF).to_bytes(4, "big")


def _gcm_keystream_plain(ek, iv: bytes, n: int, rounds) -> bytes:
    return b"".join(encrypt_block_plain(ek, _gcm_counter_block(iv, i), rounds) for i in range(n))


def gcm_encrypt_plain(key: bytes, iv: bytes, aad: bytes, plaintext: bytes, tag_len: int = 16,
                      rounds: Optional[int] = None) -> bytes:
    """Plain AES-GCM with a 96-bit IV: the ciphertext followed by the tag_len-byte tag."""
    iv, aad, plaintext = bytes(iv), bytes(aad), bytes(plaintext)
    _gcm_check_plain(iv, tag_len)
    ek = key_schedule_plain(key)
    ks = _gcm_keystream_plain(ek, iv, (len(plaintext) + 15) // 16, rounds)
    c = bytes(p ^ k for p, k in zip(plaintext, ks))
    h = encrypt_block_plain(ek, bytes(16), rounds)
    s = encrypt_block_plain(ek, iv + b"\x00\x00\x00\x01", rounds)
    return c + bytes(a ^ b for a, b in zip(ghash_plain(h, aad, c), s))[:tag_len]


def gcm_decrypt_plain(key: bytes, iv: bytes, aad: bytes, data: bytes, tag_len: int = 16,
                      rounds: Optional[int] = None):
    """data = ciphertext || received tag -> (payload, tag difference): what the server computes under FHE.  The frame
    is authentic iff the tag_len difference bytes are zero; the payload is returned either way."""
    iv, aad, data = bytes(iv), bytes(aad), bytes(data)
    _gcm_check_plain(iv, tag_len)
    if len(data) < tag_len:
        raise ValueError("data is shorter than the tag")
    c, t = data[:len(data) - tag_len], data[len(data) - tag_len:]
    ek = key_schedule_plain(key)
    ks = _gcm_keystream_plain(ek, iv, (len(c) + 15) // 16, rounds)
    h = encrypt_block_plain(ek, bytes(16), rounds)
    s = encrypt_block_plain(ek, iv + b"\x00\x00\x00\x01", rounds)
    diff = bytes(a ^ b ^ r for a, b, r in zip(ghash_plain(h, aad, c), s, t))
    return bytes(p ^ k for p, k in zip(c, ks)), diff


def gcm_format(iv: bytes, aad: bytes, data: bytes, tag_len: int):
    """The library's frame layout (tae_aesx_gcm_format) of the ciphertext `data`: (pub [n_pub][16], hashed [m][16])
    with 0^128, J0 and the counter blocks in pub and X_1 .. X_m in hashed.  Refusals are TAE_E_PARAM."""
    (ib, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(iv), _bytes_ptr(aad), _bytes_ptr(data)
    n_pub, m = C.c_size_t(0), C.c_size_t(0)
    args = (_p(ib), len(ib), a_ptr, len(ab), d_ptr, len(db), tag_len, C.byref(n_pub), C.byref(m))
    check(lib().tae_aesx_gcm_format(*args, None, None))
    pub = np.zeros((n_pub.value, 16), dtype=np.uint8)
    hashed = np.zeros((m.value, 16), dtype=np.uint8)
    check(lib().tae_aesx_gcm_format(*args, _p(pub), _p(hashed)))
    return pub, hashed


def gcm_tag_rows(iv: bytes, aad: bytes, data: bytes, tag_len: int, n_powers: int):
    """(sources [8 tag_len], chunks [8 tag_len]) of the frame's tag rows: the table bits a row sums and the refreshed
    chunks it takes, which is the level of its tag-difference bit.  m > n_powers is TAE_E_PARAM, a row of more than 64
    chunks TAE_E_NOISE."""
    (ib, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(iv), _bytes_ptr(aad), _bytes_ptr(data)
    src = np.zeros(max(8 * tag_len, 1), dtype=np.int32)
    chunks = np.zeros(max(8 * tag_len, 1), dtype=np.int32)
    check(lib().tae_aesx_gcm_tag_rows(_p(ib), len(ib), a_ptr, len(ab), d_ptr, len(db), tag_len, n_powers, _p(src),
                                      _p(chunks)))
    return src[:8 * tag_len], chunks[:8 * tag_len]


def gcm_noise_schedule_check(param_set: int, key_bits: int, rounds: int, n_powers: int, aad_len: int = 8,
                             data_len: int = 17) -> None:
    """The noise bookkeeping of the power table and of one dense frame for a fresh key, without a context or device."""
    check(lib().tae_aesx_gcm_noise_schedule_check(param_set, key_bits, rounds, n_powers, aad_len, data_len))


def gcm_long_rows(iv: bytes, aad: bytes, data: bytes, tag_len: int, n_powers: int, seg: int, n_strides: int):
    """(sources [C][128], chunks [C][128]) of the frame's segmented plan (tae_aesx_gcm_long_rows), C = ceil(m / seg):
    segment 0 holds the final rows r < 8 tag_len (table bits and one bit per product), segment c >= 1 the inner rows of
    S_c.  The refusals of gcm_long_transcipher: TAE_E_PARAM for the shape, TAE_E_NOISE for a row of more than 64 chunks."""
    (ib, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(iv), _bytes_ptr(aad), _bytes_ptr(data)
    m = (len(ab) + 15) // 16 + (len(db) + 15) // 16 + 1
    segs = max(-(-m // seg), 1) if seg >= 1 else 1
    src = np.zeros((segs, 128), dtype=np.int32)
    chunks = np.zeros((segs, 128), dtype=np.int32)
    check(lib().tae_aesx_gcm_long_rows(_p(ib), len(ib), a_ptr, len(ab), d_ptr, len(db), tag_len, n_powers, seg,
                                       n_strides, _p(src), _p(chunks)))
    return src, chunks


def gcm_long_noise_schedule_check(param_set: int, key_bits: int, rounds: int, n_powers: int, seg: int, n_strides: int,
                                  aad_len: int = 8, data_len: int = 17) -> None:
    """The noise bookkeeping of the power table, the stride key and one dense frame for a fresh key, without a context
    or device."""
    check(lib().tae_aesx_gcm_long_noise_schedule_check(param_set, key_bits, rounds, n_powers, seg, n_strides, aad_len,
                                                       data_len))


def gcm_tag_ok(client_key, tag_diff) -> bool:
    """The client's check, with the semantics of ccm_tag_ok: accepts iff every tag-difference bit decrypts to zero."""
    return ccm_tag_ok(client_key, tag_diff)


def _gcm_frames(frames, tag_len: int):
    """[(iv12, aad, data || tag), ..] -> (tae_gcm_frame array, the byte arrays it points into, the payload lengths)."""
    arr = (N.TaeGcmFrame * max(len(frames), 1))()
    keep, lens = [], []
    for i, (iv, aad, data) in enumerate(frames):
        (ib, i_ptr), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(iv), _bytes_ptr(aad), _bytes_ptr(data)
        keep += [ib, ab, db]
        arr[i].iv, arr[i].iv_len = (i_ptr.value if i_ptr else None), len(ib)
        arr[i].aad, arr[i].aad_len = (a_ptr.value if a_ptr else None), len(ab)
        arr[i].data, arr[i].len = (d_ptr.value if d_ptr else None), len(db)
        lens.append(max(len(db) - tag_len, 0))
    return arr, keep, lens


def noise_schedule_check(param_set: int, key_bits: int, rounds: int, inverse: bool = False) -> None:
    """The noise bookkeeping for a fresh key and block, without a context or device: the key expansion, then
    `rounds` cipher rounds, or with `inverse` the decryption-key derivation and `rounds` inverse rounds."""
    check(lib().tae_aesx_noise_schedule_check(param_set, key_bits, rounds, int(bool(inverse))))


# ---------------------------------------------------------------- FHE ----
def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _raw_key(key: np.ndarray, key_bits: Optional[int]):
    """An expanded or decryption key [W*32][L] as a contiguous array and its key size.  key_bits, when given,
    must be the size the array has (TAE_E_ARG otherwise)."""
    key = np.ascontiguousarray(key, dtype=np.uint64)
    if key.ndim != 2 or key.shape[0] % 32:
        raise N.TaeError(N.TAE_E_ARG, "a key is an array [words * 32][L]")
    kb = _key_bits_of_words(key.shape[0] // 32)
    if key_bits is not None and key_bits != kb:
        raise N.TaeError(N.TAE_E_ARG, f"the key has {key.shape[0] // 32} words, AES-{key_bits} needs "
                                      f"{expanded_words(key_bits)}")
    return key, kb


def _raw_table(table: np.ndarray, what: str) -> np.ndarray:
    """A table of field elements [n][128][L] as a contiguous array (TAE_E_ARG for another shape)."""
    table = np.ascontiguousarray(table, dtype=np.uint64)
    if table.ndim != 3 or table.shape[1] != 128:
        raise N.TaeError(N.TAE_E_ARG, what)
    return table


def _bit_key(key, key_bits: Optional[int]):
    flat = _flat_bits(key)
    if len(flat) % 32:
        raise N.TaeError(N.TAE_E_ARG, "a key is whole 32-bit words")
    kb = _key_bits_of_words(len(flat) // 32)
    if key_bits is not None and key_bits != kb:
        raise N.TaeError(N.TAE_E_ARG, f"the key has {len(flat) // 32} words, AES-{key_bits} needs "
                                      f"{expanded_words(key_bits)}")
    return flat, kb


def _nr(kb: int, rounds: Optional[int]) -> int:
    return kb // 32 + 6 if rounds is None else rounds


def _words(bits: List[BitCt]):
    return [[bits[w * 32 + 8 * b:w * 32 + 8 * b + 8] for b in range(4)] for w in range(len(bits) // 32)]


# ---- AEAD open: a tag verdict bit and the verdict-gated payload ----
# The CCM and GCM calls return payload bits and tag-difference bits and leave the verdict to the client.  The open joins
# them on the server: per frame one bit ok = 1 iff every difference bit is 0, and a payload that is the plaintext where
# ok = 1 and all zeros where it is not, so nothing downstream computes on a forged frame's bytes.  One tag_len per call.
AEAD_TAG_LENGTHS = (4, 6, 8, 10, 12, 13, 14, 15, 16)


def aead_open_plan(tag_len: int, payload_lens):
    """(groups per frame of every verdict level, gate groups) of a call (tae_aead_open_plan), without a device:
    tag_len 16 -> ((16, 2, 1), sum payload_lens)."""
    lens = np.ascontiguousarray(payload_lens, dtype=np.uintp).reshape(-1)
    levels, gate = C.c_int(0), C.c_size_t(0)
    groups = np.zeros(3, dtype=np.uintp)
    check(lib().tae_aead_open_plan(tag_len, _p(lens) if len(lens) else None, len(lens), C.byref(levels), _p(groups),
                                   C.byref(gate)))
    return tuple(int(g) for g in groups[:levels.value]), gate.value


def aead_open_noise_schedule_check(param_set: int, tag_len: int, plain_level: int = 9, diff_level: int = 16) -> None:
    """The noise bookkeeping of the open for payload bits at plain_level and difference bits at diff_level, without a
    context or device."""
    check(lib().tae_aead_open_noise_schedule_check(param_set, tag_len, plain_level, diff_level))


def _open_raw_args(ctx: FheContext, plain, tag_diff, tag_len: int):
    """Per-frame raw arrays -> (payload [sum len][8][L], lens, differences [n][8 tag_len][L])."""
    L = ctx.lwe_size
    frames = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8, L) for p in plain]
    diff = [np.ascontiguousarray(d, dtype=np.uint64).reshape(-1, L) for d in tag_diff]
    if len(frames) != len(diff) or any(d.shape[0] != 8 * tag_len for d in diff):
        raise N.TaeError(N.TAE_E_ARG, "one payload and 8 * tag_len difference bits per frame")
    lens = np.array([f.shape[0] for f in frames], dtype=np.uintp)
    flat = np.concatenate(frames) if frames else np.zeros((0, 8, L), dtype=np.uint64)
    return np.ascontiguousarray(flat), lens, np.ascontiguousarray(np.stack(diff)) if diff else np.zeros((0, 0, L), np.uint64)


def aead_verdict_raw(ctx: FheContext, tag_diff, tag_len: int) -> np.ndarray:
    """Host arrays: per frame [tag_len][8][L] (or one array [n][tag_len][8][L]) -> ok [n][L]."""
    n = len(tag_diff)
    diff = np.ascontiguousarray(tag_diff, dtype=np.uint64)
    if n and diff.size != n * 8 * tag_len * ctx.lwe_size:
        raise N.TaeError(N.TAE_E_ARG, "8 * tag_len difference bits per frame")
    ok = np.zeros((n, ctx.lwe_size), dtype=np.uint64)
    check(lib().tae_aead_verdict_raw(ctx._h, _p(diff), n, tag_len, _p(ok), N.TAE_MEM_HOST))
    return ok


def aead_open_raw(ctx: FheContext, plain, tag_diff, tag_len: int):
    """Host arrays: per frame the payload [len][8][L] and the differences [tag_len][8][L], as the transcipher calls
    return them -> (per frame the gated payload [len][8][L], ok [n][L])."""
    flat, lens, diff = _open_raw_args(ctx, plain, tag_diff, tag_len)
    out, ok = np.zeros_like(flat), np.zeros((len(lens), ctx.lwe_size), dtype=np.uint64)
    check(lib().tae_aead_open_raw(ctx._h, _p(flat), _p(lens), _p(diff), len(lens), tag_len, _p(out), _p(ok),
                                  N.TAE_MEM_HOST))
    res, at = [], 0
    for n in lens:
        res.append(out[at:at + int(n)])
        at += int(n)
    return res, ok


def aead_open_device(ctx: FheContext, d_plain: int, payload_lens, d_tag_diff: int, tag_len: int, d_out: int, d_ok: int):
    """Device pointers (ints) for the payload [sum len][8][L], the differences [n][tag_len][8][L], the gated payload
    and ok [n][L]: what a `*_transcipher_device` call wrote is opened without leaving the card.  payload_lens is host
    data; d_out is not d_plain."""
    lens = np.ascontiguousarray(payload_lens, dtype=np.uintp).reshape(-1)
    check(lib().tae_aead_open_raw(ctx._h, C.c_void_p(d_plain), _p(lens), C.c_void_p(d_tag_diff), len(lens), tag_len,
                                  C.c_void_p(d_out), C.c_void_p(d_ok), N.TAE_MEM_DEVICE))


def aead_open(ctx: FheContext, plain, tag_diff, payload_lens, tag_len: int):
    """BitCt: per frame the payload [len][8] and the differences [tag_len][8] (nested or flat) -> (per frame the gated
    payload [len][8] at level 9, per frame ok at level 8).  An input above the cap is NoiseTooBig."""
    lens = np.ascontiguousarray(payload_lens, dtype=np.uintp).reshape(-1)
    bits, diff = _flat_bits(plain), _flat_bits(tag_diff)
    n, total = len(lens), int(lens.sum()) if len(lens) else 0
    if len(bits) != 8 * total or len(diff) != 8 * tag_len * n:
        raise N.TaeError(N.TAE_E_ARG, "8 bits per payload byte and 8 * tag_len difference bits per frame")
    outs, oks = (C.c_void_p * max(8 * total, 1))(), (C.c_void_p * max(n, 1))()
    check(lib().tae_aead_open(ctx._h, _handles(bits) if bits else None, _p(lens) if n else None,
                              _handles(diff) if diff else None, n, tag_len, outs, oks))
    res, at = [], 0
    for f in range(n):
        ln = int(lens[f])
        res.append([[BitCt(outs[8 * (at + i) + j], ctx) for j in range(8)] for i in range(ln)])
        at += ln
    return res, [BitCt(oks[f], ctx) for f in range(n)]


def open_ok(client_key, ok) -> bool:
    """The client's reading of one verdict: a BitCt or a raw ciphertext [L] -> True iff it decrypts to 1."""
    if isinstance(ok, np.ndarray):
        return bool(int(client_key.decrypt_bits_raw(ok.reshape(1, -1))[0]))
    return bool(int(client_key.decrypt(ok).value))


def _open_frames(ctx: FheContext, res, tag_len: int):
    """What a BitCt transcipher call returns, [(bits, tag_diff), ..] -> aead_open of it."""
    return aead_open(ctx, [p for p, _ in res], [d for _, d in res], [len(p) for p, _ in res], tag_len)


class GalMulAes:
    """The method set of aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt for 128-, 192- and 256-bit keys.
    The key size is read from what is passed: `key_schedule*` from the key (16 / 24 / 32 encrypted bytes), every
    other method from the expanded or decryption key (44 / 52 / 60 words); an explicit `key_bits` that does not
    match is TAE_E_ARG.  The `_device` variants take pointers and therefore `key_bits`.  `rounds` defaults to Nr.
    """

    # ---- key expansion (FIPS-197 5.2) on the device ----
    @staticmethod
    def key_schedule(ctx: FheContext, key):
        """[16 | 24 | 32][8] BitCt (nested or flat) -> [44 | 52 | 60][4][8]."""
        kb = _flat_bits(key)
        if len(kb) not in KEY_BITS:
            raise N.TaeError(N.TAE_E_ARG, "key must be 16, 24 or 32 encrypted bytes")
        outs = (C.c_void_p * (expanded_words(len(kb)) * 32))()
        check(lib().tae_aesx_key_schedule(ctx._h, len(kb), _handles(kb), outs))
        return _words([BitCt(h, ctx) for h in outs])

    @staticmethod
    def key_schedule_raw(ctx: FheContext, key: np.ndarray) -> np.ndarray:
        """Host arrays: fresh key bits [128 | 192 | 256][L] -> expanded [W*32][L]."""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        if key.ndim != 2 or key.shape[0] not in KEY_BITS:
            raise N.TaeError(N.TAE_E_ARG, "key must be [128 | 192 | 256][L] bits")
        out = np.zeros((expanded_words(key.shape[0]) * 32, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_key_schedule_raw(ctx._h, key.shape[0], _p(key), _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def key_schedule_device(ctx: FheContext, key_bits: int, d_key: int, d_rk: int):
        """Device pointers (ints): key [key_bits][L] -> rk [W*32][L]; no ciphertext leaves the device."""
        check(lib().tae_aesx_key_schedule_raw(ctx._h, key_bits, C.c_void_p(d_key), C.c_void_p(d_rk), N.TAE_MEM_DEVICE))

    # ---- cipher ----
    @classmethod
    def encrypt_block(cls, ctx: FheContext, expanded_key, block):
        return cls.encrypt_blocks(ctx, expanded_key, [block])[0]

    @classmethod
    def encrypt_block_for_rounds(cls, ctx: FheContext, expanded_key, block, rounds: int):
        return cls.encrypt_blocks(ctx, expanded_key, [block], rounds)[0]

    @staticmethod
    def encrypt_blocks(ctx: FheContext, expanded_key, blocks, rounds: Optional[int] = None,
                       key_bits: Optional[int] = None):
        ek, kb = _bit_key(expanded_key, key_bits)
        flat = _flat_bits(blocks)
        nb = len(flat) // 128
        outs = (C.c_void_p * (128 * nb))()
        check(lib().tae_aesx_encrypt_blocks(ctx._h, kb, _handles(ek), _handles(flat), nb, _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[b * 128 + 8 * i:b * 128 + 8 * i + 8] for i in range(16)] for b in range(nb)]

    @staticmethod
    def encrypt_blocks_raw(ctx: FheContext, rk: np.ndarray, blocks: np.ndarray, rounds: Optional[int] = None,
                           key_bits: Optional[int] = None) -> np.ndarray:
        """Host arrays: rk [W*32][L], blocks [n][128][L] -> [n][128][L]."""
        rk, kb = _raw_key(rk, key_bits)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
        out = np.zeros_like(blocks)
        check(lib().tae_aesx_encrypt_blocks_raw(ctx._h, kb, _p(rk), _p(blocks), blocks.shape[0], _nr(kb, rounds),
                                                _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def encrypt_blocks_device(ctx: FheContext, key_bits: int, d_rk: int, d_blocks: int, nb: int, rounds: int,
                              d_out: int):
        """Device pointers (ints), inputs resident in HBM."""
        check(lib().tae_aesx_encrypt_blocks_raw(ctx._h, key_bits, C.c_void_p(d_rk), C.c_void_p(d_blocks), nb, rounds,
                                                C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    # ---- counter mode with public counters ----
    @staticmethod
    def ctr_keystream_raw(ctx: FheContext, rk: np.ndarray, iv: bytes, first_counter: int, n_blocks: int,
                          rounds: Optional[int] = None, key_bits: Optional[int] = None) -> np.ndarray:
        """rk [W*32][L] -> keystream blocks [n_blocks][128][L], equal word for word to encrypt_blocks_raw on
        trivial encryptions of the counter blocks."""
        rk, kb = _raw_key(rk, key_bits)
        out = np.zeros((n_blocks, 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_ctr_keystream_raw(ctx._h, kb, _p(rk), _iv8(iv), first_counter, n_blocks,
                                               _nr(kb, rounds), _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ctr_keystream_device(ctx: FheContext, key_bits: int, d_rk: int, iv: bytes, first_counter: int, n_blocks: int,
                             rounds: int, d_out: int):
        check(lib().tae_aesx_ctr_keystream_raw(ctx._h, key_bits, C.c_void_p(d_rk), _iv8(iv), first_counter, n_blocks,
                                               rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def ctr_transcipher_raw(ctx: FheContext, rk: np.ndarray, iv: bytes, first_counter: int, data: bytes,
                            rounds: Optional[int] = None, key_bits: Optional[int] = None) -> np.ndarray:
        """data: AES-CTR ciphertext bytes -> [len][8][L] FHE encryptions of the plaintext bits."""
        rk, kb = _raw_key(rk, key_bits)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.zeros((len(buf), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_ctr_transcipher_raw(ctx._h, kb, _p(rk), _iv8(iv), first_counter, _p(buf), len(buf),
                                                 _nr(kb, rounds), _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ctr_transcipher_device(ctx: FheContext, key_bits: int, d_rk: int, iv: bytes, first_counter: int, data: bytes,
                               rounds: int, d_out: int):
        """Device pointers (ints) for rk and the output [len][8][L]; iv and data are host bytes."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().tae_aesx_ctr_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_rk), _iv8(iv), first_counter, _p(buf),
                                                 len(buf), rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def ctr_transcipher(ctx: FheContext, expanded_key, iv: bytes, first_counter: int, data: bytes,
                        rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """expanded_key: [W][4][8] BitCt (nested or flat) -> [len][8] BitCt of the plaintext bits."""
        ek, kb = _bit_key(expanded_key, key_bits)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        outs = (C.c_void_p * (8 * len(buf)))()
        check(lib().tae_aesx_ctr_transcipher(ctx._h, kb, _handles(ek), _iv8(iv), first_counter, _p(buf), len(buf),
                                             _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [bits[8 * i:8 * i + 8] for i in range(len(buf))]

    # ---- inverse cipher and CBC (FIPS-197 5.3) ----
    @staticmethod
    def decrypt_key(ctx: FheContext, expanded_key, key_bits: Optional[int] = None):
        """[W][4][8] BitCt -> the decryption key [W][4][8]: words 4 .. 4Nr-1 = InvMixColumns of the round keys,
        derived on the device with fresh noise; words 0..3 and 4Nr..4Nr+3 are the expanded key's."""
        ek, kb = _bit_key(expanded_key, key_bits)
        outs = (C.c_void_p * len(ek))()
        check(lib().tae_aesx_decrypt_key(ctx._h, kb, _handles(ek), outs))
        return _words([BitCt(h, ctx) for h in outs])

    @staticmethod
    def decrypt_key_raw(ctx: FheContext, rk: np.ndarray, key_bits: Optional[int] = None) -> np.ndarray:
        rk, kb = _raw_key(rk, key_bits)
        out = np.zeros_like(rk)
        check(lib().tae_aesx_decrypt_key_raw(ctx._h, kb, _p(rk), _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def decrypt_key_device(ctx: FheContext, key_bits: int, d_rk: int, d_dk: int):
        check(lib().tae_aesx_decrypt_key_raw(ctx._h, key_bits, C.c_void_p(d_rk), C.c_void_p(d_dk), N.TAE_MEM_DEVICE))

    @classmethod
    def decrypt_block(cls, ctx: FheContext, dk, block):
        return cls.decrypt_blocks(ctx, dk, [block])[0]

    @classmethod
    def decrypt_block_for_rounds(cls, ctx: FheContext, dk, block, rounds: int):
        return cls.decrypt_blocks(ctx, dk, [block], rounds)[0]

    @staticmethod
    def decrypt_blocks(ctx: FheContext, dk, blocks, rounds: Optional[int] = None, key_bits: Optional[int] = None):
        key, kb = _bit_key(dk, key_bits)
        flat = _flat_bits(blocks)
        nb = len(flat) // 128
        outs = (C.c_void_p * (128 * nb))()
        check(lib().tae_aesx_decrypt_blocks(ctx._h, kb, _handles(key), _handles(flat), nb, _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [[bits[b * 128 + 8 * i:b * 128 + 8 * i + 8] for i in range(16)] for b in range(nb)]

    @staticmethod
    def decrypt_blocks_raw(ctx: FheContext, dk: np.ndarray, blocks: np.ndarray, rounds: Optional[int] = None,
                           key_bits: Optional[int] = None) -> np.ndarray:
        """Host arrays: dk [W*32][L], blocks [n][128][L] -> [n][128][L]."""
        dk, kb = _raw_key(dk, key_bits)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
        out = np.zeros_like(blocks)
        check(lib().tae_aesx_decrypt_blocks_raw(ctx._h, kb, _p(dk), _p(blocks), blocks.shape[0], _nr(kb, rounds),
                                                _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def decrypt_blocks_device(ctx: FheContext, key_bits: int, d_dk: int, d_blocks: int, nb: int, rounds: int,
                              d_out: int):
        check(lib().tae_aesx_decrypt_blocks_raw(ctx._h, key_bits, C.c_void_p(d_dk), C.c_void_p(d_blocks), nb, rounds,
                                                C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def cbc_transcipher(ctx: FheContext, dk, iv: bytes, data: bytes, rounds: Optional[int] = None,
                        key_bits: Optional[int] = None):
        """dk: decrypt_key's output; data: AES-CBC ciphertext bytes (whole blocks) -> [len][8] BitCt of the
        plaintext bits, padding included."""
        key, kb = _bit_key(dk, key_bits)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        outs = (C.c_void_p * (8 * len(buf)))()
        check(lib().tae_aesx_cbc_transcipher(ctx._h, kb, _handles(key), _iv16(iv), _p(buf), len(buf), _nr(kb, rounds),
                                             outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [bits[8 * i:8 * i + 8] for i in range(len(buf))]

    @staticmethod
    def cbc_transcipher_raw(ctx: FheContext, dk: np.ndarray, iv: bytes, data: bytes, rounds: Optional[int] = None,
                            key_bits: Optional[int] = None) -> np.ndarray:
        """Host arrays: dk [W*32][L] -> [len][8][L] FHE encryptions of the plaintext bits."""
        dk, kb = _raw_key(dk, key_bits)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.zeros((len(buf), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_cbc_transcipher_raw(ctx._h, kb, _p(dk), _iv16(iv), _p(buf), len(buf), _nr(kb, rounds),
                                                 _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def cbc_transcipher_device(ctx: FheContext, key_bits: int, d_dk: int, iv: bytes, data: bytes, rounds: int,
                               d_out: int):
        """Device pointers (ints) for dk and the output [len][8][L]; iv and data are host bytes."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().tae_aesx_cbc_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_dk), _iv16(iv), _p(buf), len(buf),
                                                 rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    # ---- XTS-AES decryption of a public ciphertext (IEEE 1619) ----
    # dk1 = decrypt_key of key 1, rk2 / ek2 = the expanded key 2, one key size for both.  A unit is (tweak, data)
    # or (tweak, data, first_block): tweak = 16 bytes or the data-unit number, data = the unit's ciphertext from
    # block first_block on, whole 16-byte blocks.
    @staticmethod
    def xts_tweaks_raw(ctx: FheContext, rk2: np.ndarray, tweaks, rounds: Optional[int] = None,
                       key_bits: Optional[int] = None) -> np.ndarray:
        """rk2 [W*32][L], n tweaks -> T = Enc_K2(tweak) after the identity bootstrap, [n][128][L]."""
        rk2, kb = _raw_key(rk2, key_bits)
        buf = np.frombuffer(b"".join(_xts_tweak16(t) for t in tweaks), dtype=np.uint8)
        out = np.zeros((len(tweaks), 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_xts_tweaks_raw(ctx._h, kb, _p(rk2), _p(buf), len(tweaks), _nr(kb, rounds), _p(out),
                                            N.TAE_MEM_HOST))
        return out

    @staticmethod
    def xts_masks_raw(ctx: FheContext, tweaks_ct: np.ndarray, unit_of_block, block_index) -> np.ndarray:
        """The mask stage alone: tweaks_ct [n_units][128][L] -> masks [nb][128][L], block b = alpha^block_index[b]
        of unit unit_of_block[b]."""
        tweaks_ct = np.ascontiguousarray(tweaks_ct, dtype=np.uint64)
        unit = np.ascontiguousarray(unit_of_block, dtype=np.int32)
        index = np.ascontiguousarray(block_index, dtype=np.uint64)
        out = np.zeros((len(index), 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_stage_xts_masks(ctx._h, _p(tweaks_ct), tweaks_ct.shape[0], _p(unit), _p(index), len(index),
                                        _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def xts_masks_device(ctx: FheContext, d_tweaks_ct: int, n_units: int, unit_of_block, block_index, d_masks: int):
        unit = np.ascontiguousarray(unit_of_block, dtype=np.int32)
        index = np.ascontiguousarray(block_index, dtype=np.uint64)
        check(lib().tae_stage_xts_masks(ctx._h, C.c_void_p(d_tweaks_ct), n_units, _p(unit), _p(index), len(index),
                                        C.c_void_p(d_masks), N.TAE_MEM_DEVICE))

    @staticmethod
    def xts_transcipher(ctx: FheContext, dk1, ek2, units, rounds: Optional[int] = None,
                        key_bits: Optional[int] = None):
        """dk1, ek2: [W][4][8] BitCt (nested or flat) -> [sum len][8] BitCt of the plaintext bits, units in order."""
        key1, kb = _bit_key(dk1, key_bits)
        key2, _ = _bit_key(ek2, kb)
        arr, keep, total = _xts_units(units)
        outs = (C.c_void_p * (8 * total))()
        check(lib().tae_aesx_xts_transcipher(ctx._h, kb, _handles(key1), _handles(key2), arr, len(units),
                                             _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [bits[8 * i:8 * i + 8] for i in range(total)]

    @staticmethod
    def xts_transcipher_raw(ctx: FheContext, dk1: np.ndarray, rk2: np.ndarray, units, rounds: Optional[int] = None,
                            key_bits: Optional[int] = None) -> np.ndarray:
        """Host arrays: dk1, rk2 [W*32][L] -> [sum len][8][L] FHE encryptions of the plaintext bits."""
        dk1, kb = _raw_key(dk1, key_bits)
        rk2, _ = _raw_key(rk2, kb)
        arr, keep, total = _xts_units(units)
        out = np.zeros((total, 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_xts_transcipher_raw(ctx._h, kb, _p(dk1), _p(rk2), arr, len(units), _nr(kb, rounds),
                                                 _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def xts_transcipher_device(ctx: FheContext, key_bits: int, d_dk1: int, d_rk2: int, units, rounds: int, d_out: int):
        """Device pointers (ints) for the keys and the output [sum len][8][L]; the units are host bytes."""
        arr, keep, _ = _xts_units(units)
        check(lib().tae_aesx_xts_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_dk1), C.c_void_p(d_rk2), arr, len(units),
                                                 rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    # ---- AES-CCM decryption of a public frame (RFC 3610) ----
    # data = the encrypted payload followed by the tag_len-byte encrypted tag.  The results are the payload bits
    # [len - tag_len][8] and the tag-difference bits [tag_len][8]: the client decrypts both and accepts the payload
    # iff ccm_tag_ok.  `rounds` applies to every cipher call and must be at least 2.
    @staticmethod
    def public_keystream_raw(ctx: FheContext, rk: np.ndarray, blocks16, rounds: Optional[int] = None,
                             key_bits: Optional[int] = None) -> np.ndarray:
        """rk [W*32][L], n public 16-byte blocks -> E(block) [n][128][L], equal word for word to encrypt_blocks_raw
        on trivial encryptions of the blocks; round 1 runs once per distinct (position, byte value)."""
        rk, kb = _raw_key(rk, key_bits)
        buf = np.ascontiguousarray(np.frombuffer(b"".join(bytes(b) for b in blocks16), dtype=np.uint8))
        if len(buf) % 16:
            raise N.TaeError(N.TAE_E_ARG, "public blocks are 16 bytes each")
        n = len(buf) // 16
        ko = np.zeros(max(n, 1), dtype=np.int32)
        out = np.zeros((n, 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_pub_keystream_raw(ctx._h, kb, _p(rk), 1, _p(ko), _p(buf), n, _nr(kb, rounds), _p(out),
                                               N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ccm_transcipher(ctx: FheContext, ek, nonce: bytes, aad: bytes, data: bytes, tag_len: int,
                        rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """ek: [W][4][8] BitCt (nested or flat) -> (bits [len - tag_len][8], tag_diff [tag_len][8]) BitCt."""
        key, kb = _bit_key(ek, key_bits)
        (nb, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(nonce), _bytes_ptr(aad), _bytes_ptr(data)
        n_plain = max(len(db) - tag_len, 0)
        outs, tags = (C.c_void_p * max(8 * n_plain, 1))(), (C.c_void_p * max(8 * tag_len, 1))()
        check(lib().tae_aesx_ccm_transcipher(ctx._h, kb, _handles(key), _p(nb), len(nb), a_ptr, len(ab), d_ptr, len(db),
                                             tag_len, _nr(kb, rounds), outs, tags))
        bits = [BitCt(outs[i], ctx) for i in range(8 * n_plain)]
        diff = [BitCt(tags[i], ctx) for i in range(8 * tag_len)]
        return ([bits[8 * i:8 * i + 8] for i in range(n_plain)], [diff[8 * i:8 * i + 8] for i in range(tag_len)])

    @staticmethod
    def ccm_transcipher_raw(ctx: FheContext, rk: np.ndarray, nonce: bytes, aad: bytes, data: bytes, tag_len: int,
                            rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """Host arrays: rk [W*32][L] -> (bits [len - tag_len][8][L], tag_diff [tag_len][8][L])."""
        rk, kb = _raw_key(rk, key_bits)
        (nb, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(nonce), _bytes_ptr(aad), _bytes_ptr(data)
        out = np.zeros((max(len(db) - tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        diff = np.zeros((max(tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_ccm_transcipher_raw(ctx._h, kb, _p(rk), _p(nb), len(nb), a_ptr, len(ab), d_ptr, len(db),
                                                 tag_len, _nr(kb, rounds), _p(out), _p(diff), N.TAE_MEM_HOST))
        return out, diff

    @staticmethod
    def ccm_transcipher_device(ctx: FheContext, key_bits: int, d_rk: int, nonce: bytes, aad: bytes, data: bytes,
                               tag_len: int, rounds: int, d_out: int, d_tag_diff: int):
        """Device pointers (ints) for rk, the payload bits [len - tag_len][8][L] and the tag difference
        [tag_len][8][L]; the frame is host bytes."""
        (nb, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(nonce), _bytes_ptr(aad), _bytes_ptr(data)
        check(lib().tae_aesx_ccm_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_rk), _p(nb), len(nb), a_ptr, len(ab),
                                                 d_ptr, len(db), tag_len, rounds, C.c_void_p(d_out),
                                                 C.c_void_p(d_tag_diff), N.TAE_MEM_DEVICE))

    # ---- AES-GCM decryption of public frames (SP 800-38D) ----
    # ghash_key makes the power table H^1 .. H^n_powers once per key; gcm_transcipher then takes frames
    # (iv12, aad, ciphertext || received tag) under that key and returns, per frame and in caller order, the payload
    # bits [len - tag_len][8] and the tag-difference bits [tag_len][8]: the client accepts a payload iff gcm_tag_ok.
    # A frame of m hashed blocks (padded AAD, padded ciphertext, one length block) needs n_powers >= m.
    @staticmethod
    def ghash_key(ctx: FheContext, ek, n_powers: int, rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """ek: [W][4][8] BitCt (nested or flat) -> the table as a flat list of n_powers * 128 BitCt."""
        key, kb = _bit_key(ek, key_bits)
        outs = (C.c_void_p * max(128 * n_powers, 1))()
        check(lib().tae_aesx_ghash_key(ctx._h, kb, _handles(key), n_powers, _nr(kb, rounds), outs))
        return [BitCt(outs[i], ctx) for i in range(128 * n_powers)]

    @staticmethod
    def ghash_key_raw(ctx: FheContext, rk: np.ndarray, n_powers: int, rounds: Optional[int] = None,
                      key_bits: Optional[int] = None) -> np.ndarray:
        """Host arrays: rk [W*32][L] -> hk [n_powers][128][L]."""
        rk, kb = _raw_key(rk, key_bits)
        hk = np.zeros((max(n_powers, 1), 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_ghash_key_raw(ctx._h, kb, _p(rk), n_powers, _nr(kb, rounds), _p(hk), N.TAE_MEM_HOST))
        return hk[:max(n_powers, 0)]

    @staticmethod
    def ghash_key_device(ctx: FheContext, key_bits: int, d_rk: int, n_powers: int, rounds: int, d_hk: int):
        check(lib().tae_aesx_ghash_key_raw(ctx._h, key_bits, C.c_void_p(d_rk), n_powers, rounds, C.c_void_p(d_hk),
                                           N.TAE_MEM_DEVICE))

    @staticmethod
    def gcm_transcipher(ctx: FheContext, ek, hk, frames, tag_len: int, rounds: Optional[int] = None,
                        key_bits: Optional[int] = None):
        """ek / hk BitCt (nested or flat) -> [(bits [len - tag_len][8], tag_diff [tag_len][8]), ..] BitCt."""
        key, kb = _bit_key(ek, key_bits)
        table = _flat_bits(hk)
        arr, _keep, lens = _gcm_frames(frames, tag_len)
        n, total = len(frames), sum(lens)
        outs, tags = (C.c_void_p * max(8 * total, 1))(), (C.c_void_p * max(8 * tag_len * n, 1))()
        check(lib().tae_aesx_gcm_transcipher(ctx._h, kb, _handles(key), _handles(table), len(table) // 128, arr, n,
                                             tag_len, _nr(kb, rounds), outs, tags))
        res, at = [], 0
        for f in range(n):
            bits = [BitCt(outs[8 * at + i], ctx) for i in range(8 * lens[f])]
            diff = [BitCt(tags[8 * tag_len * f + i], ctx) for i in range(8 * tag_len)]
            res.append(([bits[8 * i:8 * i + 8] for i in range(lens[f])], [diff[8 * i:8 * i + 8] for i in range(tag_len)]))
            at += lens[f]
        return res

    @staticmethod
    def gcm_transcipher_raw(ctx: FheContext, rk: np.ndarray, hk: np.ndarray, frames, tag_len: int,
                            rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """Host arrays: rk [W*32][L], hk [n_powers][128][L] -> [(bits [len - tag_len][8][L], tag_diff [tag_len][8][L]), ..]."""
        rk, kb = _raw_key(rk, key_bits)
        hk = np.ascontiguousarray(hk, dtype=np.uint64)
        if hk.ndim != 3 or hk.shape[1] != 128:
            raise N.TaeError(N.TAE_E_ARG, "a power table is an array [n_powers][128][L]")
        arr, _keep, lens = _gcm_frames(frames, tag_len)
        n, total = len(frames), sum(lens)
        out = np.zeros((total, 8, ctx.lwe_size), dtype=np.uint64)
        diff = np.zeros((n, max(tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_gcm_transcipher_raw(ctx._h, kb, _p(rk), _p(hk), hk.shape[0], arr, n, tag_len,
                                                 _nr(kb, rounds), _p(out), _p(diff), N.TAE_MEM_HOST))
        res, at = [], 0
        for f in range(n):
            res.append((out[at:at + lens[f]], diff[f]))
            at += lens[f]
        return res

    @staticmethod
    def gcm_transcipher_device(ctx: FheContext, key_bits: int, d_rk: int, d_hk: int, n_powers: int, frames, tag_len: int,
                               rounds: int, d_out: int, d_tag_diff: int):
        """Device pointers (ints) for rk, hk, the payload bits [sum (len - tag_len)][8][L] and the tag differences
        [n_frames][tag_len][8][L]; the frames are host bytes."""
        arr, _keep, _ = _gcm_frames(frames, tag_len)
        check(lib().tae_aesx_gcm_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_rk), C.c_void_p(d_hk), n_powers, arr,
                                                 len(frames), tag_len, rounds, C.c_void_p(d_out),
                                                 C.c_void_p(d_tag_diff), N.TAE_MEM_DEVICE))

    # ---- frames beyond one table: segmented GHASH ----
    # ghash_stride_key makes H^seg, H^(2 seg) .. H^(n_strides seg) once per key and seg from a table of at least seg
    # powers; gcm_long_transcipher then takes frames of up to (n_strides + 1) seg hashed blocks and returns what
    # gcm_transcipher returns.  seg <= 31 is never refused for noise.
    @staticmethod
    def ghash_stride_key(ctx: FheContext, hk, seg: int, n_strides: int):
        """hk BitCt (nested or flat) -> the stride key as a flat list of n_strides * 128 BitCt; entry 0 clones hk's
        block seg - 1."""
        table = _flat_bits(hk)
        outs = (C.c_void_p * max(128 * n_strides, 1))()
        check(lib().tae_aesx_ghash_stride_key(ctx._h, _handles(table), len(table) // 128, seg, n_strides, outs))
        return [BitCt(outs[i], ctx) for i in range(128 * n_strides)]

    @staticmethod
    def ghash_stride_key_raw(ctx: FheContext, hk: np.ndarray, seg: int, n_strides: int) -> np.ndarray:
        """Host arrays: hk [n_powers][128][L] -> sk [n_strides][128][L], sk[j - 1] = H^(seg j)."""
        hk = _raw_table(hk, "a power table is an array [n_powers][128][L]")
        sk = np.zeros((max(n_strides, 1), 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_ghash_stride_key_raw(ctx._h, _p(hk), hk.shape[0], seg, n_strides, _p(sk), N.TAE_MEM_HOST))
        return sk[:max(n_strides, 0)]

    @staticmethod
    def ghash_stride_key_device(ctx: FheContext, d_hk: int, n_powers: int, seg: int, n_strides: int, d_sk: int):
        check(lib().tae_aesx_ghash_stride_key_raw(ctx._h, C.c_void_p(d_hk), n_powers, seg, n_strides, C.c_void_p(d_sk),
                                                  N.TAE_MEM_DEVICE))

    @staticmethod
    def gcm_long_transcipher(ctx: FheContext, ek, hk, sk, seg: int, frames, tag_len: int, rounds: Optional[int] = None,
                             key_bits: Optional[int] = None):
        """ek / hk / sk BitCt (nested or flat) -> [(bits [len - tag_len][8], tag_diff [tag_len][8]), ..] BitCt."""
        key, kb = _bit_key(ek, key_bits)
        table, strides = _flat_bits(hk), _flat_bits(sk)
        arr, _keep, lens = _gcm_frames(frames, tag_len)
        n, total = len(frames), sum(lens)
        outs, tags = (C.c_void_p * max(8 * total, 1))(), (C.c_void_p * max(8 * tag_len * n, 1))()
        check(lib().tae_aesx_gcm_long_transcipher(ctx._h, kb, _handles(key), _handles(table), len(table) // 128,
                                                  _handles(strides), len(strides) // 128, seg, arr, n, tag_len,
                                                  _nr(kb, rounds), outs, tags))
        res, at = [], 0
        for f in range(n):
            bits = [BitCt(outs[8 * at + i], ctx) for i in range(8 * lens[f])]
            diff = [BitCt(tags[8 * tag_len * f + i], ctx) for i in range(8 * tag_len)]
            res.append(([bits[8 * i:8 * i + 8] for i in range(lens[f])], [diff[8 * i:8 * i + 8] for i in range(tag_len)]))
            at += lens[f]
        return res

    @staticmethod
    def gcm_long_transcipher_raw(ctx: FheContext, rk: np.ndarray, hk: np.ndarray, sk: np.ndarray, seg: int, frames,
                                 tag_len: int, rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """Host arrays: rk [W*32][L], hk [n_powers][128][L], sk [n_strides][128][L] ->
        [(bits [len - tag_len][8][L], tag_diff [tag_len][8][L]), ..]."""
        rk, kb = _raw_key(rk, key_bits)
        hk = _raw_table(hk, "a power table is an array [n_powers][128][L]")
        sk = _raw_table(sk, "a stride key is an array [n_strides][128][L]")
        arr, _keep, lens = _gcm_frames(frames, tag_len)
        n, total = len(frames), sum(lens)
        out = np.zeros((total, 8, ctx.lwe_size), dtype=np.uint64)
        diff = np.zeros((n, max(tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesx_gcm_long_transcipher_raw(ctx._h, kb, _p(rk), _p(hk), hk.shape[0], _p(sk), sk.shape[0], seg,
                                                      arr, n, tag_len, _nr(kb, rounds), _p(out), _p(diff),
                                                      N.TAE_MEM_HOST))
        res, at = [], 0
        for f in range(n):
            res.append((out[at:at + lens[f]], diff[f]))
            at += lens[f]
        return res

    @staticmethod
    def gcm_long_transcipher_device(ctx: FheContext, key_bits: int, d_rk: int, d_hk: int, n_powers: int, d_sk: int,
                                    n_strides: int, seg: int, frames, tag_len: int, rounds: int, d_out: int,
                                    d_tag_diff: int):
        """Device pointers (ints) for rk, hk, sk, the payload bits [sum (len - tag_len)][8][L] and the tag differences
        [n_frames][tag_len][8][L]; the frames are host bytes."""
        arr, _keep, _ = _gcm_frames(frames, tag_len)
        check(lib().tae_aesx_gcm_long_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_rk), C.c_void_p(d_hk), n_powers,
                                                      C.c_void_p(d_sk), n_strides, seg, arr, len(frames), tag_len,
                                                      rounds, C.c_void_p(d_out), C.c_void_p(d_tag_diff),
                                                      N.TAE_MEM_DEVICE))

    @staticmethod
    def gf128_square_raw(ctx: FheContext, elems: np.ndarray) -> np.ndarray:
        """Stage call (tae_stage_gf128_square): [count][128][L] -> the refreshed squares."""
        elems = np.ascontiguousarray(elems, dtype=np.uint64)
        out = np.zeros_like(elems)
        check(lib().tae_stage_gf128_square(ctx._h, _p(elems), elems.shape[0], _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def gf128_product_raw(ctx: FheContext, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """Stage call (tae_stage_gf128_product): a, b [count][128][L] -> the refreshed products a_c b_c."""
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        if a.shape != b.shape:
            raise N.TaeError(N.TAE_E_ARG, "the operands have one shape")
        out = np.zeros_like(a)
        check(lib().tae_stage_gf128_product(ctx._h, _p(a), _p(b), a.shape[0], _p(out), N.TAE_MEM_HOST))
        return out

    # ---- AEAD open: the transcipher call, then aead_open on what it returned ----
    @classmethod
    def ccm_open(cls, ctx: FheContext, ek, nonce: bytes, aad: bytes, data: bytes, tag_len: int,
                 rounds: Optional[int] = None, key_bits: Optional[int] = None):
        """ccm_transcipher, then the open -> (gated bits [len - tag_len][8], ok) BitCt."""
        res = cls.ccm_transcipher(ctx, ek, nonce, aad, data, tag_len, rounds, key_bits)
        plain, ok = _open_frames(ctx, [res], tag_len)
        return plain[0], ok[0]

    @classmethod
    def gcm_open(cls, ctx: FheContext, ek, hk, frames, tag_len: int, rounds: Optional[int] = None,
                 key_bits: Optional[int] = None):
        """gcm_transcipher, then the open -> (per frame the gated bits [len - tag_len][8], per frame ok) BitCt."""
        return _open_frames(ctx, cls.gcm_transcipher(ctx, ek, hk, frames, tag_len, rounds, key_bits), tag_len)

    @classmethod
    def gcm_long_open(cls, ctx: FheContext, ek, hk, sk, seg: int, frames, tag_len: int, rounds: Optional[int] = None,
                      key_bits: Optional[int] = None):
        """gcm_long_transcipher, then the open -> (per frame the gated bits, per frame ok) BitCt."""
        return _open_frames(ctx, cls.gcm_long_transcipher(ctx, ek, hk, sk, seg, frames, tag_len, rounds, key_bits),
                            tag_len)
