"""Multi-key batches: key expansion, cipher, counter mode, CBC, CCM and GCM across many AES keys under one FHE key.

A key table is `n_keys` expanded keys (or decryption keys) of one key size, `[n_keys][W*32][L]` with W = 44 / 52 /
60.  Slot `s` is an expanded key in the layout of `aes_var`, so `table[s]` can be passed to any `GalMulAes` method
as it is.  Blocks name their slot through `key_of_block`, streams through the first element of their tuple.  The
bootstraps work ciphertext by ciphertext, so the bits of different keys share their launches, and every output
word equals the one the single-key call with that slot's key gives.  A slot nothing refers to is not read.

The FHE side runs on the GPU through the C-ABI (tae_aesm_*): 1-bit parameter sets, gal-mul driver; every other
model raises TaeError (TAE_E_PARAM).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _native as N
from ._native import check, lib
from .aes_128 import _flat_bits, _iv8, _iv16
from .aes_var import KEY_BITS, _bytes_ptr, _key_bits_of_words, _nr, _open_frames, _p, _words, expanded_words
from .tfhe import BitCt, FheContext, _handles


def _raw_table(table: np.ndarray):
    """A key table [n_keys][W*32][L] as a contiguous array and its key size; a row count that is no expanded key
    is TAE_E_ARG."""
    table = np.ascontiguousarray(table, dtype=np.uint64)
    if table.ndim != 3 or table.shape[1] % 32:
        raise N.TaeError(N.TAE_E_ARG, "a key table is an array [n_keys][words * 32][L]")
    return table, _key_bits_of_words(table.shape[1] // 32)


def _bit_table(table):
    """A table of handles: a list of per-slot keys ([W][4][8] BitCt, nested or flat; None for a slot that is not
    used) -> the flat handle array, n_keys and the key size."""
    slots = [None if k is None else _flat_bits(k) for k in table]
    sizes = {len(k) for k in slots if k is not None}
    if len(sizes) != 1 or next(iter(sizes)) % 32:
        raise N.TaeError(N.TAE_E_ARG, "the slots of a key table are expanded keys of one size")
    n = next(iter(sizes))
    kb = _key_bits_of_words(n // 32)
    arr = (C.c_void_p * (n * len(slots)))()
    for s, k in enumerate(slots):
        if k is not None:
            for i, b in enumerate(k):
                arr[s * n + i] = b._h.value
    return arr, len(slots), kb


def _key_of(key_of_block, nb: int) -> np.ndarray:
    ko = np.ascontiguousarray(key_of_block, dtype=np.int32)
    if ko.shape != (nb,):
        raise N.TaeError(N.TAE_E_ARG, "key_of_block has one slot per block")
    return ko


def _ctr_streams(streams):
    """(slot, iv, first_counter, data) or (slot, iv, first_counter, None, length) -> tae_ctr_stream array, the
    buffers it points into, and the stream lengths."""
    arr = (N.TaeCtrStream * max(len(streams), 1))()
    keep, lens = [], []
    for i, st in enumerate(streams):
        slot, iv, first, data = st[:4]
        if data is None:
            if len(st) != 5:
                raise ValueError("a keystream stream is (slot, iv, first_counter, None, length)")
            n, ptr = int(st[4]), None
        else:
            buf = np.frombuffer(bytes(data), dtype=np.uint8)
            keep.append(buf)
            n, ptr = len(buf), buf.ctypes.data if len(buf) else None
        arr[i].key = slot
        arr[i].iv[:] = list(_iv8(iv))
        arr[i].first_counter = first
        arr[i].data = ptr
        arr[i].len = n
        lens.append(n)
    return arr, keep, lens


def _cbc_streams(streams):
    arr = (N.TaeCbcStream * max(len(streams), 1))()
    keep, lens = [], []
    for i, (slot, iv, data) in enumerate(streams):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        keep.append(buf)
        arr[i].key = slot
        arr[i].iv[:] = list(_iv16(iv))
        arr[i].data = buf.ctypes.data if len(buf) else None
        arr[i].len = len(buf)
        lens.append(len(buf))
    return arr, keep, lens


def _ccm_streams(streams, tag_len: int):
    """(slot, nonce, aad, data) -> tae_ccm_stream array, the buffers it points into, and the payload lengths."""
    arr = (N.TaeCcmStream * max(len(streams), 1))()
    keep, lens = [], []
    for i, (slot, nonce, aad, data) in enumerate(streams):
        (nb, _), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(nonce), _bytes_ptr(aad), _bytes_ptr(data)
        keep += [nb, ab, db]
        arr[i].key = slot
        arr[i].nonce = nb.ctypes.data
        arr[i].nonce_len = len(nb)
        arr[i].aad = a_ptr.value if a_ptr else None
        arr[i].aad_len = len(ab)
        arr[i].data = d_ptr.value if d_ptr else None
        arr[i].len = len(db)
        lens.append(max(len(db) - tag_len, 0))
    return arr, keep, lens


def _gcm_streams(streams, tag_len: int):
    """(slot, iv12, aad, data) -> tae_gcm_stream array, the buffers it points into, and the payload lengths."""
    arr = (N.TaeGcmStream * max(len(streams), 1))()
    keep, lens = [], []
    for i, (slot, iv, aad, data) in enumerate(streams):
        (ib, i_ptr), (ab, a_ptr), (db, d_ptr) = _bytes_ptr(iv), _bytes_ptr(aad), _bytes_ptr(data)
        keep += [ib, ab, db]
        arr[i].key = slot
        arr[i].iv, arr[i].iv_len = (i_ptr.value if i_ptr else None), len(ib)
        arr[i].aad, arr[i].aad_len = (a_ptr.value if a_ptr else None), len(ab)
        arr[i].data, arr[i].len = (d_ptr.value if d_ptr else None), len(db)
        lens.append(max(len(db) - tag_len, 0))
    return arr, keep, lens


def _raw_htable(htable: np.ndarray, n_keys: int) -> np.ndarray:
    htable = np.ascontiguousarray(htable, dtype=np.uint64)
    if htable.ndim != 4 or htable.shape[0] != n_keys or htable.shape[2] != 128:
        raise N.TaeError(N.TAE_E_ARG, "the power tables are an array [n_keys][n_powers][128][L]")
    return htable


def _bit_htable(htable, n_keys: int):
    """Per-slot power tables of handles ([n_powers * 128] BitCt, nested or flat; None for a slot that is not used)
    -> the flat handle array and n_powers."""
    slots = [None if t is None else _flat_bits(t) for t in htable]
    sizes = {len(t) for t in slots if t is not None}
    if len(slots) != n_keys or len(sizes) != 1 or next(iter(sizes)) % 128:
        raise N.TaeError(N.TAE_E_ARG, "one power table per slot of the key table, all of one size")
    n = next(iter(sizes))
    arr = (C.c_void_p * (n * len(slots)))()
    for s, t in enumerate(slots):
        if t is not None:
            for i, b in enumerate(t):
                arr[s * n + i] = b._h.value
    return arr, n // 128


def _split(out, lens):
    res, at = [], 0
    for n in lens:
        res.append(out[at:at + n])
        at += n
    return res


class GalMulAesMulti:
    """aes_var.GalMulAes over a key table.  The key size is read from the table (or, for `key_schedule*`, from the
    keys); the `_device` variants take pointers and therefore `key_bits` and `n_keys`.  `rounds` defaults to Nr.
    Counter-mode streams are `(slot, iv, first_counter, data)` tuples, or `(slot, iv, first_counter, None, length)`
    for the keystream; CBC streams are `(slot, iv16, data)`, CCM frames `(slot, nonce, aad, data)` and GCM frames
    `(slot, iv12, aad, data)`.  The stream methods return one result per stream."""

    # ---- key expansion (FIPS-197 5.2), all keys in one pass ----
    @staticmethod
    def key_schedule_raw(ctx: FheContext, keys: np.ndarray) -> np.ndarray:
        """Fresh key bits [n_keys][128 | 192 | 256][L] -> table [n_keys][W*32][L]."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if keys.ndim != 3 or keys.shape[1] not in KEY_BITS:
            raise N.TaeError(N.TAE_E_ARG, "keys must be [n_keys][128 | 192 | 256][L] bits")
        kb = keys.shape[1]
        out = np.zeros((keys.shape[0], expanded_words(kb) * 32, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_key_schedule_raw(ctx._h, kb, _p(keys), keys.shape[0], _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def key_schedule_device(ctx: FheContext, key_bits: int, d_keys: int, n_keys: int, d_table: int):
        """Device pointers (ints): keys [n_keys][key_bits][L] -> table [n_keys][W*32][L]."""
        check(lib().tae_aesm_key_schedule_raw(ctx._h, key_bits, C.c_void_p(d_keys), n_keys, C.c_void_p(d_table),
                                              N.TAE_MEM_DEVICE))

    @staticmethod
    def key_schedule(ctx: FheContext, keys) -> list:
        """A list of keys, each [16 | 24 | 32][8] BitCt (nested or flat) -> a list of expanded keys [W][4][8]."""
        flat = [_flat_bits(k) for k in keys]
        sizes = {len(k) for k in flat}
        if flat and (len(sizes) != 1 or next(iter(sizes)) not in KEY_BITS):
            raise N.TaeError(N.TAE_E_ARG, "keys must be 16, 24 or 32 encrypted bytes, all of one size")
        if not flat:
            return []
        kb = len(flat[0])
        n = expanded_words(kb) * 32
        outs = (C.c_void_p * (n * len(flat)))()
        check(lib().tae_aesm_key_schedule(ctx._h, kb, _handles([b for k in flat for b in k]), len(flat), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return [_words(bits[s * n:(s + 1) * n]) for s in range(len(flat))]

    # ---- decryption keys (FIPS-197 5.3.5) ----
    @staticmethod
    def decrypt_key_raw(ctx: FheContext, table: np.ndarray) -> np.ndarray:
        table, kb = _raw_table(table)
        out = np.zeros_like(table)
        check(lib().tae_aesm_decrypt_key_raw(ctx._h, kb, _p(table), table.shape[0], _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def decrypt_key_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, d_dtable: int):
        check(lib().tae_aesm_decrypt_key_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, C.c_void_p(d_dtable),
                                             N.TAE_MEM_DEVICE))

    # ---- cipher and inverse cipher, block i under slot key_of_block[i] ----
    @staticmethod
    def _blocks_raw(fn, ctx, table, key_of_block, blocks, rounds):
        table, kb = _raw_table(table)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
        ko = _key_of(key_of_block, blocks.shape[0])
        out = np.zeros_like(blocks)
        check(fn(ctx._h, kb, _p(table), table.shape[0], _p(ko), _p(blocks), blocks.shape[0], _nr(kb, rounds), _p(out),
                 N.TAE_MEM_HOST))
        return out

    @classmethod
    def encrypt_blocks_raw(cls, ctx: FheContext, table: np.ndarray, key_of_block, blocks: np.ndarray,
                           rounds: Optional[int] = None) -> np.ndarray:
        """Host arrays: table [n_keys][W*32][L], blocks [n][128][L] -> [n][128][L]."""
        return cls._blocks_raw(lib().tae_aesm_encrypt_blocks_raw, ctx, table, key_of_block, blocks, rounds)

    @classmethod
    def decrypt_blocks_raw(cls, ctx: FheContext, dtable: np.ndarray, key_of_block, blocks: np.ndarray,
                           rounds: Optional[int] = None) -> np.ndarray:
        """The same with a table of decryption keys (decrypt_key_raw)."""
        return cls._blocks_raw(lib().tae_aesm_decrypt_blocks_raw, ctx, dtable, key_of_block, blocks, rounds)

    @staticmethod
    def encrypt_blocks_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, key_of_block, d_blocks: int,
                              nb: int, rounds: int, d_out: int):
        """Device pointers (ints) for the table, the blocks and the output; key_of_block is a host array."""
        ko = _key_of(key_of_block, nb)
        check(lib().tae_aesm_encrypt_blocks_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, _p(ko),
                                                C.c_void_p(d_blocks), nb, rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def decrypt_blocks_device(ctx: FheContext, key_bits: int, d_dtable: int, n_keys: int, key_of_block, d_blocks: int,
                              nb: int, rounds: int, d_out: int):
        ko = _key_of(key_of_block, nb)
        check(lib().tae_aesm_decrypt_blocks_raw(ctx._h, key_bits, C.c_void_p(d_dtable), n_keys, _p(ko),
                                                C.c_void_p(d_blocks), nb, rounds, C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    # ---- counter mode with public counters ----
    @staticmethod
    def ctr_plan(streams) -> int:
        """Round-1 SBOX groups of the streams: their distinct (slot, byte position, byte value) triples."""
        arr, _keep, _ = _ctr_streams(streams)
        n = C.c_size_t(0)
        check(lib().tae_aesm_ctr_plan(arr, len(streams), C.byref(n)))
        return n.value

    @staticmethod
    def ctr_transcipher_raw(ctx: FheContext, table: np.ndarray, streams, rounds: Optional[int] = None) -> List[np.ndarray]:
        """Per stream [len][8][L]: FHE encryptions of the plaintext bits (of the keystream bits without data)."""
        table, kb = _raw_table(table)
        arr, _keep, lens = _ctr_streams(streams)
        out = np.zeros((sum(lens), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_ctr_transcipher_raw(ctx._h, kb, _p(table), table.shape[0], arr, len(streams),
                                                 _nr(kb, rounds), _p(out), N.TAE_MEM_HOST))
        return _split(out, lens)

    @staticmethod
    def ctr_transcipher_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, streams, rounds: int,
                               d_out: int):
        """Device pointers (ints) for the table and the output [sum len][8][L], the streams' bytes concatenated in
        stream order; the streams are host data."""
        arr, _keep, _ = _ctr_streams(streams)
        check(lib().tae_aesm_ctr_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, arr, len(streams), rounds,
                                                 C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def ctr_transcipher(ctx: FheContext, table, streams, rounds: Optional[int] = None) -> list:
        """table: a list of expanded keys ([W][4][8] BitCt; None for a slot no stream uses) -> per stream
        [len][8] BitCt."""
        arr_t, n_keys, kb = _bit_table(table)
        arr, _keep, lens = _ctr_streams(streams)
        outs = (C.c_void_p * (8 * sum(lens)))()
        check(lib().tae_aesm_ctr_transcipher(ctx._h, kb, arr_t, n_keys, arr, len(streams), _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return _split([bits[8 * i:8 * i + 8] for i in range(sum(lens))], lens)

    # ---- CBC with a public ciphertext ----
    @staticmethod
    def cbc_transcipher_raw(ctx: FheContext, dtable: np.ndarray, streams, rounds: Optional[int] = None) -> List[np.ndarray]:
        dtable, kb = _raw_table(dtable)
        arr, _keep, lens = _cbc_streams(streams)
        out = np.zeros((sum(lens), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_cbc_transcipher_raw(ctx._h, kb, _p(dtable), dtable.shape[0], arr, len(streams),
                                                 _nr(kb, rounds), _p(out), N.TAE_MEM_HOST))
        return _split(out, lens)

    @staticmethod
    def cbc_transcipher_device(ctx: FheContext, key_bits: int, d_dtable: int, n_keys: int, streams, rounds: int,
                               d_out: int):
        arr, _keep, _ = _cbc_streams(streams)
        check(lib().tae_aesm_cbc_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_dtable), n_keys, arr, len(streams), rounds,
                                                 C.c_void_p(d_out), N.TAE_MEM_DEVICE))

    @staticmethod
    def cbc_transcipher(ctx: FheContext, dtable, streams, rounds: Optional[int] = None) -> list:
        arr_t, n_keys, kb = _bit_table(dtable)
        arr, _keep, lens = _cbc_streams(streams)
        outs = (C.c_void_p * (8 * sum(lens)))()
        check(lib().tae_aesm_cbc_transcipher(ctx._h, kb, arr_t, n_keys, arr, len(streams), _nr(kb, rounds), outs))
        bits = [BitCt(h, ctx) for h in outs]
        return _split([bits[8 * i:8 * i + 8] for i in range(sum(lens))], lens)

    # ---- AES-CCM decryption of public frames (RFC 3610) ----
    # Frames are (slot, nonce, aad, data) with data = encrypted payload || encrypted tag, one tag_len for the call.
    # Per frame the result is (payload bits [len - tag_len][8], tag-difference bits [tag_len][8]).
    @staticmethod
    def public_keystream_raw(ctx: FheContext, table: np.ndarray, key_of_block, blocks16,
                             rounds: Optional[int] = None) -> np.ndarray:
        """n public 16-byte blocks, block i under slot key_of_block[i] -> E(block) [n][128][L]."""
        table, kb = _raw_table(table)
        buf = np.ascontiguousarray(np.frombuffer(b"".join(bytes(b) for b in blocks16), dtype=np.uint8))
        if len(buf) % 16:
            raise N.TaeError(N.TAE_E_ARG, "public blocks are 16 bytes each")
        n = len(buf) // 16
        ko = _key_of(key_of_block, n)
        out = np.zeros((n, 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_pub_keystream_raw(ctx._h, kb, _p(table), table.shape[0], _p(ko), _p(buf), n,
                                               _nr(kb, rounds), _p(out), N.TAE_MEM_HOST))
        return out

    @staticmethod
    def ccm_transcipher_raw(ctx: FheContext, table: np.ndarray, streams, tag_len: int,
                            rounds: Optional[int] = None) -> list:
        """Host arrays: per frame (bits [len - tag_len][8][L], tag_diff [tag_len][8][L]), in the caller's order."""
        table, kb = _raw_table(table)
        arr, _keep, lens = _ccm_streams(streams, tag_len)
        out = np.zeros((sum(lens), 8, ctx.lwe_size), dtype=np.uint64)
        diff = np.zeros((len(streams), max(tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_ccm_transcipher_raw(ctx._h, kb, _p(table), table.shape[0], arr, len(streams), tag_len,
                                                 _nr(kb, rounds), _p(out), _p(diff), N.TAE_MEM_HOST))
        return list(zip(_split(out, lens), diff))

    @staticmethod
    def ccm_transcipher_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, streams, tag_len: int,
                               rounds: int, d_out: int, d_tag_diff: int):
        """Device pointers (ints) for the table, the payload bits [sum (len - tag_len)][8][L] and the tag
        differences [n_streams][tag_len][8][L]; the frames are host data."""
        arr, _keep, _ = _ccm_streams(streams, tag_len)
        check(lib().tae_aesm_ccm_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, arr, len(streams), tag_len,
                                                 rounds, C.c_void_p(d_out), C.c_void_p(d_tag_diff), N.TAE_MEM_DEVICE))

    @staticmethod
    def ccm_transcipher(ctx: FheContext, table, streams, tag_len: int, rounds: Optional[int] = None) -> list:
        """table: a list of expanded keys ([W][4][8] BitCt; None for a slot no frame uses) -> per frame
        (bits [len - tag_len][8], tag_diff [tag_len][8]) BitCt."""
        arr_t, n_keys, kb = _bit_table(table)
        arr, _keep, lens = _ccm_streams(streams, tag_len)
        outs = (C.c_void_p * max(8 * sum(lens), 1))()
        tags = (C.c_void_p * max(8 * tag_len * len(streams), 1))()
        check(lib().tae_aesm_ccm_transcipher(ctx._h, kb, arr_t, n_keys, arr, len(streams), tag_len, _nr(kb, rounds),
                                             outs, tags))
        bits = [BitCt(outs[i], ctx) for i in range(8 * sum(lens))]
        diff = [BitCt(tags[i], ctx) for i in range(8 * tag_len * len(streams))]
        plain = _split([bits[8 * i:8 * i + 8] for i in range(sum(lens))], lens)
        per = 8 * tag_len
        return [(plain[s], [diff[s * per + 8 * i:s * per + 8 * i + 8] for i in range(tag_len)])
                for s in range(len(streams))]

    @classmethod
    def ccm_open(cls, ctx: FheContext, table, streams, tag_len: int, rounds: Optional[int] = None):
        """ccm_transcipher, then aes_var.aead_open on what it returned -> (per frame the gated bits
        [len - tag_len][8], per frame ok) BitCt."""
        return _open_frames(ctx, cls.ccm_transcipher(ctx, table, streams, tag_len, rounds), tag_len)

    # ---- AES-GCM decryption of public frames over key tables (SP 800-38D) ----
    # Frames are (slot, iv12, aad, data) with data = ciphertext || received tag, one tag_len for the call.  The power
    # tables are [n_keys][n_powers][128][L]: slot s is what aes_var.GalMulAes.ghash_key* gives on table[s].
    @staticmethod
    def ghash_key_raw(ctx: FheContext, table: np.ndarray, n_powers: int, rounds: Optional[int] = None) -> np.ndarray:
        """Host arrays: table [n_keys][W*32][L] -> htable [n_keys][n_powers][128][L]."""
        table, kb = _raw_table(table)
        out = np.zeros((table.shape[0], max(n_powers, 1), 128, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_ghash_key_raw(ctx._h, kb, _p(table), table.shape[0], n_powers, _nr(kb, rounds), _p(out),
                                           N.TAE_MEM_HOST))
        return out[:, :max(n_powers, 0)]

    @staticmethod
    def ghash_key_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, n_powers: int, rounds: int,
                         d_htable: int):
        check(lib().tae_aesm_ghash_key_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, n_powers, rounds,
                                           C.c_void_p(d_htable), N.TAE_MEM_DEVICE))

    @staticmethod
    def ghash_key(ctx: FheContext, table, n_powers: int, rounds: Optional[int] = None) -> list:
        """table: a list of expanded keys ([W][4][8] BitCt, every slot present) -> per slot [n_powers * 128] BitCt."""
        arr_t, n_keys, kb = _bit_table(table)
        if any(k is None for k in table):
            raise N.TaeError(N.TAE_E_ARG, "ghash_key reads every slot of the key table")
        per = 128 * max(n_powers, 0)
        outs = (C.c_void_p * max(per * n_keys, 1))()
        check(lib().tae_aesm_ghash_key(ctx._h, kb, arr_t, n_keys, n_powers, _nr(kb, rounds), outs))
        return [[BitCt(outs[s * per + i], ctx) for i in range(per)] for s in range(n_keys)]

    @staticmethod
    def gcm_transcipher_raw(ctx: FheContext, table: np.ndarray, htable: np.ndarray, streams, tag_len: int,
                            rounds: Optional[int] = None) -> list:
        """Host arrays: per frame (bits [len - tag_len][8][L], tag_diff [tag_len][8][L]), in the caller's order."""
        table, kb = _raw_table(table)
        htable = _raw_htable(htable, table.shape[0])
        arr, _keep, lens = _gcm_streams(streams, tag_len)
        out = np.zeros((sum(lens), 8, ctx.lwe_size), dtype=np.uint64)
        diff = np.zeros((len(streams), max(tag_len, 0), 8, ctx.lwe_size), dtype=np.uint64)
        check(lib().tae_aesm_gcm_transcipher_raw(ctx._h, kb, _p(table), table.shape[0], _p(htable), htable.shape[1], arr,
                                                 len(streams), tag_len, _nr(kb, rounds), _p(out), _p(diff),
                                                 N.TAE_MEM_HOST))
        return list(zip(_split(out, lens), diff))

    @staticmethod
    def gcm_transcipher_device(ctx: FheContext, key_bits: int, d_table: int, n_keys: int, d_htable: int, n_powers: int,
                               streams, tag_len: int, rounds: int, d_out: int, d_tag_diff: int):
        """Device pointers (ints) for both tables, the payload bits [sum (len - tag_len)][8][L] and the tag differences
        [n_streams][tag_len][8][L]; the frames are host data.  The power tables are read where they lie."""
        arr, _keep, _ = _gcm_streams(streams, tag_len)
        check(lib().tae_aesm_gcm_transcipher_raw(ctx._h, key_bits, C.c_void_p(d_table), n_keys, C.c_void_p(d_htable),
                                                 n_powers, arr, len(streams), tag_len, rounds, C.c_void_p(d_out),
                                                 C.c_void_p(d_tag_diff), N.TAE_MEM_DEVICE))

    @staticmethod
    def gcm_transcipher(ctx: FheContext, table, htable, streams, tag_len: int, rounds: Optional[int] = None) -> list:
        """table / htable: lists of expanded keys and of power tables (ghash_key), None for a slot no frame uses ->
        per frame (bits [len - tag_len][8], tag_diff [tag_len][8]) BitCt."""
        arr_t, n_keys, kb = _bit_table(table)
        arr_h, n_powers = _bit_htable(htable, n_keys)
        arr, _keep, lens = _gcm_streams(streams, tag_len)
        outs = (C.c_void_p * max(8 * sum(lens), 1))()
        tags = (C.c_void_p * max(8 * tag_len * len(streams), 1))()
        check(lib().tae_aesm_gcm_transcipher(ctx._h, kb, arr_t, n_keys, arr_h, n_powers, arr, len(streams), tag_len,
                                             _nr(kb, rounds), outs, tags))
        bits = [BitCt(outs[i], ctx) for i in range(8 * sum(lens))]
        diff = [BitCt(tags[i], ctx) for i in range(8 * tag_len * len(streams))]
        plain = _split([bits[8 * i:8 * i + 8] for i in range(sum(lens))], lens)
        per = 8 * tag_len
        return [(plain[s], [diff[s * per + 8 * i:s * per + 8 * i + 8] for i in range(tag_len)])
                for s in range(len(streams))]

    @classmethod
    def gcm_open(cls, ctx: FheContext, table, htable, streams, tag_len: int, rounds: Optional[int] = None):
        """gcm_transcipher, then aes_var.aead_open on what it returned -> (per frame the gated bits
        [len - tag_len][8], per frame ok) BitCt."""
        return _open_frames(ctx, cls.gcm_transcipher(ctx, table, htable, streams, tag_len, rounds), tag_len)
