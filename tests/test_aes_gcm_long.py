"""Segmented GHASH without a GPU (include/tfhe_aes_gpu.h "frames beyond one table"):

- the identity GHASH = S_0 + sum S_c H^(seg c) and the whole plan on plain bits, restated in tests/gcm_long_ref.py
  from tests/gcm_ref.py;
- tae_aesx_gcm_long_rows against that restatement, and against tae_aesx_gcm_tag_rows at C = 1;
- the refusals and the argument errors of the new calls;
- the host layer compiled stand-alone on plain bits (tests/native/aes_gcm_long_test.cpp), plain and as a
  -fsanitize=address,undefined binary;
- the host model's per-bit levels and ids, called in the product library (tests/native/aes_gcm_long_noise_test.cpp).
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_var
from tests import gcm_ref as R
from tests.gcm_long_ref import inner_chunks, long_plan, segment_blocks, segment_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
W = 32


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def _xor(a, b):
    return bytes(u ^ v for u, v in zip(a, b))


def _powers(h, n):
    out, p = [], h
    for _ in range(n):
        out.append(p)
        p = R.mul(p, h)
    return out


def _bits_sum(bits, row):
    return sum(bits[s] for s in row) & 1


# ---- the identity and the whole plan on plain bits ------------------------------------------------------------------
@pytest.mark.parametrize("seg,m", ((2, 5), (8, 22), (31, 93), (31, 100), (48, 97)))
def test_identity(seg, m):
    """Tests the reference, not the feature: the identity on tests/gcm_long_ref.py's segments, by tests/gcm_ref.py's
    field.  No product code runs here; the restatement it validates is what the later tests compare the library to."""
    rnd = random.Random(100 * seg + m)
    c = bytes(rnd.randrange(256) for _ in range(16 * (m - 1)))
    xs = R.hashed_blocks(b"", c)
    assert len(xs) == m
    h = _powers(R.H1, seg * (-(-m // seg)))
    acc = bytes(16)
    for s in range(-(-m // seg)):
        sc = bytes(16)
        for k, x in enumerate(segment_blocks(xs, seg, s), start=1):
            sc = _xor(sc, R.mul(x, h[k - 1]))
        acc = _xor(acc, sc if s == 0 else R.mul(sc, h[seg * s - 1]))
    assert acc == aes_var.ghash_plain(R.H1, b"", c)


@pytest.mark.parametrize("seg", (1, 2, 31))
def test_whole_plan_on_plain_bits(seg):
    """Tests the reference, not the feature: the restated plan (tests/gcm_long_ref.py) on plain bits gives
    E(J0) ^ GHASH ^ tag.  The library's own plan on plain bits is tests/native/aes_gcm_long_test.cpp."""
    rnd = random.Random(seg)
    ej0, tag = bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(16))
    for m in sorted({1, seg, seg + 1, 2 * seg, 2 * seg + 1, 100}):
        aad = bytes(rnd.randrange(256) for _ in range(16 * min(m - 1, 1)))
        c = bytes(rnd.randrange(256) for _ in range(16 * (m - 1) - len(aad)))
        assert len(R.hashed_blocks(aad, c)) == m
        powers = _powers(R.H1, seg * (-(-m // seg)))
        src = [bit for q in powers[:min(seg, m)] for bit in R.coefs(q)] + R.coefs(ej0)
        inner, final = long_plan(aad, c, 16, seg)
        for s, rows in enumerate(inner, start=1):
            # chunk sums, refresh (the identity on a bit), row sums, refresh, the product by the field's multiplication
            sc = R.from_coefs([sum(_bits_sum(src, ch) for ch in inner_chunks(row)) & 1 for row in rows])
            src += R.coefs(R.mul(sc, powers[seg * s - 1]))
        tb = min(seg, m)
        diff = []
        for r, row in enumerate(final):
            chunks = R.row_chunks(row)
            chunks[0] = [128 * tb + r] + chunks[0]
            assert len(chunks[0]) <= 56 and all(len(ch) <= 64 for ch in chunks[1:]) and len(chunks) <= 64
            diff.append((sum(_bits_sum(src, ch) for ch in chunks) + R.coefs(tag)[r]) & 1)
        assert R.from_coefs(diff) == _xor(_xor(aes_var.ghash_plain(R.H1, aad, c), ej0), tag)


def test_stride_schedule_on_plain_values():
    """Tests the reference, not the feature: tests/gcm_ref.py's power schedule on the base G_1 = H^seg (an even stride
    the square of j / 2, an odd one G_(j-1) G_1) gives H^(seg j).  The library's schedule on plain bits is in
    tests/native/aes_gcm_long_test.cpp."""
    for seg, n in ((1, 4), (2, 5), (3, 33), (31, 3)):
        powers = _powers(R.H1, seg * n)
        g = {1: powers[seg - 1]}
        for squares, products in R.power_schedule(n):
            for j in squares:
                g[j] = R.mul(g[j // 2], g[j // 2])
            for j in products:
                g[j] = R.mul(g[j - 1], g[1])
        assert [g[j] for j in range(1, n + 1)] == powers[seg - 1::seg]


# ---- the helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aad_len,data_len,seg,tag_len", ((0, 0, 1, 16), (8, 40, 2, 12), (16, 320, 8, 16), (0, 33, 1, 4),
                                                          (20, 60, 7, 16), (0, 99 * 16, 31, 16)))
def test_long_rows_match_the_restatement(aad_len, data_len, seg, tag_len):
    aad, c = bytes(range(1, 1 + aad_len)), bytes((7 * i + 3) & 255 for i in range(data_len))
    m = len(R.hashed_blocks(aad, c))
    segs = -(-m // seg)
    src, chunks = aes_var.gcm_long_rows(R.IV3, aad, c, tag_len, seg, seg, max(segs - 1, 1))
    assert src.shape == chunks.shape == (segs, 128)
    inner, final = long_plan(aad, c, tag_len, seg)
    assert list(src[0, :8 * tag_len]) == [len(r) for r in final]
    assert list(chunks[0, :8 * tag_len]) == [len(R.row_chunks(r)) for r in final]
    assert not src[0, 8 * tag_len:].any() and not chunks[0, 8 * tag_len:].any()
    for s, rows in enumerate(inner, start=1):
        assert list(src[s]) == [len(r) for r in rows]
        assert list(chunks[s]) == [len(inner_chunks(r)) for r in rows]
    if segs == 1:  # the single-table rows
        old_src, old_chunks = aes_var.gcm_tag_rows(R.IV3, aad, c, tag_len, seg)
        assert list(old_src) == list(src[0, :8 * tag_len]) and list(old_chunks) == list(chunks[0, :8 * tag_len])


def test_short_frames_are_the_single_table_rows():
    aad, c = bytes(range(20)), bytes((11 * i + 1) & 255 for i in range(60))  # m = 7
    for seg in (7, 8, 31):
        src, chunks = aes_var.gcm_long_rows(R.IV3, aad, c, 16, 31, seg, 1)
        old_src, old_chunks = aes_var.gcm_tag_rows(R.IV3, aad, c, 16, 31)
        assert src.shape == (1, 128) and list(src[0]) == list(old_src) and list(chunks[0]) == list(old_chunks)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    rows = aes_var.gcm_long_rows
    ff, a5 = bytes([0xFF]) * (100 * 16), bytes([0xA5]) * (99 * 16)
    src, chunks = rows(R.IV3, b"", ff, 16, 31, 31, 64)  # 100 blocks of 0xFF at seg = 31: accepted
    assert src.shape == (4, 128) and src.max() == 31 * 126 and chunks.max() <= 64
    # 99 blocks of 0xA5 at seg = 48: rows of 48 * 93 sources
    assert _code(lambda: rows(R.IV3, b"", a5, 16, 48, 48, 64)) == N.TAE_E_NOISE
    assert max(len(r) for r in segment_rows(R.hashed_blocks(b"", a5), 48, 1, 128)) == 48 * 93 > 55 + 63 * 64
    src, chunks = rows(R.IV3, b"", a5, 16, 31, 31, 3)  # the frame test_gpu_gcm.py shows refused: 46 chunks at most
    assert src.max() <= 31 * 93 + 3 and chunks.max() <= 46
    assert 31 * 128 + 64 <= 55 + 63 * 64  # seg <= 31 is never refused for noise
    for seg, n_powers, n_strides in ((0, 31, 3), (32, 31, 3), (65, 128, 3), (31, 31, 0), (31, 31, 65), (31, 31, 2)):
        assert _code(lambda: rows(R.IV3, b"", a5, 16, n_powers, seg, n_strides)) == N.TAE_E_PARAM
    assert _code(lambda: rows(bytes(16), b"", a5, 16, 31, 31, 3)) == N.TAE_E_PARAM
    assert _code(lambda: rows(R.IV3, b"", a5, 5, 31, 31, 3)) == N.TAE_E_PARAM
    # the shape before the rows: a refused shape with rows that would be refused too is TAE_E_PARAM
    assert _code(lambda: rows(R.IV3, b"", a5, 16, 48, 48, 1)) == N.TAE_E_PARAM


def test_noise_schedule_check():
    chk = aes_var.gcm_long_noise_schedule_check
    for kb in aes_var.KEY_BITS:
        chk(PID, kb, kb // 32 + 6, 2, 2, 2, aad_len=8, data_len=40)  # m = 5, C = 3
    chk(PID, 128, 2, 4, 4, 1, aad_len=8, data_len=20)  # C = 1
    chk(PID, 128, 10, 31, 31, 3, aad_len=0, data_len=99 * 16)  # m = 100, dense
    assert _code(lambda: chk(PID, 128, 10, 48, 48, 3, 0, 99 * 16)) == N.TAE_E_NOISE
    for args in ((PID, 128, 1, 2, 2, 2), (PID, 128, 11, 2, 2, 2), (PID, 128, 10, 2, 0, 2), (PID, 128, 10, 2, 3, 2),
                 (PID, 128, 10, 2, 2, 0), (PID, 128, 10, 2, 2, 65), (PID, 128, 10, 0, 1, 1), (PID, 160, 10, 2, 2, 2),
                 (tfhe_aes.PARAMS_WOPPBS_8BIT, 128, 10, 2, 2, 2)):
        assert _code(lambda: chk(*args, aad_len=8, data_len=40)) == N.TAE_E_PARAM, args
    assert _code(lambda: chk(PID, 128, 10, 2, 2, 1, aad_len=8, data_len=40)) == N.TAE_E_PARAM  # C - 1 = 2 > 1


def test_null_arguments():
    L = N.lib()
    key = np.zeros((44 * W, 4), dtype=np.uint64)
    out = np.zeros((128, 4), dtype=np.uint64)
    iv = np.zeros(12, dtype=np.uint8)
    rows = np.zeros(128, dtype=np.int32)
    assert L.tae_aesx_gcm_long_rows(None, 12, None, 0, None, 0, 16, 1, 1, 1, _vp(rows), _vp(rows)) == N.TAE_E_ARG
    assert L.tae_aesx_gcm_long_rows(_vp(iv), 12, None, 0, None, 0, 16, 1, 1, 1, None, _vp(rows)) == N.TAE_E_ARG
    assert L.tae_aesx_gcm_long_rows(_vp(iv), 12, None, 3, None, 0, 16, 1, 1, 1, _vp(rows), _vp(rows)) == N.TAE_E_ARG
    assert L.tae_aesx_ghash_stride_key_raw(None, None, 1, 1, 1, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_ghash_stride_key_raw(None, _vp(out), 1, 1, 1, None, N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_ghash_stride_key(None, None, 1, 1, 1, None) == N.TAE_E_ARG
    arr, _keep, _ = aes_var._gcm_frames([(bytes(12), b"", bytes(16))], 16)
    for rk, hk, sk, diff in ((None, out, out, out), (key, None, out, out), (key, out, None, out), (key, out, out, None)):
        args = [None if a is None else _vp(a) for a in (rk, hk, sk, diff)]
        assert L.tae_aesx_gcm_long_transcipher_raw(None, 128, args[0], args[1], 1, args[2], 1, 1, arr, 1, 16, 10,
                                                   _vp(out), args[3], N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_gcm_long_transcipher_raw(None, 128, _vp(key), _vp(out), 1, _vp(out), 1, 1, None, 1, 16, 10,
                                               _vp(out), _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_gcm_long_transcipher_raw(None, 160, _vp(key), _vp(out), 1, _vp(out), 1, 1, arr, 1, 16, 10,
                                               _vp(out), _vp(out), N.TAE_MEM_HOST) == N.TAE_E_PARAM
    assert L.tae_aesx_gcm_long_transcipher(None, 128, None, None, 1, None, 1, 1, arr, 1, 16, 10, None, None) == N.TAE_E_ARG


# ---- the host layer, compiled stand-alone -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_gcm_long_layer_native(tmp_path, flags):
    exe = str(tmp_path / "aes_gcm_long_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags,
                    os.path.join(ROOT, "tests", "native", "aes_gcm_long_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_noise_levels_and_ids_native(tmp_path):
    exe = str(tmp_path / "aes_gcm_long_noise_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tfhe-aes-2_amd")], check=True)
    lib = os.path.join(ROOT, "tfhe-aes-2_amd", "tfhe_aes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    os.path.join(ROOT, "tests", "native", "aes_gcm_long_noise_test.cpp"),
                    os.path.join(lib, "libtfhe_aes_amd.so"), "-o", exe, "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
