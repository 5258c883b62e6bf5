"""The stage calls in both memory kinds, and what a refused context creation leaves behind.

tae_stage_keyswitch, _pbs_shift_boolean, _bootstrap, _pfks_ggsw, _ggsw_fourier, _vertical_packing and tae_xor_batch go
through the staging scope every other entry point uses: a TAE_MEM_HOST call must return, word for word, what the
TAE_MEM_DEVICE call leaves in the caller's device arrays, zeros where a stage writes nothing; and a context whose
creation is refused after its keys reached the device must give all of its memory back.
"""
import ctypes as C

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N

pytestmark = pytest.mark.gpu

FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(torch, a):
    """A host array as a device tensor of the same words."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _words(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


def _both(torch, fn, ctx, ins, out_shape, out_dtype=np.uint64, post=()):
    """fn(ctx, *ins, out, *post, mem) on host arrays (the output pre-filled with ones) and on device tensors:
    (host output, device output).  An int in `ins` is passed as it is."""
    out = np.full(out_shape, FF, dtype=np.uint64).view(out_dtype)
    N.check(fn(ctx._h, *[_vp(a) if isinstance(a, np.ndarray) else a for a in ins], _vp(out), *post, N.TAE_MEM_HOST))
    d_ins = [_dev(torch, a) if isinstance(a, np.ndarray) else a for a in ins]
    d_out = torch.full(out_shape, -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    N.check(fn(ctx._h, *[_dp(a) if isinstance(a, torch.Tensor) else a for a in d_ins], _dp(d_out), *post, N.TAE_MEM_DEVICE))
    return out, _words(d_out, out_dtype)


def test_stage_calls_host_and_device_memory_agree(gpu_context, product_raw):
    """Count 3 through each stage (vertical packing: one group of 8 selector bits, 8 outputs), each stage fed with the
    host output of the one before, computed at count 8 for the vertical packing's sake."""
    torch = pytest.importorskip("torch")
    lib, ctx = N.lib(), gpu_context
    k, n_poly, n_small, cbs_l = 4, 512, 677, 1
    BIG, SMALL, GLWE = k * n_poly + 1, n_small + 1, (k + 1) * n_poly
    GGSW, GGSW_F = cbs_l * (k + 1) * GLWE, cbs_l * (k + 1) * (k + 1) * (n_poly // 2) * 2  # the latter in doubles
    bits = [1, 0, 1, 1, 0, 0, 1, 0]
    cts = product_raw[0].encrypt_bits_raw(bits, start_index=77_000)
    rng = np.random.default_rng(7)

    def same(got):
        host, dev = got
        assert host.shape == dev.shape and np.array_equal(host.view(np.uint64), dev.view(np.uint64))
        return host

    small = same(_both(torch, lib.tae_stage_keyswitch, ctx, [cts[:3], 3], (3, SMALL)))
    big = same(_both(torch, lib.tae_stage_pbs_shift_boolean, ctx, [small, 3, 1], (3, BIG)))
    lut_glwe = rng.integers(0, 1 << 63, size=GLWE, dtype=np.uint64)
    same(_both(torch, lib.tae_stage_bootstrap, ctx, [small, 3, lut_glwe], (3, BIG)))
    ggsw = same(_both(torch, lib.tae_stage_pfks_ggsw, ctx, [big, 3, 1], (3, GGSW)))
    same(_both(torch, lib.tae_stage_ggsw_fourier, ctx, [ggsw, 3], (3, GGSW_F), np.float64))

    # the eight Fourier GGSWs of one group, in host memory
    small8 = np.full((8, SMALL), FF)
    big8, ggsw8 = np.full((8, BIG), FF), np.full((8, GGSW), FF)
    gf8 = np.full((8, GGSW_F), FF).view(np.float64)
    N.check(lib.tae_stage_keyswitch(ctx._h, _vp(cts), 8, _vp(small8), N.TAE_MEM_HOST))
    N.check(lib.tae_stage_pbs_shift_boolean(ctx._h, _vp(small8), 8, 1, _vp(big8), N.TAE_MEM_HOST))
    N.check(lib.tae_stage_pfks_ggsw(ctx._h, _vp(big8), 8, 1, _vp(ggsw8), N.TAE_MEM_HOST))
    N.check(lib.tae_stage_ggsw_fourier(ctx._h, _vp(ggsw8), 8, _vp(gf8), N.TAE_MEM_HOST))
    assert np.array_equal(small8[:3], small) and np.array_equal(ggsw8[:3], ggsw)
    lut = rng.integers(0, 1 << 63, size=8 * n_poly, dtype=np.uint64)
    same(_both(torch, lib.tae_stage_vertical_packing, ctx, [gf8, 1, 8, lut, 8], (8, BIG)))

    # tae_xor_batch: lhs is read and written
    lhs, rhs = cts[:3].copy(), cts[3:6].copy()
    d_lhs, d_rhs = _dev(torch, lhs), _dev(torch, rhs)
    torch.cuda.synchronize()
    N.check(lib.tae_xor_batch(ctx._h, _vp(lhs), _vp(rhs), 3, None, None, None, N.TAE_MEM_HOST))
    N.check(lib.tae_xor_batch(ctx._h, _dp(d_lhs), _dp(d_rhs), 3, None, None, None, N.TAE_MEM_DEVICE))
    assert np.array_equal(lhs, cts[:3] + cts[3:6]) and np.array_equal(lhs, _words(d_lhs))
    assert np.array_equal(rhs, cts[3:6]) and np.array_equal(rhs, _words(d_rhs))


def test_pfks_ggsw_unwritten_rows_are_zero(gpu_context8):
    """tae_stage_pfks_ggsw writes the rows of its level only.  The 8-bit set has four levels: at level 2 a host caller
    gets zeros in the rows of levels 1, 3 and 4 whatever the array held, and in the rows of level 2 what the
    device-memory call writes."""
    torch = pytest.importorskip("torch")
    k, n_poly, cbs_l = 2, 1024, 4
    BIG, ROWS = k * n_poly + 1, (k + 1) * (k + 1) * n_poly
    big = np.random.default_rng(11).integers(0, 1 << 63, size=(2, BIG), dtype=np.uint64)
    host, dev = _both(torch, N.lib().tae_stage_pfks_ggsw, gpu_context8, [big, 2, 2], (2, cbs_l, ROWS))
    for lev in (1, 3, 4):
        assert not host[:, lev - 1].any(), lev
    assert host[:, 1].any() and np.array_equal(host[:, 1], dev[:, 1])


def test_refused_context_creation_holds_no_memory(gpu_context, product_raw, monkeypatch):
    """An unknown TAE_PFKS_GEMM is refused by the constructor's last step, after the keys, the Fourier bootstrapping
    key, the LUTs and the stream exist.  Four refusals in a row take less than one bootstrapping key of device memory
    (each used to keep its Fourier key, of the same size), and the next creation works."""
    torch = pytest.importorskip("torch")
    ps = tfhe_aes.PARAMS_SQRD_LVL_64
    client, keys = product_raw
    key_bytes = 8 * tfhe_aes.server_key_sizes(ps)[1]
    ptrs = [np.ascontiguousarray(a).ctypes.data_as(C.c_void_p) for a in keys]
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    monkeypatch.setenv("TAE_PFKS_GEMM", "nonsense")
    for _ in range(4):
        h = C.c_void_p()
        rc = N.lib().tae_context_create_raw(ps, 0, ptrs[0], ptrs[1], ptrs[2], N.TAE_MEM_HOST, C.byref(h))
        assert rc != 0 and not h.value
    free_after = torch.cuda.mem_get_info()[0]
    assert free_before - free_after < key_bytes, (free_before, free_after, key_bytes)
    monkeypatch.delenv("TAE_PFKS_GEMM")
    fresh = tfhe_aes.context_from_raw(ps, keys, device=0)
    ct = client.encrypt_bits_raw([1], start_index=78_000)
    outs = []
    for ctx in (fresh, gpu_context):
        out = np.full((1, 678), FF)
        N.check(N.lib().tae_stage_keyswitch(ctx._h, _vp(ct), 1, _vp(out), N.TAE_MEM_HOST))
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], np.full((1, 678), FF))
