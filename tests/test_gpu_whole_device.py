"""Whole-device batches: every output row of every hot kernel, word for word against the oracle.

The other parity tests run the blind rotations and the keyswitch GEMM on a handful of workgroups, and the tests
at the measured shapes (test_gpu_batch.py) compare two or three blocks with the oracle and only decrypt the rest.
Here each kernel gets a batch that fills the card more than twice over, assembled from a few distinct rows
(tests/tiled_batches.py: D oracle calls, B compared positions), and `compare` leaves no position out.  Each call
is made twice on the same context: the second launch runs on warm scratch, and both must equal the references.

Sizing rule.  A kernel with C rows per workgroup and a launch-bounds occupancy of O workgroups per CU gets more
than 2 O CU workgroups, the last one partial (one row).  A kernel that Engine::bootstrap only ever runs at one
workgroup per CU gets exactly that.  Sizes for CU = 256 (tiled_batches.sizes derives them from the device's CU
count; test_tiled_batches.py pins this table):

  case        kernel                          C  O  positions                          workgroups
  br512x4     br512x4<3, true, 12>            3  1  7 CU + 1 = 1793 ciphertexts        598, the last of two
  br512p16    br512p16<3, 12>                 2  1  5 CU + 1 = 1281                    641, the last of one
  br512lat    br512lat<3, 12>                 1  1  min(CU, TAE_BR_LAT_MAX) = 256      256
  br512split  br512x4 + br512lat              3  1  6 CU + 5 = 1541                    512 + 5
  br1024lat   br1024lat                       1  1  CU = 256                           256
  br1024      br1024, two per workgroup       2  1  4 CU - 1 = 1023                    512, the last of one
  br1024w     br1024w<6, 7>                   4  3  24 CU + 1 = 6145                   1537, the last of one
  br1024_nowide  the same, TAE_B1K_WIDE=0     2  1  4 CU + 1 = 1025                    513, the last of one
  br1024_one_paired / _unpaired  TAE_B1K_LAT=0  1  1  CU = 256                         256
  br1024_occ2  br1024, TAE_B1K_OCC2=1         1  2  4 CU + 1 = 1025                    1025
  s1          br512x4<7, true, 6>             3  1  7 CU + 1 = 1793                    598, the last of two
  ks64        gemm<1, 8>, n + 1 = 678       128  2  25 x 128 + 1 = 3201 rows           26 x 43 = 1118
  ks8         gemm<1, 8>, n + 1 = 786       128  2  22 x 128 + 1 = 2817 rows           23 x 50 = 1150
  vp64        br512x4<1, false, 13>, 24 out   3  1  65 groups, 1560 outputs            520
  vp8         br1024 (vertical packing), 8    2  1  129 groups, 1032 outputs           516
  cbs         tae_circuit_bootstrap_raw 8->24       300 groups: 2400 bootstraps (3 br512x4 rounds + 96 on
                                                    br512lat), 7 K-layout PFKS m-tiles, 7200 outputs
  aes         encrypt_blocks_raw, 2 rounds          128 blocks from three: 16384 bootstraps per launch

br1024 with two ciphertexts per workgroup is selected for CU < B < 4 CU only (from 4 CU on the batch goes to
br1024w), so 2 CU workgroups is the most the default selection gives it; br1024_nowide runs it at the rule's
size on a context of its own.  The vertical packing's output counts
(24 and 8) are whole workgroups; its ragged workgroups are test_gpu_vp_edges.py's.  The keyswitch takes two
m-tiles more than the smallest grid above 2 x 2 x CU.

Where the Engine reports which kernel ran, the test asserts it: pbs_main_cts (the ciphertexts the throughput
kernel took) with timing on, and last_pfks_kernel.  The 8-bit selection has no such report; its cases run on the
default context and refuse to run with a TAE_B1K_* variable set.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests import edge_inputs as E
from tests import tiled_batches as T
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
P64 = tfhe_aes.PARAMS_SQRD_LVL_64
P8 = tfhe_aes.PARAMS_WOPPBS_8BIT
SHIFT_ADD = 1 << 62  # homomorphic_shift_boolean adds 2^62 to the body before the modulus switch
# kernel selections of contexts built for one case (environment read by context_from_raw; every variable of the
# family is set, then restored)
P16_ENV = {"TAE_BR_LAT_MAX": "256", "TAE_PBS_KERNEL": "p16"}


def _b1k(lat="1", pair="1", occ2="0", wide="1"):
    return {"TAE_B1K_LAT": lat, "TAE_B1K_PAIR": pair, "TAE_B1K_OCC2": occ2, "TAE_B1K_WIDE": wide}


def _context(pid, keys, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tfhe_aes.context_from_raw(pid, keys, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


AES = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
BYTES7 = (0x53, 0x00, 0xFF, 0xA7, 0x1C, 0xE2, 0x48)
SELECTION_VARS = ("TAE_BR_LAT_MAX", "TAE_PBS_KERNEL", "TAE_B1K_LAT", "TAE_B1K_PAIR", "TAE_B1K_OCC2", "TAE_B1K_WIDE",
                  "TAE_PFKS_GEMM", "TAE_PFKS_LAYOUT")


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def default_selection():
    """The session contexts select their kernels by default: no selection variable is set."""
    assert not [v for v in SELECTION_VARS if v in os.environ], "run with the default kernel selection"


def _dev(torch, a):
    """A host array as a device tensor of the same words."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _out(torch, shape):
    out = torch.full(shape, -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return out


def _tiling(cu, case):
    B, D, seed, window = T.sizes(cu)[case]
    return B, D, T.tiling(B, D, seed, window)


def _twice(call, refs, src, rows_per_wg, what, ref_of=None):
    """Two calls on the same context, each into a fresh output: both equal the references at every position."""
    for k in (1, 2):
        T.compare(call(), refs, src, rows_per_wg, "%s, call %d" % (what, k), ref_of)


def _pmap(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


def _bits_of(byte_values):
    return [b for v in byte_values for b in aes_128.u8_to_bits(v)]


# ---- tae_stage_pbs_shift_boolean, params_sqrd_lvl_64 ---------------------------------------------------------------
@pytest.fixture(scope="module")
def pbs64(torch, product_raw, oracle_keys):
    """D = 17: the ten crafted rows of edge_inputs.crafted_small (rotation amounts 0, N, 2N, the rounding boundary,
    zeroed mask words) and seven real keyswitched ciphertexts; the level-1 references, on the device."""
    cts = product_raw[0].encrypt_bits_raw(np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], dtype=np.uint8), start_index=1_310_000)
    real = np.stack([oracle_keys.keyswitch(c) for c in cts])
    rows = np.concatenate([E.crafted_small(677, 512, real[:3], SHIFT_ADD), real[3:]])
    assert len(rows) == 17 and len({r.tobytes() for r in rows}) == 17
    refs = _pmap(lambda r: oracle_keys.homomorphic_shift_boolean(r, 1), rows)
    return _dev(torch, rows), _dev(torch, np.stack(refs))


def _shift_twice(torch, ctx, d_rows, d_refs, src, level, rows_per_wg, what, main_cts=None):
    B, big_len = len(src), d_refs.shape[1]
    d_in = T.expand(d_rows, src)

    def call():
        d_out = _out(torch, (B, big_len))
        N.check(N.lib().tae_stage_pbs_shift_boolean(ctx._h, _dp(d_in), B, level, _dp(d_out), N.TAE_MEM_DEVICE))
        if main_cts is not None:
            assert ctx.last_stage_times()["pbs_main_cts"] == main_cts, (what, ctx.last_stage_times(), main_cts)
        return d_out

    ctx.set_timing(main_cts is not None)
    try:
        _twice(call, d_refs, src, rows_per_wg, what)
    finally:
        ctx.set_timing(False)


def test_pbs_br512x4(torch, cu, default_selection, gpu_context, pbs64):
    """More than two rounds of br512x4 workgroups, the last one of two ciphertexts; the remainder CU + 1 is above
    min(TAE_BR_LAT_MAX, CU), so nothing goes to br512lat."""
    B, _, src = _tiling(cu, "br512x4")
    _shift_twice(torch, gpu_context, *pbs64, src, 1, 3, "br512x4", main_cts=B)


def test_pbs_br512p16(torch, cu, product_raw, pbs64):
    B, _, src = _tiling(cu, "br512p16")
    ctx = _context(P64, product_raw[1], P16_ENV)
    _shift_twice(torch, ctx, *pbs64, src, 1, 2, "br512p16", main_cts=B)
    del ctx


def test_pbs_br512lat(torch, cu, default_selection, gpu_context, pbs64):
    """One workgroup on every CU (at most TAE_BR_LAT_MAX): the throughput kernel takes nothing."""
    _, _, src = _tiling(cu, "br512lat")
    _shift_twice(torch, gpu_context, *pbs64, src, 1, 1, "br512lat", main_cts=0)


def test_pbs_br512x4_split(torch, cu, default_selection, gpu_context, pbs64):
    """Two whole rounds on br512x4, the last five rows on br512lat, reading and writing at an offset of 6 CU rows."""
    _, _, src = _tiling(cu, "br512split")
    _shift_twice(torch, gpu_context, *pbs64, src, 1, 3, "br512x4 + br512lat", main_cts=6 * cu)


# ---- tae_stage_pbs_shift_boolean, the 8-bit set --------------------------------------------------------------------
@pytest.fixture(scope="module")
def pbs8(torch, product_raw8, oracle_keys8):
    bits = np.array([1, 0, 1, 0, 0, 1, 1, 1, 0, 1], dtype=np.uint8)
    real = product_raw8[0].encrypt_bits_raw(bits, start_index=1_320_000)
    rows = np.concatenate([E.crafted_small(785, 1024, real[:3], SHIFT_ADD), real[3:]])
    assert len(rows) == 17 and len({r.tobytes() for r in rows}) == 17
    refs = _pmap(lambda r: oracle_keys8.homomorphic_shift_boolean(r, 2), rows)
    return _dev(torch, rows), _dev(torch, np.stack(refs))


@pytest.mark.parametrize("case,rows_per_wg", [("br1024lat", 1), ("br1024", 2), ("br1024w", 4)])
def test_pbs_8bit(torch, cu, default_selection, gpu_context8, pbs8, case, rows_per_wg):
    """CBS level 2 on the default selection: br1024lat up to CU ciphertexts, br1024 with two per workgroup below
    4 CU, br1024w from there on -- the stash slice of every ciphertext beyond a workgroup's first lies far from
    index 0, at three workgroups per CU."""
    B, _, src = _tiling(cu, case)
    assert {"br1024lat": B <= cu, "br1024": cu < B < 4 * cu, "br1024w": B >= 4 * cu}[case]
    _shift_twice(torch, gpu_context8, *pbs8, src, 2, rows_per_wg, case)


# case -> (environment of its context, rows per workgroup)
B1K_KNOBS = {"br1024_nowide": (_b1k(wide="0"), 2), "br1024_one_paired": (_b1k(lat="0"), 1),
             "br1024_one_unpaired": (_b1k(lat="0", pair="0"), 1), "br1024_occ2": (_b1k(occ2="1"), 1)}


@pytest.mark.parametrize("case", list(B1K_KNOBS))
def test_pbs_8bit_knob_selections(torch, cu, product_raw8, pbs8, case):
    """The N = 1024 forms the default selection does not reach at these sizes, each on a context of its own:
    br1024 with two ciphertexts per workgroup at the size the rule asks for (TAE_B1K_WIDE=0: more than 2 CU
    workgroups, the last of one; by default that batch goes to br1024w), the one-per-workgroup forms on every CU
    (TAE_B1K_LAT=0, two levels per pass and one), and one per workgroup at two workgroups per CU on more than
    2 x 2 x CU workgroups (TAE_B1K_OCC2=1)."""
    env, rows_per_wg = B1K_KNOBS[case]
    B, _, src = _tiling(cu, case)
    assert {"br1024_nowide": (B + 1) // 2 > 2 * cu and B % 2 == 1, "br1024_one_paired": B == cu,
            "br1024_one_unpaired": B == cu, "br1024_occ2": B > 4 * cu}[case]
    ctx = _context(P8, product_raw8[1], env)
    _shift_twice(torch, ctx, *pbs8, src, 2, rows_per_wg, case)
    del ctx


# ---- tae_s1_bootstrap, shortint_1bit ---------------------------------------------------------------------------------
def test_s1_bootstrap_two_test_vectors(torch, cu, oracle_mod):
    """br512x4<7, true, 6> with lut_mod = 2: position i takes test vector i % 2, so its reference is the oracle's
    FheContext::bootstrap of (source, i % 2): 2 D references."""
    P5 = tfhe_aes.PARAMS_SHORTINT_1BIT
    ck, keys = tfhe_aes.generate_keys_raw(P5, SEED, threads=THREADS)
    ctx = tfhe_aes.context_from_raw(P5, keys, device=0)
    ok = oracle_mod.S1Keys(None, raw=keys)
    real = ck.encrypt_bits_raw([0, 1, 1, 0, 1, 0, 0, 1, 1, 0], start_index=1_330_000)
    rows = np.concatenate([E.crafted_small(ok.p["n"], ok.p["N"], real[:3], 0), real[3:]])
    tvs = np.stack([ok.tv_from_fn(1, 0), ok.tv_from_fn(0, 1)])
    B, D, src = _tiling(cu, "s1")
    assert len(rows) == D and len({r.tobytes() for r in rows}) == D
    refs = _pmap(lambda st: ok.bootstrap(rows[st // 2], tvs[st % 2]), range(2 * D))
    d_refs, d_in = _dev(torch, np.stack(refs)), T.expand(_dev(torch, rows), src)
    ref_of = 2 * src + np.arange(B) % 2

    def call():
        d_out = _out(torch, (B, ok.L))
        N.check(N.lib().tae_s1_bootstrap(ctx._h, _dp(d_in), B, tvs.ctypes.data_as(C.c_void_p), 2, _dp(d_out),
                                         N.TAE_MEM_DEVICE))
        return d_out

    _twice(call, d_refs, src, 3, "br512x4<7, true, 6>", ref_of)
    del ctx


# ---- tae_stage_keyswitch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lvl64", "8bit"])
def test_keyswitch(request, torch, cu, default_selection, which):
    """gemm<1, 8> on more than 2 x 2 x CU tiles, the last m-tile of one row; every row against Keys.keyswitch of its
    source (seven real ciphertexts under the big key)."""
    sfx = "" if which == "lvl64" else "8"
    ctx, ok = request.getfixturevalue("gpu_context" + sfx), request.getfixturevalue("oracle_keys" + sfx)
    client = request.getfixturevalue("product_raw" + sfx)[0]
    B, D, src = _tiling(cu, "ks64" if which == "lvl64" else "ks8")
    if which == "lvl64":
        rows = client.encrypt_bits_raw(np.arange(D) & 1, start_index=1_340_000)
    else:
        rows = client.encrypt_ints_raw(np.arange(D) * 37 & 0xFF, start_index=1_340_000)
    assert rows.shape == (D, ok.K + 1)
    n_small = ok.p["n"] + 1
    assert (B + 127) // 128 * ((n_small * 8 + 127) // 128) > 4 * cu and B % 128 == 1
    d_refs = _dev(torch, np.stack(_pmap(ok.keyswitch, rows)))
    d_in = T.expand(_dev(torch, rows), src)

    def call():
        d_out = _out(torch, (B, n_small))
        N.check(N.lib().tae_stage_keyswitch(ctx._h, _dp(d_in), B, _dp(d_out), N.TAE_MEM_DEVICE))
        return d_out

    _twice(call, d_refs, src, 128, "gemm<1, 8> " + which)


# ---- tae_stage_vertical_packing ----------------------------------------------------------------------------------------
def _fourier_ggsws(torch, ctx, p, cts, keyswitch):
    """The Fourier GGSWs of `cts` through the stage calls, in device memory: [len(cts)][cbs_l (k+1)^2 N] doubles."""
    lib, n = N.lib(), len(cts)
    k, Np, levels = p["k"], p["N"], p["cbs_l"]
    glwe = (k + 1) * Np
    d_small = _dev(torch, cts)
    if keyswitch:
        d_big_in, d_small = d_small, _out(torch, (n, p["n"] + 1))
        N.check(lib.tae_stage_keyswitch(ctx._h, _dp(d_big_in), n, _dp(d_small), N.TAE_MEM_DEVICE))
    d_big = _out(torch, (n, k * Np + 1))
    d_ggsw = torch.zeros((n, levels * (k + 1) * glwe), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for level in range(1, levels + 1):
        N.check(lib.tae_stage_pbs_shift_boolean(ctx._h, _dp(d_small), n, level, _dp(d_big), N.TAE_MEM_DEVICE))
        N.check(lib.tae_stage_pfks_ggsw(ctx._h, _dp(d_big), n, level, _dp(d_ggsw), N.TAE_MEM_DEVICE))
    d_gf = torch.zeros((n, levels * (k + 1) * (k + 1) * Np), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    N.check(lib.tae_stage_ggsw_fourier(ctx._h, _dp(d_ggsw), n, _dp(d_gf), N.TAE_MEM_DEVICE))
    return d_gf


@pytest.mark.parametrize("which,n_out,rows_per_wg", [("lvl64", 24, 3), ("8bit", 8, 2)])
def test_vertical_packing(request, torch, cu, default_selection, which, n_out, rows_per_wg):
    """Groups of 8 selector GGSWs, the Fourier GGSWs of seven real bytes made with the stage calls; a LUT of random
    words; every output of every group against Keys.vertical_packing of its source group."""
    sfx = "" if which == "lvl64" else "8"
    ctx, ok = request.getfixturevalue("gpu_context" + sfx), request.getfixturevalue("oracle_keys" + sfx)
    client = request.getfixturevalue("product_raw" + sfx)[0]
    G, D, src = _tiling(cu, "vp64" if which == "lvl64" else "vp8")
    assert G * (n_out // rows_per_wg) > 2 * cu and len(BYTES7) == D
    Np, big_len = ok.p["N"], ok.K + 1
    cts = client.encrypt_bits_raw(_bits_of(BYTES7), start_index=1_350_000)  # big-key bits, or small-key bits (8-bit)
    d_gf = _fourier_ggsws(torch, ctx, ok.p, cts, keyswitch=which == "lvl64").reshape(D, -1)
    gf = d_gf.cpu().numpy().view(np.complex128)
    lut = E.random_words(np.random.default_rng(1350 + n_out), n_out * Np)
    refs = _pmap(lambda gj: ok.vertical_packing(lut[gj % n_out * Np:(gj % n_out + 1) * Np], gf[gj // n_out], 8),
                 range(D * n_out))
    d_refs, d_lut, d_in = _dev(torch, np.stack(refs)), _dev(torch, lut), T.expand(d_gf, src)
    row_src = np.repeat(src, n_out)
    ref_of = row_src * n_out + np.tile(np.arange(n_out), G)

    def call():
        d_out = _out(torch, (G * n_out, big_len))
        N.check(N.lib().tae_stage_vertical_packing(ctx._h, _dp(d_in), G, 8, _dp(d_lut), n_out, _dp(d_out),
                                                   N.TAE_MEM_DEVICE))
        return d_out

    _twice(call, d_refs, row_src, rows_per_wg, "vertical packing " + which, ref_of)


# ---- tae_circuit_bootstrap_raw -----------------------------------------------------------------------------------------
def test_circuit_bootstrap_300_groups(torch, cu, default_selection, gpu_context, oracle_keys, product_raw, golden):
    """8 -> 24 (SBOX, 2S', 3S') over 300 groups tiled from seven: 2400 bootstraps (whole br512x4 rounds plus a
    br512lat remainder inside the Engine's own sequence), the K-layout PFKS GEMM at 7 m-tiles, ggsw_to_fourier and
    the vertical packing at 300 groups; every output against the oracle's circuit bootstrap of its source group."""
    q = golden["sbox_galmul_quirk"]
    lut = gpu_context.generate_lookup_table(
        8, 24, lambda x: (q[f"{x:02x}"][0] << 16) | (q[f"{x:02x}"][1] << 8) | q[f"{x:02x}"][2])
    lut_arr = lut.as_array()
    G, D, src = _tiling(cu, "cbs")
    big_len = oracle_keys.K + 1
    cts = product_raw[0].encrypt_bits_raw(_bits_of(BYTES7), start_index=1_360_000).reshape(D, 8, big_len)
    d_refs = _dev(torch, np.stack(_pmap(lambda c: oracle_keys.circuit_bootstrap(c, lut_arr, 24), cts))).reshape(D * 24, -1)
    d_in = T.expand(_dev(torch, cts), src)
    row_src = np.repeat(src, 24)
    ref_of = row_src * 24 + np.tile(np.arange(24), G)
    rest = 8 * G % (3 * cu)
    main_cts = 8 * G - rest if (8 * G > 3 * cu and 0 < rest <= min(T.BR_LAT_MAX, cu)) else 8 * G

    def call():
        d_out = _out(torch, (G * 24, big_len))
        N.check(N.lib().tae_circuit_bootstrap_raw(gpu_context._h, _dp(d_in), G, 8, lut._h, _dp(d_out), N.TAE_MEM_DEVICE))
        t = gpu_context.last_stage_times()
        assert t["pbs_launches"] == 1 and t["pbs_main_cts"] == main_cts, (t, main_cts)
        assert gpu_context.last_pfks_kernel() == "w16"
        return d_out

    gpu_context.set_timing(True)
    try:
        _twice(call, d_refs, row_src, 3, "circuit bootstrap 8 -> 24", ref_of)
    finally:
        gpu_context.set_timing(False)


# ---- encrypt_blocks_raw ------------------------------------------------------------------------------------------------
def test_aes_128_blocks_two_rounds_every_block(torch, cu, default_selection, gpu_context, oracle_keys, product_raw, golden):
    """The measured shape (test_gpu_batch.py: 128 blocks, every CBS launch 16384 bootstraps), with the 128 block
    ciphertexts tiled from three distinct counter blocks (neighbouring blocks differ): all 128 output blocks equal
    the oracle's aes_encrypt_block of their source, and with them the linear-layer kernels at every block index."""
    g = golden["readme_ctr"]
    key, iv = bytes.fromhex(g["key"]), bytes.fromhex(g["iv"])
    client = product_raw[0]
    ek = b"".join(aes_128.key_schedule_plain(key))
    rk = client.encrypt_bits_raw(_bits_of(ek), start_index=1_370_000)
    nb, D, src = _tiling(cu, "aes")
    big_len = oracle_keys.K + 1
    blocks = aes_128.counter_blocks(iv, D)
    cts = client.encrypt_bits_raw(aes_128.blocks_to_bits(blocks), start_index=1_380_000).reshape(D, 128, big_len)
    refs = [oracle_keys.aes_encrypt_block(rk, cts[b], 2, threads=16) for b in range(D)]
    for b in range(D):
        assert aes_128.bits_to_blocks(client.decrypt_bits_raw(refs[b])) == aes_128.expand_key_and_encrypt_blocks(
            key, blocks[b:b + 1], 2)
    d_refs, d_rk, d_in = _dev(torch, np.stack(refs)), _dev(torch, rk), T.expand(_dev(torch, cts), src)

    def call():
        d_out = _out(torch, (nb, 128, big_len))
        AES.encrypt_blocks_device(gpu_context, d_rk.data_ptr(), d_in.data_ptr(), nb, 2, d_out.data_ptr())
        gpu_context.synchronize()
        return d_out

    _twice(call, d_refs, src, 1, "encrypt_blocks_raw, 128 blocks, 2 rounds")
