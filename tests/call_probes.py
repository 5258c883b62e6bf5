"""Probes for tests/test_gpu_call_order.py: one small deterministic call per Engine entry point, the scratch buffers
each one walks (USES, kept honest by tests/test_call_probes_table.py) and the sequence that runs every ordered pair of
probes sharing a buffer back to back.

A probe is `run(ctx, inputs) -> tuple of uint64 arrays` plus `check(inputs, outs)`, which decodes the outputs with the
client key and compares them with the plain model, so that "equal to the cold result" cannot mean "equally wrong".
The inputs are fresh encryptions of plain values at fixed start indices, built once (`build_inputs`, host only); the
stage probes take each other's outputs, made once by `build_stage_chain` on a context of its own.  Where a family has a
small and a large probe the large one grows what the small one left and takes the other blind rotation (lvl_64:
br512lat up to 256 bits of a launch, br512x4 above).

This module imports nothing that needs a GPU: USES, the probe list and the sequence are read on any machine.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_multi, aes_var
from tfhe_aes import shortint_1bit as S1
from tests import gcm_ref as R

BIG = 4 * 512 + 1
SMALL = 678
U64 = np.uint64
E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
A8 = aes_128.ShortintWoppbs8BitSboxPbsAesEncrypt
V = aes_var.GalMulAes
M = aes_multi.GalMulAesMulti
LVL64, W8, S1BIT = "lvl64", "w8", "s1"
PARAM_SETS = {LVL64: tfhe_aes.PARAMS_SQRD_LVL_64, W8: tfhe_aes.PARAMS_WOPPBS_8BIT, S1BIT: tfhe_aes.PARAMS_SHORTINT_1BIT}

Probe = namedtuple("Probe", "name params family size run check")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts.reshape(-1, cts.shape[-1])).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _word_bits(value, n):
    return [(value >> (n - 1 - j)) & 1 for j in range(n)]


# ---- plain data --------------------------------------------------------------------------------------------------
KEYS = (bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), bytes(range(0x10, 0x20)), bytes((7 * i + 1) & 255 for i in range(16)))
KEY256 = bytes(range(0x60, 0x80))
EK = [aes_var.key_schedule_plain(k) for k in KEYS]
IV8, IV8B = bytes.fromhex("bdd219b8a08ded1a"), bytes(range(0x70, 0x78))
IV16 = bytes(range(0xA0, 0xB0))
BLOCKS = [bytes((29 * i + 16 * b + 3) & 255 for i in range(16)) for b in range(3)]
XTS_UNIT, XTS_UNIT_B = 0x3333333333, 7
XTS_UNITS = [(XTS_UNIT, bytes((29 * i + 5) & 255 for i in range(32))), (XTS_UNIT_B, bytes((13 * i + 1) & 255 for i in range(16)), 127)]
XTS_MASK_UNIT_OF, XTS_MASK_INDEX = [0, 1, 0], [0, 1, 127]
CBS_G2, CBS_G40 = [0x53, 0xA7], [(37 * i + 11) & 255 for i in range(40)]
ID5 = [1, 0, 1, 1, 0]
STAGE_BITS = [1, 0, 1, 1, 0, 1]
PACK_BITS = [int(b) for b in np.random.default_rng(513).integers(0, 2, size=513)]
INTS8, BYTES8 = [0b10110101, 0x01, 0x80, 0xFF, 0x00], [0b10110101, 0x00, 0xFC]
S1_BITS5, S1_PKS_BITS = [0, 1, 1, 0, 1], [0, 1]
S1_TABLES3 = [[1, 0, 0, 1, 0, 1, 1, 0], [0, 0, 0, 1, 0, 1, 1, 1]]
S1_VALS3, S1_VALS8 = [0b011, 0b110, 0b101, 0b000], [0b11001001, 0b01001001, 0b00101010]


def galois(x):
    s = aes_128.SBOX[x]
    return (aes_128.gf_256_mul(s, 1) << 16) | (aes_128.gf_256_mul(s, 2) << 8) | aes_128.gf_256_mul(s, 3)


def stage_lut(x):
    return (5 * x + 3) & 7


def _ctr_plain(ek, iv, first, data, rounds):
    ks = b"".join(aes_var.encrypt_block_plain(ek, b, rounds)
                  for b in aes_128.counter_blocks(iv, (len(data) + 15) // 16, first=first))
    return _xor(data, ks)


def _cbc_plain(ek, iv, data, rounds):
    out, prev = [], iv
    for i in range(0, len(data), 16):
        out.append(_xor(aes_var.decrypt_block_plain(ek, data[i:i + 16], rounds), prev))
        prev = data[i:i + 16]
    return b"".join(out)


def _xts_masks_plain(ek2, rounds, units_and_indices):
    out = []
    for unit, j in units_and_indices:
        t = aes_var.encrypt_block_plain(ek2, aes_var._xts_tweak16(unit), rounds)
        for _ in range(j):
            t = aes_var.xts_alpha(t)
        out.append(t)
    return out


CCM_PAIR_PLAIN = [(1, bytes(range(0x10, 0x1D)), b"", bytes((7 * i + 3) & 255 for i in range(17))),     # 3 MAC blocks
                  (0, bytes(range(0x30, 0x37)), bytes(range(8)), bytes((11 * i + 1) & 255 for i in range(23)))]  # 4
CCM_SINGLE_PLAIN = (1, bytes(range(0x10, 0x1D)), bytes(range(5)), bytes((5 * i + 9) & 255 for i in range(40)))
CCM_TAG = 8
GCM_IV_B = bytes(range(0x20, 0x2C))
GCM_ONE_PLAIN = [(R.IV3, bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20)))]  # tag 12: 96 tag rows
GCM_RAGGED_PLAIN = [(R.IV3, b"", b""), (GCM_IV_B, bytes(range(15)), b""),
                    (R.IV3[::-1], b"", bytes((7 * i + 3) & 255 for i in range(17)))]  # tag 4, three frames: 96 rows
GCM_KEY, GCM_POWERS = R.KEY3, 4
GF_A = [bytes((37 * i + 5) & 255 for i in range(16)), bytes([1]) + bytes(14) + bytes([1])]
GF_B = bytes((53 * i + 201) & 255 for i in range(16))


def _ccm_frames(plain):
    return [(slot, nonce, aad, aes_var.ccm_encrypt_plain(KEYS[slot], nonce, aad, pt, CCM_TAG, rounds=2))
            for slot, nonce, aad, pt in plain]


def _gcm_frames(plain, tag_len):
    return [(iv, aad, aes_var.gcm_encrypt_plain(GCM_KEY, iv, aad, pt, tag_len, rounds=2)) for iv, aad, pt in plain]


# ---- inputs ------------------------------------------------------------------------------------------------------
def wide8_blocks(cus):
    """The 8-bit model's block count whose SubBytes launch has four ciphertexts per CU: br1024w's threshold."""
    return max(2, (4 * cus + 127) // 128)


def build_inputs(client, client8, client1, cus):
    """Everything the probes read, from the three client keys (host only).  Each array has an index range of its own."""
    at = [40_000_000]

    def enc(ck, bits):
        bits = list(bits)
        out = ck.encrypt_bits_raw(bits, start_index=at[0])
        at[0] += 100_000
        return out

    x = {"client": client, "client8": client8, "client1": client1}
    x["rk"] = [enc(client, _bits(b"".join(ek))) for ek in EK]
    x["table"] = np.stack(x["rk"])
    x["dk"] = enc(client, _bits(b"".join(aes_var.decrypt_key_plain(EK[0]))))
    x["keys"] = np.stack([enc(client, _bits(k)) for k in KEYS])
    x["key256"] = enc(client, _bits(KEY256))
    x["blocks"] = enc(client, _bits(b"".join(BLOCKS))).reshape(3, 128, BIG)
    x["cbs2"] = enc(client, _bits(bytes(CBS_G2))).reshape(2, 8, BIG)
    x["cbs40"] = enc(client, _bits(bytes(CBS_G40))).reshape(40, 8, BIG)
    x["id5"] = enc(client, ID5).reshape(5, 1, BIG)
    x["stage_in"] = enc(client, STAGE_BITS)
    x["ctr21"] = _ctr_plain(EK[0], IV8, 0xFE, bytes((53 * i + 7) & 255 for i in range(21)), 1)
    x["ctr37"] = _ctr_plain(EK[0], IV8, 0xFE, bytes((37 * i + 11) & 255 for i in range(37)), 2)
    x["cbc48"] = bytes((91 * i + 17) & 255 for i in range(48))
    x["mk_streams"] = [(1, IV8, 0xFE, bytes((19 * i + 2) & 255 for i in range(21))),
                       (0, IV8B, 5, bytes((23 * i + 4) & 255 for i in range(16)))]
    t_plain = _xts_masks_plain(EK[1], 2, [(XTS_UNIT, 0), (XTS_UNIT_B, 0)])
    x["xts_tweak_cts"] = enc(client, _bits(b"".join(t_plain))).reshape(2, 128, BIG)
    x["ccm_pair"], x["ccm_single"] = _ccm_frames(CCM_PAIR_PLAIN), _ccm_frames([CCM_SINGLE_PLAIN])[0]
    ek_g = aes_var.key_schedule_plain(GCM_KEY)
    x["gcm_rk"] = enc(client, _bits(b"".join(ek_g)))
    h = aes_var.encrypt_block_plain(ek_g, bytes(16), 2)
    powers, p = [], h
    for _ in range(GCM_POWERS):
        powers.append(p)
        p = R.mul(p, h)
    x["gcm_h"] = powers
    x["gcm_hk"] = np.stack([enc(client, _bits(q)) for q in powers])
    x["gcm_one"], x["gcm_ragged"] = _gcm_frames(GCM_ONE_PLAIN, 12), _gcm_frames(GCM_RAGGED_PLAIN, 4)
    x["gf_a"] = np.stack([enc(client, _bits(a)) for a in GF_A])
    x["gf_b"] = enc(client, _bits(GF_B))[None]
    x["pack_rows"] = enc(client, PACK_BITS)
    x["packed"] = client.encrypt_packed(PACK_BITS, start_index=77_000)
    # 8-bit model: bits under the small key
    x["rk8"] = enc(client8, _bits(b"".join(EK[0])))
    nb8 = wide8_blocks(cus)
    x["blocks8_plain"] = [bytes((17 * i + j) & 255 for j in range(16)) for i in range(nb8)]
    x["blocks8"] = enc(client8, _bits(b"".join(x["blocks8_plain"]))).reshape(nb8, 128, -1)
    x["ints8"] = client8.encrypt_ints_raw(INTS8, start_index=78_000)
    x["bytes8"] = enc(client8, _bits(bytes(BYTES8))).reshape(3, 8, -1)
    # shortint_1bit
    x["s1_bits5"] = enc(client1, S1_BITS5)
    x["s1_pks"] = enc(client1, S1_PKS_BITS)
    x["s1_mv3"] = enc(client1, [b for v in S1_VALS3 for b in _word_bits(v, 3)]).reshape(4, 3, -1)
    x["s1_mv8"] = enc(client1, [b for v in S1_VALS8 for b in _word_bits(v, 8)]).reshape(3, 8, -1)
    return x


def _stage(fn, *args):
    N.check(fn(*args))


def stage_lut_glwe():
    """A trivial GLWE whose body is 2^62 everywhere: a bootstrap gives +2^62 for a phase in [0, 1/2), -2^62 above."""
    glwe = np.zeros(5 * 512, dtype=U64)
    glwe[4 * 512:] = U64(1) << U64(62)
    return glwe


def build_stage_chain(ctx, x):
    """The stage probes' inputs: each stage's output on the six ciphertexts, in pipeline order, on `ctx`."""
    for p in PROBES:
        if p.family == "stage":
            x["stage_" + p.name] = p.run(ctx, x)[0]


# ---- the probes ---------------------------------------------------------------------------------------------------
def _stage_ks(ctx, x):
    out = np.zeros((6, SMALL), dtype=U64)
    _stage(N.lib().tae_stage_keyswitch, ctx._h, _vp(x["stage_in"]), 6, _vp(out), N.TAE_MEM_HOST)
    return (out,)


def _stage_pbs(ctx, x):
    out = np.zeros((6, BIG), dtype=U64)
    _stage(N.lib().tae_stage_pbs_shift_boolean, ctx._h, _vp(x["stage_stage_ks"]), 6, 1, _vp(out), N.TAE_MEM_HOST)
    return (out,)


def _stage_boot(ctx, x):
    small = x["stage_stage_ks"].copy()
    small[:, -1] += U64(1) << U64(62)  # phases 1/4 and 3/4: away from the sign change of the test vector
    out = np.zeros((6, BIG), dtype=U64)
    _stage(N.lib().tae_stage_bootstrap, ctx._h, _vp(small), 6, _vp(stage_lut_glwe()), _vp(out), N.TAE_MEM_HOST)
    return (out,)


def _stage_pfks(ctx, x):
    out = np.zeros((6, 1, 5, 5 * 512), dtype=U64)
    _stage(N.lib().tae_stage_pfks_ggsw, ctx._h, _vp(x["stage_stage_pbs"]), 6, 1, _vp(out), N.TAE_MEM_HOST)
    return (out,)


def _stage_fft(ctx, x):
    out = np.zeros(6 * 5 * 5 * 256 * 2, dtype=np.float64)
    _stage(N.lib().tae_stage_ggsw_fourier, ctx._h, _vp(x["stage_stage_pfks"]), 6, _vp(out), N.TAE_MEM_HOST)
    return (out.view(U64),)


def _stage_vp(ctx, x):
    lut = ctx.generate_lookup_table(6, 3, stage_lut).as_array()
    out = np.zeros((1, 3, BIG), dtype=U64)
    _stage(N.lib().tae_stage_vertical_packing, ctx._h, _vp(x["stage_stage_fft"].view(np.float64)), 1, 6, _vp(lut), 3,
           _vp(out), N.TAE_MEM_HOST)
    return (out,)


def _small_key_bits(client, cts):
    """Bits of small-key LWEs [n][n+1] on the lvl_64 client key (decrypt_bits_raw takes the big key there)."""
    s = client.secrets()[0]
    phase = cts[:, -1] - (cts[:, :-1] * s[None, :]).sum(axis=1, dtype=U64)
    return [int(v) for v in ((phase + (U64(1) << U64(62))) >> U64(63))]


def _check_stage_ks(x, o):
    assert _small_key_bits(x["client"], o[0]) == STAGE_BITS


def _check_stage_boot(x, o):
    shifted = o[0].copy()
    shifted[:, -1] += U64(1) << U64(62)  # +-2^62 -> 2^63 / 0
    assert [int(b) for b in x["client"].decrypt_bits_raw(shifted)] == [1 - b for b in STAGE_BITS]


def _check_stage_vp(x, o):
    want = stage_lut(int("".join(map(str, STAGE_BITS)), 2))
    assert [int(b) for b in x["client"].decrypt_bits_raw(o[0][0])] == _word_bits(want, 3)


def _check_chain(x, o):
    """The intermediate stages (shifted bits, GGSW rows, their transform) are pinned word for word to the oracle by
    test_gpu_parity.py; here the chain they belong to ends in a vertical packing that decrypts to the LUT's value, and
    the probe's cold output is the chain's."""


def _cbs(key, lut_args):
    def run(ctx, x):
        lut = ctx.generate_lookup_table(*lut_args)
        return (ctx.circuit_bootstrap_raw(x[key], lut),)
    return run


def _check_cbs(vals):
    def check(x, o):
        for g, v in enumerate(vals):
            assert [int(b) for b in x["client"].decrypt_bits_raw(o[0][g])] == _word_bits(galois(v), 24), g
    return check


def _check_id5(x, o):
    assert [int(b) for b in x["client"].decrypt_bits_raw(o[0])] == ID5


def _enc(nb, rounds):
    return lambda ctx, x: (E.encrypt_blocks_raw(ctx, x["rk"][0], x["blocks"][:nb], rounds),)


def _check_enc(nb, rounds):
    def check(x, o):
        got = aes_128.bits_to_blocks(x["client"].decrypt_bits_raw(o[0]))
        assert got == [aes_var.encrypt_block_plain(EK[0], b, rounds) for b in BLOCKS[:nb]]
    return check


def _ctr(key, rounds):
    return lambda ctx, x: (V.ctr_transcipher_raw(ctx, x["rk"][0], IV8, 0xFE, x[key], rounds=rounds),)


def _check_ctr(key, rounds, client="client"):
    return lambda x, o: _eq(_bytes_of(x[client], o[0]), _ctr_plain(EK[0], IV8, 0xFE, x[key], rounds))


def _eq(a, b):
    assert a == b, (a, b)


def _check_decrypt_key(x, o):
    _eq(_bytes_of(x["client"], o[0]), b"".join(aes_var.decrypt_key_plain(EK[0])))


def _check_decrypt(x, o):
    got = aes_128.bits_to_blocks(x["client"].decrypt_bits_raw(o[0]))
    assert got == [aes_var.decrypt_block_plain(EK[0], b, 2) for b in BLOCKS[:2]]


def _check_keyexp(key):
    return lambda x, o: _eq(_bytes_of(x["client"], o[0]), b"".join(aes_var.key_schedule_plain(key)))


def _check_mk_schedule(x, o):
    for s in range(3):
        _eq(_bytes_of(x["client"], o[0][s]), b"".join(EK[s]))


def _mk_enc(key_of):
    return lambda ctx, x: (M.encrypt_blocks_raw(ctx, x["table"], key_of, x["blocks"], 2),)


def _check_mk_enc(key_of):
    def check(x, o):
        got = aes_128.bits_to_blocks(x["client"].decrypt_bits_raw(o[0]))
        assert got == [aes_var.encrypt_block_plain(EK[s], b, 2) for s, b in zip(key_of, BLOCKS)]
    return check


def _check_mk_ctr(x, o):
    for (slot, iv, first, data), got in zip(x["mk_streams"], o):
        _eq(_bytes_of(x["client"], got), _ctr_plain(EK[slot], iv, first, data, 2))


def _check_xts_tweaks(x, o):
    _eq(_bytes_of(x["client"], o[0]), b"".join(_xts_masks_plain(EK[1], 2, [(XTS_UNIT, 0), (XTS_UNIT_B, 0)])))


def _check_xts_masks(x, o):
    units = (XTS_UNIT, XTS_UNIT_B)
    want = _xts_masks_plain(EK[1], 2, [(units[u], j) for u, j in zip(XTS_MASK_UNIT_OF, XTS_MASK_INDEX)])
    _eq(_bytes_of(x["client"], o[0]), b"".join(want))


def _check_xts(x, o):
    want = []
    for u in XTS_UNITS:
        first = u[2] if len(u) > 2 else 0
        for i in range(0, len(u[1]), 16):
            m, = _xts_masks_plain(EK[1], 2, [(u[0], first + i // 16)])
            want.append(_xor(aes_var.decrypt_block_plain(EK[0], _xor(u[1][i:i + 16], m), 2), m))
    _eq(_bytes_of(x["client"], o[0]), b"".join(want))


def _ccm_pair(ctx, x):
    res = M.ccm_transcipher_raw(ctx, x["table"], x["ccm_pair"], CCM_TAG, rounds=2)
    return tuple(a for pair in res for a in pair)


def _check_ccm(frames_key, plain):
    def check(x, o):
        frames = x[frames_key] if isinstance(x[frames_key], list) else [x[frames_key]]
        for f, (slot, nonce, aad, data) in enumerate(frames):
            _eq(_bytes_of(x["client"], o[2 * f]), plain[f][3])
            assert aes_var.ccm_tag_ok(x["client"], o[2 * f + 1])
            _eq((plain[f][3], bytes(CCM_TAG)), aes_var.ccm_decrypt_plain(KEYS[slot], nonce, aad, data, CCM_TAG, rounds=2))
    return check


def _ccm_single(ctx, x):
    slot, nonce, aad, data = x["ccm_single"]
    return V.ccm_transcipher_raw(ctx, x["rk"][slot], nonce, aad, data, CCM_TAG, rounds=2)


def _check_gf_square(x, o):
    for g, a in zip(o[0], GF_A):
        _eq(_bytes_of(x["client"], g), R.mul(a, a))


def _check_gf_product(x, o):
    _eq(_bytes_of(x["client"], o[0][0]), R.mul(GF_A[0], GF_B))


def _check_ghash(x, o):
    _eq([_bytes_of(x["client"], t) for t in o[0]], x["gcm_h"][:3])


def _gcm(key, tag_len):
    def run(ctx, x):
        res = V.gcm_transcipher_raw(ctx, x["gcm_rk"], x["gcm_hk"], x[key], tag_len, rounds=2)
        return tuple(a for pair in res for a in pair)
    return run


def _check_gcm(key, plain, tag_len):
    def check(x, o):
        for f, (iv, aad, pt) in enumerate(plain):
            _eq(_bytes_of(x["client"], o[2 * f]), pt)
            assert aes_var.gcm_tag_ok(x["client"], o[2 * f + 1])
            _eq(aes_var.gcm_decrypt_plain(GCM_KEY, iv, aad, x[key][f][2], tag_len, rounds=2), (pt, bytes(tag_len)))
    return check


def _pack(n):
    return lambda ctx, x: (ctx.pack(x["pack_rows"][:n]).data,)


def _check_pack(n):
    def check(x, o):
        got = x["client"].decrypt_packed(tfhe_aes.PackedBits(o[0], n, "server"))
        assert [int(b) for b in got] == PACK_BITS[:n]
    return check


def _check_unpack(x, o):
    assert [int(b) for b in x["client"].decrypt_bits_raw(o[0])] == PACK_BITS


def _aes8(nb):
    return lambda ctx, x: (A8.encrypt_blocks_raw(ctx, x["rk8"], x["blocks8"][:nb or None], rounds=1),)


def _check_aes8(nb):
    def check(x, o):
        plain = x["blocks8_plain"][:nb or None]
        got = aes_128.bits_to_blocks(x["client8"].decrypt_bits_raw(o[0]))
        assert got == [aes_var.encrypt_block_plain(EK[0], b, 1) for b in plain]
    return check


def _check_extract8(x, o):
    assert [aes_128.bits_to_u8(x["client8"].decrypt_bits_raw(b)) for b in o[0]] == INTS8


def _boot8(ctx, x):
    return (ctx.bootstrap_from_bits_raw(x["bytes8"], ctx.generate_lookup_table(8, 8, lambda v: v + 3)),)


def _check_boot8(x, o):
    assert [int(v) for v in x["client8"].decrypt_ints_raw(o[0])] == [(v + 3) & 255 for v in BYTES8]


def _s1_bootstrap(ctx, x):
    tvs = np.stack([S1.test_vector_from_cleartext_fn(ctx, f).data
                    for f in (lambda c: tfhe_aes.Cleartext(1 - c.value), lambda c: c)])  # NOT, identity
    return (S1.bootstrap_raw(ctx, x["s1_bits5"], tvs),)


def _check_s1_bootstrap(x, o):
    want = [1 - b if i % 2 == 0 else b for i, b in enumerate(S1_BITS5)]
    assert [int(b) for b in x["client1"].decrypt_bits_raw(o[0])] == want


def _check_s1_pks(x, o):
    """The GLWE's phase under the GLWE secret key: bit j at coefficient j, m 2^62 (shortint_1bit.rs:593-640)."""
    ck = x["client1"]
    k, n = ck.params["k"], ck.params["N"]
    s = ck.secrets()[1].reshape(k, n)
    glwe = o[0].reshape(k + 1, n)
    phase = glwe[k].copy()
    for i in range(k):
        for v in np.nonzero(s[i])[0]:
            rolled = np.roll(glwe[i], int(v))
            rolled[:int(v)] = U64(0) - rolled[:int(v)]  # X^N = -1
            phase -= rolled
    got = [int(b) for b in ((phase[:5] + (U64(1) << U64(61))) >> U64(62)) & U64(1)]
    assert got == S1_PKS_BITS + [0, 0, 0]


def _s1_mv(key, nbits, tables):
    def run(ctx, x):
        return (S1.calculate_multivariate_function_raw(ctx, x[key], [S1.MultivariateTestVector(nbits, t) for t in tables]),)
    return run


def _check_s1_mv(vals, tables):
    def check(x, o):
        for g, v in enumerate(vals):
            assert [int(b) for b in x["client1"].decrypt_bits_raw(o[0][g])] == [t[v] for t in tables], g
    return check


PARITY8 = [bin(i).count("1") % 2 for i in range(256)]

PROBES = [
    # ---- params_sqrd_lvl_64 ----
    # packed I/O stands first: tae_pack_bits* leaves the per-stage slots of tae_last_stage_times* to the last batched
    # call (include/tfhe_aes_gpu.h), so only before any such call are a pack's launch counts those of a cold context
    Probe("pack_3", LVL64, "packed", "small", _pack(3), _check_pack(3)),
    Probe("pack_513", LVL64, "packed", "large", _pack(513), _check_pack(513)),
    Probe("unpack_513", LVL64, "packed", "small", lambda ctx, x: (ctx.unpack_raw(x["packed"]),), _check_unpack),
    Probe("cbs_g2", LVL64, "cbs", "small", _cbs("cbs2", (8, 24, galois)), _check_cbs(CBS_G2)),
    Probe("cbs_g40", LVL64, "cbs", "large", _cbs("cbs40", (8, 24, galois)), _check_cbs(CBS_G40)),
    Probe("cbs_id5", LVL64, "cbs_id", "small", _cbs("id5", (1, 1, lambda v: v)), _check_id5),
    Probe("stage_ks", LVL64, "stage", "small", _stage_ks, _check_stage_ks),
    Probe("stage_pbs", LVL64, "stage", "small", _stage_pbs, _check_chain),
    Probe("stage_boot", LVL64, "stage", "small", _stage_boot, _check_stage_boot),
    Probe("stage_pfks", LVL64, "stage", "small", _stage_pfks, _check_chain),
    Probe("stage_fft", LVL64, "stage", "small", _stage_fft, _check_chain),
    Probe("stage_vp", LVL64, "stage", "small", _stage_vp, _check_stage_vp),
    Probe("enc_1x1", LVL64, "encrypt", "small", _enc(1, 1), _check_enc(1, 1)),
    Probe("enc_3x2", LVL64, "encrypt", "large", _enc(3, 2), _check_enc(3, 2)),
    Probe("ctr_21x1", LVL64, "ctr", "small", _ctr("ctr21", 1), _check_ctr("ctr21", 1)),
    Probe("ctr_37x2", LVL64, "ctr", "large", _ctr("ctr37", 2), _check_ctr("ctr37", 2)),
    Probe("decrypt_key", LVL64, "decrypt_key", "small", lambda ctx, x: (E.decrypt_key_raw(ctx, x["rk"][0]),),
          _check_decrypt_key),
    Probe("decrypt_2x2", LVL64, "decrypt", "small", lambda ctx, x: (V.decrypt_blocks_raw(ctx, x["dk"], x["blocks"][:2], 2),),
          _check_decrypt),
    Probe("cbc_3", LVL64, "cbc", "small", lambda ctx, x: (V.cbc_transcipher_raw(ctx, x["dk"], IV16, x["cbc48"], rounds=2),),
          lambda x, o: _eq(_bytes_of(x["client"], o[0]), _cbc_plain(EK[0], IV16, x["cbc48"], 2))),
    Probe("keyexp_128", LVL64, "key_expand", "small", lambda ctx, x: (V.key_schedule_raw(ctx, x["keys"][0]),),
          _check_keyexp(KEYS[0])),
    Probe("keyexp_256", LVL64, "key_expand", "large", lambda ctx, x: (V.key_schedule_raw(ctx, x["key256"]),),
          _check_keyexp(KEY256)),
    Probe("mk_schedule3", LVL64, "multi", "small", lambda ctx, x: (M.key_schedule_raw(ctx, x["keys"]),), _check_mk_schedule),
    Probe("mk_enc_202", LVL64, "multi", "small", _mk_enc([2, 0, 2]), _check_mk_enc([2, 0, 2])),
    Probe("mk_enc_011", LVL64, "multi", "small", _mk_enc([0, 1, 1]), _check_mk_enc([0, 1, 1])),
    Probe("mk_ctr2", LVL64, "multi", "small", lambda ctx, x: tuple(M.ctr_transcipher_raw(ctx, x["table"], x["mk_streams"], 2)),
          _check_mk_ctr),
    Probe("xts_tweaks", LVL64, "xts", "small", lambda ctx, x: (V.xts_tweaks_raw(ctx, x["rk"][1], [XTS_UNIT, XTS_UNIT_B], rounds=2),),
          _check_xts_tweaks),
    Probe("xts_masks", LVL64, "xts", "small",
          lambda ctx, x: (V.xts_masks_raw(ctx, x["xts_tweak_cts"], XTS_MASK_UNIT_OF, XTS_MASK_INDEX),), _check_xts_masks),
    Probe("xts_3x2", LVL64, "xts", "small", lambda ctx, x: (V.xts_transcipher_raw(ctx, x["dk"], x["rk"][1], XTS_UNITS, rounds=2),),
          _check_xts),
    Probe("ccm_pair", LVL64, "ccm", "small", _ccm_pair, _check_ccm("ccm_pair", CCM_PAIR_PLAIN)),
    Probe("ccm_single", LVL64, "ccm", "small", _ccm_single, _check_ccm("ccm_single", [CCM_SINGLE_PLAIN])),
    Probe("gf_square2", LVL64, "gcm", "small", lambda ctx, x: (V.gf128_square_raw(ctx, x["gf_a"]),), _check_gf_square),
    Probe("gf_product1", LVL64, "gcm", "small", lambda ctx, x: (V.gf128_product_raw(ctx, x["gf_a"][:1], x["gf_b"]),),
          _check_gf_product),
    Probe("ghash_3", LVL64, "gcm", "small", lambda ctx, x: (V.ghash_key_raw(ctx, x["gcm_rk"], 3, rounds=2),), _check_ghash),
    Probe("gcm_one", LVL64, "gcm", "small", _gcm("gcm_one", 12), _check_gcm("gcm_one", GCM_ONE_PLAIN, 12)),
    Probe("gcm_ragged3", LVL64, "gcm", "small", _gcm("gcm_ragged", 4), _check_gcm("gcm_ragged", GCM_RAGGED_PLAIN, 4)),
    # ---- the 8-bit model's set ----
    Probe("aes8_1x1", W8, "aes8", "small", _aes8(1), _check_aes8(1)),
    Probe("aes8_wide", W8, "aes8", "large", _aes8(0), _check_aes8(0)),
    Probe("ctr8_21", W8, "ctr8", "small", lambda ctx, x: (V.ctr_transcipher_raw(ctx, x["rk8"], IV8, 0xFE, x["ctr21"], rounds=1),),
          _check_ctr("ctr21", 1, "client8")),
    Probe("extract8", W8, "extract8", "small", lambda ctx, x: (ctx.extract_bits_from_ciphertext_raw(x["ints8"]),), _check_extract8),
    Probe("boot8", W8, "boot8", "small", _boot8, _check_boot8),
    # ---- shortint_1bit ----
    Probe("s1_bootstrap", S1BIT, "s1_bootstrap", "small", _s1_bootstrap, _check_s1_bootstrap),
    Probe("s1_pks", S1BIT, "s1_pks", "small", lambda ctx, x: (S1.packing_keyswitch(ctx, x["s1_pks"]),), _check_s1_pks),
    Probe("s1_mv3", S1BIT, "s1_mv", "small", _s1_mv("s1_mv3", 3, S1_TABLES3), _check_s1_mv(S1_VALS3, S1_TABLES3)),
    Probe("s1_mv8", S1BIT, "s1_mv", "large", _s1_mv("s1_mv8", 8, [PARITY8]), _check_s1_mv(S1_VALS8, [PARITY8])),
]
BY_NAME = {p.name: p for p in PROBES}

# ---- the scratch buffers each probe's call walks (engine.hpp members; aes_engine.hip / kernels.hip drivers) -------
_CB = {"d_small_", "d_big_", "d_ggsw_", "d_ggsw_f_", "d_digits_"}  # circuit_bootstrap / cbs_vp: reserve + both keyswitches
_AES = _CB | {"d_state_", "d_muls_"}                               # aes_forward, aes_decrypt_rounds, the key derivations
_PLAN = {"d_ctr_groups_", "d_ctr_map_"}                            # a counter plan (aes_ctr_chunk)
_MPLAN = _PLAN | {"d_ctr_gslot_", "d_key_of_", "d_ctr_bout_", "d_ctr_blen_"}  # aes_ctr_blocks_multi
_KEEP = {"d_pub_kout_", "d_pub_klen_"}                             # pub_pass with a second placement
_RS = {"d_rs_start_", "d_rs_src_", "d_rs_list_", "d_rs_base_", "d_rs_pub_"}  # rowsum_pass
_GCM_PROD = {"d_gcm_ops_", "d_gcm_ks_", "d_gcm_parts_", "d_gcm_a_", "d_gcm_b_", "d_pf_flags_"} | _RS  # 8192 bits: K-layout PFKS
_X8 = {"d_ints_", "d_xbuf_", "d_xsh_", "d_xks_", "d_xpbs_", "d_lut_x_"}  # bootstrap_bytes8 + extract_bits
_CCM = _AES | _MPLAN | _KEEP | {"d_ccm_keep_", "d_ccm_bytes_", "d_ccm_src_", "d_ccm_slot_", "d_ccm_order_"}
_GCM = _AES | _MPLAN | _KEEP | _RS | {"d_gcm_bytes_", "d_gcm_src_", "d_gcm_a_", "d_gcm_b_"}
USES = {
    "cbs_g2": _CB, "cbs_g40": _CB, "cbs_id5": _CB,
    "stage_ks": {"d_digits_"}, "stage_pbs": set(), "stage_boot": set(), "stage_pfks": {"d_digits_"}, "stage_fft": set(),
    "stage_vp": set(),
    "enc_1x1": _AES, "enc_3x2": _AES, "ctr_21x1": _AES | _PLAN, "ctr_37x2": _AES | _PLAN,
    "decrypt_key": _AES, "decrypt_2x2": _AES, "cbc_3": _AES, "keyexp_128": _AES, "keyexp_256": _AES,
    "mk_schedule3": _AES, "mk_enc_202": _AES | {"d_key_of_"}, "mk_enc_011": _AES | {"d_key_of_"}, "mk_ctr2": _AES | _MPLAN,
    "xts_tweaks": _AES, "xts_masks": _RS, "xts_3x2": _AES | _RS | {"d_xts_tweaks_", "d_xts_masks_"},
    "ccm_pair": _CCM, "ccm_single": _CCM,
    "gf_square2": _CB | _RS | {"d_gcm_a_", "d_gcm_b_"}, "gf_product1": _CB | _GCM_PROD,
    "ghash_3": _AES | _MPLAN | _GCM_PROD, "gcm_one": _GCM, "gcm_ragged3": _GCM,
    "pack_3": {"d_pack_", "d_digits_"}, "pack_513": {"d_pack_", "d_digits_"}, "unpack_513": set(),
    "aes8_1x1": _AES | _X8, "aes8_wide": _AES | _X8 | {"d_acc_w_"}, "ctr8_21": _AES | _X8 | _PLAN,
    "extract8": (_X8 - {"d_ints_"}) | {"d_digits_"}, "boot8": _CB,
    "s1_bootstrap": {"d_big_", "d_digits_"}, "s1_pks": {"d_s1_pks_", "d_digits_"},
    "s1_mv3": {"d_s1_in_", "d_s1_out_", "d_s1_pks_", "d_s1_tv_", "d_big_", "d_digits_"},
    "s1_mv8": {"d_s1_in_", "d_s1_out_", "d_s1_pks_", "d_s1_tv_", "d_big_", "d_digits_"},
}

# Engine members that no call rewrites: written when the context is made (or, for d_lut_x_'s siblings, once) and only
# read afterwards, or outside what a probe can reach.  One line each.
NOT_SCRATCH = {
    "d_ksk_": "keyswitch key, uploaded by the constructor",
    "d_pfpksk_": "private functional packing keyswitch key, uploaded by the constructor",
    "d_bsk_f_": "Fourier bootstrapping key, converted once by bsk_to_fourier",
    "d_twist_": "FFT twiddles, init_common", "d_untwist_": "FFT twiddles, init_common", "d_w_": "FFT twiddles, init_common",
    "d_lf_": "fused-twiddle transform table, init_common",
    "d_lut_shift_": "homomorphic_shift_boolean accumulators per CBS level, init_common",
    "d_lut24_": "8 -> 24 S-box LUT, init_common", "d_lut8_": "8 -> 8 S-box LUT, init_common",
    "d_lut_inv32_": "inverse-cipher LUT, init_common", "d_lut_inv8_": "inverse-cipher LUT, init_common",
    "d_lut_mul32_": "InvMixColumns multiples LUT, init_common", "d_lut_id1_": "1 -> 1 identity LUT, init_common",
    "d_lut_gcm_": "8 -> 7 nibble-product LUT, init_common",
    "d_wlut_sbox_": "8-bit model S-box LUT, init_common", "d_wlut_id_": "8-bit model identity LUT, init_common",
    "d_s1_sbox_tv_": "shortint_1bit S-box test vectors, init_common", "d_s1_id_tv_": "shortint_1bit identity test vector, init_common",
    "d_pf_bt_kl_": "K-layout PFKS key limbs, prepare_mfma_keys", "d_pf_corr_": "K-layout digit-offset correction, prepare_mfma_keys",
    "d_pf_bt_": "row-layout PFKS key limbs, prepare_mfma_keys", "d_ks_bt_": "keyswitch key limbs, prepare_mfma_keys",
    "d_clk_": "clock mode (set_timing(2)) only, zeroed before every stamped launch; test_timing_modes_bit_identical runs it",
}


def small_probes(params):
    return [p.name for p in PROBES if p.params == params and p.size == "small"]


def families(params=None):
    """family -> its probe names, small ones first, in list order."""
    out = {}
    for p in PROBES:
        if params is None or p.params == params:
            out.setdefault(p.family, []).append(p.name)
    return {f: sorted(v, key=lambda n: BY_NAME[n].size != "small") for f, v in out.items()}


def sharing_pairs(params):
    """Every ordered pair (a, b), a == b included, of small probes of one parameter set that share a buffer."""
    names = small_probes(params)
    return {(a, b) for a in names for b in names if USES[a] & USES[b]}


def adjacency_sequence(params):
    """A walk over the small probes in which every sharing pair is run back to back at least once.  Sharing is
    symmetric, so each connected component of the pair graph has an Euler circuit (Hierholzer, deterministic: edges
    in list order); the circuits are joined one after the other."""
    names = small_probes(params)
    out_edges = {a: [b for b in names if USES[a] & USES[b]] for a in names}
    seq = []
    for start in names:
        if not out_edges[start]:
            continue
        stack, circuit = [start], []
        while stack:
            v = stack[-1]
            if out_edges[v]:
                stack.append(out_edges[v].pop(0))
            else:
                circuit.append(stack.pop())
        seq += circuit[::-1]
    return seq


def covered_pairs(seq):
    return set(zip(seq, seq[1:]))


PIECE = 24  # probes per parametrised piece of the adjacency run


def adjacency_pieces(params):
    """The walk cut into pieces that overlap by one probe, so that no pair is lost at a cut."""
    seq = adjacency_sequence(params)
    return [seq[i:i + PIECE + 1] for i in range(0, max(len(seq) - 1, 1), PIECE)] if seq else []


TIMED_PIECE = 8  # probes per piece of the timed list-order run (each also needs its own timed cold context)


def timed_pieces(params):
    names = [p.name for p in PROBES if p.params == params]
    return [names[i:i + TIMED_PIECE] for i in range(0, len(names), TIMED_PIECE)]
