#!/usr/bin/env python3
"""GCM transciphering against CCM on the same frame sizes, and the power table, in one process.

F frames (default 64) of an 8-byte AAD and a 32-byte payload under one AES-128 key, tag of 16 bytes, 10 rounds, key
and power table resident on the device.  A GCM frame of these sizes hashes m = 4 blocks and takes 3 cipher blocks
(J0 and two counters); the CCM frame takes 4 public blocks and three chain steps.  After one warm-up of each,
alternates timed runs of
  (g) gcm_transcipher_device on the F frames, and
  (c) ccm_transcipher_device on frames of the same sizes  -- unchanged by GCM, so it is the yardstick,
and times ghash_key_device at n_powers = 4 and 16.  Checks that (g) decrypts to the payloads with all-zero tag
differences and that the table of 4 holds H .. H^4, and writes one JSON line: per-run ms, medians, spread =
(max - min) / median of each, the per-stage times of one more run of each, and the two expectations of DESIGN.md 5.14:
  - a product costs about 6.4 AES-128 blocks of PBS time: the PBS stage of one tae_stage_gf128_product against the
    PBS stage of a 64-block cipher call (8192 bits a round) per block;
  - GHASH adds about 12% to a frame's PBS launches: the identity bootstraps of the call's chunks against the
    1280 bit bootstraps of each of its cipher blocks, and the PBS stage of (g) against that of the forward cipher
    over the same public blocks alone (tae_aesm_pub_keystream_raw).

    python scripts/gcm_bench.py [--frames 64] [--rounds 10] [--runs 5] [--out profiles/gcm_64.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tfhe-aes-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEY = bytes(range(0xC0, 0xD0))
SEED = bytes(range(32))
TAG_LEN = 16
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/gcm_<frames>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"gcm_{args.frames}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_multi, aes_var

    V, M = aes_var.GalMulAes, aes_multi.GalMulAesMulti
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nf, rounds = args.frames, args.rounds
    threads = min(16, os.cpu_count() or 1)
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=threads)
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)
    rk = ck.encrypt_bits_raw([b for byte in b"".join(aes_var.key_schedule_plain(KEY)) for b in aes_128.u8_to_bits(byte)])
    rk_dev = torch.from_numpy(rk.view(np.int64)).to("cuda:0")

    def dev(shape):
        return torch.empty(shape, dtype=torch.int64, device="cuda:0")

    def bytes_of(t):
        bits = ck.decrypt_bits_raw(t.cpu().numpy().view(np.uint64).reshape(-1, L)).reshape(-1, 8)
        return bytes(aes_128.bits_to_u8(b) for b in bits)

    def stages(fn):
        ctx.set_timing(True)
        fn()
        v = (C.c_float * 8)()
        N.check(N.lib().tae_last_stage_times_v2(ctx._h, v))
        ctx.set_timing(False)
        return {k: (int(x) if k == "pbs_launches" else round(float(x), 3)) for k, x in zip(STAGES, v)}

    def timed(fn):
        t0 = time.perf_counter()
        fn()  # device outputs are complete when the call returns
        return (time.perf_counter() - t0) * 1e3

    aad = bytes(range(8))
    msgs = [bytes((f * 5 + i * 7 + 3) & 255 for i in range(32)) for f in range(nf)]
    ivs = [bytes([0x10, 0x11]) + f.to_bytes(10, "big") for f in range(nf)]
    nonces = [bytes([0x12]) + iv for iv in ivs]
    g_frames = [(ivs[f], aad, aes_var.gcm_encrypt_plain(KEY, ivs[f], aad, msgs[f], TAG_LEN, rounds)) for f in range(nf)]
    c_frames = [(0, nonces[f], aad, aes_var.ccm_encrypt_plain(KEY, nonces[f], aad, msgs[f], TAG_LEN, rounds))
                for f in range(nf)]
    hk = {n: dev((n, 128, L)) for n in (4, 16)}
    out_plain, out_diff = dev((32 * nf, 8, L)), dev((nf, TAG_LEN, 8, L))
    torch.cuda.synchronize()

    def run_hk(n):
        V.ghash_key_device(ctx, 128, rk_dev.data_ptr(), n, rounds, hk[n].data_ptr())

    def run_g():
        V.gcm_transcipher_device(ctx, 128, rk_dev.data_ptr(), hk[4].data_ptr(), 4, g_frames, TAG_LEN, rounds,
                                 out_plain.data_ptr(), out_diff.data_ptr())

    def run_c():
        M.ccm_transcipher_device(ctx, 128, rk_dev.data_ptr(), 1, c_frames, TAG_LEN, rounds, out_plain.data_ptr(),
                                 out_diff.data_ptr())

    paths = (("hk4", lambda: run_hk(4)), ("hk16", lambda: run_hk(16)), ("g", run_g), ("c", run_c))
    for _, fn in paths:
        fn()  # the warm-up
    h = aes_var.encrypt_block_plain(aes_var.key_schedule_plain(KEY), bytes(16), rounds)
    want, p = b"", h
    for _ in range(4):
        want, p = want + p, aes_var.gf128_mul_plain(p, h)
    assert bytes_of(hk[4]) == want and bytes_of(hk[16][:4]) == want, "the power table is wrong"
    run_g()
    assert bytes_of(out_plain) == b"".join(msgs), "GCM does not decrypt to the payloads"
    assert not any(bytes_of(out_diff)), "a tag differs"

    ms = {k: [] for k, _ in paths}
    for _ in range(args.runs):
        for k, fn in paths:
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    st = {k: stages(fn) for k, fn in paths}

    # expectation 1: one product against the cipher's PBS time per block at 8192 bits a launch
    ab = dev((2, 128, L))
    ab.copy_(hk[4][:2])
    prod = dev((1, 128, L))
    st_prod = stages(lambda: N.check(N.lib().tae_stage_gf128_product(ctx._h, ab[0:1].data_ptr(), ab[1:2].data_ptr(), 1,
                                                                      prod.data_ptr(), N.TAE_MEM_DEVICE)))
    blocks = torch.zeros((64, 128, L), dtype=torch.int64, device="cuda:0")
    enc = torch.empty_like(blocks)
    st_aes = stages(lambda: V.encrypt_blocks_device(ctx, 128, rk_dev.data_ptr(), blocks.data_ptr(), 64, 10, enc.data_ptr()))
    pbs_per_block = st_aes["pbs"] / 64
    # expectation 2: the chunk refreshes against the cipher blocks' bootstraps, by count and by PBS stage time
    n_chunks = sum(int(aes_var.gcm_tag_rows(iv, aad, d[:-TAG_LEN], TAG_LEN, 4)[1].sum()) for iv, aad, d in g_frames)
    pub = np.frombuffer(b"".join(bytes(b) for iv, a, d in g_frames for b in aes_var.gcm_format(iv, a, d[:-TAG_LEN], TAG_LEN)[0][1:]),
                        dtype=np.uint8)
    n_pub = len(pub) // 16
    ks, ko = dev((n_pub, 128, L)), np.zeros(n_pub, dtype=np.int32)
    st_pub = stages(lambda: N.check(N.lib().tae_aesm_pub_keystream_raw(
        ctx._h, 128, C.c_void_p(rk_dev.data_ptr()), 1, ko.ctypes.data_as(C.c_void_p), pub.ctypes.data_as(C.c_void_p),
        n_pub, rounds, C.c_void_p(ks.data_ptr()), N.TAE_MEM_DEVICE)))
    res = {
        "what": "gcm_transcipher_device (g) against ccm_transcipher_device on the same frame sizes (c); ghash_key_device at "
                "4 and 16 powers (hk4, hk16); prod = one tae_stage_gf128_product, aes64 = a 64-block cipher call, pub = "
                "the forward cipher over (g)'s public blocks alone: stage times only",
        "frames": nf, "aad_bytes": 8, "payload_bytes": 32, "tag_bytes": TAG_LEN, "rounds": rounds, "runs": args.runs,
        "hashed_blocks_per_frame": 4, "cipher_blocks_per_gcm_frame": 3,
        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in ms.items()},
        **{f"{k}_median_ms": round(v, 3) for k, v in med.items()},
        **{f"{k}_spread": round(v, 4) for k, v in spread.items()},
        "g_minus_c_ms": round(med["g"] - med["c"], 3),
        "ratio_g_over_c": round(med["g"] / med["c"], 4),
        "larger_spread_ms": round(max(spread["g"] * med["g"], spread["c"] * med["c"]), 3),
        "outputs_decrypt_correctly": True,
        **{f"{k}_stage_ms": v for k, v in st.items()},
        "prod_stage_ms": st_prod, "aes64_stage_ms": st_aes, "pub_stage_ms": st_pub,
        "product_in_aes_blocks_of_pbs_time": round(st_prod["pbs"] / pbs_per_block, 3),
        "product_in_aes_blocks_expected": 6.4,
        "ghash_refreshes": n_chunks, "cipher_bit_bootstraps": 1280 * n_pub,
        "ghash_share_of_bootstraps": round(n_chunks / (1280 * n_pub), 4),
        "ghash_share_of_pbs_time": round((st["g"]["pbs"] - st_pub["pbs"]) / st_pub["pbs"], 4),
        "ghash_share_expected": 0.12,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
