#!/usr/bin/env python3
"""Decryption and CBC transciphering against encryption, in one process.

FIPS-197 C.1 key, N blocks (default 128) x 10 rounds, keys resident on the device.  The decryption key is
derived on the device (timed once, with its stage times).  After one warm-up of each, alternates timed runs of
  (a) encrypt_blocks_device  -- unchanged by the inverse cipher, so it is the yardstick,
  (b) decrypt_blocks_device on (a)'s output, and
  (c) cbc_transcipher_device on N public ciphertext blocks,
checks that (b) decrypts to (a)'s plaintexts and (c) to the CBC message, and writes one JSON line: per-run ms,
medians, ratios b/a and c/a, spread = (max - min) / median of each, and the per-stage times of one run of
each from tae_last_stage_times_v2.

    python scripts/decrypt_bench.py [--blocks 128] [--rounds 10] [--runs 5] [--out profiles/decrypt_128.json]
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

KEY = bytes(range(16))
IV = bytes(range(0xA0, 0xB0))
SEED = bytes(range(32))
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/decrypt_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if args.rounds != 10:
        print("note: the CBC leg always runs 10 rounds", file=sys.stderr)
    out_path = args.out or os.path.join(ROOT, "profiles", f"decrypt_{args.blocks}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128

    E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nb = args.blocks
    threads = min(16, os.cpu_count() or 1)
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=threads)
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)
    ek = aes_128.key_schedule_plain(KEY)
    rk = ck.encrypt_bits_raw([b for byte in b"".join(ek) for b in aes_128.u8_to_bits(byte)])
    rk_dev = torch.from_numpy(rk.view(np.int64)).to("cuda:0")
    dk_dev = torch.empty_like(rk_dev)
    pts = [bytes((i * 16 + j) & 255 for j in range(16)) for i in range(nb)]
    blk = ck.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1)).reshape(nb, 128, L)
    blk_dev = torch.from_numpy(blk.view(np.int64)).to("cuda:0")
    out_a = torch.empty_like(blk_dev)
    out_b = torch.empty_like(blk_dev)
    out_c = torch.empty_like(blk_dev)
    msg = b"".join(pts)
    data = aes_128.cbc_encrypt_plain(KEY, IV, msg)
    torch.cuda.synchronize()

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

    def derive():
        N.check(N.lib().tae_aes_decrypt_key_raw(ctx._h, C.c_void_p(rk_dev.data_ptr()), C.c_void_p(dk_dev.data_ptr()),
                                                N.TAE_MEM_DEVICE))

    def run_a():
        E.encrypt_blocks_device(ctx, rk_dev.data_ptr(), blk_dev.data_ptr(), nb, args.rounds, out_a.data_ptr())

    def run_b():
        E.decrypt_blocks_device(ctx, dk_dev.data_ptr(), out_a.data_ptr(), nb, args.rounds, out_b.data_ptr())

    def run_c():
        E.cbc_transcipher_device(ctx, dk_dev.data_ptr(), IV, data, out_c.data_ptr())

    derive()
    dk_ms = [timed(derive) for _ in range(3)]
    dk_stage = stages(derive)
    run_a()
    run_b()
    run_c()

    def plain_of(t):
        return aes_128.bits_to_blocks(ck.decrypt_bits_raw(t.cpu().numpy().view(np.uint64)))

    assert plain_of(out_b) == pts, "decrypt(encrypt(x)) does not decrypt to x"
    assert b"".join(plain_of(out_c)) == msg, "the CBC transcipher does not decrypt to the message"
    ms_a, ms_b, ms_c = [], [], []
    for _ in range(args.runs):
        ms_a.append(timed(run_a))
        ms_b.append(timed(run_b))
        ms_c.append(timed(run_c))
    med = {k: statistics.median(v) for k, v in (("a", ms_a), ("b", ms_b), ("c", ms_c))}
    spread = lambda ms, m: (max(ms) - min(ms)) / m
    res = {
        "what": "encrypt_blocks_device (a), decrypt_blocks_device (b), cbc_transcipher_device (c)",
        "blocks": nb, "rounds": args.rounds, "runs": args.runs,
        "a_ms": [round(x, 3) for x in ms_a], "b_ms": [round(x, 3) for x in ms_b], "c_ms": [round(x, 3) for x in ms_c],
        "a_median_ms": round(med["a"], 3), "b_median_ms": round(med["b"], 3), "c_median_ms": round(med["c"], 3),
        "ratio_b_over_a": round(med["b"] / med["a"], 4), "ratio_c_over_a": round(med["c"] / med["a"], 4),
        "a_spread": round(spread(ms_a, med["a"]), 4), "b_spread": round(spread(ms_b, med["b"]), 4),
        "c_spread": round(spread(ms_c, med["c"]), 4),
        "outputs_decrypt_correctly": True,
        "a_stage_ms": stages(run_a), "b_stage_ms": stages(run_b), "c_stage_ms": stages(run_c),
        "decrypt_key_ms": [round(x, 3) for x in dk_ms], "decrypt_key_stage_ms": dk_stage,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
