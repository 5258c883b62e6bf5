#!/usr/bin/env python3
"""AES-192 / AES-256 against AES-128, in one process: the key expansion and the cipher.

Keys resident on the device, one warm-up of each leg, then `--runs` (default 5) alternating timed runs.

(a) Key expansion.  aes_128's key_schedule_raw with device memory -- the host-driven schedule, one upload /
    launch / download per step, unchanged by the device expansion, so it is the yardstick -- against
    GalMulAes.key_schedule_device at 128, 192 and 256 bits.  The 128-bit words of both are asserted equal.
(b) Cipher.  N blocks (default 128) x 10 rounds through aes_128's encrypt_blocks_device -- the yardstick --
    against x 12 rounds at 192 bits and x 14 at 256.  The bootstrap counts predict ratios 1.2 and 1.4.

Every output is checked by decryption.  Writes one JSON line: per-run ms, medians, spread = (max - min) / median
of each leg, the ratios, and the per-stage times of one run of each from tae_last_stage_times_v2.

    python scripts/aes256_bench.py [--blocks 128] [--runs 5] [--out profiles/aes256_<blocks>.json]
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

SEED = bytes(range(32))
SIZES = (128, 192, 256)
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each leg (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/aes256_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"aes256_{args.blocks}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_var

    E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
    V = aes_var.GalMulAes
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nb = args.blocks
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=min(16, os.cpu_count() or 1))
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)

    def bits(data):
        return [b for byte in data for b in aes_128.u8_to_bits(byte)]

    def dev(a):
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    def host(t):
        return t.cpu().numpy().view(np.uint64)

    keys = {kb: bytes(range(kb // 8)) for kb in SIZES}
    key_dev = {kb: dev(ck.encrypt_bits_raw(bits(keys[kb]))) for kb in SIZES}
    rk_dev = {kb: torch.empty((aes_var.expanded_words(kb) * 32, L), dtype=torch.int64, device="cuda:0") for kb in SIZES}
    rk_host_driven = torch.empty_like(rk_dev[128])
    pts = [bytes((i * 16 + j) & 255 for j in range(16)) for i in range(nb)]
    blk_dev = dev(ck.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1)).reshape(nb, 128, L))
    out_dev = {kb: torch.empty_like(blk_dev) for kb in SIZES}
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

    def ks_host_driven():
        N.check(N.lib().tae_aes_key_schedule_raw(ctx._h, C.c_void_p(key_dev[128].data_ptr()),
                                                 C.c_void_p(rk_host_driven.data_ptr()), N.TAE_MEM_DEVICE))

    def ks(kb):
        return lambda: V.key_schedule_device(ctx, kb, key_dev[kb].data_ptr(), rk_dev[kb].data_ptr())

    def enc(kb):
        if kb == 128:  # the yardstick: the entry point AES-128 has always had
            return lambda: E.encrypt_blocks_device(ctx, rk_dev[128].data_ptr(), blk_dev.data_ptr(), nb, 10,
                                                   out_dev[128].data_ptr())
        return lambda: V.encrypt_blocks_device(ctx, kb, rk_dev[kb].data_ptr(), blk_dev.data_ptr(), nb, kb // 32 + 6,
                                               out_dev[kb].data_ptr())

    legs = {"ks_host_driven_128": ks_host_driven}
    legs.update({f"ks_device_{kb}": ks(kb) for kb in SIZES})
    enc_legs = {f"encrypt_{kb}": enc(kb) for kb in SIZES}

    def measure(group):
        for fn in group.values():  # warm-up
            fn()
        ms = {k: [] for k in group}
        for _ in range(args.runs):
            for k, fn in group.items():
                ms[k].append(timed(fn))
        return ms

    ms = measure(legs)
    assert np.array_equal(host(rk_host_driven), host(rk_dev[128])), "the two 128-bit expansions differ"
    for kb in SIZES:
        got = ck.decrypt_bits_raw(host(rk_dev[kb])).reshape(-1, 8)
        want = b"".join(aes_var.key_schedule_plain(keys[kb]))
        assert bytes(aes_128.bits_to_u8(b) for b in got) == want, f"the {kb}-bit expansion decrypts wrongly"
    ms.update(measure(enc_legs))
    for kb in SIZES:
        ek = aes_var.key_schedule_plain(keys[kb])
        got = aes_128.bits_to_blocks(ck.decrypt_bits_raw(host(out_dev[kb])))
        assert got == [aes_var.encrypt_block_plain(ek, p) for p in pts], f"AES-{kb} decrypts wrongly"

    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "what": "key expansion: host-driven aes_128 schedule vs device expansion; cipher: 10 / 12 / 14 rounds",
        "blocks": nb, "runs": args.runs,
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        "ks_128_host_driven_over_device": round(med["ks_host_driven_128"] / med["ks_device_128"], 4),
        "ks_ratio_192_over_128": round(med["ks_device_192"] / med["ks_device_128"], 4),
        "ks_ratio_256_over_128": round(med["ks_device_256"] / med["ks_device_128"], 4),
        "encrypt_ratio_192_over_128": round(med["encrypt_192"] / med["encrypt_128"], 4),
        "encrypt_ratio_256_over_128": round(med["encrypt_256"] / med["encrypt_128"], 4),
        "expected_encrypt_ratios": {"192": 1.2, "256": 1.4},
        "ks_128_words_equal": True, "outputs_decrypt_correctly": True,
        "stage_ms": {k: stages(fn) for k, fn in list(legs.items())[1:] + list(enc_legs.items())},
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
