#!/usr/bin/env python3
"""XTS transciphering against CBC transciphering, in one process.

IEEE 1619 vector 4 keys, N blocks (default 128) x 10 rounds as U data units (default 4: 512-byte sectors at 128
blocks), keys resident on the device.  After one warm-up of each, alternates timed runs of
  (a) cbc_transcipher_device on N public ciphertext blocks  -- unchanged by XTS, so it is the yardstick, and
  (b) xts_transcipher_device on the U units,
and times, in the same process,
  (c) what XTS adds per call by itself: encrypt_blocks_device of U blocks plus the 1 -> 1 identity circuit bootstrap
      of their 128 U bits, and
  (m) the mask stage alone (tae_stage_xts_masks on device arrays, N blocks).
Checks that (a) and (b) decrypt to their messages and writes one JSON line: per-run ms, medians, spread =
(max - min) / median of each, (b) - (a) against (c), and the per-stage times of one more run of (a), (b) and (c)
from tae_last_stage_times_v2; linear_b_minus_a_ms is the time of the launches XTS adds to the linear layer (the
tweak cipher's, the masks and the last add).

    python scripts/xts_bench.py [--blocks 128] [--units 4] [--rounds 10] [--runs 5] [--out profiles/xts_128.json]
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

KEY1 = bytes.fromhex("27182818284590452353602874713526")
KEY2 = bytes.fromhex("31415926535897932384626433832795")
IV = bytes(range(0xA0, 0xB0))
SEED = bytes(range(32))
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--units", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/xts_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if args.blocks % args.units:
        ap.error("--blocks must be a multiple of --units")
    out_path = args.out or os.path.join(ROOT, "profiles", f"xts_{args.blocks}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_var

    V = aes_var.GalMulAes
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nb, nu, rounds = args.blocks, args.units, args.rounds
    per_unit = nb // nu
    threads = min(16, os.cpu_count() or 1)
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=threads)
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)

    def resident(key):
        rk = ck.encrypt_bits_raw([b for byte in b"".join(aes_var.key_schedule_plain(key)) for b in aes_128.u8_to_bits(byte)])
        return torch.from_numpy(rk.view(np.int64)).to("cuda:0")

    rk1_dev, rk2_dev = resident(KEY1), resident(KEY2)
    dk1_dev = torch.empty_like(rk1_dev)
    V.decrypt_key_device(ctx, 128, rk1_dev.data_ptr(), dk1_dev.data_ptr())
    msg = bytes((i * 7 + 3) & 255 for i in range(16 * nb))
    cbc_data = aes_var.cbc_encrypt_plain(KEY1, IV, msg)
    units = [(u, aes_var.xts_encrypt_plain(KEY1, KEY2, u, msg[16 * per_unit * u:16 * per_unit * (u + 1)]))
             for u in range(nu)]
    out_a = torch.empty((nb, 128, L), dtype=torch.int64, device="cuda:0")
    out_b = torch.empty_like(out_a)
    # (c): the tweaks as trivial ciphertexts, the cipher's output, the refreshed bits
    tweak_bits = aes_128.blocks_to_bits([u.to_bytes(16, "little") for u in range(nu)]).astype(np.uint64)
    triv = np.zeros((nu, 128, L), dtype=np.uint64)
    triv[:, :, -1] = tweak_bits << np.uint64(63)
    triv_dev = torch.from_numpy(triv.view(np.int64)).to("cuda:0")
    enc_dev = torch.empty_like(triv_dev)
    t_dev = torch.empty_like(triv_dev)
    masks_dev = torch.empty_like(out_a)
    ident = ctx.generate_lookup_table(1, 1, lambda x: x)
    unit_of = [b // per_unit for b in range(nb)]
    index = [b % per_unit for b in range(nb)]
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

    def run_a():
        V.cbc_transcipher_device(ctx, 128, dk1_dev.data_ptr(), IV, cbc_data, rounds, out_a.data_ptr())

    def run_b():
        V.xts_transcipher_device(ctx, 128, dk1_dev.data_ptr(), rk2_dev.data_ptr(), units, rounds, out_b.data_ptr())

    def run_c_cipher():
        V.encrypt_blocks_device(ctx, 128, rk2_dev.data_ptr(), triv_dev.data_ptr(), nu, rounds, enc_dev.data_ptr())

    def run_c_refresh():
        N.check(N.lib().tae_circuit_bootstrap_raw(ctx._h, C.c_void_p(enc_dev.data_ptr()), 128 * nu, 1, ident._h,
                                                  C.c_void_p(t_dev.data_ptr()), N.TAE_MEM_DEVICE))

    def run_c():
        run_c_cipher()
        run_c_refresh()

    def run_m():
        V.xts_masks_device(ctx, t_dev.data_ptr(), nu, unit_of, index, masks_dev.data_ptr())

    for fn in (run_a, run_b, run_c, run_m):
        fn()

    def plain_of(t):
        return b"".join(aes_128.bits_to_blocks(ck.decrypt_bits_raw(t.cpu().numpy().view(np.uint64))))

    if rounds == 10:
        assert plain_of(out_a) == msg, "the CBC transcipher does not decrypt to the message"
        assert plain_of(out_b) == msg, "the XTS transcipher does not decrypt to the message"
    ms = {k: [] for k in "abcm"}
    for _ in range(args.runs):
        for k, fn in (("a", run_a), ("b", run_b), ("c", run_c), ("m", run_m)):
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    st = {"a": stages(run_a), "b": stages(run_b), "c_cipher": stages(run_c_cipher), "c_refresh": stages(run_c_refresh)}
    res = {
        "what": "cbc_transcipher_device (a), xts_transcipher_device (b), encrypt_blocks_device of the tweaks + their "
                "identity bootstrap (c), tae_stage_xts_masks (m)",
        "blocks": nb, "units": nu, "rounds": rounds, "runs": args.runs,
        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in ms.items()},
        **{f"{k}_median_ms": round(v, 3) for k, v in med.items()},
        **{f"{k}_spread": round(v, 4) for k, v in spread.items()},
        "b_minus_a_ms": round(med["b"] - med["a"], 3),
        "b_minus_a_minus_c_ms": round(med["b"] - med["a"] - med["c"], 3),
        "larger_spread_ms": round(max(spread["a"] * med["a"], spread["b"] * med["b"]), 3),
        "ratio_b_over_a": round(med["b"] / med["a"], 4),
        "outputs_decrypt_correctly": rounds == 10,
        "a_stage_ms": st["a"], "b_stage_ms": st["b"], "c_cipher_stage_ms": st["c_cipher"],
        "c_refresh_stage_ms": st["c_refresh"],
        "linear_b_minus_a_ms": round(st["b"]["linear"] - st["a"]["linear"], 3),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
