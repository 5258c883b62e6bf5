#!/usr/bin/env python3
"""The AEAD open against the GCM call it follows, in one process.

F frames (default 64) of an 8-byte AAD and a 32-byte payload under one AES-128 key, tag of 16 bytes, 10 rounds, key
and power table resident on the device.  After one warm-up of each, alternates timed runs of
  (g) gcm_transcipher_device on the F frames  -- unchanged by the open, so it is the yardstick,
  (o) the same followed by aead_open_device on what it wrote, and
  (v) aead_verdict_raw (device memory) alone on (g)'s tag differences.
Checks that (o) decrypts to the payloads with every ok = 1, and writes one JSON line: per-run ms, medians, spread =
(max - min) / median of each, the per-stage times and PBS launch counts of one more run of each (for (o): of the open
alone), and the two expectations of DESIGN.md 5.18:
  - (o) - (g) is about 9/80 of the PBS time of the payload's cipher blocks: the gate is 9 bit bootstraps per byte, the
    cipher 8 per byte in each of 10 rounds.  The PBS stage of the open against the PBS stage of a cipher call over the
    same number of blocks;
  - the verdict's levels * cbs_l PBS launches are small: F * 128, F * 16 and F * 8 bits at tag_len 16.

    python scripts/aead_open_bench.py [--frames 64] [--rounds 10] [--runs 5] [--out profiles/aead_open.json]
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
PAYLOAD = 32
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/aead_open.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", "aead_open.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_var

    V = aes_var.GalMulAes
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

    def bits_of(t):
        return ck.decrypt_bits_raw(t.cpu().numpy().view(np.uint64).reshape(-1, L))

    def bytes_of(t):
        return bytes(aes_128.bits_to_u8(b) for b in bits_of(t).reshape(-1, 8))

    def stages(fn):
        ctx.set_timing(True)
        fn()
        v = (C.c_float * 8)()
        N.check(N.lib().tae_last_stage_times_v2(ctx._h, v))
        main_cts = ctx.last_stage_times()["pbs_main_cts"]  # the ciphertexts the throughput kernel took
        ctx.set_timing(False)
        res = {k: (int(x) if k == "pbs_launches" else round(float(x), 3)) for k, x in zip(STAGES, v)}
        res["pbs_main_cts"] = int(main_cts)
        return res

    def timed(fn):
        t0 = time.perf_counter()
        fn()  # device outputs are complete when the call returns
        return (time.perf_counter() - t0) * 1e3

    aad = bytes(range(8))
    msgs = [bytes((f * 5 + i * 7 + 3) & 255 for i in range(PAYLOAD)) for f in range(nf)]
    ivs = [bytes([0x10, 0x11]) + f.to_bytes(10, "big") for f in range(nf)]
    frames = [(ivs[f], aad, aes_var.gcm_encrypt_plain(KEY, ivs[f], aad, msgs[f], TAG_LEN, rounds)) for f in range(nf)]
    lens = [PAYLOAD] * nf
    hk = dev((4, 128, L))
    plain, diff = dev((PAYLOAD * nf, 8, L)), dev((nf, TAG_LEN, 8, L))
    gated, ok = dev((PAYLOAD * nf, 8, L)), dev((nf, L))
    torch.cuda.synchronize()
    V.ghash_key_device(ctx, 128, rk_dev.data_ptr(), 4, rounds, hk.data_ptr())

    def run_g():
        V.gcm_transcipher_device(ctx, 128, rk_dev.data_ptr(), hk.data_ptr(), 4, frames, TAG_LEN, rounds, plain.data_ptr(),
                                 diff.data_ptr())

    def run_open():
        aes_var.aead_open_device(ctx, plain.data_ptr(), lens, diff.data_ptr(), TAG_LEN, gated.data_ptr(), ok.data_ptr())

    def run_o():
        run_g()
        run_open()

    def run_v():
        N.check(N.lib().tae_aead_verdict_raw(ctx._h, C.c_void_p(diff.data_ptr()), nf, TAG_LEN, C.c_void_p(ok.data_ptr()),
                                             N.TAE_MEM_DEVICE))

    paths = (("g", run_g), ("o", run_o), ("v", run_v))
    for _, fn in paths:
        fn()  # the warm-up
    run_o()
    assert bytes_of(gated) == b"".join(msgs), "the open does not decrypt to the payloads"
    assert list(bits_of(ok)) == [1] * nf, "a verdict is not 1"

    ms = {k: [] for k, _ in paths}
    for _ in range(args.runs):
        for k, fn in paths:
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    st = {"g": stages(run_g), "open": stages(run_open), "v": stages(run_v)}

    # the expectation: the gate's 9 bits a byte against the cipher's 8 bits a byte and round, over the payload's blocks
    n_blocks = PAYLOAD * nf // 16
    blocks = torch.zeros((n_blocks, 128, L), dtype=torch.int64, device="cuda:0")
    enc = torch.empty_like(blocks)
    st_aes = stages(lambda: V.encrypt_blocks_device(ctx, 128, rk_dev.data_ptr(), blocks.data_ptr(), n_blocks, rounds,
                                                    enc.data_ptr()))
    groups, gate_groups = aes_var.aead_open_plan(TAG_LEN, lens)
    res = {
        "what": "gcm_transcipher_device (g); the same followed by aead_open_device (o); aead_verdict_raw on device "
                "memory alone (v); open = the open of (o) alone and aes = a cipher call over the payload's blocks: stage "
                "times only",
        "frames": nf, "aad_bytes": 8, "payload_bytes": PAYLOAD, "tag_bytes": TAG_LEN, "rounds": rounds, "runs": args.runs,
        "payload_blocks": n_blocks, "verdict_groups_per_frame": list(groups), "gate_groups": gate_groups,
        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in ms.items()},
        **{f"{k}_median_ms": round(v, 3) for k, v in med.items()},
        **{f"{k}_spread": round(v, 4) for k, v in spread.items()},
        "o_minus_g_ms": round(med["o"] - med["g"], 3),
        "ratio_o_over_g": round(med["o"] / med["g"], 4),
        "larger_spread_ms": round(max(spread["g"] * med["g"], spread["o"] * med["o"]), 3),
        "outputs_decrypt_correctly": True,
        **{f"{k}_stage_ms": v for k, v in st.items()},
        "aes_stage_ms": st_aes,
        "open_pbs_over_cipher_pbs": round(st["open"]["pbs"] / st_aes["pbs"], 4),
        "open_pbs_over_cipher_pbs_expected": round((9 * PAYLOAD * nf + sum(groups) * 8 * nf) / (128.0 * rounds * n_blocks), 4),
        "gate_share_expected": round(9.0 / (8 * rounds), 4),
        "o_minus_g_over_cipher_pbs": round((med["o"] - med["g"]) / st_aes["pbs"], 4),
        "verdict_bit_bootstraps": [g * 8 * nf for g in groups],
        "verdict_pbs_launches": st["v"]["pbs_launches"],
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
