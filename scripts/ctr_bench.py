#!/usr/bin/env python3
"""A/B of the counter-mode keystream against the per-block entry point, in one process.

README key and iv, counters 1..N (default 128 blocks x 10 rounds), rk resident on the device.  After one
warm-up of each, alternates timed runs of
  (a) encrypt_blocks_device on device-resident TRIVIAL counter ciphertexts (the per-block path), and
  (b) ctr_keystream_device (no counter ciphertexts; round 1 on the deduplicated groups),
asserts that both give identical words, and writes one JSON line (per-run ms, medians, ratio b/a, spread =
(max - min) / median of each, the round-1 group count, per-stage times of one run of each from
tae_last_stage_times_v2, and the computed host -> device bytes per call of both paths).

    python scripts/ctr_bench.py [--blocks 128] [--rounds 10] [--runs 5] [--out profiles/ctr_keystream_128.json]
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

README_KEY = bytes.fromhex("76b8e0ada0f13d90405d6ae55386bd28")
README_IV = bytes.fromhex("bdd219b8a08ded1a")
SEED = bytes(range(32))
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/ctr_keystream_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"ctr_keystream_{args.blocks}.json")

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
    ek = b"".join(aes_128.key_schedule_plain(README_KEY))
    rk = ck.encrypt_bits_raw([b for byte in ek for b in aes_128.u8_to_bits(byte)])
    rk_dev = torch.from_numpy(rk.view(np.int64)).to("cuda:0")
    # (a)'s input: trivial encryptions of the counter blocks (zero mask, bit << 63 on the body)
    bits = aes_128.blocks_to_bits(aes_128.counter_blocks(README_IV, nb)).astype(np.uint64)
    cts = np.zeros((nb, 128, L), dtype=np.uint64)
    cts[:, :, -1] = bits << np.uint64(63)
    blk_dev = torch.from_numpy(cts.view(np.int64)).to("cuda:0")
    out_a = torch.empty_like(blk_dev)
    out_b = torch.empty_like(blk_dev)
    torch.cuda.synchronize()

    def run_a():
        E.encrypt_blocks_device(ctx, rk_dev.data_ptr(), blk_dev.data_ptr(), nb, args.rounds, out_a.data_ptr())

    def run_b():
        E.ctr_keystream_device(ctx, rk_dev.data_ptr(), README_IV, 1, nb, args.rounds, out_b.data_ptr())

    def timed(fn):
        t0 = time.perf_counter()
        fn()  # device outputs are complete when the call returns
        return (time.perf_counter() - t0) * 1e3

    def stages(fn):
        ctx.set_timing(True)
        fn()
        v = (C.c_float * 8)()
        N.check(N.lib().tae_last_stage_times_v2(ctx._h, v))
        ctx.set_timing(False)
        return {k: (int(x) if k == "pbs_launches" else round(float(x), 3)) for k, x in zip(STAGES, v)}

    run_a()
    run_b()
    assert torch.equal(out_a, out_b), "the counter-mode keystream differs from the per-block path"
    ms_a, ms_b = [], []
    for _ in range(args.runs):
        ms_a.append(timed(run_a))
        ms_b.append(timed(run_b))
    assert torch.equal(out_a, out_b), "the counter-mode keystream differs from the per-block path"
    med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
    spread = lambda ms, med: (max(ms) - min(ms)) / med
    res = {
        "what": "ctr_keystream_device (b) vs encrypt_blocks_device on trivial counter ciphertexts (a)",
        "blocks": nb, "rounds": args.rounds, "runs": args.runs,
        "round1_groups": aes_128.ctr_plan(README_IV, 1, nb), "round1_groups_per_block_path": nb * 16,
        "a_ms": [round(x, 3) for x in ms_a], "b_ms": [round(x, 3) for x in ms_b],
        "a_median_ms": round(med_a, 3), "b_median_ms": round(med_b, 3), "ratio_b_over_a": round(med_b / med_a, 4),
        "a_spread": round(spread(ms_a, med_a), 4), "b_spread": round(spread(ms_b, med_b), 4),
        "b_faster_by_more_than_spread": bool((med_a - med_b) / med_a > max(spread(ms_a, med_a), spread(ms_b, med_b))),
        "outputs_identical": True,
        "a_stage_ms": stages(run_a), "b_stage_ms": stages(run_b),
        # computed, not measured: the counter ciphertexts of (a) against the iv and first counter of (b)
        "a_upload_bytes_per_call": nb * 128 * L * 8, "b_upload_bytes_per_call": 16,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
