#!/usr/bin/env python3
"""Multi-key batches against the single-key paths, in one process.

Keys resident on the device, one warm-up of each leg, then `--runs` (default 5) alternating timed runs; the host
clock around calls that return after a device synchronise.  In every leg the yardstick is the single-key path
(aes_var.GalMulAes), which the multi-key work does not change.

(a) Key expansion, 128-bit, K = 8, 32, 128 keys: K consecutive GalMulAes.key_schedule_device calls against one
    GalMulAesMulti.key_schedule_device call.
(b) CTR transcipher, `--blocks` (default 128) blocks in total split evenly over K = 1, 8, 32, 128 keys, 10 rounds:
    K consecutive GalMulAes.ctr_transcipher_device calls against one GalMulAesMulti.ctr_transcipher_device call.

The outputs of the two sides of every comparison are asserted word-identical, and the K = 128 transcipher output
is checked by decryption.  Writes one JSON line: per-run ms, medians, spread = (max - min) / median of each side,
the ratios, and the per-stage times (HIP events, tae_last_stage_times_v2) of one extra batched run and of one
single-key call.

    python scripts/multikey_bench.py [--blocks 128] [--runs 5] [--out profiles/multikey_<blocks>.json]
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
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")
IV = bytes(range(0xC0, 0xC8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each side (at least 5)")
    ap.add_argument("--keys", type=int, nargs="+", default=[8, 32, 128], help="key counts of leg (a)")
    ap.add_argument("--out", default=None, help="default: profiles/multikey_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"multikey_{args.blocks}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_multi, aes_var

    V = aes_var.GalMulAes
    M = aes_multi.GalMulAesMulti
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nb = args.blocks
    kmax = max(args.keys + [nb])
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=min(16, os.cpu_count() or 1))
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)
    rows = 44 * 32

    def bits(data):
        return [b for byte in data for b in aes_128.u8_to_bits(byte)]

    def dev(a):
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    def host(t):
        return t.cpu().numpy().view(np.uint64)

    def say(msg):
        print(msg, file=sys.stderr, flush=True)

    plain_keys = [bytes((k * 37 + j * 11 + 5) & 255 for j in range(16)) for k in range(kmax)]
    keys_dev = dev(ck.encrypt_bits_raw([b for k in plain_keys for b in bits(k)]).reshape(kmax, 128, L))
    seq_table = torch.empty((kmax, rows, L), dtype=torch.int64, device="cuda:0")
    bat_table = torch.empty_like(seq_table)
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

    def compare(seq, bat, same):
        """One warm-up of each side, args.runs alternating runs, the outputs asserted identical."""
        seq()
        bat()
        assert same(), "the batched call and the single-key calls give different words"
        ms = {"sequential": [], "batched": []}
        for _ in range(args.runs):
            ms["sequential"].append(timed(seq))
            ms["batched"].append(timed(bat))
        assert same(), "the batched call and the single-key calls give different words"
        med = {k: statistics.median(v) for k, v in ms.items()}
        return {"ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                "median_ms": {k: round(v, 3) for k, v in med.items()},
                "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                "sequential_over_batched": round(med["sequential"] / med["batched"], 4)}

    # ---- (a) key expansion ----
    leg_a = {}
    for K in args.keys:
        def seq(K=K):
            for k in range(K):
                V.key_schedule_device(ctx, 128, keys_dev[k].data_ptr(), seq_table[k].data_ptr())

        def bat(K=K):
            M.key_schedule_device(ctx, 128, keys_dev.data_ptr(), K, bat_table.data_ptr())

        r = compare(seq, bat, lambda K=K: torch.equal(seq_table[:K], bat_table[:K]))
        r["stage_ms_batched"] = stages(bat)
        r["stage_ms_single_key_call"] = stages(
            lambda: V.key_schedule_device(ctx, 128, keys_dev[0].data_ptr(), seq_table[0].data_ptr()))
        leg_a[str(K)] = r
        say(f"(a) K={K}: {r['median_ms']} ratio {r['sequential_over_batched']}")
    M.key_schedule_device(ctx, 128, keys_dev.data_ptr(), kmax, bat_table.data_ptr())  # the table of leg (b)
    got = ck.decrypt_bits_raw(host(bat_table[kmax - 1])).reshape(-1, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in got) == b"".join(aes_var.key_schedule_plain(plain_keys[kmax - 1]))

    # ---- (b) counter-mode transciphering, nb blocks over K keys ----
    leg_b = {}
    msg = bytes((i * 29 + 3) & 255 for i in range(16 * nb))
    out_seq = torch.empty((16 * nb, 8, L), dtype=torch.int64, device="cuda:0")
    out_bat = torch.empty_like(out_seq)
    for K in [k for k in (1, 8, 32, 128) if k <= nb and nb % k == 0]:
        per = nb // K
        streams = []
        for k in range(K):
            first = 1 + k * per
            m = msg[16 * per * k:16 * per * (k + 1)]
            streams.append((k, IV, first, aes_var.ctr_xor_plain(plain_keys[k], IV, first, m)))

        def seq(K=K, per=per, streams=streams):
            for k, iv, first, data in streams:
                V.ctr_transcipher_device(ctx, 128, bat_table[k].data_ptr(), iv, first, data, 10,
                                         out_seq[16 * per * k].data_ptr())

        def bat(streams=streams):
            M.ctr_transcipher_device(ctx, 128, bat_table.data_ptr(), kmax, streams, 10, out_bat.data_ptr())

        r = compare(seq, bat, lambda: torch.equal(out_seq, out_bat))
        r["blocks_per_key"] = per
        r["round1_groups"] = M.ctr_plan(streams)
        r["stage_ms_batched"] = stages(bat)
        s0 = streams[0]
        r["stage_ms_single_key_call"] = stages(
            lambda: V.ctr_transcipher_device(ctx, 128, bat_table[0].data_ptr(), s0[1], s0[2], s0[3], 10,
                                             out_seq.data_ptr()))
        if K == 1:  # the two sides do the same work: do the medians agree within the spreads?
            gap = abs(r["median_ms"]["sequential"] - r["median_ms"]["batched"])
            width = max(max(v) - min(v) for v in r["ms"].values())
            r["k1_gap_ms"], r["k1_widest_range_ms"], r["k1_within_spread"] = round(gap, 3), round(width, 3), gap <= width
        bits_out = ck.decrypt_bits_raw(host(out_bat)).reshape(-1, 8)
        assert bytes(aes_128.bits_to_u8(b) for b in bits_out) == msg, f"K={K}: the transciphered bits decrypt wrongly"
        leg_b[str(K)] = r
        say(f"(b) K={K}: {r['median_ms']} ratio {r['sequential_over_batched']}")

    res = {
        "what": "multi-key batches against K consecutive single-key calls: (a) 128-bit key expansion, "
                "(b) 10-round CTR transcipher of `blocks` blocks split evenly over K keys",
        "blocks": nb, "runs": args.runs, "key_expansion": leg_a, "ctr_transcipher": leg_b,
        "outputs_word_identical": True, "outputs_decrypt_correctly": True,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
