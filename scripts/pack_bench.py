#!/usr/bin/env python3
"""What packing a batch's result costs, against the batch itself, in one process.

FIPS-197 C.1 key, N blocks (default 128) x 10 rounds, keys resident on the device.  After one warm-up of each,
alternates timed runs of
  (a) encrypt_blocks_device               -- unchanged by the packed I/O, so it is the yardstick,
  (b) the same followed by pack_device of its 128 N output bits on the device,
checks that the packed result decrypts to the ciphertext blocks, and writes one JSON line: per-run ms, medians,
(b) - (a), spread = (max - min) / median of each, the pack stage's own time from HIP events and the PFKS stage
time of one round in the same run, the bytes copied to the host with packing and without and the time of both
copies, and the std and maximum of the error that packing added (packed phase minus input phase, client side).

    python scripts/pack_bench.py [--blocks 128] [--rounds 10] [--runs 5] [--out profiles/pack_128.json]
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
SEED = bytes(range(32))
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")
U64 = np.uint64


def glwe_phases(glwes, glwe_sk, k, n):
    """B - sum_p A_p S_p (mod X^N + 1) of every GLWE under the binary key: [G][N] uint64."""
    c, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    src, neg = (c - i) % n, i > c
    out = []
    for g in glwes:
        polys = g.reshape(k + 1, n)
        phase = polys[k].copy()
        for p in range(k):
            terms = polys[p][src]
            terms = np.where(neg, U64(0) - terms, terms)
            phase -= (terms * glwe_sk[p * n:(p + 1) * n].astype(U64)[None, :]).sum(axis=1, dtype=U64)
        out.append(phase)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each leg (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/pack_<blocks>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"pack_{args.blocks}.json")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128

    E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nb = args.blocks
    count = 128 * nb
    glwes, words = tfhe_aes.packed_len(pid, count)
    threads = min(16, os.cpu_count() or 1)
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=threads)
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)
    ek = aes_128.key_schedule_plain(KEY)
    rk = ck.encrypt_bits_raw([b for byte in b"".join(ek) for b in aes_128.u8_to_bits(byte)])
    rk_dev = torch.from_numpy(rk.view(np.int64)).to("cuda:0")
    pts = [bytes((i * 16 + j) & 255 for j in range(16)) for i in range(nb)]
    blk = ck.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1)).reshape(nb, 128, L)
    blk_dev = torch.from_numpy(blk.view(np.int64)).to("cuda:0")
    out_dev = torch.empty_like(blk_dev)
    packed_dev = torch.empty((glwes, words // glwes), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()  # device outputs are complete when the call returns; a copy to the host is synchronous
        return (time.perf_counter() - t0) * 1e3, r

    def run_a():
        E.encrypt_blocks_device(ctx, rk_dev.data_ptr(), blk_dev.data_ptr(), nb, args.rounds, out_dev.data_ptr())

    def pack():
        ctx.pack_device(out_dev.data_ptr(), count, packed_dev.data_ptr())

    def run_b():
        run_a()
        pack()

    run_a()
    run_b()
    ms_a, ms_b = [], []
    for _ in range(args.runs):
        ms_a.append(timed(run_a)[0])
        ms_b.append(timed(run_b)[0])

    # one more run of (b) with HIP-event stage times: the pack stage and the rounds' PFKS stage of the same run
    ctx.set_timing(True)
    run_b()
    v = (C.c_float * 8)()
    N.check(N.lib().tae_last_stage_times_v2(ctx._h, v))
    pack_ms = ctx.last_pack_time()
    ctx.set_timing(False)
    stage = {k: (int(x) if k == "pbs_launches" else round(float(x), 3)) for k, x in zip(STAGES, v)}
    pfks_launches = stage["pbs_launches"]  # one private functional keyswitch per CBS-level PBS launch
    pfks_round_ms = stage["pfks"] / max(1, pfks_launches)
    pfks_kernel = ctx.last_pfks_kernel()

    # the two ways home
    copy_packed_ms, packed = timed(lambda: packed_dev.cpu().numpy().view(U64))
    copy_full_ms, full = timed(lambda: out_dev.cpu().numpy().view(U64))
    want = [aes_128.encrypt_block_plain(ek, p, args.rounds) for p in pts]
    got = aes_128.decrypt_byte_array_packed(ck, tfhe_aes.PackedBits(packed, count, "server"))
    assert got == b"".join(want), "the packed result does not decrypt to the ciphertext blocks"
    assert aes_128.bits_to_blocks(ck.decrypt_bits_raw(full)) == want

    # added noise, client side: phase of packed coefficient j minus the phase of input LWE j
    _, glwe_sk = ck.secrets()
    p = ck.params
    lwes = full.reshape(count, L)
    in_phase = lwes[:, -1] - (lwes[:, :-1] * glwe_sk.astype(U64)[None, :]).sum(axis=1, dtype=U64)
    out_phase = glwe_phases(packed, glwe_sk, p["k"], p["N"]).reshape(-1)[:count]
    added = (out_phase - in_phase).view(np.int64).astype(np.float64)

    med_a, med_b = statistics.median(ms_a), statistics.median(ms_b)
    spread = lambda ms, m: (max(ms) - min(ms)) / m
    res = {
        "what": "encrypt_blocks_device (a), the same followed by pack_device of its output bits (b)",
        "blocks": nb, "rounds": args.rounds, "runs": args.runs, "bits": count, "glwes": glwes,
        "a_ms": [round(x, 3) for x in ms_a], "b_ms": [round(x, 3) for x in ms_b],
        "a_median_ms": round(med_a, 3), "b_median_ms": round(med_b, 3),
        "b_minus_a_ms": round(med_b - med_a, 3), "b_minus_a_over_a": round((med_b - med_a) / med_a, 5),
        "a_spread": round(spread(ms_a, med_a), 4), "b_spread": round(spread(ms_b, med_b), 4),
        "pack_stage_ms": round(pack_ms, 3), "pfks_stage_ms_per_round": round(pfks_round_ms, 3),
        "pack_over_pfks_round": round(pack_ms / pfks_round_ms, 4) if pfks_round_ms else None,
        "pfks_kernel": pfks_kernel, "b_stage_ms": stage,
        "bytes_to_host_packed": int(packed.nbytes), "bytes_to_host_unpacked": int(full.nbytes),
        "copy_packed_ms": round(copy_packed_ms, 3), "copy_unpacked_ms": round(copy_full_ms, 3),
        "added_noise_log2_std": round(float(np.log2(added.std())), 3),
        "added_noise_log2_max": round(float(np.log2(np.abs(added).max())), 3),
        "outputs_decrypt_correctly": True,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
