#!/usr/bin/env python3
"""CCM transciphering against the block cipher at the same batch sizes, in one process.

F frames (default 64) of an 8-byte AAD and a 32-byte payload under one AES-128 key, tag of 8 bytes, 10 rounds, the
key resident on the device: one public-block batch of 4 F blocks (A_0, A_1, A_2 and B_0 of every frame) and three
chain steps of F blocks.  After one warm-up of each, alternates timed runs of
  (a) ccm_transcipher_device on the F frames, and
  (b) encrypt_blocks_device at the same sequence of batch sizes, 4 F, F, F, F  -- unchanged by CCM, so it is the
      yardstick,
and the same pair for one frame (batches 4, 1, 1, 1): the chain is latency-bound at small stream counts.
Checks that (a) decrypts to the payloads with all-zero tag differences and writes one JSON line: per-run ms,
medians, spread = (max - min) / median of each, (a) - (b), and the per-stage times of one more run of (a) and of
(k), the keyed block cipher at the same batch sizes (tae_aesm_encrypt_blocks_raw on a table of one key, whose linear
launches are timed as CCM's are).  linear_a_minus_k_ms is what CCM's own launches cost: three absorb kernels, the
tag kernel and the second placement of the first pass, less the three round-0 launches the absorb kernels replace.

    python scripts/ccm_bench.py [--frames 64] [--rounds 10] [--runs 5] [--out profiles/ccm_64.json]
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
TAG_LEN = 8
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=None, help="default: profiles/ccm_<frames>.json")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    out_path = args.out or os.path.join(ROOT, "profiles", f"ccm_{args.frames}.json")

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

    aad = bytes(range(8))
    msgs = [bytes((f * 5 + i * 7 + 3) & 255 for i in range(32)) for f in range(nf)]
    nonces = [bytes([0x10, 0x11, 0x12]) + f.to_bytes(10, "big") for f in range(nf)]
    frames = [(0, nonces[f], aad, aes_var.ccm_encrypt_plain(KEY, nonces[f], aad, msgs[f], TAG_LEN, rounds))
              for f in range(nf)]
    sizes = {"many": (4 * nf, nf, nf, nf), "one": (4, 1, 1, 1)}
    out_plain = torch.empty((32 * nf, 8, L), dtype=torch.int64, device="cuda:0")
    out_diff = torch.empty((nf, TAG_LEN, 8, L), dtype=torch.int64, device="cuda:0")
    blocks = torch.zeros((4 * nf, 128, L), dtype=torch.int64, device="cuda:0")  # trivial zero blocks
    enc = torch.empty_like(blocks)
    key_of = np.zeros(4 * nf, dtype=np.int32)
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

    def run_a(n=nf):
        M.ccm_transcipher_device(ctx, 128, rk_dev.data_ptr(), 1, frames[:n], TAG_LEN, rounds, out_plain.data_ptr(),
                                 out_diff.data_ptr())

    def run_b(which="many"):
        for nb in sizes[which]:
            V.encrypt_blocks_device(ctx, 128, rk_dev.data_ptr(), blocks.data_ptr(), nb, rounds, enc.data_ptr())

    def keyed(nb):
        M.encrypt_blocks_device(ctx, 128, rk_dev.data_ptr(), 1, key_of[:nb], blocks.data_ptr(), nb, rounds,
                                enc.data_ptr())

    paths = (("a", run_a), ("b", run_b), ("a1", lambda: run_a(1)), ("b1", lambda: run_b("one")))
    for _, fn in paths:
        fn()
    run_a()
    got = ck.decrypt_bits_raw(out_plain.cpu().numpy().view(np.uint64).reshape(-1, L)).reshape(-1, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in got) == b"".join(msgs), "CCM does not decrypt to the payloads"
    assert not ck.decrypt_bits_raw(out_diff.cpu().numpy().view(np.uint64).reshape(-1, L)).any(), "a tag differs"

    ms = {k: [] for k, _ in paths}
    for _ in range(args.runs):
        for k, fn in paths:
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    st_a = stages(run_a)
    st_k = [stages(lambda nb=nb: keyed(nb)) for nb in sizes["many"]]
    linear_k = sum(s["linear"] for s in st_k)
    res = {
        "what": "ccm_transcipher_device (a) against encrypt_blocks_device at the batch sizes 4F, F, F, F (b); a1 / b1 "
                "the same for one frame; k = the keyed block cipher at the sizes of (b), stage times only",
        "frames": nf, "aad_bytes": 8, "payload_bytes": 32, "tag_bytes": TAG_LEN, "rounds": rounds, "runs": args.runs,
        "batches": list(sizes["many"]),
        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in ms.items()},
        **{f"{k}_median_ms": round(v, 3) for k, v in med.items()},
        **{f"{k}_spread": round(v, 4) for k, v in spread.items()},
        "a_minus_b_ms": round(med["a"] - med["b"], 3),
        "larger_spread_ms": round(max(spread["a"] * med["a"], spread["b"] * med["b"]), 3),
        "ratio_a_over_b": round(med["a"] / med["b"], 4),
        "a1_minus_b1_ms": round(med["a1"] - med["b1"], 3),
        "outputs_decrypt_correctly": True,
        "a_stage_ms": st_a, "k_stage_ms": st_k,
        "linear_a_minus_k_ms": round(st_a["linear"] - linear_k, 3),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
