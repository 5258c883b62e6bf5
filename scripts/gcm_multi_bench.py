#!/usr/bin/env python3
"""GCM over key tables against the single-key calls, key by key, in one process.

K AES-128 keys (default 16) resident on the device as one key table, F frames per key (default 4) of an 8-byte AAD and a
32-byte payload, tag of 16 bytes, 10 rounds.  After one warm-up of each, alternates timed runs of
  (mk4, mk16)  M.ghash_key_device over the table at n_powers = 4 and 16,
  (sk4, sk16)  K sequential V.ghash_key_device calls, one per slot                  -- the yardstick,
  (mg)         M.gcm_transcipher_device on all K F frames in one call,
  (sg)         K sequential V.gcm_transcipher_device calls of F frames each        -- the yardstick.
The single-key calls are unchanged by the key-table path.  Checks that the tables of both paths hold the same words
and that (mg) writes the words of (sg), decrypts the payloads, and writes one JSON line: per-run ms, medians, spread =
(max - min) / median, and the stage times and PBS launch counts of one more run of each (summed over the K calls for
the sequential paths).

    python scripts/gcm_multi_bench.py [--keys 16] [--frames-per-key 4] [--rounds 10] [--runs 5] [--out profiles/gcm_multi.json]
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
TAG_LEN = 16
STAGES = ("keyswitch", "pbs", "pfks", "ggsw_fft", "vertical_packing", "extract_bits", "linear", "pbs_launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--frames-per-key", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of each path (at least 5)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcm_multi.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")

    import torch  # device memory only
    import tfhe_aes
    from tfhe_aes import _native as N
    from tfhe_aes import aes_128, aes_multi, aes_var

    V, M = aes_var.GalMulAes, aes_multi.GalMulAesMulti
    pid = tfhe_aes.PARAMS_SQRD_LVL_64
    L = tfhe_aes.bit_len(pid)
    nk, fpk, rounds = args.keys, args.frames_per_key, args.rounds
    nf = nk * fpk
    threads = min(16, os.cpu_count() or 1)
    ck, raw = tfhe_aes.generate_keys_raw(pid, SEED, threads=threads)
    ctx = tfhe_aes.context_from_raw(pid, raw, device=0)
    keys = [bytes((0x31 * s + 0x0B * i + 5) & 255 for i in range(16)) for s in range(nk)]
    table = np.stack([ck.encrypt_bits_raw([b for byte in b"".join(aes_var.key_schedule_plain(k))
                                           for b in aes_128.u8_to_bits(byte)]) for k in keys])
    tab_dev = torch.from_numpy(table.view(np.int64)).to("cuda:0")
    kw = table.shape[1]

    def dev(shape):
        return torch.empty(shape, dtype=torch.int64, device="cuda:0")

    def bytes_of(t):
        bits = ck.decrypt_bits_raw(t.cpu().numpy().view(np.uint64).reshape(-1, L)).reshape(-1, 8)
        return bytes(aes_128.bits_to_u8(b) for b in bits)

    def stage_values():
        v = (C.c_float * 8)()
        N.check(N.lib().tae_last_stage_times_v2(ctx._h, v))
        return [float(x) for x in v]

    def stages(calls):
        """The stage times of a path, summed over its calls."""
        ctx.set_timing(True)
        total = [0.0] * 8
        for fn in calls:
            fn()
            total = [a + b for a, b in zip(total, stage_values())]
        ctx.set_timing(False)
        return {k: (int(x) if k == "pbs_launches" else round(x, 3)) for k, x in zip(STAGES, total)}

    def timed(calls):
        t0 = time.perf_counter()
        for fn in calls:
            fn()  # device outputs are complete when a call returns
        return (time.perf_counter() - t0) * 1e3

    aad = bytes(range(8))
    msgs = [bytes((f * 5 + i * 7 + 3) & 255 for i in range(32)) for f in range(nf)]
    ivs = [bytes([0x10, 0x11]) + f.to_bytes(10, "big") for f in range(nf)]
    slot_of = [f // fpk for f in range(nf)]  # frames in slot order, so the sequential results concatenate to the call's
    data = [aes_var.gcm_encrypt_plain(keys[slot_of[f]], ivs[f], aad, msgs[f], TAG_LEN, rounds) for f in range(nf)]
    m_frames = [(slot_of[f], ivs[f], aad, data[f]) for f in range(nf)]
    s_frames = [[(ivs[f], aad, data[f]) for f in range(s * fpk, (s + 1) * fpk)] for s in range(nk)]
    mhk = {n: dev((nk, n, 128, L)) for n in (4, 16)}
    shk = {n: dev((nk, n, 128, L)) for n in (4, 16)}
    m_plain, m_diff = dev((32 * nf, 8, L)), dev((nf, TAG_LEN, 8, L))
    s_plain, s_diff = dev((32 * nf, 8, L)), dev((nf, TAG_LEN, 8, L))
    torch.cuda.synchronize()

    def mk(n):
        return [lambda: M.ghash_key_device(ctx, 128, tab_dev.data_ptr(), nk, n, rounds, mhk[n].data_ptr())]

    def sk(n):
        return [lambda s=s: V.ghash_key_device(ctx, 128, tab_dev[s].data_ptr(), n, rounds, shk[n][s].data_ptr())
                for s in range(nk)]

    mg = [lambda: M.gcm_transcipher_device(ctx, 128, tab_dev.data_ptr(), nk, mhk[4].data_ptr(), 4, m_frames, TAG_LEN,
                                           rounds, m_plain.data_ptr(), m_diff.data_ptr())]
    sg = [lambda s=s: V.gcm_transcipher_device(ctx, 128, tab_dev[s].data_ptr(), shk[4][s].data_ptr(), 4, s_frames[s],
                                               TAG_LEN, rounds, s_plain[32 * fpk * s:].data_ptr(), s_diff[fpk * s:].data_ptr())
          for s in range(nk)]
    paths = (("mk4", mk(4)), ("sk4", sk(4)), ("mk16", mk(16)), ("sk16", sk(16)), ("mg", mg), ("sg", sg))
    for _, calls in paths:
        timed(calls)  # the warm-up
    assert kw == 44 * 32
    for n in (4, 16):
        assert torch.equal(mhk[n], shk[n]), "the key-table path and the single-key path give different power tables"
    assert torch.equal(m_plain, s_plain) and torch.equal(m_diff, s_diff), "the frame calls give different words"
    assert bytes_of(m_plain) == b"".join(msgs), "GCM does not decrypt to the payloads"
    assert not any(bytes_of(m_diff)), "a tag differs"

    ms = {k: [] for k, _ in paths}
    for _ in range(args.runs):
        for k, calls in paths:
            ms[k].append(timed(calls))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    st = {k: stages(calls) for k, calls in paths}
    res = {
        "what": "GCM over a key table (mk4, mk16: ghash_key_device at 4 and 16 powers; mg: gcm_transcipher_device, one "
                "call) against the single-key calls slot by slot (sk4, sk16, sg: the sum of `keys` sequential calls)",
        "keys": nk, "frames_per_key": fpk, "frames": nf, "aad_bytes": 8, "payload_bytes": 32, "tag_bytes": TAG_LEN,
        "rounds": rounds, "runs": args.runs,
        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in ms.items()},
        **{f"{k}_median_ms": round(v, 3) for k, v in med.items()},
        **{f"{k}_spread": round(v, 4) for k, v in spread.items()},
        "mk4_over_sk4": round(med["mk4"] / med["sk4"], 4), "mk16_over_sk16": round(med["mk16"] / med["sk16"], 4),
        "mg_over_sg": round(med["mg"] / med["sg"], 4),
        "same_words_as_single_key": True, "outputs_decrypt_correctly": True,
        **{f"{k}_stage_ms": v for k, v in st.items()},
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
