"""Whole-device batches assembled from a few distinct rows (tests/test_gpu_whole_device.py).

The oracle is too slow for thousands of distinct rows, and it does not have to check them: a batch of B rows
tiled from D distinct sources needs D oracle calls, and then every one of the B positions can be compared word
for word.  What the tiling must not do is hide a mistake: a kernel that reads its neighbour's slot, or the row
a tile height or a round of workgroups away, has to meet a different source there.  `assignment` draws the
pattern, `check_pattern` states the three properties it must have (test_tiled_batches.py pins them on the CPU
for every shape the GPU tests use), `sizes` derives the batch sizes from the CU count, and `expand` /
`compare` work on device tensors so that no test builds a gigabyte on the host.
"""
import numpy as np

WINDOW = 4            # the largest ciphertexts-per-workgroup of any kernel (br1024w)
CU_COUNTS = (256, 304)
TILE_HEIGHTS = (128, 384)  # rows per m-tile of gemm<1, 8> / the row-layout PFKS GEMM, and of the K-layout PFKS GEMMs
BR_LAT_MAX = 256      # the default TAE_BR_LAT_MAX


def assignment(B: int, D: int, seed: int, window: int = WINDOW) -> np.ndarray:
    """src_of[0..B): the distinct source row placed at each batch position.  Each position takes a source
    uniformly among those not used in the previous window - 1 positions, so every `window` consecutive
    positions hold `window` distinct sources (D > window).  Ciphertext batches use the default window of 4;
    batches of AES blocks (128 ciphertexts each, far wider than any workgroup) are tiled from three blocks
    with window = 2: neighbours differ."""
    assert D > window >= 1 and B >= 1
    rng = np.random.default_rng(seed)
    src = np.empty(B, dtype=np.int64)
    for i in range(B):
        recent = src[max(0, i - (window - 1)):i]
        free = np.setdiff1d(np.arange(D), recent)
        src[i] = free[rng.integers(len(free))]
    return src


def strides(D: int) -> list:
    """Every distance at which a kernel could read a counterpart row: C x CUs for C ciphertexts per workgroup
    (the same slot one round of workgroups later), the GEMM tile heights, and the number of sources."""
    return sorted({c * cu for c in range(1, WINDOW + 1) for cu in CU_COUNTS} | set(TILE_HEIGHTS) | {D})


def check_pattern(src_of: np.ndarray, D: int, window: int = WINDOW, extra_strides=()) -> None:
    """The three properties of a tiling (assertions; the message names the property that fails)."""
    src_of = np.asarray(src_of)
    B = len(src_of)
    assert src_of.min() >= 0 and src_of.max() < D
    # distinct windows: a swap of two slots inside a workgroup changes words
    for d in range(1, window):
        same = np.nonzero(src_of[d:] == src_of[:-d])[0]
        assert same.size == 0, ("window", window, "positions", int(same[0]), int(same[0]) + d)
    # every source in every slot of every workgroup size: crafted rows reach every slot
    for C in range(1, window + 1):
        for j in range(min(C, B)):
            missing = set(range(D)) - set(src_of[j::C].tolist())
            assert not missing, ("slot", j, "of", C, "never holds sources", sorted(missing))
    # no hiding stride: a row read from P positions away is another source more often than not
    for P in sorted(set(strides(D)) | set(extra_strides)):
        if P < B:
            share = float(np.mean(src_of[P:] == src_of[:-P]))
            assert share < 0.5, ("stride", P, "share of equal sources", share)


def tiling(B: int, D: int, seed: int, window: int = WINDOW) -> np.ndarray:
    """The assignment of a case, checked: a pattern without the three properties raises.  The seeds in `sizes`
    are pinned so that every case passes at both CU counts of CU_COUNTS (test_tiled_batches.py); a batch of a few
    dozen positions per slot can miss a source in some slot, and such a case got another seed there."""
    src_of = assignment(B, D, seed, window)
    check_pattern(src_of, D, window)
    return src_of


def sized(C: int, O: int, CU: int) -> int:
    """The sizing rule for a kernel with C rows per workgroup and a launch-bounds occupancy of O workgroups per
    CU: the smallest batch whose workgroup count exceeds 2 O CU with a last workgroup of one row (partial for
    C > 1)."""
    return C * 2 * O * CU + 1


def ks_rows(n_small: int, CU: int) -> int:
    """tae_stage_keyswitch on gemm<1, 8> (128 x 128 tiles, launch bounds of two workgroups per CU): two m-tiles
    more than the smallest count whose grid exceeds 2 x 2 x CU workgroups, the last m-tile of one row.  The
    grid then exceeds the bound by more than a whole column of n-tiles."""
    n_tiles = ((n_small + 1) * 8 + 127) // 128
    m_tiles = 4 * CU // n_tiles + 1 + 2
    return (m_tiles - 1) * 128 + 1


def sizes(CU: int) -> dict:
    """case -> (batch positions B, distinct sources D, seed, window), the arguments of `tiling`.  A position is a
    ciphertext, except for the vertical packing and the circuit bootstrap (a group of 8 selector bits) and the AES
    case (a block)."""
    lat = min(CU, BR_LAT_MAX)
    return {
        # tae_stage_pbs_shift_boolean, params_sqrd_lvl_64
        "br512x4": (7 * CU + 1, 17, 1, WINDOW),       # 3 per workgroup, O = 1; remainder CU + 1 stays on br512x4
        "br512p16": (5 * CU + 1, 17, 2, WINDOW),      # 2 per workgroup, O = 1; remainder CU + 1 stays on br512p16
        "br512lat": (lat, 17, 20, WINDOW),             # one per workgroup, at most one workgroup per CU by selection
        "br512split": (6 * CU + 5, 17, 4, WINDOW),    # two whole br512x4 rounds + five rows on br512lat
        # tae_stage_pbs_shift_boolean, the 8-bit set
        "br1024lat": (CU, 17, 21, WINDOW),             # B <= CU by selection
        "br1024": (4 * CU - 1, 17, 6, WINDOW),        # CU < B < 4 CU by selection: its largest, 2 CU workgroups
        "br1024w": (sized(4, 3, CU), 17, 7, WINDOW),  # 4 per workgroup, O = 3
        "br1024_nowide": (sized(2, 1, CU), 17, 15, WINDOW),  # TAE_B1K_WIDE=0: br1024's two per workgroup by the rule
        # the selections behind the A/B knobs: one per workgroup up to CU (TAE_B1K_LAT=0, with TAE_B1K_PAIR=1 / 0), and
        # one per workgroup at two workgroups per CU above it (TAE_B1K_OCC2=1: C = 1, O = 2)
        "br1024_one_paired": (CU, 17, 22, WINDOW),
        "br1024_one_unpaired": (CU, 17, 34, WINDOW),
        "br1024_occ2": (sized(1, 2, CU), 17, 18, WINDOW),
        # tae_s1_bootstrap, shortint_1bit: br512x4<7, true, 6>
        "s1": (7 * CU + 1, 17, 8, WINDOW),
        # tae_stage_keyswitch
        "ks64": (ks_rows(677, CU), 7, 9, WINDOW),
        "ks8": (ks_rows(785, CU), 7, 10, WINDOW),
        # tae_stage_vertical_packing: 24 outputs on 8 workgroups (O = 1) / 8 outputs on 4 workgroups (O = 1) per group
        "vp64": (2 * CU // 8 + 1, 7, 65, WINDOW),
        "vp8": (2 * CU // 4 + 1, 7, 12, WINDOW),
        # tae_circuit_bootstrap_raw 8 -> 24: 2400 bootstraps, 7 K-layout m-tiles
        "cbs": (300, 7, 13, WINDOW),
        # encrypt_blocks_raw: 128 blocks from three
        "aes": (128, 3, 14, 2),
    }


def expand(rows, src_of):
    """rows [D][...] (device tensor) -> the batch [B][...] with row src_of[i] at position i, on the device."""
    import torch
    idx = torch.from_numpy(np.ascontiguousarray(src_of, dtype=np.int64)).to(rows.device)
    return rows.index_select(0, idx).contiguous()


def compare(out, refs, src_of, C: int, what, ref_of=None) -> None:
    """Every row of out [B][...] equals the reference row of its source, refs [R][...] (device tensors of the same
    word type).  Row i is compared with refs[ref_of[i]]; ref_of defaults to src_of (it differs where a reference
    depends on more than the source, e.g. on the test vector i % 2).  No position is left out.  C is the rows
    per workgroup (or per tile) of the kernel, for the message only."""
    import torch
    src_of = np.asarray(src_of)
    ref_of = src_of if ref_of is None else np.asarray(ref_of)
    B = out.shape[0]
    assert B == len(src_of) == len(ref_of), (what, "rows", B, "positions", len(src_of))
    o, r = out.reshape(B, -1), refs.reshape(refs.shape[0], -1)
    assert o.dtype == r.dtype and o.shape[1] == r.shape[1], (what, o.dtype, r.dtype, o.shape, r.shape)
    idx = torch.from_numpy(np.ascontiguousarray(ref_of, dtype=np.int64)).to(o.device)
    wrong = torch.zeros(B, dtype=torch.bool, device=o.device)
    step = max(1, (1 << 25) // o.shape[1])  # about 256 MB of expected words at a time
    for a in range(0, B, step):
        wrong[a:a + step] = (o[a:a + step] != r.index_select(0, idx[a:a + step])).any(dim=1)
    n_wrong = int(wrong.sum())
    if n_wrong:
        lines = []
        for i in wrong.nonzero().flatten()[:10].tolist():
            word = int((o[i] != r[int(ref_of[i])]).nonzero()[0])
            lines.append("position %d: workgroup %d slot %d source %d first differing word %d"
                         % (i, i // C, i % C, int(src_of[i]), word))
        raise AssertionError("%s: %d of %d rows differ from the oracle (%d rows per workgroup)\n  %s"
                             % (what, n_wrong, B, C, "\n  ".join(lines)))
