"""The tilings of tests/test_gpu_whole_device.py on the CPU: for every case and both CU counts of the card
family, the pattern that the GPU test will use has the three properties of tiled_batches.check_pattern, stated
here once more in plain loops, and the batch sizes follow the sizing rule.  `compare` is run on CPU tensors:
it passes on a faithful batch and names workgroup, slot, source and word of a wrong one."""
import numpy as np
import pytest

from tests import tiled_batches as T

CASES = [(cu, name) for cu in T.CU_COUNTS for name in T.sizes(cu)]


@pytest.mark.parametrize("cu,name", CASES)
def test_pattern_properties(cu, name):
    B, D, seed, window = T.sizes(cu)[name]
    src = T.tiling(B, D, seed, window)
    assert src.shape == (B,) and np.array_equal(src, T.tiling(B, D, seed, window))  # seeded: the same every time
    assert D > window and (window == T.WINDOW or name == "aes")
    # distinct windows
    for i in range(B - window + 1):
        assert len(set(src[i:i + window].tolist())) == window, i
    # every source in every slot
    for C in range(1, window + 1):
        for j in range(C):
            assert {int(src[i]) for i in range(j, B, C)} == set(range(D)), (C, j)
    # no hiding stride
    want = {c * x for c in (1, 2, 3, 4) for x in (256, 304)} | {128, 384, D}
    assert set(T.strides(D)) == want
    for P in want:
        if P < B:
            equal = sum(int(src[i] == src[i + P]) for i in range(B - P))
            assert 2 * equal < B - P, (P, equal, B - P)


def test_assignment_draws_every_free_source():
    """Uniform among the free sources: over a long batch every source follows every other one (at distance 4,
    where it is free again) about equally often."""
    D = 7
    src = T.assignment(20000, D, 5)
    T.check_pattern(src, D)
    counts = np.bincount(src, minlength=D)
    assert counts.min() > 0.9 * len(src) / D and counts.max() < 1.1 * len(src) / D
    with pytest.raises(AssertionError):
        T.assignment(10, 4, 0)  # D >= 5 for windows of four


def test_check_pattern_refuses_bad_tilings():
    with pytest.raises(AssertionError, match="window"):
        T.check_pattern(np.resize(np.array([0, 1, 2, 0, 3, 4, 5, 6]), 2000), 7)
    with pytest.raises(AssertionError, match="slot"):
        T.check_pattern(np.resize(np.arange(8), 2000), 8)  # period 8: slot j of four holds sources j and j + 4 only
    # period 1024 = 4 x 256 (a period whose ends fit together, so that windows and slots are in order)
    period = next(a for a in (T.assignment(1024, 7, s) for s in range(100)) if len(set(a[-3:]) | set(a[:3])) == 6)
    with pytest.raises(AssertionError, match="stride"):
        T.check_pattern(np.resize(period, 3000), 7)


@pytest.mark.parametrize("cu", T.CU_COUNTS)
def test_sizing_rule(cu):
    s = {k: v[0] for k, v in T.sizes(cu).items()}
    wgs = lambda B, C: (B + C - 1) // C
    # C per workgroup, O per CU: more than 2 O CU workgroups, the last one partial
    for name, C, O in (("br512x4", 3, 1), ("br512p16", 2, 1), ("br1024w", 4, 3), ("br1024_nowide", 2, 1), ("s1", 3, 1)):
        assert wgs(s[name], C) > 2 * O * cu and s[name] % C != 0, name
    # Engine::bootstrap's selection (kernels.hip): nothing of these batches goes to br512lat ...
    for name, C in (("br512x4", 3), ("br512p16", 2)):
        assert s[name] % (C * cu) > min(256, cu), name
    # ... the split batch gives it five rows after two whole rounds, and the latency kernels run one per CU
    assert s["br512split"] // (3 * cu) == 2 and s["br512split"] % (3 * cu) == 5
    assert s["br512lat"] == min(256, cu) and s["br1024lat"] == s["br1024_one_paired"] == s["br1024_one_unpaired"] == cu
    assert s["br1024_occ2"] > 2 * 2 * cu
    assert cu < s["br1024"] < 4 * cu <= s["br1024w"] and s["br1024"] % 2 == 1 and wgs(s["br1024"], 2) == 2 * cu
    # gemm<1, 8>: two workgroups per CU, 128-row m-tiles, the last of one row
    for name, n in (("ks64", 677), ("ks8", 785)):
        n_tiles = -(-(n + 1) * 8 // 128)
        assert wgs(s[name], 128) * n_tiles > 2 * 2 * cu and s[name] % 128 == 1, name
    assert s["vp64"] * 8 > 2 * cu and s["vp8"] * 4 > 2 * cu
    assert s["cbs"] == 300 and s["aes"] == 128
    if cu == 256:
        assert s == {"br512x4": 1793, "br512p16": 1281, "br512lat": 256, "br512split": 1541, "br1024lat": 256,
                     "br1024": 1023, "br1024w": 6145, "br1024_nowide": 1025, "br1024_one_paired": 256,
                     "br1024_one_unpaired": 256, "br1024_occ2": 1025, "s1": 1793, "ks64": 3201, "ks8": 2817, "vp64": 65, "vp8": 129,
                     "cbs": 300, "aes": 128}


def test_expand_and_compare_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    refs = torch.from_numpy(rng.integers(-2**62, 2**62, size=(7, 3, 50), dtype=np.int64))
    src = T.assignment(200, 7, 9)
    batch = T.expand(refs, src)
    assert batch.shape == (200, 3, 50) and all(torch.equal(batch[i], refs[src[i]]) for i in range(200))
    T.compare(batch, refs, src, 3, "faithful")
    # one word of one row, and a swap of two slots of one workgroup
    bad = batch.clone()
    bad[100, 1, 7] += 1
    bad[[30, 31]] = bad[[31, 30]]
    with pytest.raises(AssertionError) as e:
        T.compare(bad, refs, src, 3, "seeded")
    msg = str(e.value)
    assert "seeded: 3 of 200 rows differ" in msg
    assert "position 30: workgroup 10 slot 0 source %d first differing word" % src[30] in msg
    assert "position 100: workgroup 33 slot 1 source %d first differing word 57" % src[100] in msg
    # a reference per (source, test vector): ref_of
    refs2 = torch.cat([refs, refs + 1])
    ref_of = src + 7 * (np.arange(200) % 2)
    out2 = batch + torch.from_numpy(np.arange(200) % 2).reshape(-1, 1, 1)
    T.compare(out2, refs2, src, 3, "two test vectors", ref_of=ref_of)
    with pytest.raises(AssertionError, match="rows"):
        T.compare(batch[:199], refs, src, 3, "a row short")
