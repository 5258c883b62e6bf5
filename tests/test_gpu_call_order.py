"""A call's output depends on its inputs alone: call-order and cold-context parity for every Engine entry point.

engine.hpp keeps some sixty grow-on-demand device buffers that about fifteen entry-point families share, and the rest
of the GPU suite visits one warm context per parameter set in one fixed file order.  Here every probe of
tests/call_probes.py (the smallest deterministic call that still walks its entry point's buffers, decoded once against
the plain model) is compared word for word, `np.array_equal` on whole outputs, with its own output as the FIRST call of
a fresh context:

- cold: a fresh context runs a family's small probes, its large ones, the small ones again;
- forward / reverse: one fresh context runs all probes in list order, another in reverse;
- adjacent sharers: every ordered pair of small probes that share a buffer (call_probes.USES) runs back to back at
  least once on one context, in parametrised pieces that also pass alone, with the suite's refused calls in between;
- timing on: the forward order with set_timing(True) gives the same words and, per probe, the launch counts of the
  probe timed as the first call of a fresh context (nothing accumulates, the event pool is recycled);
- caller stream: a mode-layer device entry point whose keys arrive by a non-blocking copy on a side stream.

Free device memory is poisoned before each fresh context: a few GiB are filled with -1 and released, so that the
engine's new allocations are unlikely to start out zeroed.  That is best effort: nothing makes the allocator hand the
same pages back.  Every fresh context is deleted when its test is done; at most two live next to the session's.
"""
import gc

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tests import call_probes as P
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

POISON_WORDS = (2 << 30) // 8  # 2 GiB of int64
PARAMS = (P.LVL64, P.W8, P.S1BIT)


def _poison():
    import torch
    fill = torch.full((POISON_WORDS,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    del fill
    torch.cuda.empty_cache()


def _counts(ctx):
    t = ctx.last_stage_times()
    return t["pbs_launches"], t["pbs_main_cts"]


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


class Bench:
    """The module's keys, inputs and cold references (made on demand, once)."""

    def __init__(self, raw):
        self.raw = raw
        self.cold_words, self.cold_counts = {}, {}
        self.x = None

    def fresh(self, params, timing=False):
        if tfhe_aes.device_count() < 1:
            pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
        gc.collect()
        _poison()
        ctx = tfhe_aes.context_from_raw(P.PARAM_SETS[params], self.raw[params][1], device=0)
        if timing:
            ctx.set_timing(True)
        return ctx

    def inputs(self):
        if self.x is None:
            import torch
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            x = P.build_inputs(self.raw[P.LVL64][0], self.raw[P.W8][0], self.raw[P.S1BIT][0], cus)
            ctx = self.fresh(P.LVL64)
            P.build_stage_chain(ctx, x)
            del ctx
            self.x = x
        return self.x

    def cold(self, name):
        """The probe's output as the first call of a fresh context, checked once against the plain model."""
        if name not in self.cold_words:
            probe, x = P.BY_NAME[name], self.inputs()
            ctx = self.fresh(probe.params)
            out = probe.run(ctx, x)
            del ctx
            probe.check(x, out)
            if probe.family == "stage":
                assert np.array_equal(out[0], x["stage_" + name])  # the chain that ends in stage_vp's decoded value
            self.cold_words[name] = out
        return self.cold_words[name]

    def cold_timed(self, name):
        """The launch counts of the probe timed as the first call of a fresh context; its words are the cold ones."""
        if name not in self.cold_counts:
            probe = P.BY_NAME[name]
            want = self.cold(name)
            ctx = self.fresh(probe.params, timing=True)
            out = probe.run(ctx, self.inputs())
            self.cold_counts[name] = _counts(ctx)
            del ctx
            assert _same(out, want), name
        return self.cold_counts[name]

    def run_and_compare(self, ctx, names):
        for name in names:
            self.cold(name)  # before the first call: a reference made later would put a third context next to ctx
        for i, name in enumerate(names):
            got = P.BY_NAME[name].run(ctx, self.x)
            assert _same(got, self.cold(name)), "%s differs from its cold reference as call %d of %s" % (name, i, names)


@pytest.fixture(scope="module")
def bench(product_raw, product_raw8):
    raw = {P.LVL64: product_raw, P.W8: product_raw8,
           P.S1BIT: tfhe_aes.generate_keys_raw(tfhe_aes.PARAMS_SHORTINT_1BIT, SEED, threads=16)}
    return Bench(raw)


# ---- cold --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(P.families()))
def test_cold_family(bench, family):
    """Small probes, large probes, the small ones again, as the very first calls of a fresh context."""
    names = P.families()[family]
    small = [n for n in names if P.BY_NAME[n].size == "small"]
    seq = names + small
    for n in seq:
        bench.cold(n)
    ctx = bench.fresh(P.BY_NAME[names[0]].params)
    outs = [P.BY_NAME[n].run(ctx, bench.x) for n in seq]
    del ctx
    for i, (n, out) in enumerate(zip(seq, outs)):
        assert _same(out, bench.cold(n)), "%s differs from its cold reference as call %d of %s" % (n, i, seq)
    for j, n in enumerate(small):
        assert _same(outs[j], outs[len(names) + j]), n


def test_every_probe_has_a_family_and_a_table_row():
    assert {n for names in P.families().values() for n in names} == set(P.BY_NAME) == set(P.USES)


# ---- forward and reverse -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", (False, True), ids=("forward", "reverse"))
@pytest.mark.parametrize("params", PARAMS)
def test_list_order(bench, params, reverse):
    names = [p.name for p in P.PROBES if p.params == params]
    names = names[::-1] if reverse else names
    for n in names:
        bench.cold(n)
    ctx = bench.fresh(params)
    try:
        bench.run_and_compare(ctx, names)
    finally:
        del ctx


# ---- adjacent sharers, refusals in between ---------------------------------------------------------------------------
def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def _refusals(ctx, x):
    """The refused calls the suite already knows (test_gpu_gcm / _ccm / _xts / _edges), as (call, code)."""
    rk, hk, dk = x["gcm_rk"], x["gcm_hk"], x["dk"]
    tag = bytes(16)
    if "big_hk" not in x:
        x["big_hk"] = np.zeros((128, 128, P.BIG), dtype=np.uint64)  # never read: the refusal comes first
    long_frame = (P.R.IV3, b"", bytes([0xA5]) * (99 * 16) + tag)
    slot, nonce, aad, frame = x["ccm_single"]
    lut8 = ctx.generate_lookup_table(8, 8, lambda v: v)
    return [
        (lambda: P.V.gcm_transcipher_raw(ctx, rk, x["big_hk"], [long_frame], 16), N.TAE_E_NOISE),
        (lambda: P.V.gcm_transcipher_raw(ctx, rk, hk, [(P.R.IV3, b"", tag)], 5), N.TAE_E_PARAM),
        (lambda: P.V.gcm_transcipher_raw(ctx, rk, hk, [(P.R.IV3, bytes(80), tag)], 16), N.TAE_E_PARAM),  # m = 6 > 4
        (lambda: P.V.ccm_transcipher_raw(ctx, x["rk"][slot], bytes(6), aad, frame, 8), N.TAE_E_PARAM),
        (lambda: P.V.ccm_transcipher_raw(ctx, x["rk"][slot], nonce, aad, frame, 8, rounds=1), N.TAE_E_PARAM),
        (lambda: P.V.xts_transcipher_raw(ctx, dk, x["rk"][1], [(P.XTS_UNIT, bytes(17))]), N.TAE_E_PARAM),
        (lambda: P.V.xts_masks_raw(ctx, x["xts_tweak_cts"], [0, 2], [0, 1]), N.TAE_E_ARG),
        (lambda: ctx.circuit_bootstrap_raw(np.zeros((1, 7, P.BIG), dtype=np.uint64), lut8), N.TAE_E_ARG),
    ]


class _Shared:
    """The one context the pieces of a run share: made for the first piece that asks, replaced when the parameter set
    or the timing mode changes, so that it and a cold reference's are the only fresh contexts alive."""
    key, ctx = None, None

    def get(self, bench, params, timing=False):
        if self.key != (params, timing):
            self.ctx = None
            self.ctx, self.key = bench.fresh(params, timing), (params, timing)
        return self.ctx


@pytest.fixture(scope="module")
def shared(bench):
    s = _Shared()
    yield s
    s.ctx = None


PIECES = [(params, i) for params in PARAMS for i in range(len(P.adjacency_pieces(params)))]


@pytest.mark.parametrize("params,piece", PIECES, ids=["%s-%02d" % pi for pi in PIECES])
def test_adjacent_sharers(bench, shared, params, piece):
    """One piece of the walk of call_probes.adjacency_sequence: every consecutive pair shares a buffer (or joins two
    components).  On lvl_64 a refused call goes between every third pair; the next probe's output must not notice."""
    names = P.adjacency_pieces(params)[piece]
    for n in names:
        bench.cold(n)
    ctx, x = shared.get(bench, params), bench.x
    refusals = _refusals(ctx, x) if params == P.LVL64 else []
    for i, name in enumerate(names):
        if refusals and i % 3 == 1:
            call, code = refusals[(piece + i // 3) % len(refusals)]
            assert _code(call) == code
        got = P.BY_NAME[name].run(ctx, x)
        assert _same(got, bench.cold(name)), "%s after %s differs from its cold reference" % (name, names[i - 1] if i else None)


# ---- timing on ---------------------------------------------------------------------------------------------------
TIMED = [(params, i) for params in PARAMS for i in range(len(P.timed_pieces(params)))]


@pytest.mark.parametrize("params,piece", TIMED, ids=["%s-%d" % pi for pi in TIMED])
def test_timing_on(bench, shared, params, piece):
    """The list order with set_timing(True), in pieces on one timed context: the words are the cold ones, and after
    every probe the launch counts are those of the probe timed as the first call of a fresh context."""
    names = P.timed_pieces(params)[piece]
    for n in names:
        bench.cold_timed(n)
    ctx = shared.get(bench, params, timing=True)
    for i, name in enumerate(names):
        got = P.BY_NAME[name].run(ctx, bench.x)
        counts = _counts(ctx)
        assert _same(got, bench.cold(name)), name
        assert counts == bench.cold_timed(name), (name, i, counts, bench.cold_timed(name))
    if params == P.LVL64 and piece == len(P.timed_pieces(params)) - 1:
        # the one documented exception (include/tfhe_aes_gpu.h, tae_last_pack_time): a pack leaves the per-stage
        # slots to the last batched call.  After the last probe, whose counts are not a cold context's, it must
        # change nothing; in the list it stands before every batched call and equals its cold counts above
        before = _counts(ctx)
        assert before[0] > 0 and before != bench.cold_timed("pack_3")
        assert _same(P.BY_NAME["pack_3"].run(ctx, bench.x), bench.cold("pack_3"))
        assert _counts(ctx) == before


# ---- caller stream -------------------------------------------------------------------------------------------------
def test_caller_stream_xts_device(bench):
    """xts_transcipher_device orders itself after the caller's stream only: both keys arrive by a non-blocking copy
    and an in-place fix-up on a torch side stream right before the call; the output equals the host-array call's.
    None restores the default."""
    torch = pytest.importorskip("torch")
    want = bench.cold("xts_3x2")[0]
    x = bench.x
    side = torch.cuda.Stream()
    h_dk = torch.from_numpy(x["dk"].view(np.int64)).pin_memory()
    h_rk = torch.from_numpy(x["rk"][1].view(np.int64)).pin_memory()
    d_dk = torch.zeros(h_dk.shape, dtype=torch.int64, device="cuda")
    d_rk = torch.zeros(h_rk.shape, dtype=torch.int64, device="cuda")
    d_out = torch.full(want.shape, -1, dtype=torch.int64, device="cuda")
    ctx = bench.fresh(P.LVL64)
    torch.cuda.synchronize()
    try:
        ctx.set_caller_stream(side)
        with torch.cuda.stream(side):
            d_dk.copy_(h_dk, non_blocking=True)
            d_rk.copy_(h_rk, non_blocking=True)
            d_rk.add_(0)
        P.V.xts_transcipher_device(ctx, 128, d_dk.data_ptr(), d_rk.data_ptr(), P.XTS_UNITS, 2, d_out.data_ptr())
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
        ctx.set_caller_stream(None)
        d_out.fill_(-1)
        torch.cuda.synchronize()
        P.V.xts_transcipher_device(ctx, 128, d_dk.data_ptr(), d_rk.data_ptr(), P.XTS_UNITS, 2, d_out.data_ptr())
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
    finally:
        ctx.set_caller_stream(None)
        del ctx
