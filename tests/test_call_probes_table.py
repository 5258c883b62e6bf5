"""Keeps tests/call_probes.py honest against the source (CPU only): every device buffer the Engine owns is either walked
by some probe (USES) or listed, with a reason, as something no call rewrites; and the adjacency walk of
tests/test_gpu_call_order.py runs every ordered pair of probes that share a buffer back to back."""
import os
import re

import pytest

from tests import call_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe-aes-2_amd", "csrc")
MEMBER = re.compile(r"\bd_\w+_\b")


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _code(src):
    """The source without its // comments (the members named in prose do not count)."""
    return "\n".join(line.split("//")[0] for line in src.splitlines())


def engine_members():
    """The d_..._ data members of class Engine."""
    src = _code(_read("engine.hpp"))
    body = src[src.index("class Engine"):]
    return set(MEMBER.findall(body))


def grown_members():
    """The members the drivers call .grow( or .upload( on (rowsum_pass: through its up( helper) or pass to ensure_digits(:
    the buffers a call may free and reallocate."""
    out = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")):
            continue
        for m in re.finditer(r"\b(d_\w+_)\.(?:grow|upload)\(|\b(?:up|ensure_digits)\(\s*(d_\w+_)\b", _code(_read(name))):
            out.add(m.group(1) or m.group(2))
    return out


def test_the_parsers_see_the_engine():
    members, grown = engine_members(), grown_members()
    assert len(members) >= 60 and {"d_state_", "d_rs_pub_", "d_gcm_a_", "d_s1_tv_", "d_bsk_f_"} <= members
    assert len(grown) >= 40 and {"d_state_", "d_digits_", "d_key_of_", "d_rs_pub_", "d_acc_w_"} <= grown
    assert grown <= members


def test_every_buffer_has_a_probe_or_a_reason():
    probed = set().union(*P.USES.values())
    members, grown = engine_members(), grown_members()
    assert not probed & set(P.NOT_SCRATCH), "a buffer is either probed or exempt"
    missing = members - probed - set(P.NOT_SCRATCH)
    assert not missing, "no probe walks %s: add one to tests/call_probes.py (or a reason to NOT_SCRATCH)" % sorted(missing)
    assert probed | set(P.NOT_SCRATCH) <= members, sorted((probed | set(P.NOT_SCRATCH)) - members)
    # whatever a driver grows or uploads into is scratch: it needs a probe, a reason does not do
    assert grown - {"d_clk_"} <= probed, sorted(grown - probed)
    assert all(len(reason.split()) >= 2 for reason in P.NOT_SCRATCH.values())


def test_the_table_has_a_row_per_probe():
    assert set(P.USES) == set(P.BY_NAME) and len(P.BY_NAME) == len(P.PROBES)
    for p in P.PROBES:
        assert p.params in P.PARAM_SETS and p.size in ("small", "large"), p.name
    for fam, names in P.families().items():
        assert P.BY_NAME[names[0]].size == "small", fam  # every family starts from a small probe
        assert len({P.BY_NAME[n].params for n in names}) == 1, fam


@pytest.mark.parametrize("params", sorted(P.PARAM_SETS))
def test_the_walk_covers_every_sharing_pair(params):
    pairs = P.sharing_pairs(params)
    seq = P.adjacency_sequence(params)
    assert pairs, params
    assert pairs <= P.covered_pairs(seq), sorted(pairs - P.covered_pairs(seq))
    assert set(seq) <= set(P.small_probes(params))
    # ... and so do the pieces the GPU module runs, each of a few dozen calls
    pieces = P.adjacency_pieces(params)
    in_pieces = set().union(*(P.covered_pairs(piece) for piece in pieces))
    assert pairs <= in_pieces
    assert all(2 <= len(piece) <= P.PIECE + 1 for piece in pieces)
    assert len(seq) <= len(pairs) + len(P.small_probes(params))  # an Euler circuit per component: no pair twice
