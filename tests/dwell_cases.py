"""Read sets with move tables shared by the tests of the dwell channel (tests/test_dwell.py on the host, tests/test_dwell_gpu.py on the
device): three generated sets at the matrix depths 89 and 55, one of which goes through the over-deep selection, a set by hand that holds
every combination of I and D ops the rule names, and packed tables that take the table kernel to its step edges.  Every set is made once
and left unchanged by the tests."""
import functools
import os

import numpy as np

from clair3_amd import synthetic as syn
from tests.fa_cases import by_hand

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fa_dwell_tables.npz")

SETS = {
    "plain": (dict(n_sites=120, depth=30, read_len=(60, 200), seed=81), dict()),
    "every_op": (dict(n_sites=120, depth=25, read_len=(60, 200), seed=82, d_then_i=0.006, i_then_d=0.006, pad=0.2, eqx=True, ref_other=0.03,
                      non_acgt=0.02, ins=0.02, dele=0.01), dict(max_indel_length=2)),
    "over_deep": (dict(n_sites=50, depth=70, read_len=(60, 200), seed=83), dict(matrix_depth=55, seed=9)),
}
REF = "ACGT" * 100


@functools.lru_cache(maxsize=None)
def generated(name):
    """(rs, ex, moves, centres, cfg) of SETS[name], in coordinate order"""
    spec, cfg = SETS[name]
    rs0 = syn.make_read_set(**spec)
    ex0 = syn.make_read_extras(rs0, spec["seed"] + 1, duplicate_names=0.03)
    mv0 = syn.make_read_moves(rs0, ex0, spec["seed"] + 2, stall=0.03, untagged=0.08, surplus=0.08, short=0.08)
    rs = syn.sort_read_set(rs0)
    return rs, syn.sort_read_extras(rs0, ex0), syn.sort_read_moves(rs0, mv0), np.arange(rs["start"], rs["end"], 2), cfg


def moves_by_hand(tables):
    """c3_read_moves arrays from a list of per-read tables (None: no tag)"""
    t = [np.zeros(0, np.int8) if x is None else np.asarray(x, np.int8) for x in tables]
    return {"mv_first": np.concatenate([[0], np.cumsum([len(x) for x in t])]).astype(np.int64), "mv": np.concatenate(t) if t else np.zeros(0, np.int8)}


def table_of(dwells, stride=5, lead=0, value=1):
    """the move table of a read whose k-th base dwells dwells[k] entries"""
    mv = [stride] + [0] * lead
    for d in dwells:
        mv += [value] + [0] * (d - 1)
    return mv


@functools.lru_cache(maxsize=None)
def op_kinds():
    """(rs, ex, moves, centres, kinds): 48 reads over centre 130 of "ACGT" * 100, cycling through the op combinations the rule names.  Every
    base of read i dwells 1 + (i + its query offset) % 5 entries; both strands"""
    c = 130
    kinds = ("I", "II", "ID", "DI", "M", "IPI", "front_I", "D")
    reads = []
    for i in range(48):
        kind = kinds[i % 8]
        pos = c - 12 + 5 * i // 48  # (coordinate order)
        head, tail = REF[pos:c + 1], REF[c + 1:c + 15]
        m = len(head)
        cigar, seq = {
            "I": (f"{m}M2I14M", head + "GT" + tail), "II": (f"{m}M1I2I14M", head + "G" + "TT" + tail),
            "ID": (f"{m}M2I2D12M", head + "GA" + tail[2:]), "DI": (f"{m}M2D3I12M", head + "CCC" + tail[2:]),
            "M": (f"{m + 14}M", head + tail), "IPI": (f"{m}M1I1P2I14M", head + "A" + "CC" + tail),
            "front_I": (f"2I{m + 14}M", "TT" + head + tail), "D": (f"{m}M3D11M", head + tail[3:])}[kind]
        reads.append((pos, 16 * (i // 8 % 2), 60, cigar, seq))
    rs, ex = by_hand(reads, quals=[(3 * i) % 40 for i in range(48)], haps=[i % 3 for i in range(48)], ref=REF)
    qlen = syn.query_lengths(rs)
    moves = moves_by_hand([table_of([1 + (i + q) % 5 for q in range(int(n))], lead=i % 3) for i, n in enumerate(qlen)])
    return rs, ex, moves, [c - 16, c, c + 1, c + 2, c + 16], [kinds[i % 8] for i in range(48)]


def golden_tables():
    """(mv, l, reverse, tagged, sig or None) per table of the fixture"""
    with np.load(GOLDEN) as z:
        for i in range(len(z["l"])):
            mv = z["mv"][z["mv_first"][i]:z["mv_first"][i + 1]]
            sig = z["sig"][z["sig_first"][i]:z["sig_first"][i + 1]] if z["has"][i] else None
            yield mv, int(z["l"][i]), bool(z["reverse"][i]), bool(z["tagged"][i]), sig
