"""Lookup tables in plain Python: the numbers of the witness tape's lookup opcode block (include/mp2g.h enum mp2g_witness_op_lut),
the eager values of recursion.Builder.add_lookup_from_index, and prove()'s set_lookup_wires as circuits.fill_lookup_row restates it
(the padding of the LookupGate rows, the LookupTableGate rows, the multiplicities). The library's replays do the same in
csrc/lookup_wires.hip and csrc/witness_ops.h; nothing here is on a hot path."""
from collections import Counter

import numpy as np

# the third opcode block of the public tape format (the first block's numbers are recursion.py's OP_*, the second gf5.py's)
OP_LOOKUP, OP_LUT_END = 40, 41
NUM_LU_SLOTS, NUM_LUT_SLOTS = 40, 26  # LookupGate / LookupTableGate num_slots with 80 routed wires
MAX_LUTS = 16                         # MP2G_MAX_LUTS


def table(pairs):
    """[(input, output)] of u16 pairs, each input once (the multiplicities of a table with a repeated input are not defined)"""
    pairs = [(int(a), int(b)) for a, b in pairs]
    assert 1 <= len(pairs) <= 65536, "a table holds 1 .. 65536 entries"
    assert all(0 <= a < 65536 and 0 <= b < 65536 for a, b in pairs), "table entries are u16 pairs"
    assert len({a for a, _ in pairs}) == len(pairs), "a lookup table holds an input twice"
    return pairs


def output(pairs, x):
    """LookupGenerator: the table's output for x, 0 when the table has no such input"""
    return dict(pairs).get(int(x), 0)


def rows_needed(table_len, n_lookups):
    """(LookupGate rows, LookupTableGate rows) CircuitBuilder::add_all_lookups appends for one table"""
    return max(1, -(-n_lookups // NUM_LU_SLOTS)), -(-table_len // NUM_LUT_SLOTS)


def info(pairs, n_lookups, first_row):
    """the dict a built circuit keeps per table (Circuit.luts): the table and where its rows are -- the LookupGate rows from
    first_row = last_lu_row up, then the LookupTableGate rows last_lut_row .. first_lut_row (the table runs DOWN from the last)"""
    n_lu, n_lut = rows_needed(len(pairs), n_lookups)
    return {"table": np.array(pairs, dtype=np.uint16).reshape(-1, 2), "n_lookups": n_lookups, "last_lu_row": first_row,
            "last_lut_row": first_row + n_lu, "first_lut_row": first_row + n_lu + n_lut - 1}


def fill_wires(wires, info):
    """set_lookup_wires for one table on wires[col][row] (anything indexable that way), info as above. The looked-up slots are read,
    everything else written."""
    pairs = [(int(a), int(b)) for a, b in info["table"]]
    entry = {p: e for e, p in enumerate(pairs)}
    mult = Counter()
    for j in range((info["last_lut_row"] - info["last_lu_row"]) * NUM_LU_SLOTS):
        r, c = info["last_lu_row"] + j // NUM_LU_SLOTS, 2 * (j % NUM_LU_SLOTS)
        if j >= info["n_lookups"]:
            wires[c][r], wires[c + 1][r] = pairs[0]
        e = entry.get((int(wires[c][r]), int(wires[c + 1][r])))
        if e is not None:
            mult[e] += 1
    for e in range((info["first_lut_row"] - info["last_lut_row"] + 1) * NUM_LUT_SLOTS):
        r, c = info["first_lut_row"] - e // NUM_LUT_SLOTS, 3 * (e % NUM_LUT_SLOTS)
        wires[c][r], wires[c + 1][r], wires[c + 2][r] = (pairs[e][0], pairs[e][1], mult[e]) if e < len(pairs) else (0, 0, 0)
