"""Lane / register model of the GROUP-WISE exchanges of the channel-pair FIR transforms (nmx_k_bank_w64c.h, G = 3 row groups,
M = 1536; nmx_k_bank_w64e.h, G = 4, M = 2048): pure Python, no GPU, no library.

A transform keeps 8 G complex points per lane and exchanges them four times through LDS (A -> B, B -> C forward; C' -> B',
B' -> A' inverse).  The whole-tile form (tools/model_w64c.py, tools/model_w64e.py) writes all 8 G rows of 72 points and reads
them back in the next pass's pattern.  The kernels run each exchange as G rounds through ONE 8-row tile: round g writes the
eight registers whose rows are 8 g .. 8 g + 7 to row (k_a & 7) and reads row group g back, every operation of all rounds
issued in one block; a wave's LDS operations execute in issue order.

Every point is a label here, so the model proves, for both transforms and all four exchanges, that
  * each (lane, register) receives the value the whole-tile exchange delivers,
  * every access stays inside the 8-row tile (576 complex points),
  * every access is bank-conflict free per 32-lane half (8-byte accesses: 32 slots),
  * no cell is overwritten while a read of its value is still to be issued, and every row's last read of round g is issued
    before the first write of round g + 1 to it.
The offsets are restated from the headers (nmx_w64g_p1 .. p4, nmx_w64c_lane_setup), in complex points."""

import pytest

L, ROW, TILE = 64, 72, 8 * 72


def ka(G, i):            # pass-A register i = 8 r + p holds k_a = G p + r
    return G * (i & 7) + (i >> 3)


# lane bases (nmx_w64c_lane_setup) and register offsets INSIDE the 8-row tile (nmx_w64g_p1 .. p4)
def a1(l): return l
def a2(l): return (l >> 3) * ROW + (l & 7)
def a4(l): return (l >> 3) * ROW + 9 * (l & 7)
def p1(G, i): return ROW * (ka(G, i) & 7)
def p2(i): return 8 * (i & 7)
def p3(i): return 9 * (i & 7)
def p4(i): return i & 7


# the whole-tile patterns the group-wise ones replace (nmx_k_bank_w64c.h before: P1 .. P4 with 576 (i >> 3))
def full1(G, l, i): return ka(G, i) * ROW + l
def full2(l, i): return a2(l) + 576 * (i >> 3) + 8 * (i & 7)
def full3(l, i): return a2(l) + 576 * (i >> 3) + 9 * (i & 7)
def full4(l, i): return a4(l) + 576 * (i >> 3) + (i & 7)


def group1(G, g):        # the registers of P1 whose rows are 8 g .. 8 g + 7, in issue order
    return [i for i in range(8 * G) if ka(G, i) >> 3 == g]


def schedule(G, which):
    """Issue order of one exchange: [(op, register, address(lane))], op "w" / "r" -- nmx_w64g_xch_ab / _bc / _cb / _ba."""
    ops = []
    for g in range(G):
        regs = [8 * g + i for i in range(8)]
        if which == "ab":
            ops += [("w", i, lambda l, i=i: a1(l) + p1(G, i)) for i in group1(G, g)]
            ops += [("r", i, lambda l, i=i: a2(l) + p2(i)) for i in regs]
        elif which == "bc":
            ops += [("w", i, lambda l, i=i: a2(l) + p3(i)) for i in regs]
            ops += [("r", i, lambda l, i=i: a4(l) + p4(i)) for i in regs]
        elif which == "cb":
            ops += [("w", i, lambda l, i=i: a4(l) + p4(i)) for i in regs]
            ops += [("r", i, lambda l, i=i: a2(l) + p3(i)) for i in regs]
        else:
            ops += [("w", i, lambda l, i=i: a2(l) + p2(i)) for i in regs]
            ops += [("r", i, lambda l, i=i: a1(l) + p1(G, i)) for i in group1(G, g)]
    return ops


def whole_tile(G, which):
    """{(lane, register): label} the whole-tile exchange delivers; a label is the (lane, register) that wrote it."""
    wr, rd = {"ab": (lambda l, i: full1(G, l, i), full2), "bc": (full3, full4), "cb": (full4, full3),
              "ba": (full2, lambda l, i: full1(G, l, i))}[which]
    tile = {}
    for l in range(L):
        for i in range(8 * G):
            assert wr(l, i) not in tile
            tile[wr(l, i)] = (l, i)
    assert len(tile) == L * 8 * G
    return {(l, i): tile[rd(l, i)] for l in range(L) for i in range(8 * G)}


def conflict_free(addrs):
    return all(len({a % 32 for a in addrs[32 * h:32 * h + 32]}) == 32 for h in range(2))


@pytest.mark.parametrize("which", ["ab", "bc", "cb", "ba"])
@pytest.mark.parametrize("G", [3, 4])
def test_group_wise_exchange(G, which):
    want = whole_tile(G, which)
    readers = {}                      # label -> reads of it still to be issued
    for label in want.values():
        readers[label] = readers.get(label, 0) + 1
    ops = schedule(G, which)
    assert sum(o[0] == "w" for o in ops) == sum(o[0] == "r" for o in ops) == 8 * G   # nothing added, nothing serialised
    assert sorted(i for o, i, _ in ops if o == "w") == sorted(i for o, i, _ in ops if o == "r") == list(range(8 * G))
    tile, got = {}, {}
    last_read, first_write = {}, {}   # (row, round) -> issue index
    for n, (op, i, addr) in enumerate(ops):
        addrs = [addr(l) for l in range(L)]
        assert all(0 <= a < TILE for a in addrs), (G, which, op, i, min(addrs), max(addrs))
        assert conflict_free(addrs), (G, which, op, i)
        rnd = (ka(G, i) >> 3) if (which, op) in (("ab", "w"), ("ba", "r")) else i >> 3
        for l, a in enumerate(addrs):
            if op == "w":
                if a in tile:
                    assert readers[tile[a]] == 0, f"G={G} {which}: register {i} overwrites a value that is still to be read"
                tile[a] = (l, i)
                first_write.setdefault((a // ROW, rnd), n)
            else:
                got[(l, i)] = tile[a]
                readers[tile[a]] -= 1
                last_read[(a // ROW, rnd)] = n
    assert got == want
    assert all(v == 0 for v in readers.values())
    for row in range(8):
        for g in range(G - 1):
            assert last_read[(row, g)] < first_write[(row, g + 1)], (G, which, row, g)


@pytest.mark.parametrize("G", [3, 4])
def test_rounds_of_the_pass_a_pattern(G):
    """Every block of eight consecutive rows is written by exactly eight registers, one per row of the tile."""
    seen = []
    for g in range(G):
        regs = group1(G, g)
        assert len(regs) == 8 and sorted(ka(G, i) & 7 for i in regs) == list(range(8))
        seen += regs
    assert sorted(seen) == list(range(8 * G))
    # a round's reads land in registers 8 g .. 8 g + 7, which still hold values of later rounds: hence the second array
    assert any(i < 8 and ka(G, i) >> 3 > 0 for i in range(8 * G))


def test_dropping_the_group_term_keeps_the_banks():
    """8 rows x 72 points x 2 words = 1152 words = 18 x 64 banks: the address loses a multiple of the bank count."""
    assert (576 * 2) % 64 == 0
    for l in range(L):
        for i in range(32):
            assert (full2(l, i) - (a2(l) + p2(i))) % 576 == 0 and (full3(l, i) - (a2(l) + p3(i))) % 576 == 0
            assert (full4(l, i) - (a4(l) + p4(i))) % 576 == 0
            for G in (3, 4):
                if i < 8 * G:
                    assert (full1(G, l, i) - (a1(l) + p1(G, i))) % 576 == 0
