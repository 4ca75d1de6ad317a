"""The ring model of stream_tuples_wave on the CPU (tests/tuple_ring.py): the loop's index arithmetic, replayed, decodes every dwordx4 of
a body exactly once and loads nothing else; the model's rows add up to the segment; the grid reaches every regime the model names.
"""
import collections

import numpy as np

from tests import tuple_geometry as tg
from tests import tuple_ring as tr

U, RING, ROW = tr.U, tr.RING, tr.ROW


def bodies():
    """n4 of every grid cell, every n4 up to three rows more than two revolutions of one wave, and the edges of the long cases."""
    out = {tr.body_dwordx4(rows, rem) for rows in tr.ROWS + tr.LONG_ROWS for rem in tr.REMAINDERS}
    out |= set(range(0, (2 * RING + 3) * ROW + 1))
    out |= {ROW * rows + d for rows in tr.LONG_ROWS + (4 * RING, 4 * RING + U) for d in (-65, -64, -63, -1, 0, 1)}
    return sorted(out)


def test_the_replayed_loop_decodes_every_dwordx4_once_and_loads_only_its_own_rows():
    for n4 in bodies():
        rows = (n4 + ROW - 1) // ROW
        for nw in (1, 2):
            seen = np.zeros(n4, np.int64)
            k_total = 0
            for wid in range(nw):
                s, loads, decoded = tr.replay(n4, nw, wid)
                assert len(loads) == len(decoded) == s.K, (n4, nw, wid)        # a load per row of the wave, none for a row it does not have
                assert max(s.G, 1) * RING - s.pad == s.K and (s.G == 0) == (s.K == 0)          # (an idle wave: all of revolution 0 is empty)
                assert 0 <= s.pad <= RING and (s.pad < RING or s.G == 0)
                for j, keep in decoded:
                    assert j.min() >= 0 and j.max() <= n4 - 1                   # clamped into the body
                    row = int(j[0]) // ROW
                    assert (row // U) % nw == wid                               # the dealing: batch b belongs to wave b % NW
                    assert (j[keep] == row * ROW + np.flatnonzero(keep)).all()  # the lanes kept read their own dwordx4
                    assert keep.all() or (row == rows - 1 and n4 % ROW and keep.sum() == n4 % ROW)
                    assert keep.all() == (row * ROW + ROW <= n4)                # masked exactly where the row is not whole
                    np.add.at(seen, j[keep], 1)
                k_total += s.K
            assert k_total == rows and (seen == 1).all(), (n4, nw)


def test_the_models_rows_add_up_to_the_segment():
    g = tr.build_grid()
    for layout in ("guarded", "padded"):
        for t, tile in enumerate(g.layouts[layout][1]):
            begin, end = int(tile["tuple_begin"]), int(tile["tuple_end"])
            e = tg.ends_model(begin, end)
            assert e.head + 4 * e.n4 + e.tail == end - begin
            for nw in (1, 2):
                m = tr.ring_model(begin, end, nw)
                assert sum(w.rows for w in m.waves) == m.rows == -(-e.n4 // ROW)
                for wid, w in enumerate(m.waves):
                    s, loads, decoded = tr.replay(e.n4, nw, wid)
                    assert w.rows == len(decoded) and w.refills == max(s.G - 1, 0) * RING and w.idle == (w.rows == 0)
                    masked = [i for i, (_, keep) in enumerate(decoded) if not keep.all()]
                    assert (w.mask != "none") == bool(masked), tr.cell_name(g, t, layout)
                    if masked:            # where the model says: a slot of revolution 0, or the very last step
                        first_rev = RING - s.pad
                        want = {"revolution 0, slot U-1": U - 1 - s.pad, "revolution 0, slot 2U-1": first_rev - 1, "last slot": s.K - 1}[w.mask]
                        assert masked == [want], tr.cell_name(g, t, layout)
            if layout == "guarded" or g.ring_cells[t][0] == 0:
                a, _, rows, rem = g.ring_cells[t]
                assert e.n4 == tr.body_dwordx4(rows, rem) and e.head == (4 - a) % 4 and begin % 4 == (a if layout == "guarded" else 0)


def test_the_grid_reaches_every_regime_of_the_ring():
    g = tr.build_grid()
    cells = tr.grid_cells()
    assert g.n_tiles == len(cells) == 4 * (3 * (len(tr.ROWS + tr.LONG_ROWS) - 1) + 1)
    assert {(rows, rem) for _, _, rows, rem in cells} >= {(rows, rem) for rows in tr.ROWS if rows for rem in tr.REMAINDERS}
    ends = collections.Counter((tg.ends_model(int(t["tuple_begin"]), int(t["tuple_end"])).head > 0, tg.ends_model(int(t["tuple_begin"]), int(t["tuple_end"])).tail > 0)
                               for t in g.layouts["guarded"][1])
    assert all(ends[k] >= 12 for k in ((False, False), (False, True), (True, False), (True, True))), ends
    table = collections.Counter()
    for tile in g.layouts["guarded"][1]:
        table.update(tr.regimes_of(int(tile["tuple_begin"]), int(tile["tuple_end"])))
    want = tr.reachable_regimes()
    missing = sorted(want - set(table))
    print("regimes of the ring reachable up to %d rows: %d" % (max(tr.LONG_ROWS), len(want)))
    for r in sorted(want):
        print("%4d  %s" % (table[r], " ".join(str(x) for x in r)))
    assert not missing, missing
    named = set(table)
    # what the loop can be in, by name: no refill (one revolution), the refill loop once, twice, more; an idle wave; the short batch in
    # either half of the ring; a masked row in revolution 0 and in the last slot; a whole last row
    for nw, wid in ((1, 0), (2, 0), (2, 1)):
        mine = {r[2:] for r in named if r[0] == "ring%d" % nw and r[1] == wid}
        assert {r[1] for r in mine if r[0] == "revolutions"} == {0, 1, 2, 3, 4}, (nw, wid)
        for path in ("alone", "refilled"):
            rev0 = {r[2:] for r in mine if r[0] == "revolution 0" and r[1] == path}
            assert {r[0] for r in rev0} == {"0", "<U", "U", ">U"}, (nw, wid, path)
            assert {r[1] for r in rev0} == {False, True}, (nw, wid, path)
            assert {r[2] for r in rev0} >= {"none", "revolution 0, slot U-1", "revolution 0, slot 2U-1"}, (nw, wid, path)
        assert {r[1] for r in mine if r[0] == "last revolution"} == {False, True}, (nw, wid)
    # the padded layout (every segment on a multiple of four) reaches them too
    padded = set()
    for tile in g.layouts["padded"][1]:
        padded.update(tr.regimes_of(int(tile["tuple_begin"]), int(tile["tuple_end"])))
    assert not want - padded, sorted(want - padded)


def test_the_two_references_agree_on_the_ring_grid():
    from pisces_amd import _abi
    g = tr.build_grid()
    cfg = _abi.default_config(emit_zero_coverage_refs=1)
    tensor = tg.count_tensor(g.positions, g.tuples, g.region_loci, cfg.min_base_call_quality)
    assert tensor.sum() == len(g.tuples) == sum(length for _, length, _, _ in g.ring_cells)
    rows, nloci = tg.oracle_rows(g, cfg)
    assert nloci == g.region_loci and len(np.unique(rows["position"])) == g.region_loci
    assert tg.rows_agree_with_tensor(rows, tensor, g.ref) > 9 * g.region_loci
