"""The tuple path's geometry grid on the CPU (tests/tuple_geometry.py): the grid reaches every regime the loop models know of, the two
references agree with each other before either judges the device, and the observation-log cases hold what they were built for.
"""
import collections
import re

import numpy as np

from pisces_amd import _abi
from tests import tuple_geometry as tg

K = tg.K


def regime_table(g, layout="guarded"):
    """Tiles per regime, over the layout's own tuple_begin / tuple_end."""
    n = collections.Counter()
    for tile in g.layouts[layout][1]:
        n.update(tg.regimes_of(int(tile["tuple_begin"]), int(tile["tuple_end"])))
    return n


def test_constants_come_from_the_source():
    assert K.B == 4 * 64 * K.wave_unroll and K.block_iter4 == K.block * K.unroll
    assert K.log_chunk % 256 == 0 and K.local_tiles >= 64 and K.gather_direct_tiles >= 1024
    # a source with another unroll moves the grid: nothing here is a copy of the numbers
    kt = re.sub(r"(#\s*define\s+PISCES_WAVE_UNROLL\s+)\d+", r"\g<1>4", tg._source("kernels.hip.h"))
    k4 = tg.parse_constants(kernels_text=kt)
    assert k4.wave_unroll == 4 and k4.B == 1024 and max(tg.grid_lengths(k4)) == tg.MAX_BATCHES * 1024 + 4
    want = tg.reachable_regimes(k4)
    got = set()
    for length in tg.grid_lengths(k4):
        for a in range(4):
            got.update(tg.regimes_of(a, a + length, k4))
    assert not want - got, sorted(want - got)


def test_the_models_account_for_every_word_exactly_once():
    """The models replayed word by word: head + 4 * body + tail is the segment, the waves' batches are disjoint and cover the body, and the
    clamped, masked last batch keeps exactly the body's dwordx4."""
    for a in range(4):
        for length in list(range(0, 40)) + [K.B - 1, K.B, K.B + 5, 2 * K.B + 3, 5 * K.B - 2]:
            e = tg.ends_model(a, a + length)
            assert e.head + 4 * e.n4 + e.tail == length and 0 <= e.tail <= 3 and (e.degenerate or 0 <= e.head <= 3)
            assert not e.degenerate or (e.n4 == 0 and e.tail == 0 and e.head == length <= 2 and a != 0)
            for nw in (1, 2):
                m = tg.wave_model(a, a + length, nw)
                seen = []
                for wid, w in enumerate(m.waves):
                    mine = list(range(wid, m.nb, nw))
                    assert len(mine) == w.batches and w.idle == (not mine)
                    if mine:
                        assert w.batches == 1 + 2 * ((w.batches - 1) // 2) + int(w.odd)
                        assert w.mask == (mine[-1] == m.nb - 1 and e.n4 % K.wave_batch4 != 0)
                    seen += mine
                assert sorted(seen) == list(range(m.nb))
                assert sum(w.mask for w in m.waves) == int(m.nb > 0 and not m.last_full)


def test_the_grid_reaches_every_regime_of_every_form():
    g = tg.build_grid()
    assert g.n_tiles == len(tg.grid_lengths()) * 4 and len(tg.grid_lengths()) == 12 + 5 * tg.MAX_BATCHES + 2
    assert [int(t["tuple_begin"]) % 4 for t in g.layouts["guarded"][1]] == [a for a, _ in g.cells]
    assert all(int(t["tuple_begin"]) % 4 == 0 for t in g.layouts["padded"][1])
    for layout in ("guarded", "padded"):
        buf, tiles = g.layouts[layout]
        assert [int(t["tuple_end"] - t["tuple_begin"]) for t in tiles] == [length for _, length in g.cells]
        owned = np.zeros(len(buf), bool)
        for t, seg in zip(tiles, g.segments):
            assert not owned[t["tuple_begin"]:t["tuple_end"]].any() and (buf[t["tuple_begin"]:t["tuple_end"]] == seg).all()
            owned[t["tuple_begin"]:t["tuple_end"]] = True
        rest = buf[~owned]
        assert (rest == (tg.guard_word() if layout == "guarded" else _abi.TUPLE_PAD)).all()
        if layout == "guarded":   # a real observation in front of and behind every segment, 1..7 of them
            assert not owned[0] and not owned[-1]
            assert all(buf[t["tuple_begin"] - 1] == tg.guard_word() and buf[t["tuple_end"]] == tg.guard_word() for t in tiles)
            runs = np.diff(np.flatnonzero(np.r_[True, owned, True])) - 1          # guard words between owned words (0 inside a segment)
            assert runs.max() <= 7 * 5                                            # (the empty tiles' guards run together)
            assert _abi.tuple_fields(np.array([tg.guard_word()], np.uint32))[3][0] == _abi.ALLELE_A
    want = tg.reachable_regimes()
    table = regime_table(g)
    missing = sorted(want - set(table))
    assert not missing, missing
    assert all(table[r] >= 1 for r in want)
    by_form = collections.Counter(r[0] for r in want)
    print("regimes reachable up to %d batches: %d %s" % (tg.MAX_BATCHES, len(want), dict(by_form)))
    for r in sorted(want):
        print("%4d  %s" % (table[r], " ".join(str(x) for x in r)))
    assert by_form["wave1"] >= 13 and by_form["wave2"] >= 2 * 19 and by_form["block"] >= 3 and by_form["ends"] >= 16   # (the 256-thread form has 7 when 13 batches make 3 iterations)
    # a list that stops at 11 batches has no wave 1 of the two-wave form with two or more pairs AND the epilogue (nor a third full iteration
    # of the 256-thread form)
    short = set()
    for length in tg.grid_lengths(max_batches=11):
        for a in range(4):
            short.update(tg.regimes_of(a, a + length))
    lost = want - short
    print("lost by a list that stops at 11 batches:", sorted(lost))
    assert sum(r[:5] == ("wave2", 1, False, 2, True) for r in lost) == 2 and all(r[0] in ("wave2", "block") for r in lost)
    # the padded layout (every segment on a multiple of four) reaches every loop regime too
    padded = regime_table(g, "padded")
    assert not {r for r in want if r[0] != "ends"} - set(padded)


def test_the_inert_grid_salts_every_kind_where_it_says():
    plain, salted, kinds = tg.build_inert_grid()
    assert plain.n_tiles == salted.n_tiles == len(tg.INERT_TILE_LOCI) * 3 * 4
    seen = collections.Counter(k for ks in kinds for k in ks)
    assert set(seen) == set(tg.INERT_KINDS) and min(seen.values()) >= 8
    for t in range(plain.n_tiles):
        s, p = salted.segments[t], plain.segments[t]
        locus, anchor, direction, allele, _ = _abi.tuple_fields(s)
        inert = (locus >= plain.n_loci[t]) | (allele >= 6) | (direction == 3) | (anchor >= _abi.NUM_ANCHORS)
        assert inert.sum() == len(kinds[t]) == len(s) - len(p) and (s[~inert] == p).all()
        assert inert[-1] and (len(s) < 5 or inert[-5]), t        # the segment's last word, and the one four in front of it
    last_x4 = tail = 0
    for t, tile in enumerate(salted.layouts["guarded"][1]):
        e = tg.ends_model(int(tile["tuple_begin"]), int(tile["tuple_end"]))
        tail += e.tail > 0
        last_x4 += e.tail == 0 and e.n4 > 0
    assert tail >= 8 and last_x4 >= 4
    assert (plain.n_loci == 56).sum() == 12 and (plain.n_loci == 1).sum() == 12


def test_the_two_references_agree_on_the_grid():
    """numpy.bincount over the tuple fields against the oracle's rows, cell by cell where a row shows a cell (folded over anchors as the
    oracle folds them); with zero-coverage Reference rows on, every locus has a row."""
    g = tg.build_grid()
    cfg = _abi.default_config(emit_zero_coverage_refs=1)
    tensor = tg.count_tensor(g.positions, g.tuples, g.region_loci, cfg.min_base_call_quality)
    assert tensor.sum() == len(g.tuples) == sum(length for _, length in g.cells)
    rows, nloci = tg.oracle_rows(g, cfg)
    assert nloci == g.region_loci and len(np.unique(rows["position"])) == g.region_loci
    assert tg.rows_agree_with_tensor(rows, tensor, g.ref) > 9 * g.region_loci
    # the rows show most cells: where the depth is the grid's nearly every locus has its three variant rows
    deep = np.repeat([length >= 30 * tg.TILE for _, length in g.cells], tg.TILE)          # thirty reads a locus
    li = rows["position"] - 1
    assert (np.bincount(li[deep[li]], minlength=g.region_loci)[deep] >= 3).mean() > 0.9
    plain, _, _ = tg.build_inert_grid()
    cfg0 = _abi.default_config()
    rows, _ = tg.oracle_rows(plain, cfg0)
    tg.rows_agree_with_tensor(rows, tg.count_tensor(plain.positions, plain.tuples, plain.region_loci, cfg0.min_base_call_quality), plain.ref)


def test_the_log_cases_hold_what_they_were_built_for():
    c = K.log_chunk
    sizes = tg.chunk_edge_sizes()
    assert {n - c for n in sizes} >= {-1, 0, 1} and {n - 2 * c for n in sizes} >= {-1, 1, 255, 257}
    for n in sizes:
        case = tg.chunk_edge_case(n)
        assert len(case.positions) == n and sum(p.stop - p.start for p in case.parts) == n and len({p.stop - p.start for p in case.parts}) == 3
        spans = tg.chunk_spans(case.positions)
        assert len(spans) == -(-n // c) and spans[-1][2] == (n % c or c)
        assert min(hi - lo for lo, hi, m in spans if m > 256) >= 3 * tg.TILES_PER_BLOCK - 8   # a chunk holds (nearly) every tile
        if n >= tg.CHUNK_EDGE_LOCI:
            assert len(np.unique(case.positions)) == tg.CHUNK_EDGE_LOCI
    far = tg.far_tile_case()
    tiles = tg.log_tile_of(far.positions)
    n_tiles = int(tiles.max()) + 1
    assert n_tiles > 1024 and n_tiles > K.local_tiles and tg.FAR_LOCI // tg.BLOCK > 64
    assert -(-n_tiles // 1024) == 2                                       # bucket_scan_kernel: two tiles a thread
    depth = np.bincount(far.positions)[1:]
    assert set(np.unique(depth)) == {2, 3}
    spans = tg.chunk_spans(far.positions)
    far_chunks = [i for i, (lo, hi, _) in enumerate(spans) if hi - lo >= K.local_tiles]
    assert len(far_chunks) >= 2 and far_chunks[0] == 0
    # a tile that the per-entry branch writes to (from chunk 0) and the privatised branch too (from a chunk where it is near the lowest)
    lo0 = spans[0][0]
    far_tiles = np.unique(tiles[:c][tiles[:c] - lo0 >= K.local_tiles])
    assert len(far_tiles) >= 2
    both = 0
    for t in far_tiles:
        for i in np.unique(np.flatnonzero(tiles == t) // c):
            if 0 <= t - spans[i][0] < K.local_tiles:
                both += 1
                break
    assert both == len(far_tiles)
    assert len({p.stop - p.start for p in far.parts}) == 3
