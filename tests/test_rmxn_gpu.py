"""The RMxN filter on the device, on every path that states it, against the plain statement of RMxNCalculator (tests/rmxn_ref.py).

The device holds three statements of the filter: rmxn_should_filter_snv_lds (the 128-byte LDS window of every tile kernel),
rmxn_should_filter_snv (global memory: the tile kernels beyond rmxn_min_repetitions 32, call_spanning_kernel's SNVs) and
rmxn_length_for_indel (insertions, deletions, MNVs in call_spanning_kernel).  Here: the reference's own table
(tests/golden/rmxn_cases.json) through the product, the directed grids of tests/rmxn_cases.py (tile edges, the eight-neighbour shortcut,
the LDS margin at 31..34 under 32 / 33 / 40 repetitions, chromosome ends, N, the frequency limit, unit lengths 0 and 1; bookends, the
ratchet, the byte pool) on every surface, and a seeded fuzz.  A row's bit is compared with the statement's answer for the row's own
support and coverage; tests/test_rmxn_cpu.py shows on the CPU that the layouts hold what they were built for.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc
from tests import rmxn_cases as rc
from tests.test_read_store import env, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
T = rc.table()
NO_SWITCH = dict(PISCES_HIP_KERNEL=None, PISCES_HIP_STORE_WAVES=None, PISCES_HIP_TILE_LOCI=None, PISCES_HIP_READ_PATH=None, PISCES_HIP_MNV_SPLIT=None)


def run_candidates(chrom, alleles, cfg, overhang=0):
    """Counts through AddObservations, what does not come from counts through AddCandidates, one flush: {key: (bit, support, coverage)}."""
    from pisces_amd import engine
    pos, tup, _, _ = rc.observations_of(chrom, alleles, overhang)
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(chrom)
        c.AddObservations(pos, tup)
        cands = rc.candidate_dicts(alleles)
        if cands:
            c.AddCandidates(cands)
        rows, strings = c.CallWithAlleles()
    return rc.bits_of_rows(rows, strings)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the reference's table
# ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_table_through_the_product(torch_cuda):
    """Every sequence of the table on one chromosome (an N between them), flat coverage 20, every allele a candidate with support 4 (the
    table's 0.20), MNV calling on, the collapser and every other filter off: under each of the five settings of a case its alleles' rows
    carry the fixture's answer, and every other allele's row the statement's."""
    chrom, placed = rc.joined_table(T)
    alleles = [a for _, al in placed for a in al]
    by_setting = {}
    for case, al in placed:
        for max_unit, min_rep, limit, flagged in rc.table_settings(T, case):
            by_setting.setdefault((max_unit, min_rep, limit), []).append((case, al, flagged))
    n = 0
    for setting, cases in by_setting.items():
        got = run_candidates(chrom, alleles, rc.config(*setting))
        rc.check(got, chrom, alleles, *setting)
        for case, al, flagged in cases:
            for a in al:
                bit, support, coverage = got[rc.key_of(a)]
                assert (bit, support, coverage) == (flagged, rc.COV // 5, rc.COV), (case["line"], a, setting, got[rc.key_of(a)])
                n += 1
    assert n == 275


# The cases whose repeat reaches index 0 of their own sequence (several ratchet back to it), and those whose repeat runs to its last base
# (the N*ACAC... family among them), by source line.
REACH_INDEX_0 = [22, 23, 24, 26, 27, 29, 30, 42, 54, 55, 56, 59, 60, 61, 64, 65, 67, 68, 81, 82]
REACH_LAST_BASE = [22, 23, 24, 26, 27, 29, 30, 42, 45, 48, 50, 54, 55, 56, 59, 60, 61, 64, 65, 67, 68, 76, 78, 81, 82, 83, 84, 85, 86]


def test_reference_table_cases_at_the_ends_of_their_own_chromosome(torch_cuda):
    """The cases named above, each with its own sequence as the whole chromosome (counts also behind the last base: some of the table's
    deletions reach past their sequence), under its five settings."""
    lines = sorted(set(REACH_INDEX_0) | set(REACH_LAST_BASE))
    cases = [c for c in T["cases"] if c["line"] in lines]
    assert len(cases) == len(lines) == 29
    for case in cases:
        seq = case["sequence"].replace("*", "")
        alleles = rc.table_alleles(case)
        for max_unit, min_rep, limit, flagged in rc.table_settings(T, case):
            got = run_candidates(seq, alleles, rc.config(max_unit, min_rep, limit), overhang=rc.OVERHANG)
            for a in alleles:
                assert got[rc.key_of(a)] == (flagged, rc.COV // 5, rc.COV), (case["line"], a, (max_unit, min_rep, limit), got[rc.key_of(a)])


def test_reference_table_snvs_from_counts(torch_cuda):
    """The table's single-base cases with their support in the allele counts and MNV calling off: the tile kernel of the flush decides."""
    chrom, placed = rc.joined_table(T)
    snv_cases = [(case, al) for case, al in placed if al[0].category == "Snv"]
    assert [c["line"] for c, _ in snv_cases] == [22, 40, 81, 82]
    alleles = []
    for _, al in snv_cases:
        al[0].from_counts = True
        alleles += al
    for setting in sorted({s[:3] for case, _ in snv_cases for s in rc.table_settings(T, case)}):
        got = run_candidates(chrom, alleles, rc.config(*setting, call_mnvs=0))
        rc.check(got, chrom, alleles, *setting)
        for case, al in snv_cases:
            for max_unit, min_rep, limit, flagged in rc.table_settings(T, case):
                if (max_unit, min_rep, limit) == setting:
                    assert got[rc.key_of(al[0])] == (flagged, rc.COV // 5, rc.COV), (case["line"], setting)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the directed SNV grid on every surface
# ------------------------------------------------------------------------------------------------------------------------------------
_GRID = {}


def _snv_grid():
    if not _GRID:
        chrom, alleles, built = rc.snv_grid()
        rc.snv_grid_holds(chrom, alleles, built)   # no device run passes by lacking a case
        pos, tup, stream, tiles = rc.observations_of(chrom, alleles)
        counts_of = {rc.key_of(a): (a.support, rc.COV) for a in alleles if not a.no_row}
        expected = {s: rc.expected_bits(chrom, alleles, *s, counts_of) for s in rc.SNV_SETTINGS}
        _GRID.update(chrom=chrom, alleles=alleles, pos=pos, tup=tup, stream=stream, tiles=tiles, reads=rc.reads_of(chrom, alleles), expected=expected)
    return SimpleNamespace(**_GRID)


def _snv_bits(rows, strings=None):
    if strings is None:
        letters = np.array(list(_abi.BASE_OF_ALLELE) + ["?", "?"])
        info = rows["info"].astype(np.int64)
        strings = list(zip(letters[_abi.info_ref(info)].tolist(), letters[_abi.info_alt(info)].tolist()))
    return rc.bits_of_rows(rows, strings)


def _assert_grid(got, g, setting, where):
    want = g.expected[setting]
    assert got.keys() == want.keys(), (where, setting)   # (and so no row for the alternate base over the reference N)
    wrong = [(a.name, got[rc.key_of(a)], want[rc.key_of(a)]) for a in g.alleles if not a.no_row and got[rc.key_of(a)] != (want[rc.key_of(a)], a.support, rc.COV)]
    assert not wrong, (where, setting, len(wrong), wrong[:10])


@pytest.mark.parametrize("form", ["block", "wave", "wave2", "auto"])
def test_snv_grid_on_the_tile_surface(torch_cuda, form):
    """pisces_hip_call_tiles in every form of the hot kernel, the tiles cut as the streaming surface cuts them (ragged at every block's
    end and at the chromosome's)."""
    from pisces_amd import engine
    from tests.test_gpu_parity import run_fused
    g = _snv_grid()
    view = SimpleNamespace(tuples=torch_cuda.from_numpy(g.stream.view(np.int32)).cuda(), tiles=torch_cuda.from_numpy(g.tiles.view(np.uint8)).cuda(),
                           n_tiles=len(g.tiles), ref=torch_cuda.from_numpy(np.frombuffer(g.chrom.encode(), np.uint8).copy()).cuda(), ref_len=len(g.chrom))
    assert (g.tiles["n_loci"] < rc.TILE).sum() >= 2
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form)):
        for setting in rc.SNV_SETTINGS:
            with engine.HipVariantCaller(rc.config(*setting, call_mnvs=0)) as caller:
                rows, _ = run_fused(torch_cuda, caller, view)
            _assert_grid(_snv_bits(rows), g, setting, form)


def test_snv_grid_on_the_counts_fed_call_phase(torch_cuda):
    """AddObservations + Call: call_counts_kernel."""
    from pisces_amd import engine
    g = _snv_grid()
    with env(**NO_SWITCH):
        for setting in rc.SNV_SETTINGS:
            with engine.HipVariantCaller(rc.config(*setting, call_mnvs=0)) as c:
                c.SetReference(g.chrom)
                c.AddObservations(g.pos, g.tup)
                rows, strings = c.CallWithAlleles()
            _assert_grid(_snv_bits(rows, strings), g, setting, "counts")


READ_SURFACES = {"store_1_wave": dict(PISCES_HIP_STORE_WAVES=1), "store_2_waves": dict(PISCES_HIP_STORE_WAVES=2), "store_4_waves": dict(PISCES_HIP_STORE_WAVES=4),
                 "store_16_waves": dict(PISCES_HIP_STORE_WAVES=16), "tile_48_loci": dict(PISCES_HIP_TILE_LOCI=48), "tile_64_loci": dict(PISCES_HIP_TILE_LOCI=64),
                 "log_chain": dict(PISCES_HIP_READ_PATH="log"), "call_mnvs": dict(), "call_mnvs_unsplit": dict(PISCES_HIP_MNV_SPLIT=0)}


@pytest.mark.parametrize("how", list(READ_SURFACES))
def test_snv_grid_from_reads(torch_cuda, how):
    """AddAlleleCounts + Call: call_store_tiles_kernel with 1, 2, 4 and 16 waves a tile and with tiles of 48 and 64 loci, the observation-log
    chain, and — MNV calling on — the SNV candidates of the read walk: in the split form the tile kernels still call them, in the earlier
    form (PISCES_HIP_MNV_SPLIT=0) every one of them goes through call_spanning_kernel."""
    from pisces_amd import engine
    g = _snv_grid()
    with env(**dict(NO_SWITCH, **READ_SURFACES[how])):
        for setting in rc.SNV_SETTINGS:
            with engine.HipVariantCaller(rc.config(*setting, call_mnvs=1 if how.startswith("call_mnvs") else 0)) as c:
                c.SetReference(g.chrom)
                c.AddAlleleCounts(g.reads)
                rows, strings = c.CallWithAlleles()
            _assert_grid(_snv_bits(rows, strings), g, setting, how)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the directed spanning grid
# ------------------------------------------------------------------------------------------------------------------------------------
def test_spanning_grid_through_the_candidate_kernel(torch_cuda):
    """Insertions, deletions and MNVs as candidates (call_spanning_kernel, rmxn_length_for_indel): unit lengths 1..6 against unit-length
    limits 0, 1, 2, 5 and 8, a repeat only a prefix or only a suffix sees, repeats at both ends, 40 inserted bases in the byte pool, the
    ratchet to index 0, the repeat that runs to the last base, MNVs at position 1 and on the last base."""
    chrom, alleles, built = rc.spanning_grid()
    rc.spanning_grid_holds(chrom, alleles, built)
    flagged = 0
    for setting in rc.SPAN_SETTINGS:
        exp = rc.check(run_candidates(chrom, alleles, rc.config(*setting)), chrom, alleles, *setting)
        flagged += sum(exp.values())
    assert 0.15 * len(alleles) * len(rc.SPAN_SETTINGS) <= flagged <= 0.6 * len(alleles) * len(rc.SPAN_SETTINGS)


def test_spanning_grid_from_reads(torch_cuda):
    """The same alleles where reads can show them (all but the two with nothing aligned behind them): the device's read walk finds them —
    the 40 inserted bases in the byte pool —, call_spanning_kernel filters them."""
    from pisces_amd import engine
    chrom, alleles, _ = rc.spanning_grid()
    batch, shown = rc.spanning_reads(chrom, alleles)
    ref = np.frombuffer(chrom.encode(), np.uint8)
    with env(**NO_SWITCH):
        for setting in rc.SPAN_SETTINGS:
            with engine.HipVariantCaller(rc.config(*setting)) as c:
                c.SetReference(chrom)
                c.AddAlleleCounts(batch)
                rows, strings = c.CallWithAlleles()
            got = rc.bits_of_rows(rows, strings)
            assert got.keys() == {rc.key_of(a) for a in shown}, setting
            rc.check(got, chrom, shown, *setting)
            want, want_strings, _, _ = orc.run_reads_full(batch, ref, 1, len(chrom), rc.config(*setting))
            assert got == rc.bits_of_rows(want, want_strings), setting   # (bit, support and coverage of every row are the oracle's too)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) seeded fuzz
# ------------------------------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz_on_the_device(torch_cuda):
    """The generator of the CPU fuzz, three seeds, 250 alleles a seed on 3000 bases: SNVs from counts, the rest as candidates; twelve
    settings a seed with repetitions from {0, 1, 2, 3, 4, 9, 32, 33}."""
    cases = []
    for seed in rc.FUZZ_SEEDS:
        chrom, alleles = rc.fuzz_layout(seed)
        assert len(alleles) == 250
        for setting in rc.fuzz_settings(seed, repetitions=(0, 1, 2, 3, 4, 9, 32, 33)):
            exp = rc.check(run_candidates(chrom, alleles, rc.config(*setting)), chrom, alleles, *setting, where="seed %d" % seed)
            cases += [(a, len(chrom), setting[0], exp[rc.key_of(a)]) for a in alleles]
    rc.fuzz_is_not_vacuous(cases)
