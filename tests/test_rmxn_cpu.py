"""The RMxN filter (RMxNCalculator.ShouldFilter, FILTER R5x9) on the CPU: the reference's own table
(tests/golden/rmxn_cases.json, from RMxNFilterCalculatorTests.cs) against the plain statement (tests/rmxn_ref.py) and against the oracle,
the directed grids of the device tests against what they were built for, and a seeded fuzz of the oracle against the statement.
"""
import numpy as np
import pytest

from tests import orc
from tests import rmxn_cases as rc
from tests import rmxn_ref

T = rc.table()


def test_the_fixture_is_the_reference_table():
    assert len(T["cases"]) == 36 and sum(len(c["alleles"]) for c in T["cases"]) == 55 and len(T["assertions"]) == 6
    assert [x["line"] for x in T["not_in_table"]] == [53, 70]
    assert T["allele_support"] / T["total_coverage"] == T["frequency"] == 0.20
    assert sum(len(c["alleles"]) * len(rc.table_settings(T, c)) for c in T["cases"]) == 275
    for c in T["cases"]:   # the alleles as ExecuteRMxNTest builds them
        seq = c["sequence"].replace("*", "")
        for a in c["alleles"]:
            assert a["position"] == c["sequence"].index("*")
            if a["category"] in ("Snv", "Mnv"):
                assert a["alt"] == c["variant"] and seq[a["position"] - 1:a["position"] - 1 + len(a["ref"])] == a["ref"]
            else:
                assert a["ref"][0] == a["alt"][0] == seq[a["position"] - 1] and c["variant"] in (a["ref"][1:], a["alt"][1:])


def test_the_statement_gives_every_assertion_of_the_reference_table():
    n = 0
    for c in T["cases"]:
        seq = c["sequence"].replace("*", "")
        for a in c["alleles"]:
            for x in T["assertions"]:   # all six, the repeated one too
                got = rmxn_ref.should_filter(a["category"], a["position"], a["ref"], a["alt"], seq, c["max_unit"], c["repeats"] + x["min_rep_delta"],
                                             np.float32(x["frequency_limit"]), T["allele_support"], T["total_coverage"])
                assert got == bool(x["flagged"]), (c["line"], a, x)
                n += 1
            # the expected count is the smaller component itself
            c1, c2 = rmxn_ref.component_lengths(a["category"], a["position"], a["ref"], a["alt"], seq, c["max_unit"])
            assert min(c1, c2) == c["repeats"], (c["line"], a, c1, c2)
    assert n == 55 * 6


@pytest.mark.parametrize("case", T["cases"], ids=lambda c: "line%d" % c["line"])
def test_the_oracle_gives_every_assertion_of_the_reference_table(case):
    """Each case's sequence as the whole chromosome, through AlleleCaller.Call (orc.call_candidates): flat coverage 20 (behind the last base too: some
    deletions of the table reach past their sequence), support 4 — the table's 0.20 — and every other filter off."""
    seq = case["sequence"].replace("*", "")
    alleles = rc.table_alleles(case)
    for max_unit, min_rep, limit, flagged in rc.table_settings(T, case):
        got = rc.oracle_run(seq, alleles, rc.config(max_unit, min_rep, limit), overhang=rc.OVERHANG)
        for a in alleles:
            bit, support, coverage = got[rc.key_of(a)]
            assert (support, coverage) == (rc.COV // 5, rc.COV) and rmxn_ref.frequency(support, coverage) == np.float32(0.2), (a, support, coverage)
            assert bit == flagged, (case["line"], a, (max_unit, min_rep, limit))


def test_the_joined_table_keeps_every_answer():
    """The chromosome of the device test (every sequence, an N between them): the statement's answers on it are the fixture's."""
    chrom, placed = rc.joined_table(T)
    for case, alleles in placed:
        for a in alleles:
            assert a.category == "Insertion" or chrom[a.position - 1] == a.ref[0]
            for max_unit, min_rep, limit, flagged in rc.table_settings(T, case):
                assert rmxn_ref.should_filter(a.category, a.position, a.ref, a.alt, chrom, max_unit, min_rep, np.float32(limit), 4, 20) == bool(flagged), (case["line"], a)


def test_the_directed_snv_grid_holds_what_it_was_built_for():
    chrom, alleles, built = rc.snv_grid()
    rc.snv_grid_holds(chrom, alleles, built)
    reads = rc.reads_of(chrom, alleles)
    # the reads show the counts: no two SNVs share a read within an MNV's reach
    snvs = sorted(a.position for a in alleles)
    assert len(reads.position) == rc.COV * -(-len(chrom) // 50) and min(np.diff(snvs)) == 1


def test_the_observations_of_the_snv_grid_are_its_counts():
    """The oracle fed with the grid's observations one by one (the candidates are then its own): the rows of the oracle fed with the
    counts and the alleles, and no row over the reference N — no candidate is made where the reference base is no A, C, G or T, so
    the filter never sees one."""
    from pisces_amd import _abi
    chrom, alleles, _ = rc.snv_grid()
    pos, tup, stream, tiles = rc.observations_of(chrom, alleles)
    cfg = rc.config(5, 9, call_mnvs=0)
    rows, _ = orc.run_observations(pos, tup, np.frombuffer(chrom.encode(), np.uint8), 1, len(chrom), cfg)
    letters = np.array(list(_abi.BASE_OF_ALLELE))
    info = rows["info"].astype(np.int64)
    got = rc.bits_of_rows(rows, list(zip(letters[_abi.info_ref(info)].tolist(), letters[_abi.info_alt(info)].tolist())))
    assert got == rc.oracle_run(chrom, alleles, cfg) and len(got) == len(alleles) - 1
    assert tiles["n_loci"].sum() == len(chrom) and tiles["tuple_end"][-1] - 1 == len(tup) == rc.COV * len(chrom) and (tiles["n_loci"] < rc.TILE).sum() >= 2


@pytest.mark.parametrize("setting", rc.SNV_SETTINGS, ids=lambda s: "u%d_m%d_f%g" % s)
def test_the_oracle_on_the_directed_snv_grid(setting):
    chrom, alleles, _ = rc.snv_grid()
    got = rc.oracle_run(chrom, alleles, rc.config(*setting))
    exp = rc.check(got, chrom, alleles, *setting)
    assert all((got[rc.key_of(a)][1:]) == (a.support, rc.COV) for a in alleles if not a.no_row)
    if setting[0] >= 1 and setting[1] > 0:
        assert 0 < sum(exp.values()) < len(exp)
    if setting[:2] == (0, 0):   # no bookends, every component 0: min(0, 0) >= 0 flags whatever is below the limit
        assert sum(exp.values()) == sum(1 for a in alleles if a.support < 7 and not a.no_row)
    if setting[0] < 0 or setting[:2] == (0, 1):
        assert sum(exp.values()) == 0


def test_the_directed_spanning_grid_holds_what_it_was_built_for():
    rc.spanning_grid_holds(*rc.spanning_grid())


@pytest.mark.parametrize("setting", rc.SPAN_SETTINGS, ids=lambda s: "u%d_m%d_f%g" % s)
def test_the_oracle_on_the_directed_spanning_grid(setting):
    chrom, alleles, _ = rc.spanning_grid()
    rc.check(rc.oracle_run(chrom, alleles, rc.config(*setting)), chrom, alleles, *setting)


def test_the_oracle_on_the_spanning_grid_from_reads():
    """The same alleles found in reads (orc.run_reads_full: the finder, then AlleleCaller.Call): every allele a read can show has its row
    under every setting, with the statement's answer."""
    chrom, alleles, _ = rc.spanning_grid()
    batch, shown = rc.spanning_reads(chrom, alleles)
    assert len(shown) == len(alleles) - len(rc.NOT_FROM_READS) and {a.category for a in shown} == {"Mnv", "Insertion", "Deletion"}
    ref = np.frombuffer(chrom.encode(), np.uint8)
    for setting in rc.SPAN_SETTINGS:
        rows, strings, _, _ = orc.run_reads_full(batch, ref, 1, len(chrom), rc.config(*setting))
        got = rc.bits_of_rows(rows, strings)
        assert got.keys() == {rc.key_of(a) for a in shown}
        rc.check(got, chrom, shown, *setting)


def test_seeded_fuzz_of_the_oracle_against_the_statement():
    cases = []
    for seed in rc.FUZZ_SEEDS:
        chrom, alleles = rc.fuzz_layout(seed)
        assert len(alleles) == 250   # the generator builds only valid alleles: none is skipped
        for setting in rc.fuzz_settings(seed):
            got = rc.oracle_run(chrom, alleles, rc.config(*setting))
            exp = rc.check(got, chrom, alleles, *setting, where="seed %d" % seed)
            cases += [(a, len(chrom), setting[0], exp[rc.key_of(a)]) for a in alleles]
    flagged = rc.fuzz_is_not_vacuous(cases)
    print("fuzz: %d decisions, %d flagged" % (len(cases), flagged))
