"""FilterType.IndelRepeatLength without a GPU: pisces_hip_indel_repeat_length (csrc/indel_repeat.h, the source indel_repeat_kernel
compiles too) against the plain-Python statement of AlleleProcessor.ComputeIndelRepeatLength (tests/indel_repeat_ref.py), both against the
reference's own two tests (tests/golden/indel_repeat_cases.json), and the R<n> name in the host VCF formatter.

The reference's IndelRepeat test holds 26 ExecuteRepeatTest rows (VariantProcessorTests.cs:88-126; the extractor counts them), each
expanded as ExecuteRepeatTest :343-371 does into 100 offsets from the chromosome start and 100 lengths to the chromosome end, an insertion
and a deletion each: 26 * 400 = 10 400 decisions, held for the statement and for the entry.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi, engine
from pisces_amd._native import lib
from tests import indel_repeat_ref as ref
from tests.test_vcf_format import CAT_INS, CAT_SNV, GT, record

G = os.path.join(os.path.dirname(__file__), "golden")
CAT = {"Snv": _abi.CAT_SNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION, "Mnv": _abi.CAT_MNV, "Reference": _abi.CAT_REFERENCE}
# GetPadding :422-430: Unicode symbols joined by "X"; CreateRepeat puts a "Z" where the variant is anchored.  No decision looks at a filler
# character except to find that it is not a base of the unit (units are over A, C, T), so "#" stands for every symbol.
PADDING = "X".join("#" * 1200)


def table():
    with open(os.path.join(G, "indel_repeat_cases.json")) as f:
        return json.load(f)


def entry(category, position, ref_allele, alt_allele, reference):
    """pisces_hip_indel_repeat_length as it returns: the length, or a PISCES_E_* code."""
    r, a, s = ref_allele.encode(), alt_allele.encode(), reference.encode()
    return lib.pisces_hip_indel_repeat_length(CAT[category], int(position), r, len(r), a, len(a), s if s else None, len(s))


def create_repeat(repeat_unit, num_repeats, coordinate, length_to_end=1000):
    """CreateRepeat :405-420 with its defaults (repeatRelativeToVariant 0, isDeletion false)."""
    s = PADDING[:coordinate - 1] + "Z" + repeat_unit * num_repeats + PADDING[:1000]
    assert len(s) >= coordinate + length_to_end
    return s[:coordinate + length_to_end]


def repeat_variant(variant_bases, deletion):
    """CreateRepeatVariant :385-403 (category, ref, alt)"""
    return ("Deletion", "A" + variant_bases, "A") if deletion else ("Insertion", "A", "A" + variant_bases)


def expanded(row):
    """ExecuteRepeatTest :343-371: (chromosome, position, deletion?, expected) — 400 of them."""
    unit, n, threshold, flagged = row["repeat_unit"], row["repeats_in_reference"], row["threshold"], row["flagged"]
    for i in range(100):
        position = i + len(unit)
        chrom = create_repeat(unit, n, position)
        yield chrom, position, False, flagged
        yield chrom, position, True, flagged
        chrom = create_repeat(unit, n, 1000, length_to_end=i)
        yield chrom, 1000, False, flagged and threshold * len(unit) < i
        yield chrom, 1000, True, flagged and threshold * len(unit) < i


def test_the_references_rows_expanded():
    t = table()
    assert len(t["rows"]) == 26 and [r["line"] for r in t["rows"]] == sorted(r["line"] for r in t["rows"])
    assert not set(PADDING + "Z") & set("".join(r["repeat_unit"] + r["variant_bases"] for r in t["rows"]))
    n = 0
    wrong = []
    for row in t["rows"]:
        for chrom, position, deletion, want in expanded(row):
            category, r, a = repeat_variant(row["variant_bases"], deletion)
            stated = ref.is_flagged(row["threshold"], category, position, r, a, chrom)
            length = entry(category, position, r, a, chrom)
            got = length >= 0 and row["threshold"] <= length
            if stated != want or got != want or length != ref.indel_repeat_length(category, position, r, a, chrom):
                wrong.append((row["line"], position, len(chrom), deletion, want, stated, length))
            n += 1
    assert n == 400 * len(t["rows"]) == 10400
    assert not wrong, (len(wrong), wrong[:10])


def test_chromosome_edge_cases():
    e = table()["edge"]
    chrom = e["sequence_base"] * e["sequence_length"]
    assert len(chrom) == 75 and (e["category"], e["ref"], e["alt"], e["threshold"]) == ("Insertion", "A", "AA", 2)
    lo, hi = e["flagged_positions"]
    assert (lo, hi) == (0, 73) and e["not_flagged_positions"] == [74, 75]
    for p in range(lo, hi + 1):
        assert ref.is_flagged(2, "Insertion", p, "A", "AA", chrom), p
        assert entry("Insertion", p, "A", "AA", chrom) >= 2, p
    for p in e["not_flagged_positions"]:
        assert not ref.is_flagged(2, "Insertion", p, "A", "AA", chrom), p
        assert entry("Insertion", p, "A", "AA", chrom) == 1, p   # GetRepeatLength's early return
    # one base outside still answers (Substring(Length, 0) is the empty string); decidedly outside the reference throws
    assert entry("Insertion", 76, "A", "AA", chrom) == ref.indel_repeat_length("Insertion", 76, "A", "AA", chrom) == 1
    for p in e["throws_positions"] + [78, 1000, 2 ** 31 - 1, -50, -1000, -2 ** 31]:
        for category, r, a in (("Insertion", "A", "AA"), ("Deletion", "AA", "A"), ("Snv", "A", "C")):
            with pytest.raises(ref.ArgumentOutOfRange):
                ref.indel_repeat_length(category, p, r, a, chrom)
            assert entry(category, p, r, a, chrom) == _abi.E_INVALID_ARG, (category, p)
        # (an MNV or Reference allele returns before the flanks are cut, :83; so does every allele on an empty reference, :82)
        assert entry("Mnv", p, "AA", "CC", chrom) == entry("Reference", p, "A", "A", chrom) == entry("Insertion", p, "A", "AA", "") == 0
    assert entry("Insertion", -49, "A", "AA", chrom) == ref.indel_repeat_length("Insertion", -49, "A", "AA", chrom) == 1
    with pytest.raises(engine.PiscesHipError):
        engine.indel_repeat_length(_abi.CAT_INSERTION, 77, "A", "AA", chrom)
    assert engine.indel_repeat_length(_abi.CAT_INSERTION, 40, "A", "AA", chrom) == ref.indel_repeat_length("Insertion", 40, "A", "AA", chrom)
    # arguments that are no alleles
    assert lib.pisces_hip_indel_repeat_length(_abi.CAT_INSERTION, 5, b"A", 1, None, 2, chrom.encode(), 75) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_indel_repeat_length(_abi.CAT_DELETION, 5, b"", 0, b"A", 1, chrom.encode(), 75) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_indel_repeat_length(_abi.CAT_INSERTION, 5, b"A", 1, b"AA", 2, None, 75) == _abi.E_INVALID_ARG
    # the chromosome is upper-cased as it is read (:100-103), the allele is not
    assert entry("Insertion", 40, "A", "AA", chrom.lower()) == ref.indel_repeat_length("Insertion", 40, "A", "AA", chrom.lower()) > 8


def fuzz_draws(seed, n):
    """(category, position, ref, alt, chromosome): chromosomes of 1..300 bases over two or three letters with a planted run of a unit of
    1..60 bases; the variant bases are one to three copies of the unit (or unrelated); positions at the run's unit boundaries, anywhere,
    at 1, 2, L - 1, L and — rarely — at 0 and L + 1."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        letters = list(rng.choice(list("ACGT"), int(rng.integers(2, 4)), replace=False))
        u = int(rng.integers(1, 6)) if rng.random() < 0.7 else int(rng.integers(1, 61))
        unit = "".join(rng.choice(letters, u))
        length = int(rng.integers(1, 301))
        copies = int(rng.integers(0, 41)) if u <= 5 else int(rng.integers(0, 6))
        start = int(rng.integers(0, length))
        chrom = "".join(rng.choice(letters, start)) + unit * copies
        chrom = (chrom + "".join(rng.choice(letters, max(0, length - len(chrom)))))[:length]
        how = rng.random()
        if how < 0.2:
            position = [1, 2, length - 1, length][int(rng.integers(0, 4))]
        elif how < 0.23:
            position = [0, length + 1][int(rng.integers(0, 2))]
        elif how < 0.8:
            position = start + u * int(rng.integers(0, copies + 1))   # anchored in front of a copy: position + 1 is the copy's first base
        else:
            position = int(rng.integers(1, length + 1))
        position = min(max(position, 0), length + 1)
        k = int(rng.integers(1, 4))
        variant = unit * k if u * k <= 60 and rng.random() < 0.85 else "".join(rng.choice(letters, int(rng.integers(1, 61))))
        anchor = chrom[position - 1] if 1 <= position <= length else "N"
        c = rng.random()
        if c < 0.43:
            yield "Insertion", position, anchor, anchor + variant, chrom
        elif c < 0.86:
            yield "Deletion", position, anchor + variant, anchor, chrom
        elif c < 0.91:
            yield "Snv", position, anchor, letters[0], chrom
        elif c < 0.96:
            yield "Mnv", position, anchor + variant[:3], variant[:3] + anchor, chrom
        else:
            yield "Reference", position, anchor, anchor, chrom


def test_seeded_fuzz():
    n = 20000
    at_least_8 = below_8 = early = backtracked = cut = simplified = long_deletion = 0
    ends = set()
    wrong = []
    for category, position, r, a, chrom in fuzz_draws(20261020, n):
        trace = {}
        want = ref.indel_repeat_length(category, position, r, a, chrom, trace)
        got = entry(category, position, r, a, chrom)
        if got != want:
            wrong.append((category, position, r, a, chrom, want, got))
        if category in ("Snv", "Mnv", "Reference"):
            assert want == 0
        at_least_8 += want >= 8
        below_8 += want < 8
        early += bool(trace.get("early"))
        backtracked += trace.get("backtracked", 0) >= 2
        cut += bool(trace.get("cut"))
        if category in ("Insertion", "Deletion"):
            bases = (a if category == "Insertion" else r)[1:]
            simplified += len(ref.simplify_repeat_unit(bases)) < len(bases)
            long_deletion += category == "Deletion" and len(bases) > 50
            if position in (1, 2, len(chrom) - 1, len(chrom)):
                ends.add("first" if position == 1 else "second" if position == 2 else "last" if position == len(chrom) else "last but one")
    assert not wrong, (len(wrong), wrong[:5])
    # the draws reach every return path of GetRepeatLength, and both sides of the usual threshold
    assert early >= 100 and backtracked >= 100 and cut >= 100, (early, backtracked, cut)
    assert at_least_8 >= n // 10 and below_8 >= n // 10, (at_least_8, below_8)
    assert simplified >= 100 and long_deletion >= 100 and ends == {"first", "second", "last", "last but one"}, (simplified, long_deletion, ends)


def test_simplified_unit_is_the_shortest_period():
    """SimplifyRepeatUnit's split test on strings where a shorter prefix repeats without generating the whole."""
    for bases, unit in (("AA", "A"), ("ATCATC", "ATC"), ("AAT", "AAT"), ("ATAAT", "ATAAT"), ("ATATA", "ATATA"), ("AATAAT", "AAT"), ("ABAB" * 3, "AB"),
                        ("AAAAAT", "AAAAAT"), ("TAAAAA", "TAAAAA"), ("ACACAC", "AC"), ("A", "A")):
        assert ref.simplify_repeat_unit(bases) == unit
        chrom = "G" * 10 + unit * 12 + "G" * 60
        want = ref.indel_repeat_length("Insertion", 10, "G", "G" + bases, chrom)
        assert entry("Insertion", 10, "G", "G" + bases, chrom) == want == (12 if len(unit) <= 3 else want)


# ---- the host formatter ------------------------------------------------------------------------------------------------------------
def test_host_formatter_names_the_filter_between_ab_and_rmxn():
    every = tuple(range(13))
    r = record(567, "A", "A", GT["0/1"], CAT_INS, 100, 20, 80, 20, 20, filters=every)
    alleles = [("A", "AT")]
    f = engine.format_vcf("chr1", r, alleles=alleles, indel_repeat_filter=8).split("\t")[6]
    assert f == "LowDP;q30;NC;SB;AB;R8;R5x9;LowVariantFreq;ForcedReport;MultiAllelicSite;LowGQ"
    assert engine.format_vcf("chr1", r, alleles=alleles, indel_repeat_filter=10).split("\t")[6].split(";")[5] == "R10"
    # threshold null: the bit prints nothing — the text of the same row without the bit (the reference's MapFilter throws here)
    without = record(567, "A", "A", GT["0/1"], CAT_INS, 100, 20, 80, 20, 20, filters=tuple(b for b in every if b != _abi.FILTER_INDEL_REPEAT_LENGTH))
    for null in (0, -1):
        assert engine.format_vcf("chr1", r, alleles=alleles, indel_repeat_filter=null) == engine.format_vcf("chr1", without, alleles=alleles)
    assert engine.format_vcf("chr1", r, alleles=alleles) == engine.format_vcf("chr1", without, alleles=alleles)
    only = record(567, "A", "A", GT["0/1"], CAT_INS, 100, 20, 80, 20, 20, filters=(_abi.FILTER_INDEL_REPEAT_LENGTH,))
    assert engine.format_vcf("chr1", only, alleles=alleles, indel_repeat_filter=8).split("\t")[6] == "R8"
    assert engine.format_vcf("chr1", only, alleles=alleles).split("\t")[6] == "PASS"


def test_host_formatter_merges_the_filter_once_on_a_crushed_position():
    a = record(100, "A", "A", GT["0/1"], CAT_INS, 200, 50, 150, 100, 100, filters=(_abi.FILTER_INDEL_REPEAT_LENGTH, 4))
    b = record(100, "A", "A", GT["0/1"], CAT_INS, 200, 20, 150, 100, 100, filters=(0, _abi.FILTER_INDEL_REPEAT_LENGTH))
    c = record(100, "A", "T", GT["0/1"], CAT_SNV, 200, 20, 150, 100, 100, filters=(5,))
    text = engine.format_vcf("chr7", np.concatenate([a, b, c]), alleles=[("A", "AT"), ("A", "ATT"), ("A", "T")], crush=1, indel_repeat_filter=8)
    lines = text.rstrip("\n").split("\n")
    assert len(lines) == 1 and lines[0].split("\t")[6] == "LowDP;R8;SB;LowVariantFreq"


def test_default_vcf_config_leaves_the_threshold_null():
    cfg = _abi.PiscesVcfConfig()
    cfg.indel_repeat_filter = 77
    assert lib.pisces_hip_vcf_default_config(C.byref(cfg)) == 0
    assert cfg.indel_repeat_filter == 0
    assert C.sizeof(_abi.PiscesVcfConfig) == 44 and _abi.PiscesVcfConfig._fields_[-1][0] == "indel_repeat_filter"
    assert lib.pisces_hip_abi_version() == _abi.ABI_VERSION == 9
