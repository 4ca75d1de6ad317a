"""What tests/test_bam_amplicon_gpu.py relies on, asserted without a device: the statement of GetStringTag on hand-made auxiliary bytes,
and every case file of tests/bam_amplicon_cases.py read back by the plain BAM reader — the names, types, placements and record counts the
device tests take for granted are really in the bytes."""
import struct

import numpy as np
import pytest

from tests import amplicon_cases as S
from tests import bam_amplicon_cases as K
from tests import bam_synth


def test_the_statement_of_get_string_tag():
    name = K.amplicon_name
    assert name(b"") is None and name(b"NMC\x02MDZ12\0") is None
    assert name(b"XNZabc\0") == b"abc" and name(b"XNHabc\0") == b"abc" and name(b"XNzabc\0") == b"abc" and name(b"XNhabc\0") == b"abc"
    assert name(b"XNZ\0") == b"" and name(b"XNZ\0") is not None                                  # the empty name is a name
    assert name(b"XNAq") == b"q" and name(b"XNaq") == b"q" and name(b"XNCq") == b"q" and name(b"XNcq") == b"q"
    assert name(b"XNZfirst\0XNZsecond\0") == b"first"                                             # the first field decides
    assert name(b"XNAqXNZsecond\0") == b"q"
    assert name(b"COZXNZfake\0") is None and name(b"COZXNZfake\0XNZreal\0") == b"real"            # field by field, not a byte search
    assert name(b"XIi" + b"XNZ\0" + b"XNZreal\0") == b"real"                                     # (the int's four bytes read like a field)
    assert name(bam_synth.aux_of_every_type() + b"XNZbehind\0") == b"behind"                      # B arrays are stepped over
    for ty in b"iIsSfB":
        with pytest.raises(K.BadTagType):
            name(b"XN" + bytes([ty]) + b"\0\0\0\0\0\0\0\0\0")
    with pytest.raises(K.BadTagType):
        name(b"XNi" + struct.pack("<i", 7) + b"XNZlater\0")                                       # a later field does not rescue it
    assert K.first_appearance_ids([b"b", None, b"a", b"b", b""])[0].tolist() == [0, -1, 1, 0, 2]
    assert K.first_appearance_ids([b"x", b"a"], known=[b"a", b"b"]) [0].tolist() == [2, 0]


def test_the_shapes_case_holds_every_shape_it_promises():
    bam = K.shapes_case()
    keep, reads = K.read_back(bam.file())
    assert len(reads) == bam.n_records == 704 and 600 < len(keep) < 704
    assert bam.n_chunks >= 3 and 100 < len(bam.array) / bam.n_records < 220                       # about 700 records of about 150 bytes
    assert len(keep) == int(bam.keep(0).sum())
    names = [K.amplicon_name(r["tags"]) for r in keep]
    distinct = {n for n in names if n is not None}
    assert {len(n) for n in distinct} >= {0, 1, 7, 40, 250}
    assert None in names and b"" in distinct
    # types, as the bytes have them
    types = {bytes([r["tags"][r["tags"].index(b"XN") + 2]]) for r in keep if r["tags"].startswith(b"XN") or b"\0XN" in r["tags"] or b"\x02XN" in r["tags"]}
    assert types >= {b"Z", b"H", b"A", b"c", b"C"}
    # placements: first, behind every value type (B arrays among them), last, absent
    every = bam_synth.aux_of_every_type()
    assert any(r["tags"].startswith(b"XNZ") and len(r["tags"]) > 20 for r in keep)
    assert any(r["tags"].startswith(every + b"XNZ") for r in keep) and b"XBB" in every
    assert any(r["tags"].endswith(K.xn(K.NAMES_7[0])) and not r["tags"].startswith(b"XN") for r in keep)
    # two XN fields: the statement takes the first, and the second's name is nobody's
    twice = [r for r in keep if r["tags"].count(b"XNZ") == 2 and b"second_never_wins" in r["tags"]]
    assert len(twice) >= 40 and all(K.amplicon_name(r["tags"]) in K.NAMES_7 for r in twice) and b"second_never_wins" not in distinct
    # the bytes XNZfake inside another field's value: with and without a real field behind
    fake = [r for r in keep if b"XNZfake" in r["tags"]]
    assert {K.amplicon_name(r["tags"]) is None for r in fake} == {True, False} and b"fake" not in distinct
    # XD and XN on one record, in either order
    both = [r for r in keep if b"XDZ" in r["tags"] and K.amplicon_name(r["tags"]) is not None]
    assert {r["tags"].index(b"XDZ") < r["tags"].index(b"XNZ") for r in both} == {True, False}
    # the same one-byte name through four types
    q = {bytes([r["tags"][r["tags"].index(b"XN") + 2]]) for r in keep if K.amplicon_name(r["tags"]) == b"q" and b"fake" not in r["tags"]}
    assert q >= {b"Z", b"H", b"A", b"c"}
    # the records ShouldSkipRead drops carry names no kept read has, one kind each
    dropped = [r for r in reads if not any(r is k for k in keep)]
    dropped_names = {K.amplicon_name(r["tags"]) for r in dropped}
    assert dropped_names == {b"skipped_" + k.encode() for k in K.SKIP_KINDS} and not dropped_names & distinct
    assert {r["ref"] for r in dropped} == {"chr1", "chr2"}
    # ids are well defined: every kept tag has a string type
    ids, table = K.first_appearance_ids(names)
    assert len(table) == len(distinct) and (ids == -1).sum() == names.count(None) and [table[i] for i in ids if i >= 0] == [n for n in names if n is not None]


def test_the_probe_case_holds_near_equal_names():
    names, bam = K.probe_case()
    keep, reads = K.read_back(bam.file())
    assert len(keep) == len(reads) == len(names)
    assert [K.amplicon_name(r["tags"]) for r in keep] == names                                     # in file order
    pool = set(names) - {None}
    assert len(pool) == len(K.LAST_BYTE) + len(K.PREFIXES) and all(names.count(n) == 3 for n in pool)
    assert len({len(n) for n in K.LAST_BYTE}) == 1 and len(set(K.LAST_BYTE)) == len(K.LAST_BYTE) == 496
    family = [n for n in K.LAST_BYTE if n[:-1] == K.LAST_BYTE[0][:-1]]
    assert len(family) == 62 and len({n[-1] for n in family}) == 62                               # these differ in their last byte only
    assert {b"amp1", b"amp10", b"amp100"} <= pool and all(b.startswith(a) for a, b in zip(K.PREFIXES[:9], K.PREFIXES[1:9]))


def test_the_regrow_case_outgrows_the_first_table():
    names, bam = K.regrow_case()
    keep, reads = K.read_back(bam.file())
    assert len(keep) == len(reads) == 6000
    got = [K.amplicon_name(r["tags"]) for r in keep]
    assert got == names and len(set(got)) == 3000 > 2048                                           # more than half of 4 096 slots
    assert K.first_appearance_ids(got)[0].tolist() == list(range(3000)) * 2
    names2, bam2 = K.second_case()
    keep2, _ = K.read_back(bam2.file())
    got2 = [K.amplicon_name(r["tags"]) for r in keep2]
    assert got2 == names2 and len(set(got2)) == 20
    assert len(set(got2) & set(names)) == 10 and got2[0] not in names and got2[1] in names       # interleaved, a new one first
    ids2, table = K.first_appearance_ids(got2, known=K.first_appearance_ids(got)[1])
    assert sorted(set(ids2.tolist()) - set(range(3000))) == list(range(3000, 3010)) and len(table) == 3010


def test_the_bad_type_case():
    keep, reads = K.read_back(K.bad_type_case().file())
    assert len(keep) == len(reads) == 12
    bad = []
    for i, r in enumerate(keep):
        try:
            assert K.amplicon_name(r["tags"]).startswith(b"ok")
        except K.BadTagType:
            bad.append(i)
    assert bad == [5, 9] and keep[5]["tags"][:3] == b"XNi" and keep[9]["tags"][:3] == b"XNf"


@pytest.mark.parametrize("which", ["filter", "planted"])
def test_the_scenario_files_hold_the_scenarios_reads_and_names(which):
    if which == "filter":
        ref, reads, ids = S.filter_scenario()
    else:
        sc = S.planted_scenario(*S.PLANTED_SEEDS[0])
        ref, reads, ids = sc["ref"], sc["reads"], sc["ids"]
    bam = K.scenario_file(ref, reads, ids)
    keep, everything = K.read_back(bam.file())
    assert len(keep) == len(everything) == len(reads)
    assert [K.amplicon_name(r["tags"]) for r in keep] == [K.name_of_id(i) for i in ids]
    assert -1 in ids and len({i for i in ids if i >= 0}) >= 2                                      # untagged carriers, several amplicons
    for r, k in zip(reads, keep):
        assert (k["pos"], k["cigar"], k["seq"], k["qual"].tobytes(), bool(k["flag"] & 0x10)) == (r["pos"], [tuple(c) for c in r["cigar"]], r["seq"], bytes(r["quals"]), r["reverse"])
    assert any((r["pos"] - 1) % 1000 // 64 != (r["pos"] + 98) % 1000 // 64 for r in reads)        # reads across a 64-locus tile edge
