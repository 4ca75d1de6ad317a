"""Writes tests/golden/vead_cases.json: the facts of the reference's Scylla unit tests (src/test/VariantPhasing.Tests), transcribed by hand
as data (README_vead.md says which lines each key comes from).  Positions are Read.Position: BamAlignment.Position + 1.
    python tests/golden/make_vead_cases.py"""
import json
import os

MNV_READ = dict(position=3, cigar="2S8M4S", bases="AA" + "ACGTACGT" + "GGGG", quals=0)
finder = []


def case(name, read, min_q, sites, segments, expected, last_pos=None):
    c = dict(name=name, **read, min_q=min_q, sites=sites, segments=dict(zip("MID", segments)), expected=expected)
    if last_pos is not None:
        c["last_pos"] = last_pos
    finder.append(c)


case("FindVariantMNVResults", MNV_READ, 0, [[4, "TA", "CG"], [10, "TTT", "T"]], (1, 0, 0), [[4, "TA", "CG"], [10, "T", "T"]])
case("FindCompetingNResults", MNV_READ, 10, [[4, "TA", "CG"], [4, "TARR", "CGTA"], [4, "T", "T"], [4, "TA", "T"], [4, "T", "TAAA"]], (1, 0, 0),
     [[4, "N", "N"]] * 5)
case("FindCompetingDisAgreeingMNVResults", MNV_READ, 0, [[4, "TA", "CG"], [4, "TARR", "CCTA"]], (1, 0, 0), [[4, "TA", "CG"], [4, "X", "X"]])
case("FindColocatedAgreeingMNVResults", MNV_READ, 0, [[4, "TA", "CG"], [4, "TARR", "CGTA"]], (1, 0, 0), [[4, "TA", "CG"], [4, "TARR", "CGTA"]])
case("FindAgreeingOverlappingMNVResults", MNV_READ, 0, [[4, "TAAC", "CGTA"], [6, "ACCC", "TACG"]], (1, 0, 0), [[4, "TAAC", "CGTA"], [6, "ACCC", "TACG"]])
case("FindMultipleMNVResults", MNV_READ, 0, [[4, "TA", "CG"], [7, "GG", "AC"]], (1, 0, 0), [[4, "TA", "CG"], [7, "GG", "AC"]])

DEL_SITES = [[1389296, "TCACA", "T"], [1389304, "A", "G"], [1389353, "C", "T"]]
r1 = dict(position=1389292, cigar="5M4D65M6S", bases="CTGCTCACGTGCCGATGTGGAGTGCCCGCCTGCTCACACCAGCCCATGTGTAGTGCCCGCCTGCTCACACCAGGCC", quals=0)
r2 = dict(position=1389305, cigar="27S49M", bases="AGTGCAGTGGGCTGCTCTTCACAGAGGTGCCGATGTGGAGTGCCCGCCTGCTCACACGTGCCCATGTGGAGTGCCT", quals=0)
r3 = dict(position=1389306, cigar="12S28M36S", bases="GCCTGCTCACGGGCCGATGTGGGGTGCCCGCCTGCTCACAGTACCCGCCGGGGGGGGGCGGCCTGCGCTCTCCAGG", quals=0)
r4 = dict(position=1389310, cigar="32S44M", bases="GCTGGAGTCGGCGCCTGCTGACAGAGGTGCCAATGTGGAGGGCCCGCCTGCTCACACGTGCCCATGTGGAGTGCCT", quals=0)
r5 = dict(position=1389312, cigar="47M2I26M", bases="GTGTAGTGCCAGCCTGCTCACACGTGACCATGTGTTGTGCCTGCCTGCTCTCACACGTGCCCATGTGGAGTGCCC", quals=0)
r6 = dict(position=1389312, cigar="47M2I26M", bases="GTGTAGTGCCCGCCTGCTCTCACGTGCCCATGTGGTGTGCCCGCCTGCTCTCACACGTGCCCATGTGGAGTGCCC", quals=0)
N3 = lambda: [[1389296, "N", "N"], [1389304, "N", "N"]]
case("ProcessWithDeletionsReadTest r1", r1, 0, DEL_SITES, (2, 0, 1), [[1389296, "TCACA", "T"], [1389304, "A", "G"], [1389353, "C", "C"]])
case("ProcessWithDeletionsReadTest r1 minq 10", r1, 10, DEL_SITES, (2, 0, 1), N3() + [[1389353, "N", "N"]])
case("ProcessWithDeletionsReadTest r2", r2, 0, DEL_SITES, (1, 0, 0), N3() + [[1389353, "C", "T"]])
case("ProcessWithDeletionsReadTest r3", r3, 0, DEL_SITES, (1, 0, 0), None)
case("ProcessWithDeletionsReadTest r4", r4, 0, DEL_SITES, (1, 0, 0), N3() + [[1389353, "C", "T"]])
case("ProcessWithDeletionsReadTest r5", r5, 0, DEL_SITES, (2, 1, 0), N3() + [[1389353, "C", "T"]])
case("ProcessWithDeletionsReadTest r6", r6, 0, DEL_SITES, (2, 1, 0), [None, None, [1389353, "C", "C"]])

case("ProcessOneDeletionReadTest", dict(position=121416521, cigar="68M18D7M",
                                        bases="AGGCGGCTAGCGTGGTGGACCCGGGCCGCGTGGCCCTGTGGCAGCCGAGCCATGGTTTCTAAACTGAGTCTGGCG", quals=0), 0,
     [[121416588, "GCCAGCTGCAGACGGAGCT", "G"]], (2, 0, 1), [[121416588, "GCCAGCTGCAGACGGAGCT", "G"]])

ins_read = dict(position=121432115, cigar="71M3I7M", bases="GGGCCCCCCCCAGGGCCAGGCCCGGGACCTGCGCTGCCCGCTCACAGCTCCCCTGGCCTGCCTCCACCTACCTACCCCCCC", quals=0)
v1, v2, v3, v4 = [121432185, "C", "CCTA"], [121432186, "C", "CGGG"], [121432187, "C", "CGGG"], [121432188, "C", "C"]
case("ProcessInsertionReadTest one", ins_read, 0, [v1], (2, 1, 0), [[121432185, "C", "CCTA"]])
case("ProcessInsertionReadTest PICS-1123", ins_read, 0, [v1, v2, v3], (2, 1, 0), [[121432185, "C", "CCTA"], [121432186, "C", "C"], [121432187, "C", "C"]])
case("ProcessInsertionReadTest slightly different", ins_read, 0, [v2, v3, v4], (2, 1, 0), [[121432186, "C", "C"], [121432187, "C", "C"], [121432188, "C", "C"]])

del_read = dict(position=121432115, cigar="71M3D10M", bases=ins_read["bases"], quals=0)
d1, d2, d3, d4 = [121432185, "CGGG", "C"], [121432186, "CAA", "C"], [121432187, "CCACAC", "C"], [121432188, "C", "C"]
case("ProcessMixedDeletionsReadTest one", del_read, 0, [d1], (2, 0, 1), [[121432185, "CGGG", "C"]])
case("ProcessMixedDeletionsReadTest three", del_read, 0, [d1, d2, d3], (2, 0, 1), [[121432185, "CGGG", "C"], [121432186, "N", "N"], [121432187, "N", "N"]])
case("ProcessMixedDeletionsReadTest shifted", del_read, 0, [d2, d3, d4], (2, 0, 1), [[121432186, "N", "N"], [121432187, "N", "N"], [121432188, "N", "N"]])

case("CheckSimpleSNPQuery", MNV_READ, 0, [], (1, 0, 0), [], last_pos=11)
mix_read = dict(position=3, cigar="2S4M2I4M4S", bases="AA" + "ACGT" + "GG" + "ACGT" + "GGGG", quals=0)
case("FindMixOfInsertionsAndSnpsromReadTest at 6", mix_read, 0, [[6, "T", "T"], [6, "T", "TTT"], [6, "TTT", "T"]], (2, 1, 0),
     [[6, "T", "T"], [6, "X", "X"], [6, "T", "T"]], last_pos=11)
case("FindMixOfInsertionsAndSnpsromReadTest at 7", mix_read, 0, [[7, "A", "A"], [7, "A", "AAA"], [7, "AAA", "A"]], (2, 1, 0),
     [[7, "A", "A"], [7, "A", "A"], [7, "A", "A"]], last_pos=11)

T, D, R, I = "FoundThisVariant", "FoundDifferentVariant", "FoundReferenceVariant", "HaveInsufficientData"
checks = []
for family, look, rows in [
    ("CheckWeCanFindASnpInARead", [4, "T", "C"], [(2, "AACAA", T), (4, "C", T), (2, "AAGAA", D), (4, "G", D), (2, "AATAA", R), (4, "T", R), (2, "AANAA", I), (4, "N", I)]),
    ("CheckWeCanFindAnMNVInARead_healthyMNV", [4, "TA", "CC"], [(2, "AACCAA", T), (4, "CC", T), (2, "AAGCAA", D), (4, "GC", D), (2, "AATAA", R), (4, "TA", R), (4, "T", I),
                                                               (2, "AANAA", I), (4, "NN", I)]),
    ("CheckWeCanFindAnMNVInARead_pathologicalMNV", [4, "ATA", "ACG"], [(4, "ACG", T), (3, "AACGA", T), (5, "C", I), (3, "AATAA", R), (3, "GGGGG", D), (3, "AACAA", D),
                                                                    (5, "CAA", I), (5, "CG", I)]),
    ("CheckWeCanFindARefInARead", [4, "T", "T"], [(2, "AATCAA", T), (4, "TC", T), (2, "AAGCAA", D), (4, "GC", D), (2, "AATAA", T), (4, "TA", T), (4, "T", T), (2, "AANAA", I),
                                                  (4, "NN", I)]),
]:
    for p, alt, state in rows:
        checks.append(dict(family=family, look=look, segment=[p, alt], state=state))

SITES5 = [[100, "A", "C"], [400, "A", "C"], [505, "A", "C"], [703, "A", "T"], [800, "A", "C"]]
READS1 = [[10, "ACGT", 30], [96, "ACGT", 30], [100, "ACGT", 30], [300, "ACGT", 30], [400, "ACGT", 19], [500, "ACGT", 30], [700, "ACGT", 30], [800, "ACGT", 30],
          [805, "ACGT", 30], [900, "ACGT", 30]]
get_veads = [
    dict(name="GetVeads five sites", sites=SITES5, reads=READS1, min_q=20, min_map_quality=20, last_with_look_ahead=801, group_read_positions=[100, 700, 800], n_veads=[1, 1, 1]),
    dict(name="GetVeads with the long deletion", sites=SITES5 + [[790, "ACAGTGAAAGACTTGTGAC", "C"]], reads=READS1, min_q=20, min_map_quality=20, last_with_look_ahead=809,
         group_read_positions=[100, 700, 800], n_veads=[1, 1, 1]),
    dict(name="GetVeads boundary", sites=SITES5 + [[790, "ACAGTGAAAGACTTGTGAC", "C"]], reads=[[10, "ACGT", 30], [96, "ACGT", 30], [97, "ACGT", 30]], min_q=20, min_map_quality=20,
         last_with_look_ahead=809, group_read_positions=[97], n_veads=[1]),
]
group_veads = [
    dict(name="Four Ns", sites=[[100, "C", "C"], [101, "G", "N"]], reads=["CN"] * 4, memberships=[4]),
    dict(name="Sample 129", sites=[[100, "A", "G"], [100, "A", "A"], [100, "N", "N"], [101, "N", "N"], [101, "C", "A"], [101, "C", "C"]],
         reads=["GN", "GC", "AC", "GA", "NC", "NA"], memberships=[1, 1, 1, 1, 1, 1]),
    dict(name="Ten grouped reads",
         sites=[[100, "C", "C"], [100, "C", "A"], [100, "N", "N"], [101, "N", "N"], [101, "C", "A"], [101, "C", "C"], [102, "C", "A"], [103, "C", "A"], [104, "N", "N"],
                [104, "C", "A"], [104, "C", "C"], [105, "C", "A"]],
         reads=["NNAAAA", "NNAAAA", "NAAANA", "NAAANA", "NNAAAA", "CCCCCC", "NAAANA", "NAAANA", "NAAANA", "AAAANA"], memberships=[3, 5, 1, 1]),
]
S2 = [[10, "A", "C"], [15, "G", "A"]]
filters = dict(
    past=[dict(sites=S2, reads=[[6, False], [8, False], [11, False], [14, False], [15, False], [16, False], [17, True]]),
          dict(sites=[[10, "A", "C"], [15, "G", "GAAA"]], reads=[[15, False], [16, False], [17, False], [18, False], [19, False], [20, True]]),
          dict(sites=[[10, "A", "C"], [15, "GAAA", "G"]], reads=[[18, False], [19, False], [20, True]]),
          dict(sites=[[10, "A", "ATTTTTTT"], [15, "G", "A"]], reads=[[16, False], [17, False], [18, False], [20, True]])],
    skip=[dict(sites=S2, reads=[[6, True], [7, False], [12, False], [16, False]])],
    clipped=[dict(sites=[[10, "A", "C"], [15, "G", "A"], [25, "T", "G"]], soft_clip_end_before=9, soft_clip_pos_after=26,
                  reads=[[6, "4M", False], [8, "4M", False], [15, "4M", False], [8, "1M3S", False], [8, "2M2S", True], [8, "3M1S", True], [25, "1S3M", True],
                         [26, "2S2M", True], [27, "3S1M", False]]),
             dict(sites=[[10, "ACC", "A"], [25, "TCC", "T"]], soft_clip_end_before=10, soft_clip_pos_after=28, reads=[]),
             dict(sites=[[10, "A", "ACC"], [25, "T", "TCC"]], soft_clip_end_before=10, soft_clip_pos_after=26, reads=[])],
    range_of_interest=[dict(sites=[[120, "N", "N"], [121, "N", "N"]], first=120, last_in_vcf=121, last_with_look_ahead=122)],
)
doc = dict(finder_cases=finder, check_cases=checks, get_veads=get_veads, group_veads=group_veads, filters=filters)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "vead_cases.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(len(finder), len(checks))
