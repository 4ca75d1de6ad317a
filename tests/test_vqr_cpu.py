"""VariantQualityRecalibration without a GPU: the plain-Python statement (tests/vqr_ref.py) against the reference's own known answers
(tests/golden/vqr_cases.json), and the library's host entries (pisces_hip_vqr_count, pisces_hip_vqr_tables: csrc/vqr.h, the source the
kernels compile) against the same answers and against the statement on seeded rows and counts."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import vqr_cases, vqr_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "vqr_cases.json")))
DEFAULTS = engine.vqr_options()   # (a library without the VQR entries fails here: no test of this file passes on one)


def _counts_of_file(name):
    c = G["counts"][name]
    return {"by": dict(zip(G["categories"], (float(x) for x in c["by_category"]))), "npv": float(c["num_possible_variants"])}


def _by_chromosome(vcf):
    out = []
    for v in G["vcfs"][vcf]:
        if not out or out[-1][0] != v["chrom"]:
            out.append((v["chrom"], []))
        out[-1][1].append(R.row_of_vcf(v))
    return out


def _lib_options(o):
    return engine.vqr_options(**o)


def _strain_file(vcf, o, library):
    """SignatureSorter.StrainVcf over a golden VCF, a chromosome a call: ((by_category, num_possible) x 2, suspect (chrom, pos, ref, alt))"""
    suspects = []
    if library:
        arr = engine.vqr_counts_array()
        for chrom, rows in _by_chromosome(vcf):
            _, s = engine.vqr_count(R.records_of_rows(rows), _lib_options(o), counts=arr)
            suspects += [[chrom, r["position"], r["ref"], r["alt"]] for i, r in enumerate(rows) if s is not None and s[i]]
        pair = R.counts_of_struct(arr)
    else:
        basic, edge = R.new_counts(), R.new_counts()
        for chrom, rows in _by_chromosome(vcf):
            _, _, s = R.strain(rows, o["extent_of_edge_region"], bool(o["do_amplicon_position_checks"]), basic=basic, edge=edge)
            suspects += [[chrom, r["position"], r["ref"], r["alt"]] for i, r in enumerate(rows) if s[i]]
        pair = R.counts_pair(basic, edge)
    if o["loci_count"] > 0:   # ForceTotalPossibleMutations before the files are written (SignatureSorter.cs:78-82)
        pair = [(by, o["loci_count"]) for by, _ in pair]
    return pair, suspects


# ---- the reference's known answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("library", [False, True], ids=["statement", "library"])
def test_signature_sorter_counts_files(library):
    for test, vcf, counts, which in (("WriteCountsFile", "TestSignatureSorter.vcf", "Expected.counts", 0),
                                     ("WriteCountsFileGivenLociCounts", "TestSignatureSorter.vcf", "ExpectedGivenLociNum.counts", 0),
                                     ("WriteEdgeCountsFile", "FindEdges.vcf", "Expected.edgecounts", 1),
                                     ("WriteEdgeCountsFileGivenLociCounts", "FindEdges.vcf", "ExpectedGivenLociNum.edgecounts", 1)):
        o = R.options(**G["options"][test])
        pair, suspects = _strain_file(vcf, o, library)
        exp = G["counts"][counts]
        assert list(pair[which][0]) == exp["by_category"], (test, pair[which][0])
        assert pair[which][1] == exp["num_possible_variants"], test
        if which == 1:
            assert suspects == G["edgevariants"] and len(suspects) == 16, test


def test_did_we_detect_an_edge_buffers():
    """EdgeIssueCountDataTests.DidWeDetectAnEdge: the statement on every buffer; the library on those a row array can express (empty
    slots at the ends only, one chromosome: a foreign row in the middle of a window cannot reach a call that sees one chromosome)"""
    through_library = 0
    for case in G["did_we_detect_an_edge"]:
        foreign = any(b is not None and b[0] != "chr1" for b in case["buffer"])
        buf = [None if (b is None or b[0] != "chr1") else (b[1], b[2]) for b in case["buffer"]]
        t = case["test_index"]
        assert R.did_we_detect_an_edge(t, buf) == case["expected"], case["line"]
        there = [b for b in buf if b is not None]
        if foreign or len(there) <= t or any(b is None for b in buf[:len(there)]):
            continue
        rows = [{"position": p, "total_coverage": c, "allele_support": 10, "variant_qscore": 100, "genotype_qscore": 100, "noise_level": 20,
                 "filter_bits": 0, "type": "Snv", "ref": "A", "alt": "G"} for p, c in there]
        _, s = engine.vqr_count(R.records_of_rows(rows), engine.vqr_options(do_amplicon_position_checks=1, extent_of_edge_region=3), lo=t, hi=t + 1)
        assert bool(s[t]) == case["expected"], case["line"]
        through_library += 1
    assert through_library >= 12


def test_update_variant_facts():
    """RecalTests.UpdateVariant / InsertNewQ / HaveInfoToUpdateQ on the statement"""
    u = G["update_variant"]
    name_bit = {"LowVariantQscore": 3, "OffTarget": 11}
    for filter_q, before, after in u["filter_cases"]:
        row = dict(u["allele"], filter_bits=sum(1 << name_bit[n] for n in before), position=1, type="Snv", ref="C", alt="A")
        R.update_variant_qscore_and_refilter(u["max_qscore"], filter_q, {u["category"]: u["rate"]}, row, u["category"], False)
        assert {k: row[k] for k in u["expected"]} == u["expected"]
        assert row["filter_bits"] == sum(1 << name_bit[n] for n in after)
    row = dict(u["allele"], filter_bits=0)
    R.insert_new_q({u["category"]: u["rate"]}, row, u["category"], u["insert_new_q"]["new_q"], True)
    assert {k: row[k] for k in u["insert_new_q"]["expected"]} == u["insert_new_q"]["expected"]
    assert R.have_info_to_update_q(dict(u["allele"])) == (True, float(u["have_info"]["depth"]), float(u["have_info"]["call_count"]))
    assert R.have_info_to_update_q(dict(u["allele"], variant_qscore=0))[0] is False


def _golden_tables(test, library):
    """(options, tables as the statement's dict, rows and suspects by chromosome) of the two recalibration goldens"""
    o = R.options(**G["options"][test])
    if test == "RecalibrateDirtyVcf":
        chroms = _by_chromosome("TestWithArtifacts.vcf")
        basic, edge = _counts_of_file("Dirty.counts"), R.new_counts()
        per = [(rows, None) for _, rows in chroms]
    else:
        chroms = _by_chromosome("TestEdgeExample.vcf")
        basic, edge = R.new_counts(), R.new_counts()
        per = []
        for _, rows in chroms:
            _, _, s = R.strain(rows, o["extent_of_edge_region"], True, basic=basic, edge=edge)
            per.append((rows, s))
    if library:
        T = R.tables_of_struct(engine.vqr_tables(engine.vqr_counts_array(R.counts_pair(basic, edge)), _lib_options(o)))
    else:
        T = R.tables(o, basic, edge)
    return o, T, per


@pytest.mark.parametrize("library_tables", [False, True], ids=["statement", "library-tables"])
@pytest.mark.parametrize("test,expected", [("RecalibrateDirtyVcf", "ExpectedDirty.vcf.recal"), ("RecalibrateDirtyVcfs", "ExpectedEdgeExample.vcf.recal")])
def test_recalibrated_vcfs(test, expected, library_tables):
    """every row of the two expected .recal files (QUAL, GQ, NL, FILTER), with the statement's tables and with the library's"""
    o, T, per = _golden_tables(test, library_tables)
    got = []
    for rows, s in per:
        R.apply(o, T, rows, s)
        got += R.fields_of_rows(rows)
    exp = R.fields_of_rows([R.row_of_vcf(v) for v in G["vcfs"][expected]])
    assert len(exp) == (10 if test == "RecalibrateDirtyVcf" else 24)
    assert got == exp
    if test == "RecalibrateDirtyVcfs":
        assert R.INT_MIN in T["edge_risk"].values()   # the golden holds edge-risk rates of int.MinValue


# ---- library == statement on seeded input -------------------------------------------------------------------------------------------
def test_count_matches_statement_on_seeded_rows():
    """20 000 row sets of 1..400 rows at every extent the window logic differs at, sub-ranges included"""
    rng = np.random.default_rng(20240611)
    sizes = np.concatenate([np.arange(1, 41), [63, 64, 65, 129, 130, 255, 256, 257, 399, 400]])
    bad = []
    for it in range(20000):
        n = int(rng.choice(sizes)) if it % 50 else int(rng.integers(1, 401))
        extent = int(rng.choice([0, 1, 2, 4, 64]))
        rows = vqr_cases.make_rows(rng, n)
        lo, hi = 0, n
        if rng.random() < 0.3:
            lo = int(rng.integers(0, n + 1))
            hi = int(rng.integers(lo, n + 1))
        basic, edge, s = R.strain(rows, extent, True, lo, hi)
        arr, got_s = engine.vqr_count(R.records_of_rows(rows), engine.vqr_options(do_amplicon_position_checks=1, extent_of_edge_region=extent), lo, hi)
        if R.counts_of_struct(arr) != R.counts_pair(basic, edge) or list(got_s[lo:hi]) != s[lo:hi]:
            bad.append((it, n, extent, lo, hi))
    assert not bad, bad[:10]


def test_count_without_edge_checks_counts_the_basic_half_only():
    rng = np.random.default_rng(5)
    rows = vqr_cases.make_rows(rng, 300)
    basic, _, _ = R.strain(rows, 4, False)
    arr, s = engine.vqr_count(R.records_of_rows(rows), engine.vqr_options())
    assert s is None and R.counts_of_struct(arr) == R.counts_pair(basic, R.new_counts())
    # counts are added to: a second call doubles them
    engine.vqr_count(R.records_of_rows(rows), engine.vqr_options(), counts=arr)
    assert R.counts_of_struct(arr)[0][1] == 600


def _same_tables(a, b):
    for k in ("basic", "edge", "edge_risk"):
        if (a[k] or {}) != (b[k] or {}):
            return False
    x, y = a["general_edge_risk_increase"], b["general_edge_risk_increase"]
    if a["edge_risk"] is None:
        return True
    return (x != x and y != y) or x == y


def test_tables_match_statement_on_seeded_counts():
    rng = np.random.default_rng(77)
    bad, int_min_seen, in_table = [], 0, 0
    for it in range(5000):
        basic, edge = vqr_cases.count_vector(rng)
        o = R.options(do_basic_checks=int(rng.random() < 0.85), do_amplicon_position_checks=int(rng.random() < 0.7),
                      loci_count=int(rng.choice([-1, 0, 1, 1000, 10 ** 6])) if rng.random() < 0.3 else -1,
                      base_q_noise=int(rng.choice([20, 30, 0, 45])), z_factor=float(rng.choice([0.0, 0.5, 2.0, 3.0])))
        exp = R.tables(o, basic, edge)
        got = R.tables_of_struct(engine.vqr_tables(engine.vqr_counts_array(R.counts_pair(basic, edge)), _lib_options(o)))
        if not _same_tables(exp, got):
            bad.append((it, o, exp, got))
        int_min_seen += bool(exp["edge_risk"]) and R.INT_MIN in exp["edge_risk"].values()
        in_table += len(exp["basic"] or {})
        # the basic and edge tables never hold int.MinValue: count / loci + QtoP(base) is a positive finite number
        assert R.INT_MIN not in (exp["basic"] or {}).values() and R.INT_MIN not in (exp["edge"] or {}).values()
    assert not bad, bad[:3]
    assert int_min_seen > 100 and in_table > 1000


def test_threshold_is_strict_and_all_equal_counts_make_no_table():
    basic = R.new_counts()
    for k in R.SNV_CATEGORIES:
        basic["by"][k] = 7.0
    basic["npv"] = 1000.0
    for z in (0.0, 2.0):
        t = engine.vqr_tables(engine.vqr_counts_array(R.counts_pair(basic, R.new_counts())), engine.vqr_options(z_factor=z))
        assert t.basic_mask == 0 and R.tables(R.options(z_factor=z), basic, R.new_counts())["basic"] == {}
    basic["by"]["CtoT"] = 8.0   # one above the other eleven: mean 7, sigma 0
    t = engine.vqr_tables(engine.vqr_counts_array(R.counts_pair(basic, R.new_counts())), engine.vqr_options())
    assert t.basic_mask == 1 << 5 and t.basic[5] == R.cs_int(R.p_to_q(8.0 / 1000.0 + R.q_to_p(20)))


def test_int_min_rate_never_reaches_the_poisson_evaluation():
    """A rate of int.MinValue only lives in the edge-risk table, where the update subsamples: QtoP is +inf, subSampleToThis 0, so a row
    with depth is cut to (0, 0) and a row without depth has none — AssignPoissonQScore returns 0 before any Poisson tail.  The device's
    update (csrc/vqr.h update_q) relies on this."""
    rng = np.random.default_rng(9)
    R.INT_MIN_REACHED_POISSON[0] = 0
    o = R.options(do_amplicon_position_checks=1, filter_qscore=30)
    T = {"basic": {"CtoT": 12}, "edge": {c: 9 for c in R.SNV_CATEGORIES}, "edge_risk": {c: R.INT_MIN for c in R.SNV_CATEGORIES}}
    rows = vqr_cases.make_rows(rng, 4000, snv_share=0.9, depths=[0, 1, 2, 5000])
    R.apply(o, T, rows, [1] * len(rows))
    hit = [r for r in rows if r["noise_level"] == R.INT_MIN]
    assert len(hit) > 1000 and all(r["variant_qscore"] == 0 and r["genotype_qscore"] == 0 for r in hit)
    assert R.INT_MIN_REACHED_POISSON[0] == 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults():
    assert C.sizeof(_abi.PiscesVqrOptions) == 48 and C.sizeof(_abi.PiscesVqrCounts) == 136 and C.sizeof(_abi.PiscesVqrTables) == 168
    assert _abi.PiscesVqrTables.general_edge_risk_increase.offset == 160 and _abi.PiscesVqrOptions.z_factor.offset == 32
    got = {k: getattr(DEFAULTS, k) for k in R.DEFAULT_OPTIONS}
    assert got == R.DEFAULT_OPTIONS   # VQROptions.cs:11-22 and the base options' MinimumBaseCallQuality 20 / MinimumVariantQScoreFilter 30
    assert _abi.ABI_VERSION == 9
    assert _abi.VQR_CATEGORIES == R.CATEGORIES


def _last_error():
    return engine.lib.pisces_hip_last_error(None).decode()


def test_refusals():
    lib = engine.lib
    recs = R.records_of_rows(vqr_cases.make_rows(np.random.default_rng(1), 10))
    arr = engine.vqr_counts_array()
    sus = np.zeros(10, dtype=np.uint8)
    o = engine.vqr_options()
    p = recs.ctypes.data
    assert lib.pisces_hip_vqr_default_options(None) == _abi.E_INVALID_ARG
    # null arguments
    assert lib.pisces_hip_vqr_count(None, p, 10, 0, 10, arr, None) == _abi.E_INVALID_ARG and "null" in _last_error()
    assert lib.pisces_hip_vqr_count(C.byref(o), None, 10, 0, 10, arr, None) == _abi.E_INVALID_ARG and "null" in _last_error()
    assert lib.pisces_hip_vqr_count(C.byref(o), p, 10, 0, 10, None, None) == _abi.E_INVALID_ARG and "null" in _last_error()
    assert lib.pisces_hip_vqr_tables(None, arr, C.byref(_abi.PiscesVqrTables())) == _abi.E_INVALID_ARG and "null" in _last_error()
    assert lib.pisces_hip_vqr_tables(C.byref(o), None, C.byref(_abi.PiscesVqrTables())) == _abi.E_INVALID_ARG and "null" in _last_error()
    assert lib.pisces_hip_vqr_tables(C.byref(o), arr, None) == _abi.E_INVALID_ARG and "null" in _last_error()
    # extent_of_edge_region outside 0..64
    for extent in (-1, 65):
        bad = engine.vqr_options(extent_of_edge_region=extent)
        assert lib.pisces_hip_vqr_count(C.byref(bad), p, 10, 0, 10, arr, sus.ctypes.data) == _abi.E_INVALID_ARG and "extent_of_edge_region" in _last_error()
        assert lib.pisces_hip_vqr_tables(C.byref(bad), arr, C.byref(_abi.PiscesVqrTables())) == _abi.E_INVALID_ARG and "extent_of_edge_region" in _last_error()
    # lo / hi outside [0, n]
    for lo, hi in ((-1, 5), (0, 11), (6, 5)):
        assert lib.pisces_hip_vqr_count(C.byref(o), p, 10, lo, hi, arr, None) == _abi.E_INVALID_ARG and "rows [" in _last_error()
    assert lib.pisces_hip_vqr_count(C.byref(o), p, -1, 0, 0, arr, None) == _abi.E_INVALID_ARG
    # edge checks on without the suspect bytes
    edges = engine.vqr_options(do_amplicon_position_checks=1)
    assert lib.pisces_hip_vqr_count(C.byref(edges), p, 10, 0, 10, arr, None) == _abi.E_INVALID_ARG and "suspect" in _last_error()
    # nothing was counted by a refused call
    assert R.counts_of_struct(arr) == R.counts_pair(R.new_counts(), R.new_counts())
    # the device entries refuse a null handle before anything else
    assert lib.pisces_hip_vqr_count_device(None, C.byref(o), None, 0, None, 0, 0, None, None, None) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_vqr_apply_device(None, C.byref(o), C.byref(_abi.PiscesVqrTables()), None, 0, None, None, None, None) == _abi.E_INVALID_ARG
    # n = 0 is a call like any other
    assert lib.pisces_hip_vqr_count(C.byref(o), None, 0, 0, 0, arr, None) == 0


def test_entries_are_exported():
    from pisces_amd import _native
    for name in ("pisces_hip_vqr_default_options", "pisces_hip_vqr_count_device", "pisces_hip_vqr_count", "pisces_hip_vqr_tables", "pisces_hip_vqr_apply_device"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
