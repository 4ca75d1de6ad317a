"""The reference's own unit-test known answers through the PRODUCT (libpisceship.so), not through the oracle.

tests/test_oracle_golden.py pins the oracle (a CPU restatement, test infrastructure) with these tables; the product's host collapser,
MNV reallocator, per-locus genotypers and candidate kernel were until now only compared WITH the oracle — and product and oracle are
restatements of the same C# by one author, so a shared misreading would pass.  Here the expectations come from the JSON files under
tests/golden/ (transcribed from the reference's tests, file:line in each), and the code that runs is the library's:

  * CPU (no GPU needed: host code of the product behind its C ABI)
      mnv_reallocator_cases.json   MNVReallocatorTests.cs:18-662            -> pisces_hip_reallocate_failed_mnvs
      diploid_cases.json           GenotypeCalculatorTest.cs, DiploidGenotypeQualityCalculatorTests.cs, HaploidGenotypeCalculatorTests.cs
                                                                             -> pisces_hip_set_genotypes, pisces_hip_diploid_genotype_qscore
  * GPU (through pisces_hip_add_observations + pisces_hip_add_candidates + pisces_hip_flush_ex: counts injected cell by cell as the
    tests' mock IAlleleSource returns them, candidates as the tests build them)
      collapser_cases.json         VariantCollapserTests.cs:18-204, 869-1033  -> the flush's collapser, frequencies from the device's counts
      coverage_spanning.json       CoverageCalculatorTests.cs:69-702          -> the candidate kernel's coverage / the tile kernels' point coverage
      caller_matrix.json           VariantCallerTests.cs:27-277               -> IsCallable by coverage / frequency / q-score, reference pruning
      done_processing.json         RegionStateManagerTests.cs:707-781         -> the flush's block choice and DoneProcessing: a cleared block's counts read 0, held blocks keep theirs
      gapped_mnv_ref.json          RegionStateManagerTests.cs:136-169; RegionStateTests.cs:282-325 -> pisces_hip_add_gapped_mnv_ref / pisces_hip_get_gapped_mnv_ref
      region_candidates.json       RegionStateTests.cs:339-437                -> the rows of GetAllCandidates' candidates: Reference rows by coverage and interval set
      caller_mnv_cases.json        VariantCallerTests.cs:307-656              -> MNV reallocation as the flush drives it: block edge, interval edge, reference support taken
      gapped_mnv_ref_support.json  VariantCallerTests.cs:658-763              -> the reference support the gaps of a flush's MNVs take from its Reference rows
    (region_state.json's `deletions`, RegionStateManagerTests.cs:597-704, is read input: tests/test_gpu_parity.py beside the other read scenarios)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
load = lambda name: json.load(open(os.path.join(G, name)))
ALLELE = {"A": 0, "G": 1, "C": 2, "T": 3, "N": 4, "Deletion": 5, "Del": 5}
DIR = {"F": 0, "R": 1, "S": 2}
CAT = {"Snv": _abi.CAT_SNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION, "Mnv": _abi.CAT_MNV, "Reference": _abi.CAT_REFERENCE}
GT_CODE = {"HeterozygousAlt1Alt2": 0, "Alt12LikeNoCall": 1, "HeterozygousAltRef": 2, "HomozygousAlt": 3, "HomozygousRef": 4,
           "RefLikeNoCall": 5, "AltLikeNoCall": 6, "RefAndNoCall": 7, "AltAndNoCall": 8}


# ============================================================================================ CPU: the host half as functions
def _candidates(items):
    arr = (_abi.PiscesCandidate * max(1, len(items)))()
    pool = bytearray()
    for i, d in enumerate(items):
        c = arr[i]
        c.position, c.category = d["position"], d["category"]
        c.ref_len, c.alt_len = len(d["ref"]), len(d["alt"])
        for k in range(3):
            c.support_by_dir[k] = d["dirs"][k]
        c.allele_offset = len(pool)
        pool += d["ref"].encode() + d["alt"].encode()
    return arr, np.frombuffer(bytes(pool) or b"\0", dtype=np.uint8).copy(), len(pool)


def _product_reallocate(failed, callable_, block_max):
    from pisces_amd import _native
    both = list(failed) + list(callable_)
    arr, pool, nb = _candidates(both)
    cap = len(callable_) + 64 * max(len(failed), 1)
    out_c, out_o = (_abi.PiscesCandidate * cap)(), (_abi.PiscesCandidate * cap)()
    out_pool = np.zeros(1 << 16, dtype=np.uint8)
    nc, no, nbytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    f_ptr = C.cast(arr, C.c_void_p)
    c_ptr = C.c_void_p(C.addressof(arr) + len(failed) * C.sizeof(_abi.PiscesCandidate))
    rc = _native.lib.pisces_hip_reallocate_failed_mnvs(f_ptr, len(failed), c_ptr, len(callable_), pool.ctypes.data, nb,
                                                       -1 if block_max is None else int(block_max), C.cast(out_c, C.c_void_p), cap, C.byref(nc),
                                                       C.cast(out_o, C.c_void_p), cap, C.byref(no), out_pool.ctypes.data, len(out_pool), C.byref(nbytes))
    assert rc == 0, rc

    def rows(a, n):
        out = []
        for i in range(n):
            c = a[i]
            o = c.allele_offset
            out.append({"position": c.position, "ref": bytes(out_pool[o:o + c.ref_len]).decode(), "alt": bytes(out_pool[o + c.ref_len:o + c.ref_len + c.alt_len]).decode(),
                        "dirs": [c.support_by_dir[k] for k in range(3)], "category": c.category})
        return out
    return rows(out_c, nc.value), rows(out_o, no.value)


def _as_the_product_holds_it(d):
    """The reference's tests build CalledAlleles whose AlleleSupport and SupportByDirection are set independently (a callable allele with
    AlleleSupport 5 and no directional support).  The product keeps ONE number: AlleleSupport is the sum of support_by_dir.  An allele
    without directional support is therefore handed over with its AlleleSupport in the first direction — the order the reallocator ranks
    overlapping alleles in (longer first, then more AlleleSupport) is the test's, and what it must ADD (the failed MNV's directional
    support) is checked direction by direction."""
    dirs = list(d["dirs"])
    if sum(dirs) == 0 and d["support"] != 0:
        dirs = [d["support"], 0, 0]
    return {"position": d["position"], "ref": d["ref"], "alt": d["alt"], "category": d["category"], "dirs": dirs}


def _norm(rows):
    return sorted((r["position"], r["ref"], r["alt"], tuple(r["dirs"]), r["category"]) for r in rows)


@pytest.mark.parametrize("case", load("mnv_reallocator_cases.json")["cases"], ids=lambda c: c["name"][:40])
def test_product_mnv_reallocator_reference_cases(case):
    """MNVReallocatorTests.cs:18-662 through the library's own MnvReallocator (mnv_reallocate_failed, the function pisces_hip_flush runs
    between its two device passes): who takes the failed MNV's support, what is broken down to smaller MNVs / SNVs, what goes to the
    next block.  Expected directional support = the callable allele's own + what the test expects it to gain."""
    failed = [_as_the_product_holds_it(d) for d in case["failed"]]
    callable_ = [_as_the_product_holds_it(d) for d in case["callable"]]
    got_callable, got_outside = _product_reallocate(failed, callable_, case["max"])
    own = {}
    for d_in, d_held in zip(case["callable"], callable_):
        own[(d_in["position"], d_in["ref"], d_in["alt"])] = (d_in, d_held["dirs"])

    def expected(rows):
        out = []
        for r in rows:
            k = (r["position"], r["ref"], r["alt"])
            if k in own:   # what the allele gains in the test (directional support; AlleleSupport alone where the failed MNV has none), on top of what the product was given
                given, held = own[k]
                gain = [r["dirs"][i] - given["dirs"][i] for i in range(3)]
                if not any(gain):
                    gain = [r["support"] - given["support"], 0, 0]
                dirs = [held[i] + gain[i] for i in range(3)]
            else:          # an allele the reallocator makes: it carries the failed MNV's support
                dirs = _as_the_product_holds_it(r)["dirs"]
            out.append({"position": r["position"], "ref": r["ref"], "alt": r["alt"], "dirs": dirs, "category": r["category"]})
        return out
    if "expect_callable" in case:
        assert _norm(got_callable) == _norm(expected(case["expect_callable"]))
    for want in case.get("expect_callable_contains", []):
        assert _norm(got_callable).count(_norm(expected([want]))[0]) == 1
    assert _norm(got_outside) == _norm(expected(case["expect_outside"]))


def _product_genotypes(alleles, ploidy, min_depth, min_gq=0, max_gq=0):
    from pisces_amd import _native
    cfg = _abi.default_config(ploidy=ploidy, min_coverage=min_depth, min_genotype_qscore=min_gq, max_genotype_qscore=max_gq)
    arr = (_abi.PiscesGenotypeAllele * max(1, len(alleles)))()
    pool = bytearray()
    for i, d in enumerate(alleles):
        a = arr[i]
        a.category, a.ref_len, a.alt_len = d["category"], len(d["ref"]), len(d["alt"])
        a.support, a.coverage, a.reference_support = d["support"], d["coverage"], d["ref_support"]
        a.allele_offset = len(pool)
        pool += d["ref"].encode() + d["alt"].encode()
    poola = np.frombuffer(bytes(pool) or b"\0", dtype=np.uint8).copy()
    gt = _native.lib.pisces_hip_set_genotypes(C.byref(cfg), arr, len(alleles), poola.ctypes.data, len(pool))
    return gt, [int(arr[i].prune) for i in range(len(alleles))], [int(arr[i].genotype) for i in range(len(alleles))]


_DIPLOID = load("diploid_cases.json")


@pytest.mark.parametrize("case", _DIPLOID["genotype_scenarios"], ids=lambda c: "%s-%s-%s" % (c["genotype"], c["ref_freqs"], c["alt_freqs"]))
def test_product_diploid_genotype_scenarios(case):
    """GenotypeCalculatorTest.DiploidGenotypeScenarios through its harness (:107-147) and the library's DiploidThresholdingGenotyper
    (diploid.cpp, the host pass of pisces_hip_flush in PloidyModel.DiploidByThresholding)."""
    cov = case["coverage"]
    alleles, ref_freq = [], 0.0
    for rf in case["ref_freqs"]:
        sup = int(np.float32(rf) * np.float32(cov))
        alleles.append({"category": _abi.CAT_REFERENCE, "ref": "A", "alt": "A", "support": sup, "coverage": cov, "ref_support": sup})
        ref_freq = float(np.float32(rf))
    if ref_freq == 0:
        ref_freq = 1.0 - float(np.sum(np.array(case["alt_freqs"], dtype=np.float32), dtype=np.float32))
    for vf in case["alt_freqs"]:
        alleles.append({"category": _abi.CAT_SNV, "ref": "A", "alt": "T", "support": int(np.float32(vf) * np.float32(cov)), "coverage": cov,
                        "ref_support": int(ref_freq * cov)})
    gt, prune, per = _product_genotypes(alleles, _abi.PLOIDY_DIPLOID if hasattr(_abi, "PLOIDY_DIPLOID") else 1, _DIPLOID["min_depth_to_genotype"])
    assert gt == GT_CODE[case["genotype"]] and sum(prune) == case["prune"]
    assert all(g == gt for g in per)


@pytest.mark.parametrize("table", _DIPLOID["genotype_qscores"], ids=lambda t: "%s-%d" % (t["genotype"], t["depth"]))
def test_product_diploid_genotype_qscores(table):
    """DiploidGenotypeQualityCalculatorTests (:16-96, :103-117) through TestCalculation (:124-134) and the library's calculator."""
    from pisces_amd import _native
    gt = GT_CODE[table["genotype"]]
    for f, want in zip(table["frequencies"], table["expected"]):
        depth = float(table["depth"])
        support = int(depth * f)
        if table["genotype"] == "HomozygousRef":
            support = int(depth * (1.0 - f))
        assert _native.lib.pisces_hip_diploid_genotype_qscore(gt, int(depth), support, 0, 2147483647) == want, (table["genotype"], depth, f)


@pytest.mark.parametrize("want,prune,ref_freq,alt_freqs,coverage", [
    (9, 2, 0.80, [0.01, 0.01], 1000),     # HemizygousRefTest
    (11, 2, 0.70, [0.01, 0.01], 1000),    # NoCallDueToRefMajorVf
    (11, 2, 0.22, [0.75, 0.01], 1000),    # NoCallDueToRefMinorVf
    (11, 2, 0.80, [0.01, 0.01], 10),      # NoCallDueToCoverge
    (10, 1, 0.10, [0.75, 0.01], 1000),    # HemizygousAlt
])
def test_product_haploid_genotype_scenarios(want, prune, ref_freq, alt_freqs, coverage):
    """HaploidGenotypeCalculatorTests.cs:59-96 through its harness (:20-57) and the library's HaploidGenotyper."""
    sup = int(np.float32(ref_freq) * np.float32(coverage))
    alleles = [{"category": _abi.CAT_REFERENCE, "ref": "A", "alt": "A", "support": sup, "coverage": coverage, "ref_support": sup}]
    for vf in alt_freqs:
        alleles.append({"category": _abi.CAT_SNV, "ref": "A", "alt": "T", "support": int(np.float32(vf) * np.float32(coverage)),
                        "coverage": coverage, "ref_support": int(float(np.float32(ref_freq)) * coverage)})
    gt, pr, per = _product_genotypes(alleles, 2, 100, min_gq=0, max_gq=100)
    assert gt == want and sum(pr) == prune and all(g == gt for g in per)


# ============================================================================================ GPU: through the flush
@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _stage(c, cells):
    """cells: {(position, allele type, direction, anchor bin): count} -> that many observations each (IAlleleSource.GetAlleleCount then
    returns exactly these cells)."""
    pos, tup = [], []
    for (p, a, d, anchor), n in cells.items():
        if n <= 0:
            continue
        q = 255 if a == 5 else 30
        pos += [p] * n
        tup += [_abi.tuple_pack(0, anchor, d, a, q)] * n
    if pos:
        c.AddObservations(np.array(pos, dtype=np.int32), np.array(tup, dtype=np.uint32))


def _permissive(**kw):
    """Every candidate comes back as a row: no coverage / frequency / q-score threshold, no filter."""
    base = dict(min_coverage=0, min_variant_qscore=0, min_frequency=0.0, rmxn_max_repeat_length=-1, variant_qscore_filter=-1, low_depth_filter=-1,
                variant_freq_filter=-1.0, no_call_filter_threshold=-1.0)
    base.update(kw)
    return _abi.default_config(**base)


@pytest.mark.gpu
@pytest.mark.parametrize("case", load("collapser_cases.json")["cases"], ids=lambda c: c["name"])
def test_product_collapser_reference_cases(torch_cuda, case):
    """VariantCollapserTests (HappyPath :18-65, NegativeCases :112-204, suites :949-1033) through ExecuteTest's set-up (:869-916): every
    candidate with support [1, 0, 0], a state in which every allele count is 1, thresholds 0 — and the library's flush: candidates in
    through pisces_hip_add_candidates, counts through pisces_hip_add_observations, the collapser between them and the candidate kernel.
    What comes back: as many insertion / deletion rows as the test expects candidates to be left, TotalNumCollapsed, the survivor's
    support; in the given and in the reversed order."""
    from pisces_amd import engine
    ref = np.frombuffer(b"ACGT" * 16, dtype=np.uint8)
    cfg = _permissive(collapse=1, collapse_freq_threshold=0.0, collapse_freq_ratio_threshold=0.0, include_reference_calls=0)
    cells = {(p, a, d, 5): 1 for p in range(1, 40) for a in range(6) for d in range(3)}
    for order in (case["candidates"], list(reversed(case["candidates"]))):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(ref)
            _stage(c, cells)
            c.AddCandidates([{"position": x["pos"], "category": CAT[x["category"]], "ref": x["ref"], "alt": x["alt"], "support_by_dir": (1, 0, 0),
                              "open_left": x["open_left"], "open_right": x["open_right"]} for x in order])
            recs, alleles = c.CallWithAlleles()
            stats = c.Stats()
        rows = [(r, a) for r, a in zip(recs, alleles) if _abi.info_category(r["info"]) in (_abi.CAT_INSERTION, _abi.CAT_DELETION)]
        assert len(rows) == case["expected_count"], [(int(r["position"]), a) for r, a in rows]
        assert stats["TotalNumCollapsed"] == len(order) - case["expected_count"]
        if case["expected_support_first"] is not None:
            assert int(rows[0][0]["allele_support"]) == case["expected_support_first"]


def _coverage_cells(case):
    cells = {}
    for row in case["counts"]:
        a = ALLELE[row["allele"]]
        if "dirs" in row:
            for d, v in enumerate(row["dirs"]):
                cells[(row["coord"], a, d, 5)] = v
        else:
            for d, per in enumerate(row["anchors"]):
                for anchor, v in per.items():
                    cells[(row["coord"], a, d, int(anchor))] = v
    return cells


def _coverage_row(case, support, well_anchored):
    """The row the library reports for the case's allele with the given stitched support / well-anchored support."""
    from pisces_amd import engine
    v = case["allele"]
    ref = bytearray(b"A" * 32)
    ref[v["pos"] - 1:v["pos"] - 1 + len(v["ref"])] = v["ref"].encode()
    cat = v["category"]
    # SNV candidates are the caller's only with MNV calling on (off: they are the allele counts); a Reference allele is the gVCF's
    cfg = _permissive(call_mnvs=1 if cat in ("Snv", "Mnv") else 0, include_reference_calls=1 if cat == "Reference" else 0, collapse=0, max_mnv_length=8)
    # (a Reference allele on a locus whose counts show other bases: the library makes SNV candidates of those bases unless the candidates
    # are the read walk's alone — MNV calling on in its earlier form, where the tile kernels emit Reference records only)
    if cat == "Reference":
        cfg = _permissive(call_mnvs=1, include_reference_calls=1, collapse=0)
    old = os.environ.get("PISCES_HIP_MNV_SPLIT")
    if cat == "Reference":
        os.environ["PISCES_HIP_MNV_SPLIT"] = "0"
    try:
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(np.frombuffer(bytes(ref), dtype=np.uint8))
            _stage(c, _coverage_cells(case))
            if case.get("taken_ref"):
                c.AddGappedMnvRefCount({v["pos"]: case["taken_ref"]})
            if cat != "Reference":
                c.AddCandidates([{"position": v["pos"], "category": CAT[cat], "ref": v["ref"], "alt": v["alt"], "support_by_dir": (0, 0, support),
                                  "well_anchored_by_dir": (0, 0, well_anchored)}])
            recs, alleles = c.CallWithAlleles()
    finally:
        if cat == "Reference":
            if old is None:
                os.environ.pop("PISCES_HIP_MNV_SPLIT", None)
            else:
                os.environ["PISCES_HIP_MNV_SPLIT"] = old
    rows = [r for r, a in zip(recs, alleles) if int(r["position"]) == v["pos"] and a == (v["ref"], v["alt"]) and _abi.info_category(r["info"]) == CAT[cat]]
    assert len(rows) == 1, [(int(r["position"]), a) for r, a in zip(recs, alleles)]
    return rows[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", load("coverage_spanning.json")["cases"], ids=lambda c: c["name"])
def test_product_coverage_calculator_reference_cases(torch_cuda, case):
    """CoverageCalculatorTests.ComputeCoverage_* (:69-702) through the library: the counts of the test's mock allele source cell by cell
    (allele, direction, anchor bin), the allele as a candidate (or, a Reference allele, as the gVCF's), and the coverage the record comes
    back with.  The product always tracks anchors (TrackedAnchorSize 5), so an insertion is run the three anchor-aware ways of the test's
    harness (:704-760: fully anchored, fully unanchored, half and half); alleles of other kinds do not look at the bins."""
    exp_dir, exp_total = case["by_dir"], case["total"]
    cat = case["allele"]["category"]

    def check(row, by_dir, total, support):
        assert int(row["total_coverage"]) == total
        got = [int(x) for x in row["coverage_by_dir"]][: len(by_dir)]
        assert got == list(by_dir)
        if case.get("check_aux", True):
            if cat == "Reference":
                assert int(row["allele_support"]) == case.get("snv_ref", 0)
            elif cat == "Snv":
                assert int(row["reference_support"]) == case.get("snv_ref", 0)
            else:
                assert int(row["reference_support"]) == total - support
    if cat != "Insertion":
        row = _coverage_row(case, 5, 5)
        check(row, exp_dir, exp_total, 5)
        if "expect_ref_support" in case:
            assert int(row["reference_support"]) == case["expect_ref_support"]
        return
    suspicious = case.get("suspicious", 0)
    aware = case.get("by_dir_anchor_aware")
    check(_coverage_row(case, 5, 5), aware if aware is not None else exp_dir, sum(aware) if aware is not None else exp_total - suspicious, 5)
    check(_coverage_row(case, 5, 0), exp_dir, exp_total, 5)
    from_unanchored = np.float32(suspicious) * np.float32(0.5)
    total_support = int(from_unanchored + np.float32(0.5) * np.float32(exp_total - suspicious))
    check(_coverage_row(case, total_support, int(total_support - from_unanchored)), exp_dir, exp_total, total_support)


_MATRIX = load("caller_matrix.json")


@pytest.mark.gpu
@pytest.mark.parametrize("sc", _MATRIX["scenarios"], ids=lambda s: s["name"])
def test_product_allele_caller_matrix(torch_cuda, sc):
    """VariantCallerTests.EvaluateVariants (:27-277) through the library: the mock state's counts (100 / 1 for every allele and direction
    at the high- / low-coverage coordinate), the test's candidates (SNV candidates are the caller's with MNV calling on), its thresholds —
    and the alleles that come back.  Candidates on chr1..chr4 are separate loci with one coordinate: one handle each.  A Reference
    candidate cannot be handed over (Reference alleles are the gVCF's: RegionState.GetAllCandidates): a scenario that lists one runs with
    reference calls on for its chromosome, which changes IsCallable only through the minimum coverage — the one scenario where that
    matters (a Reference allele kept because the variant fails the coverage test without gVCF) is not expressible and is skipped."""
    from pisces_amd import engine
    from tests import orc
    if sc["name"] == "reference_kept_when_the_variant_fails_coverage":
        pytest.skip("a Reference candidate without reference calls cannot be brought through the C ABI")
    ov = {k: v for k, v in sc["config"].items() if k in ("max_variant_qscore", "noise_level", "min_coverage", "min_variant_qscore", "min_frequency",
                                                          "low_gq_filter", "max_genotype_qscore")}
    if "min_frequency_num" in sc["config"]:
        ov["min_frequency"] = float(np.float32(sc["config"]["min_frequency_num"]) / np.float32(sc["config"]["min_frequency_den"]))
    if "min_variant_qscore_from" in sc["config"]:   # "one above the q-score of support 40 at coverage 1500": the q-score golden of QualityCalculatorTests pins the oracle's
        f = sc["config"]["min_variant_qscore_from"]
        ov["min_variant_qscore"] = orc.lib.orc_poisson_qscore(f["support"], f["coverage"], 20, 100) + f["plus"]
    by_chr = {}
    for name in sc["candidates"]:
        by_chr.setdefault(_MATRIX["candidates"][name]["chr"], []).append(_MATRIX["candidates"][name])
    got = []
    for chrom, cands in sorted(by_chr.items()):
        has_ref = any(x["category"] == "Reference" for x in cands)
        cfg = _abi.default_config(rmxn_max_repeat_length=-1, variant_qscore_filter=-1, low_depth_filter=-1, variant_freq_filter=-1.0,
                                  no_call_filter_threshold=-1.0, call_mnvs=1, collapse=0,
                                  **dict(ov, include_reference_calls=1 if has_ref else sc["config"]["include_reference_calls"]))
        cells = {}
        for p in sorted({x["pos"] for x in cands}):
            mult = _MATRIX["counts_per_allele_direction"][str(p)]
            cells.update({(p, a, d, 5): mult for a in range(6) for d in range(3)})
        # The mock state shows every base on every locus; the test's candidates are all the candidates there are.  Where the chromosome has
        # a variant candidate its locus is the candidate path's (a caller's candidate marks it); a chromosome with a Reference candidate
        # only runs MNV calling in its earlier form (PISCES_HIP_MNV_SPLIT=0: SNV candidates are never made from the counts).
        only_reference = all(x["category"] == "Reference" for x in cands)
        old = os.environ.get("PISCES_HIP_MNV_SPLIT")
        if only_reference:
            os.environ["PISCES_HIP_MNV_SPLIT"] = "0"
        try:
            with engine.HipVariantCaller(cfg) as c:
                c.SetReference(np.frombuffer(b"A" * 600, dtype=np.uint8))
                _stage(c, cells)
                c.AddCandidates([{"position": x["pos"], "category": CAT[x["category"]], "ref": x["ref"], "alt": x["alt"], "support_by_dir": tuple(x["support"])}
                                 for x in cands if x["category"] != "Reference"])
                recs, alleles = c.CallWithAlleles()
        finally:
            if only_reference:
                if old is None:
                    os.environ.pop("PISCES_HIP_MNV_SPLIT", None)
                else:
                    os.environ["PISCES_HIP_MNV_SPLIT"] = old
        for r, a in zip(recs, alleles):
            cat = _abi.info_category(r["info"])
            got.append((chrom, int(r["position"]), a[0], a[1], cat, None if cat == _abi.CAT_REFERENCE else int(r["allele_support"])))
    want = []
    for name in sc["called"]:
        x = _MATRIX["candidates"][name]
        want.append((x["chr"], x["pos"], x["ref"], x["alt"], CAT[x["category"]], None if x["category"] == "Reference" else sum(x["support"])))
    assert sorted(got, key=str) == sorted(want, key=str)


# ---- region state, caller and MNV paths: the tables tests/test_oracle_golden.py pins the oracle with, through the library -----------
_DONE = load("done_processing.json")


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["default", "every batch its own segment"])
@pytest.mark.parametrize("flush", ["copying flush", "CallBegin + CallEnd"])
def test_product_done_processing_reference_case(torch_cuda, flush, placement):
    """RegionStateManagerTests.DoneProcessing (:707-781) through the library: six 1-base reads in six blocks, an SNV candidate and a
    deletion whose 3500-base reference allele reaches from block 3001-4000 to 6501, one flush per upTo of the test and after each the
    GetAlleleCount values it asserts.  A flushed block's counts read 0 (the read store calls its floor "not a compaction": what it
    serves for a cleared block is checked here), block 3001-4000 keeps its count while the deletion reaches past upTo and block
    5001-6000 keeps its count behind it.  With copying flushes and with the CallBegin / CallEnd pair, in both placements of the store."""
    from pisces_amd import engine
    from tests.test_read_store import STORE_MODES, env
    g = _DONE
    ref = bytearray(b"A" * 8100)
    ref[0] = ord("T")
    cfg = _abi.default_config(block_size=g["block_size"], rmxn_max_repeat_length=-1)
    cands = []
    for x in g["candidates"]:
        ref_allele = x["ref_base"] * x["ref_length"] if "ref_length" in x else x["ref"]
        cands.append({"position": x["pos"], "category": CAT[x["category"]], "ref": ref_allele, "alt": x["alt"], "support_by_dir": tuple(x["support"])})
    with env(PISCES_HIP_READ_PATH=None, **STORE_MODES[placement]):
        with engine.HipVariantCaller(cfg) as c:
            count = lambda e: [e[0], e[1], e[2], c.GetAlleleCount(e[0], ALLELE[e[1]], DIR[e[2]])]
            c.SetReference(bytes(ref))
            c.AddAlleleCounts([{"pos": r["pos"], "seq": r["seq"], "cigar": [("M", len(r["seq"]))], "quals": [r["qual"]] * len(r["seq"])} for r in g["reads"]])
            assert [count(e) for e in g["expect_before"]] == g["expect_before"]
            c.AddCandidates(cands)
            for step in g["steps"]:
                if flush == "copying flush":
                    c.Call(step["up_to"])
                else:
                    c.CallBegin(step["up_to"])
                    c.CallEnd()
                assert [count(e) for e in step["expect"]] == step["expect"], step["up_to"]


@pytest.mark.gpu
def test_product_gapped_mnv_ref_add_and_get(torch_cuda):
    """RegionStateManagerTests.AddAndGetGappedMnvRefCount (:136-169) and RegionStateTests.AddAndGetGappedMnvReferenceCounts (:282-302)
    through pisces_hip_add_gapped_mnv_ref / pisces_hip_get_gapped_mnv_ref: counts add up per position, an add of 0 and positions not
    named change nothing.  The handle is the manager (blocks on demand), so the single RegionState's out-of-region add and get
    (:305-325) follow what include/pisces_hip.h promises instead: any position > 0 is accepted, a position never named reads 0, a
    position <= 0 is refused by both entries and a refused add adds nothing of its call."""
    from pisces_amd import engine
    g = load("gapped_mnv_ref.json")
    for steps in (g["manager"]["steps"], g["region"]["steps"]):
        with engine.HipVariantCaller(_abi.default_config()) as c:
            for step in steps:
                c.AddGappedMnvRefCount(dict(map(tuple, step["add"])))
                assert [[p, c.GetGappedMnvRefCount(p)] for p, _ in step["expect"]] == step["expect"]
    e = g["region_errors"]
    with engine.HipVariantCaller(_abi.default_config()) as c:
        c.AddGappedMnvRefCount(dict(map(tuple, e["add"])))
        everything = lambda: [c.GetGappedMnvRefCount(p) for p in range(e["start"], e["end"] + 1)]
        before = everything()
        nonzero = dict(map(tuple, e["expect_all_after"]["nonzero"]))
        assert before == [nonzero.get(p, 0) for p in range(e["start"], e["end"] + 1)]
        outside, n = e["add_outside"]
        assert c.GetGappedMnvRefCount(outside) == 0 and c.GetGappedMnvRefCount(2 ** 31 - 1) == 0   # never named: 0, however far out
        c.AddGappedMnvRefCount({outside: n})                  # the manager makes the block: accepted, and nothing else moves
        assert c.GetGappedMnvRefCount(outside) == n and everything() == before
        for bad in (0, -5):
            with pytest.raises(engine.PiscesHipError):
                c.GetGappedMnvRefCount(bad)
            with pytest.raises(engine.PiscesHipError):
                c.AddGappedMnvRefCount({e["start"]: 7, bad: 1})   # refused as a whole: the valid position before it is not added either
        assert c.GetGappedMnvRefCount(outside) == n and everything() == before


_REGION_CANDIDATES = load("region_candidates.json")


@pytest.mark.gpu
@pytest.mark.parametrize("v", _REGION_CANDIDATES["variants"], ids=lambda v: v["name"])
def test_product_region_candidates_reference_cases(torch_cuda, v):
    """RegionStateTests.ExecuteTest_GetCandidates (:339-437), all four of :258-279 (with / without Reference candidates = gVCF or not,
    with / without intervals), through the library.  The library reports rows, not candidates: the expected rows are the golden's
    candidate list after ShouldReport (AlleleCaller.cs:260-263: inside the intervals when there are any) and after the reference pruning
    of ComputeGenotypeAndFilterAllele (:146-147: a Reference allele leaves where a variant is called); every threshold is off, so each
    remaining candidate is one row.  Checked: position, category, support by direction; on Reference rows also AlleleSupport and
    TotalCoverage; and the whole row set against the oracle's for the same state.
    Visible on the oracle only (test_get_all_candidates_reference_cases): that the SNV at 15 stays a *candidate* outside the intervals,
    and the Reference candidates [0, 0, 5] at 5 and [5, 5, 0] at 15, which the SNVs called there prune from the rows.
    MNV calling on in its earlier form (PISCES_HIP_MNV_SPLIT=0): SNV candidates are the host's, none is made from the counts."""
    from pisces_amd import engine
    from tests import orc
    from tests.test_gpu_parity import assert_records_match
    from tests.test_read_store import env
    g = _REGION_CANDIDATES
    cfg = _permissive(call_mnvs=1, collapse=0, include_reference_calls=1 if v["with_reference"] else 0, emit_zero_coverage_refs=1 if v["with_intervals"] else 0)
    cells = {(r["pos"], ALLELE[r["allele"]], DIR[r["dir"]], g["anchor_index"]): r["n"] for r in g["counts"]}
    with env(PISCES_HIP_MNV_SPLIT=0):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(g["reference"])
            if v["with_intervals"]:
                c.SetIntervals([tuple(iv) for iv in g["intervals"]])
            _stage(c, cells)
            c.AddCandidates([{"position": x["pos"], "category": CAT[x["category"]], "ref": x["ref"], "alt": x["alt"], "support_by_dir": tuple(x["support"])}
                             for x in g["candidates"]])
            recs, alleles = c.CallWithAlleles()
    inside = lambda p: not v["with_intervals"] or any(a <= p <= b for a, b in g["intervals"])
    reported = [x for x in v["expect"] if inside(x["pos"])]
    variant_at = {x["pos"] for x in reported if x["category"] != "Reference"}
    want = [x for x in reported if x["category"] != "Reference" or x["pos"] not in variant_at]
    got = sorted((int(r["position"]), _abi.info_category(r["info"]), a[0], a[1], tuple(int(k) for k in r["support_by_dir"])) for r, a in zip(recs, alleles))
    assert got == sorted((x["pos"], CAT[x["category"]], x["ref"], x["alt"], tuple(x["support"])) for x in want)
    coverage = {}
    for r in g["counts"]:
        coverage[r["pos"]] = coverage.get(r["pos"], 0) + r["n"]
    for r in recs:
        if _abi.info_category(r["info"]) == _abi.CAT_REFERENCE:
            x = [x for x in want if x["pos"] == int(r["position"])][0]
            assert int(r["allele_support"]) == sum(x["support"]) and int(r["total_coverage"]) == coverage.get(x["pos"], 0), x
    # the same state through the oracle: every row, field by field
    st = orc.State(g["region"][0], g["region"][1] - g["region"][0] + 1)
    for x in g["candidates"]:
        st.add_candidate(orc.make_candidate(x["pos"], CAT[x["category"]], x["ref"], x["alt"], support=tuple(x["support"])))
    for (p, a, d, anchor), n in cells.items():
        st.set_count(p, a, d, anchor, n)
    if v["with_intervals"]:
        st.set_intervals([tuple(iv) for iv in g["intervals"]])
    exp = st.call_all(g["reference"], cfg)
    assert_records_match(recs, exp)


_CALLER_MNV = load("caller_mnv_cases.json")


def _caller_mnv_run(sc, candidates, split_env):
    """One handle for the scenario: the mock state's counts at the positions its candidates span (multiplier x 6 alleles x 3 directions),
    a reference that agrees with the SNV / MNV candidates' reference alleles (so the gaps of ATCTGTGA over TTTTTTTT are gaps), the
    candidates, one flush; returns (rows, alleles, candidates the state holds afterwards)."""
    from pisces_amd import engine
    from tests.test_oracle_golden import caller_mnv_config, caller_mnv_multiplier
    from tests.test_read_store import env
    lo, hi = sc["positions_touched"]
    ref = bytearray(b"A" * 2100)
    for want_point_alleles in (False, True):   # (a deletion's reference allele first: where the two disagree, the MNV's is the reference)
        for x in sc["candidates"]:
            if (x["category"] in ("Snv", "Mnv")) == want_point_alleles:
                ref[x["pos"] - 1:x["pos"] - 1 + len(x["ref"])] = x["ref"].encode()
    cells = {(p, a, d, 5): caller_mnv_multiplier(sc, p) for p in range(lo, hi + 1) for a in range(6) for d in range(3)}
    # MaxClearedPosition 2000 with candidates that reach 2002: the batch GetCandidatesToProcess makes for an upTo in block 2001-3000 that
    # is not below those candidates' ends (RegionStateManager.cs:295-320; at upTo = 2000 block 1001-2000 is held by its own MNVs, :306)
    up_to = None if sc["max_cleared_position"] is None or hi <= sc["max_cleared_position"] else hi
    with env(PISCES_HIP_MNV_SPLIT=split_env):
        with engine.HipVariantCaller(caller_mnv_config(sc, block_size=1000)) as c:
            c.SetReference(bytes(ref))
            if sc["intervals"]:
                c.SetIntervals([tuple(iv) for iv in sc["intervals"]])
            _stage(c, cells)
            c.AddCandidates([{"position": x["pos"], "category": CAT[x["category"]], "ref": x["ref"], "alt": x["alt"], "support_by_dir": tuple(x["support"])}
                             for x in candidates])
            recs, alleles = c.CallWithAlleles(up_to)
            held = c.GetCandidates()
    return recs, alleles, held


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["split", "PISCES_HIP_MNV_SPLIT=0"])
@pytest.mark.parametrize("sc", _CALLER_MNV["scenarios"], ids=lambda s: s["name"])
def test_product_allele_caller_mnv_reallocation_cases(torch_cuda, sc, form):
    """VariantCallerTests.CallVariants_MnvReallocation / _MnvTakingRefSupport / _MnvReallocatesToDifferentBlock /
    _MnvReallocatesToSnvOutsideInterval (:307-656) through the library's flush, in both forms of MNV calling: who gains the failed MNVs'
    support, the failed MNVs gone, no Reference row with the support the test rules out, ReferenceSupport 290 on the SNV under the
    gapped MNV and nothing taken anywhere else, the passing deletion as it is without the MNV, exactly the three candidates handed to
    block 2001-3000 (GetCandidates after the flush: category, position, alleles, support), exactly two called alleles at the interval edge.
    The tests' batches hold no Reference candidates; here a gVCF scenario also has the Reference rows of the staged positions."""
    from tests.test_oracle_golden import caller_mnv_multiplier
    split_env = None if form == "split" else 0
    recs, alleles, held = _caller_mnv_run(sc, sc["candidates"], split_env)
    rows = [(int(r["position"]), _abi.info_category(r["info"]), a[0], a[1], r) for r, a in zip(recs, alleles)]
    listing = [x[:4] + (int(x[4]["allele_support"]),) for x in rows]
    same = lambda x, e: x[:4] == (e["pos"], CAT[e["category"]], e["ref"], e["alt"])
    for e in sc["expect_called"]:
        hit = [x[4] for x in rows if same(x, e)]
        assert len(hit) == 1, (e, listing)
        for field in ("allele_support", "total_coverage", "reference_support"):
            if field in e:
                assert int(hit[0][field]) == e[field], (e, field, listing)
        if "frequency" in e:
            assert np.float32(hit[0]["allele_support"]) / np.float32(hit[0]["total_coverage"]) == np.float32(e["frequency"])
    for e in sc["expect_absent"]:
        assert not [x for x in rows if same(x, e)], (e, listing)
    for e in sc["expect_no_reference_row"]:
        for x in rows:
            if x[0] == e["pos"] and x[1] == _abi.CAT_REFERENCE:
                assert "allele_support" in e or "allele_support_above" in e, (e, listing)
                assert int(x[4]["allele_support"]) != e.get("allele_support") and not int(x[4]["allele_support"]) > e.get("allele_support_above", 1 << 30), (e, listing)
    if "expect_called_count" in sc:
        assert len([x for x in rows if x[1] != _abi.CAT_REFERENCE]) == sc["expect_called_count"], listing
    if "expect_gapped_mnv_ref" in sc:
        taken = dict(map(tuple, sc["expect_gapped_mnv_ref"]))
        # "the lookup holds 306 and nothing else": a Reference row of another position has all three directions of its base
        refs = [x for x in rows if x[1] == _abi.CAT_REFERENCE and x[0] not in taken]
        assert refs, listing
        for x in refs:
            assert int(x[4]["allele_support"]) == 3 * caller_mnv_multiplier(sc, x[0]), listing
        # the passing deletion: the row it has when the gapped MNV is not there at all
        alone = _caller_mnv_run(sc, [x for x in sc["candidates"] if x["category"] != "Mnv"], split_env)
        deletion = lambda rs, als: [r for r, a in zip(rs, als) if _abi.info_category(r["info"]) == _abi.CAT_DELETION]
        (with_mnv,), (without,) = deletion(recs, alleles), deletion(alone[0], alone[1])
        for field in ("allele_support", "total_coverage", "reference_support", "coverage_by_dir"):
            assert (with_mnv[field] == without[field]).all(), field
    got_held = sorted((x["position"], x["category"], x["ref"], x["alt"], tuple(x["support_by_dir"])) for x in held)
    assert got_held == sorted((x["pos"], CAT[x["category"]], x["ref"], x["alt"], tuple(x["support"])) for x in sc.get("expect_handed_to_next_block", []))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["split", "PISCES_HIP_MNV_SPLIT=0"])
def test_product_ref_support_taken_by_gapped_mnvs(torch_cuda, form):
    """VariantCallerTests.GetRefSupportFromGappedMnvs (:658-763) through a gVCF flush over the eight alleles as candidates (no threshold:
    all are callable), counts staged at the asserted positions only — the reference base, (40, 30, 30) by direction.  The Reference rows
    at 13, 124, 78901 and 78903 lose exactly 15, 36, 25 and 25.  At a position the test asserts absent nothing is lost: its Reference
    row has the staged 100 — it must be there where no candidate starts (14, 125, 457, 458, 78902, 78904); where an MNV, a deletion or
    an insertion is called the Reference allele is pruned (AlleleCaller.cs:146-147) and there is nothing to lose; at 93000 the SNV row's
    ReferenceSupport is the staged 100."""
    from pisces_amd import engine
    from tests.test_read_store import env
    g = load("gapped_mnv_ref_support.json")
    ref = bytearray(b"A" * g["reference_length"])
    for a in g["alleles"]:
        ref[a["pos"] - 1:a["pos"] - 1 + len(a["ref"])] = a["ref"].encode()
    staged = (40, 30, 30)
    taken = dict(map(tuple, g["expect"]))
    cells = {(p, ALLELE[chr(ref[p - 1])], d, 5): staged[d] for p in list(taken) + g["expect_absent"] for d in range(3)}
    cfg = _permissive(call_mnvs=1, collapse=0, include_reference_calls=1, max_mnv_length=8)
    with env(PISCES_HIP_MNV_SPLIT=None if form == "split" else 0):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(bytes(ref))
            _stage(c, cells)
            c.AddCandidates([{"position": a["pos"], "category": CAT[a["category"]], "ref": a["ref"], "alt": a["alt"], "support_by_dir": (a["allele_support"], 0, 0)}
                             for a in g["alleles"]])
            recs, alleles = c.CallWithAlleles()
    listing = [(int(r["position"]), _abi.info_category(r["info"]), a, int(r["allele_support"])) for r, a in zip(recs, alleles)]
    for a in g["alleles"]:   # every allele is called as it was handed in
        assert (a["pos"], CAT[a["category"]], (a["ref"], a["alt"]), a["allele_support"]) in listing, (a, listing)
    reference_rows = {}
    for r in recs:
        if _abi.info_category(r["info"]) == _abi.CAT_REFERENCE:
            assert int(r["position"]) not in reference_rows
            reference_rows[int(r["position"])] = int(r["allele_support"])
    starts = {a["pos"] for a in g["alleles"]}
    assert {p: reference_rows.get(p) for p in taken} == {p: sum(staged) - n for p, n in taken.items()}, listing
    for p in g["expect_absent"]:
        if p not in starts:
            assert reference_rows.get(p) == sum(staged), (p, listing)
        else:
            assert reference_rows.get(p, sum(staged)) == sum(staged), (p, listing)
    (snv,) = [r for r in recs if _abi.info_category(r["info"]) == _abi.CAT_SNV]
    assert int(snv["position"]) == 93000 and int(snv["reference_support"]) == sum(staged)
