"""Pins oracle/ (the CPU restatement of the reference path) against the reference's own
known-answer tables (tests/golden/*.json, transcribed from the xUnit tests cited there)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc

G = os.path.join(os.path.dirname(__file__), "golden")
INT_MAX = 2**31 - 1


def load(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)


GT = {"HeterozygousAlt1Alt2": 0, "Alt12LikeNoCall": 1, "HeterozygousAltRef": 2, "HomozygousAlt": 3, "HomozygousRef": 4,
      "RefLikeNoCall": 5, "AltLikeNoCall": 6, "RefAndNoCall": 7, "AltAndNoCall": 8}
ALLELE = {"A": 0, "G": 1, "C": 2, "T": 3, "N": 4, "D": 5}
DIR = {"F": 0, "R": 1, "S": 2}


# ---------------------------------------------------------------- q-score (MathNet boundary)
def test_variant_qscore_table():
    g = load("qscore.json")
    nl = g["noise_level"]
    for row in g["compute"]:
        assert orc.lib.orc_poisson_qscore(row["support"], row["coverage"], nl, INT_MAX) == row["q"], row
        assert orc.lib.orc_poisson_qscore(row["support"], row["coverage"], nl, 100) == min(100, row["q"]), row


def test_assign_pvalue_table():
    g = load("qscore.json")
    for row in g["assign_pvalue"]:
        p = orc.lib.orc_assign_pvalue(row["support"], row["coverage"], 20)
        assert round(abs(p - row["p"]), row["decimals"]) == 0, (row, p)  # xUnit Assert.Equal(a, b, precision)
        assert orc.lib.orc_poisson_qscore(row["support"], row["coverage"], 20, 100) == row["final_q_cap100"]


def test_qscore_cap_and_bad_input():
    g = load("qscore.json")
    c = g["cap"]
    assert orc.lib.orc_poisson_qscore(c["support"], c["coverage"], 20, 1000) == c["uncapped"]
    assert orc.lib.orc_poisson_qscore(c["support"], c["coverage"], 20, c["max_q_below"]) == c["max_q_below"]
    for k, cov, nl in g["bad_input"]:
        assert orc.lib.orc_poisson_qscore(k, cov, nl, 100) == 0


def test_excel_truth_depth500_and_raw_q():
    g = load("qscore.json")
    for row in g["excel_depth500"]:
        p = orc.lib.orc_assign_pvalue(row["support"], 500, 20)
        assert abs(p - row["p"]) < 5e-5
        assert abs(orc.lib.orc_p_to_q(p) - row["q"]) < 5e-5
    r = g["raw_q_depth10000"]
    raw = orc.lib.orc_raw_poisson_qscore(r["support"], r["coverage"], 20)
    assert abs(raw - r["raw_q"]) < 5e-5
    assert (r["chernoff_q"] - raw) / r["chernoff_q"] <= 0.03


def test_mathnet_restatement_against_scipy():
    """Cross-check of the restated MathNet functions (only possible where scipy exists)."""
    sp = pytest.importorskip("scipy.special")
    for a, x in [(1, 0.5), (5, 1.0), (25, 5.0), (10, 2.0), (3, 7.5), (250, 50.0), (40, 60.0), (700, 650.0)]:
        got = orc.lib.orc_mathnet_gamma_lower_regularized(a, x)
        assert got == pytest.approx(float(sp.gammainc(a, x)), rel=1e-12, abs=1e-300)
    for z in [0.7, 1.0, 2.5, 10.0, 171.0, 495.0, 9995.0]:
        assert orc.lib.orc_mathnet_gamma_ln(z) == pytest.approx(float(sp.gammaln(z)), rel=1e-13, abs=1e-13)
    for k, lam in [(0, 1.0), (4, 5.0), (24, 5.0), (249, 50.0)]:
        assert orc.lib.orc_poisson_cdf(k, lam) == pytest.approx(float(sp.pdtr(k, lam)), rel=1e-10)


def test_mathnet_restatement_on_dense_grids_against_scipy():
    """The MathNet.Numerics 4.5.1 functions of the hot path (VariantQualityCalculator.cs:36-47: Poisson.CumulativeDistribution and
    ProbabilityLn; StrandBiasCalculator.cs:164 / the diploid q-scores: BetaRegularized) are restated from their published algorithms
    (the package is not under /root/reference) and the reference's own tests pin them at some twenty values; this holds the
    restatement to an INDEPENDENT implementation (scipy's cephes / boost routines) on dense grids of the arguments the path produces —
    supports up to 600, coverages up to 20 000, noise levels 20-40 — and the variant q-score itself, end to end, to the reference's formula
    evaluated through scipy's survival function: the north star's own tolerance (+-1 Phred) may be used at rounding edges, nowhere else."""
    sp = pytest.importorskip("scipy.special")
    st = pytest.importorskip("scipy.stats")
    L = orc.lib
    # regularized lower incomplete gamma P(a, x)
    worst = 0.0
    for a in (1, 2, 3, 5, 8, 13, 25, 50, 99, 100, 101, 250, 500, 699, 700, 701, 1000, 2500, 5000, 10000):
        for f in (0.01, 0.1, 0.5, 0.8, 0.95, 1.0, 1.05, 1.25, 2.0, 4.0):
            x = a * f
            want = float(sp.gammainc(a, x))
            got = L.orc_mathnet_gamma_lower_regularized(float(a), float(x))
            if want > 1e-290:
                worst = max(worst, abs(got - want) / want)
            else:
                assert got < 1e-280
    assert worst < 2e-10, worst
    # ln Gamma
    for z in np.concatenate([np.logspace(-1, 5, 240), np.arange(1, 700, 7.0)]):
        assert L.orc_mathnet_gamma_ln(float(z)) == pytest.approx(float(sp.gammaln(z)), rel=2e-13, abs=2e-13), z
    # Poisson: MathNet's CDF and ln PMF, and the repository's own Poisson.Cdf (stats/Poisson.cs:26-128)
    for lam in (0.05, 0.5, 1.0, 2.5, 5.0, 10.0, 20.0, 50.0, 100.0, 200.0, 500.0):
        ks = np.unique(np.concatenate([np.arange(0, 40), np.linspace(0, 3 * lam + 60, 60).astype(int)]))
        for k in ks:
            want = float(st.poisson.cdf(int(k), lam))
            if want > 1e-280:
                assert L.orc_mathnet_poisson_cdf(lam, float(k)) == pytest.approx(want, rel=5e-10), (lam, k)
                own = L.orc_poisson_cdf(float(k), lam)
                assert own == -1.0 or own == pytest.approx(want, rel=5e-9), (lam, k, own, want)   # (-1: the reference's "did not converge")
            assert L.orc_mathnet_poisson_ln_pmf(lam, int(k)) == pytest.approx(float(st.poisson.logpmf(int(k), lam)), rel=1e-11, abs=1e-11), (lam, k)
    # regularized incomplete beta (Binomial.CumulativeDistribution of the Diploid strand-bias model and the diploid q-scores)
    if hasattr(L, "orc_mathnet_beta_regularized"):
        L.orc_mathnet_beta_regularized.restype = C.c_double
        L.orc_mathnet_beta_regularized.argtypes = [C.c_double, C.c_double, C.c_double]
        for a in (0.5, 1, 2, 5, 20, 100, 500, 2000):
            for b in (0.5, 1, 3, 10, 50, 400, 3000):
                for x in (0.001, 0.02, 0.2, 0.5, 0.8, 0.98, 0.999):
                    want = float(sp.betainc(a, b, x))
                    if 1e-280 < want:
                        assert L.orc_mathnet_beta_regularized(float(a), float(b), float(x)) == pytest.approx(want, rel=2e-9), (a, b, x)
    # the variant q-score end to end: Q = round(min(maxQ, -10 log10(1 - CDF(k - 1; cov * 10^(-NL / 10))))) (VariantQualityCalculator.cs:27-65)
    rng = np.random.default_rng(20260930)
    n, off, edge = 0, 0, 0
    for nl in (20, 30, 40):
        cov = np.unique(np.concatenate([np.arange(1, 60), rng.integers(60, 20_001, 700)]))
        for c in cov:
            lam = float(c) * 10.0 ** (-nl / 10.0)
            ks = np.unique(np.concatenate([np.arange(1, min(int(c), 12) + 1), rng.integers(1, min(int(c), 600) + 1, 12)]))
            logsf = st.poisson.logsf(ks - 1, lam)
            for k, ls in zip(ks, logsf):
                raw = -10.0 * float(ls) / np.log(10.0)
                # (the reference forms 1 - CDF in double precision: below p ~ 1e-12 its q-score is the cancellation's — 149 where the exact
                # tail gives 166 at support 10 of coverage 10 — which the restatement follows operation by operation and which only MathNet's
                # own bits, pinned by the reference's tables above, can check; the default cap of the q-score is 100)
                if not np.isfinite(raw) or raw > 120.0:
                    continue
                got = L.orc_poisson_qscore(int(k), int(c), nl, 1 << 30)
                want = int(np.rint(max(raw, 0.0)))
                n += 1
                if got != want:
                    off += 1
                    assert abs(got - want) <= 1 and abs(raw - np.floor(raw) - 0.5) < 1e-6, (k, c, nl, got, raw)   # a rounding edge, nothing else
    assert n > 8_000 and off <= n // 2000, (n, off)


# ---------------------------------------------------------------- strand bias
def test_strand_bias_somatic_rows():
    g = load("strand_bias.json")
    for row in g["somatic_extended"]:
        r = orc.strand_bias(row["cov"], row["sup"], row["q_noise"], row["min_vf"], row["thr"], _abi.SB_EXTENDED)
        if row["gatk"] == "-inf":
            assert r.bias_score == 0 and r.gatk_bias_score == -math.inf
        else:
            assert round(abs(r.bias_score - row["bias"]), row["decimals"]) == 0
            assert round(abs(r.gatk_bias_score - row["gatk"]), row["decimals"]) == 0
        assert bool(r.bias_acceptable) == row["acceptable"]
    f = g["forced_poisson"]
    r = orc.strand_bias(f["cov"], f["sup"], f["q_noise"], f["min_vf"], f["thr"], _abi.SB_POISSON)
    assert r.bias_score == 1.0 and r.gatk_bias_score == 0


def _execute_sb(f, r, s, q=20, thr=0.5, model=_abi.SB_POISSON):
    # the reference's ExecuteTest harness (StrandBiasCalculatorTests.cs:363-393)
    sup = [int(f[0] * f[1]), int(r[0] * r[1]), int(s[0] * s[1])]
    return orc.strand_bias([f[1], r[1], s[1]], sup, q, 0.01, thr, model)


def test_strand_bias_both_strand_flags():
    g = load("strand_bias.json")
    for row in g["both_strands_poisson"]:
        # the reference builds the frequencies as float32 (0.1f, ...)
        f = (float(np.float32(row["f"][0])), row["f"][1])
        r = (float(np.float32(row["r"][0])), row["r"][1])
        s = (float(np.float32(row["s"][0])), row["s"][1])
        res = _execute_sb(f, r, s)
        assert bool(res.var_present_on_both) == row["var"], row
        assert bool(res.cov_present_on_both) == row["cov"], row


def test_strand_bias_threshold_sweeps():
    g = load("strand_bias.json")
    h = g["happy_path_poisson"]
    for rev_depth in range(h["rev_depth_range"][0], h["rev_depth_range"][1]):
        res = _execute_sb((h["fwd_freq"], h["fwd_depth"]), (h["rev_freq"], rev_depth),
                          (h["stitched_freq"], h["stitched_depth"]))
        if rev_depth == 0:
            assert res.bias_acceptable
        else:
            assert not res.bias_acceptable
            thr = float(np.float32(res.bias_score + 0.00001))
            assert _execute_sb((h["fwd_freq"], h["fwd_depth"]), (h["rev_freq"], rev_depth),
                               (h["stitched_freq"], h["stitched_depth"]), 20, thr).bias_acceptable
    v = g["varying_coverage_poisson"]
    ff = 0.01
    while ff < 0.10:
        for fc in range(v["fwd_cov"][0], v["fwd_cov"][1] + 1, v["fwd_cov"][2]):
            assert _execute_sb((ff, fc), tuple(v["rev"]), tuple(v["stitched"])).bias_acceptable
        ff += 0.01


# ---------------------------------------------------------------- somatic genotype / GQ
def test_somatic_genotype_scenarios():
    g = load("somatic_genotype.json")
    pv = g["passing_variant"]
    for row in g["genotype_cases"]:
        cov = row["total_coverage"]
        if row["is_reference"]:
            cat, sup, refsup = _abi.CAT_REFERENCE, pv["reference"]["allele_support"], 0
        else:
            refsup = int(np.float32(row["ref_frequency"]) * np.float32(cov))  # (int)(refFrequency * totalCoverage)
            cat, sup = _abi.CAT_SNV, cov - refsup
        gt = orc.lib.orc_somatic_genotype(cat, cov, sup, refsup, g["genotype_min_freq_filter"], g["genotype_min_depth"])
        assert gt == GT[row["genotype"]], row


def test_somatic_gq_table():
    g = load("somatic_genotype.json")["gq"]
    depth = g["depth"]
    for case in g["cases"]:
        for freq, exp in zip(case["freqs"], case["expected"]):
            gt = GT[case["genotype"]]
            support = int(depth * freq)
            if case["genotype"] in ("HomozygousRef", "RefAndNoCall"):
                support = int(depth * (1.0 - freq))
            got = orc.lib.orc_somatic_gq(gt, g["variant_q"], depth, support, case["lod"], g["min_gq"], g["max_gq"])
            assert got == exp, (case["genotype"], case["lod"], freq, got, exp)


# ---------------------------------------------------------------- region state
def _mk(rd, default_q):
    dirs = None
    if "dirs" in rd:
        dirs = [DIR[rd["dirs"]]] * len(rd["seq"])
    posmap = None
    if "posmap_unmapped_index" in rd:
        posmap = [rd["pos"] + i for i in range(len(rd["seq"]))]
        posmap[rd["posmap_unmapped_index"]] = -1
    return orc.make_read(rd["pos"], rd["seq"], cigar=rd.get("cigar"), quals=rd.get("quals"),
                         qual_all=rd.get("qual", default_q), dirs=dirs, posmap=posmap)


def test_add_and_get_allele_counts():
    g = load("region_state.json")["add_and_get"]
    st = orc.State(900, 300, min_bq=g["min_quality"])
    for rd in g["reads"]:
        assert st.add_allele_counts(_mk(rd, g["min_quality"])) == 0
    for pos, a, d, n in g["expect"]:
        assert st.get_allele_count(pos, ALLELE[a], DIR[d]) == n, (pos, a, d)
    assert st.add_allele_counts(_mk(g["then_read"], g["min_quality"])) == 0
    for pos, a, d, n in g["expect_after"]:
        assert st.get_allele_count(pos, ALLELE[a], DIR[d]) == n, (pos, a, d)


def test_poor_quality_and_terminal_deletions():
    g = load("region_state.json")["poor_qual_deletions"]
    for sc in g["scenarios"]:
        st = orc.State(900, 300, min_bq=g["min_quality"])
        for rd in sc["reads"]:
            assert st.add_allele_counts(_mk(rd, 30)) == 0
        for e in sc["expect_ranges"]:
            for pos in range(e["from"], e["to"] + 1):
                assert st.get_allele_count(pos, ALLELE[e["allele"]], DIR[e["dir"]]) == e["count"], (sc["name"], pos, e)


def test_anchor_adjusted_counts():
    g = load("region_state.json")["anchor_adjusted"]
    st = orc.State(1, 10)
    for anchor, v in g["matrix"].items():
        st.set_count(2, _abi.ALLELE_A, _abi.DIR_FORWARD, int(anchor), v)
    for c in g["cases"]:
        got = st.get_allele_count(2, _abi.ALLELE_A, _abi.DIR_FORWARD, c["min"], -1 if c["max"] is None else c["max"],
                                  c["from_end"], c["symmetric"])
        assert got == c["expect"], c


def test_anchor_bins_of_a_read():
    """GetAnchorType (RegionStateManager.cs:83-116): left side 0..4, well anchored 5, right side 6..10,
    ties go right."""
    st = orc.State(100, 40)
    st.add_allele_counts(orc.make_read(100, "A" * 12))
    c = st.counts()
    bins = [int(np.argmax(c[i, _abi.ALLELE_A, 0])) for i in range(12)]
    assert bins == [0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10]
    st = orc.State(100, 40)
    st.add_allele_counts(orc.make_read(100, "A" * 5))
    c = st.counts()
    assert [int(np.argmax(c[i, _abi.ALLELE_A, 0])) for i in range(5)] == [0, 1, 8, 9, 10]


# ---------------------------------------------------------------- coverage + filters
def test_coverage_point_happy_path():
    g = load("coverage.json")["point"]
    st = orc.State(1, 10)
    for row in g["counts"]:
        for d, v in enumerate(row["by_dir"]):
            st.set_count(g["variant"]["pos"], ALLELE[row["allele"]], d, 5, v)
    v = g["variant"]
    cand = orc.make_candidate(v["pos"], _abi.CAT_SNV, v["ref"], v["alt"], support=(v["support"], 0, 0))
    called = orc.OrcCalled()
    orc.lib.orc_called_from_candidate(C.byref(called), C.byref(cand))
    orc.lib.orc_coverage_compute(C.byref(called), st.h, 1, 0)
    assert list(called.coverage_by_dir) == g["expect_cov_by_dir"]
    assert called.total_coverage == g["expect_total"]
    assert called.reference_support == g["expect_ref_support"]


def test_fraction_no_calls():
    g = load("filters.json")
    cfg = _abi.default_config()
    rows = g["fraction_no_calls"] + [dict(total_coverage=g["happy_path"]["total_coverage"],
                                          num_no_calls=g["happy_path"]["num_no_calls"],
                                          expect=g["happy_path"]["expect_fraction"])]
    for row in rows:
        st = orc.State(1, 4)
        st.set_count(1, _abi.ALLELE_T, 0, 5, row["total_coverage"])  # coverage lands on T, no-calls on N
        st.set_count(1, _abi.ALLELE_N, 0, 5, row["num_no_calls"])
        cand = orc.make_candidate(1, _abi.CAT_SNV, "A", "T", support=(min(10, row["total_coverage"]), 0, 0))
        called = orc.OrcCalled()
        orc.lib.orc_called_from_candidate(C.byref(called), C.byref(cand))
        orc.lib.orc_process_variant(C.byref(called), st.h, C.byref(cfg))
        assert called.fraction_no_calls == np.float32(row["expect"])


# ---------------------------------------------------------------- candidate finder
def test_finder_snv_basics_and_open_ends():
    ref = "ACGTACGTACGTACGTACGT"
    rd = orc.make_read(3, "GTACGAAC")  # ref[2:10] = GTACGTAC -> T>A at pos 8, fully anchored
    c = orc.find_candidates(rd, ref)
    assert [(x.position, x.ref, x.alt, x.category) for x in c] == [(8, b"T", b"A", _abi.CAT_SNV)]
    assert (c[0].open_left, c[0].open_right) == (0, 0)
    assert list(c[0].support_by_dir) == [1, 0, 0] and list(c[0].well_anchored_by_dir) == [1, 0, 0]
    # mismatch on the first / last aligned base is open ended (Annotate, CandidateVariantFinder.cs:514-541)
    rd = orc.make_read(3, "TTACGTAG")
    c = orc.find_candidates(rd, ref)
    assert [(x.position, x.open_left, x.open_right) for x in c] == [(3, 1, 0), (10, 0, 1)]
    assert list(c[0].well_anchored_by_dir) == [0, 0, 0]
    # a mismatch before a low-quality base is open on the right (:110-118); a low-quality mismatch is no candidate
    rd = orc.make_read(3, "GTACGAAC", quals=[30, 30, 30, 30, 30, 30, 10, 30])
    c = orc.find_candidates(rd, ref)
    assert [(x.position, x.open_left, x.open_right) for x in c] == [(8, 0, 1)]
    rd = orc.make_read(3, "GTACGAAC", quals=[30, 30, 30, 30, 30, 10, 30, 30])
    assert orc.find_candidates(rd, ref) == []


def test_finder_indels():
    ref = "ACGTACGTACGTACGTACGT"
    rd = orc.make_read(3, "GTACCCGTAC", cigar="4M2I4M")
    c = orc.find_candidates(rd, ref)
    assert [(x.position, x.ref, x.alt, x.category) for x in c] == [(6, b"C", b"CCC", _abi.CAT_INSERTION)]
    rd = orc.make_read(3, "GTACAC", cigar="4M2D2M")  # deletes GT at 7,8
    c = orc.find_candidates(rd, ref)
    assert [(x.position, x.ref, x.alt, x.category) for x in c] == [(6, b"CGT", b"C", _abi.CAT_DELETION)]


def test_mnv_build_up():
    ref = "ACGTACGTACGTACGTACGT"
    rd = orc.make_read(3, "GTTGGTAC")  # AC->TG at 5,6
    c = orc.find_candidates(rd, ref, call_mnvs=True, max_mnv=3, max_gap=1)
    assert [(x.position, x.ref, x.alt, x.category) for x in c] == [(5, b"AC", b"TG", _abi.CAT_MNV)]
    c = orc.find_candidates(rd, ref, call_mnvs=False)
    assert [(x.position, x.ref, x.alt) for x in c] == [(5, b"A", b"T"), (6, b"C", b"G")]


# ---------------------------------------------------------------- caller flow
def test_call_all_simple_snv_gvcf():
    """Depth-100 pileup with a 20 % SNV: reference rows everywhere, the SNV replaces the reference row at its
    locus (AlleleCaller.cs:146-147), genotypes 0/0 and 0/1."""
    ref = "ACGTACGTACGTACGTACGTACGTACGTAC"
    st = orc.State(1, 30)
    cfg = _abi.default_config()
    for i in range(100):
        seq = list(ref[4:24])
        if i < 20:
            seq[8] = "G" if ref[12] != "G" else "T"  # position 13
        rd = orc.make_read(5, "".join(seq), reverse=(i % 2 == 1))
        for c in orc.find_candidates(rd, ref):
            st.add_candidate(c)
        st.add_allele_counts(rd)
    out = st.call_all(ref, cfg)
    assert len(out) == 20
    assert list(out["position"]) == list(range(5, 25))
    row = out[out["position"] == 13][0]
    assert _abi.info_category(row["info"]) == _abi.CAT_SNV
    assert row["allele_support"] == 20 and row["total_coverage"] == 100 and row["reference_support"] == 80
    assert row["variant_qscore"] == 100 and _abi.info_genotype(row["info"]) == _abi.GT_HET_ALT_REF
    assert row["filter_bits"] == 0
    others = out[out["position"] != 13]
    assert (others["total_coverage"] == 100).all() and (others["allele_support"] == 100).all()
    assert all(_abi.info_genotype(i) == _abi.GT_HOM_REF for i in others["info"])
    # GQ of a 0/0 call: PtoQ(QtoP(100) + Poisson.Cdf(0, 0.01*100)) = -10 log10(e^-1) = 4.34 -> 4
    assert (others["genotype_qscore"] == 4).all()


# ---------------------------------------------------------------- spanning coverage (insertions / deletions / MNVs)
_CAT = {"Snv": _abi.CAT_SNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION, "Mnv": _abi.CAT_MNV,
        "Reference": _abi.CAT_REFERENCE}


def _stage_counts(case, taken_ref=0):
    st = orc.State(1, 16)
    for row in case["counts"]:
        a = ALLELE[row["allele"]]
        if "dirs" in row:
            for d, v in enumerate(row["dirs"]):
                st.set_count(row["coord"], a, d, 5, v)
        else:
            for d, per in enumerate(row["anchors"]):
                for anchor, v in per.items():
                    st.set_count(row["coord"], a, d, int(anchor), v)
    if taken_ref:
        orc.lib.orc_add_gapped_mnv_ref(st.h, case["allele"]["pos"], taken_ref)
    return st


def _compute(case, support, well_anchored, consider_anchor):
    st = _stage_counts(case, case.get("taken_ref", 0))
    v = case["allele"]
    cand = orc.make_candidate(v["pos"], _CAT[v["category"]], v["ref"], v["alt"], support=(0, 0, support),
                              well_anchored=(0, 0, well_anchored))
    called = orc.OrcCalled()
    orc.lib.orc_called_from_candidate(C.byref(called), C.byref(cand))
    orc.lib.orc_coverage_compute(C.byref(called), st.h, 1 if consider_anchor else 0, 0)
    return called


@pytest.mark.parametrize("case", load("coverage_spanning.json")["cases"], ids=lambda c: c["name"])
def test_coverage_calculator_reference_cases(case):
    """CoverageCalculatorTests.ComputeCoverage_* through the reference's own harness (ComputeCoverageTest): anchors ignored,
    then for insertions anchor-aware with fully anchored, fully unanchored and half-and-half support."""
    exp_dir, exp_total = case["by_dir"], case["total"]
    check_aux = case.get("check_aux", True)
    cat = case["allele"]["category"]

    def check(called, by_dir, total, weight):
        assert called.total_coverage == total
        assert list(called.coverage_by_dir)[: len(by_dir)] == by_dir
        if check_aux:
            if cat == "Reference":
                assert called.allele_support == case.get("snv_ref", 0)
            elif cat == "Snv":
                assert called.reference_support == case.get("snv_ref", 0)
            else:
                assert called.reference_support == total - called.allele_support
        assert called.unanchored_weight == weight

    c = _compute(case, 5, 5, False)
    check(c, exp_dir, exp_total, 0.0)
    if "expect_ref_support" in case:
        assert c.reference_support == case["expect_ref_support"]
    if cat != "Insertion":
        return
    suspicious = case.get("suspicious", 0)
    aware = case.get("by_dir_anchor_aware")
    check(_compute(case, 5, 5, True), aware if aware is not None else exp_dir,
          sum(aware) if aware is not None else exp_total - suspicious, 0.0)
    check(_compute(case, 5, 0, True), exp_dir, exp_total, 1.0)
    from_unanchored = np.float32(suspicious) * np.float32(0.5)
    total_support = int(from_unanchored + np.float32(0.5) * np.float32(exp_total - suspicious))
    check(_compute(case, total_support, int(total_support - from_unanchored), True), exp_dir, exp_total, 1.0 if suspicious > 0 else 0.0)


def test_synthetic_fixture_is_what_the_oracle_produces():
    """tests/golden/synthetic_small.npz (made by tests/golden/make_synthetic_golden.py) is reproducible."""
    z = np.load(os.path.join(G, "synthetic_small.npz"))
    cfg = _abi.default_config()
    exp, nloci = orc.run_observations(z["positions"], z["tuples"], z["ref"], int(z["region_start"]), int(z["n_loci"]), cfg)
    assert exp.tobytes() == z["expected"].tobytes() and nloci == int(z["n_candidate_loci"])


# ---------------------------------------------------------------- AlleleCaller matrix (IsCallable, reference pruning)
@pytest.mark.parametrize("sc", load("caller_matrix.json")["scenarios"], ids=lambda s: s["name"])
def test_allele_caller_matrix(sc):
    g = load("caller_matrix.json")
    ov = {k: v for k, v in sc["config"].items() if k in ("max_variant_qscore", "noise_level", "min_coverage", "include_reference_calls",
                                                          "min_variant_qscore", "min_frequency", "low_gq_filter", "max_genotype_qscore")}
    if "min_frequency_num" in sc["config"]:
        ov["min_frequency"] = float(np.float32(sc["config"]["min_frequency_num"]) / np.float32(sc["config"]["min_frequency_den"]))
    if "min_variant_qscore_from" in sc["config"]:
        f = sc["config"]["min_variant_qscore_from"]
        ov["min_variant_qscore"] = orc.lib.orc_poisson_qscore(f["support"], f["coverage"], 20, 100) + f["plus"]
    cfg = _abi.default_config(rmxn_max_repeat_length=-1, variant_qscore_filter=-1, low_depth_filter=-1, variant_freq_filter=-1.0,
                              no_call_filter_threshold=-1.0, **ov)
    st = orc.State(1, 600)
    for pos_s, mult in g["counts_per_allele_direction"].items():
        for a in range(6):
            for d in range(3):
                st.set_count(int(pos_s), a, d, 5, mult)
    names = sc["candidates"]
    cands = [orc.make_candidate(g["candidates"][n]["pos"], _CAT[g["candidates"][n]["category"]], g["candidates"][n]["ref"],
                                g["candidates"][n]["alt"], support=tuple(g["candidates"][n]["support"])) for n in names]
    recs, full, _ = orc.call_candidates(st, cands, cfg)
    # MatchVariants (VariantCallerTests.cs:776-789): position, alleles, type (the chromosome label is not part of the state)
    def key(c):
        return (c["pos"], c["ref"], c["alt"], _CAT[c["category"]], sum(c["support"]))
    got = sorted((f.position, f.ref.decode(), f.alt.decode(), f.category, f.allele_support) for f in full)
    assert got == sorted(key(g["candidates"][n]) for n in sc["called"])


# ---------------------------------------------------------------- candidate finder: the reference's deletion / insertion cases
_FINDER = load("finder_cases.json")
_TYPE = {"Snv": _abi.CAT_SNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION, "Mnv": _abi.CAT_MNV}


def _finder_case_inputs(case, start=101):
    ops = orc.parse_cigar(case["cigar"])
    clip = ops[0][1] if ops and ops[0][0] == "S" else 0
    ref = "N" * (start - 1 - clip) + case["ref_under_read"] + "NNNNN"      # CandidateVariantsTest ctor, VariantFinderTests.cs:28-41
    return start, ops, ref


@pytest.mark.parametrize("case", _FINDER["cases"], ids=lambda c: "%s-%s-%s-%d-%d" % (c["test"][:3], c["cigar"], "".join(map(str, c["quals"][:8])), c["max_mnv_length"], c["max_gap"]))
def test_finder_reference_cases_oracle(case):
    start, ops, ref = _finder_case_inputs(case)
    if not case["read"]:
        pytest.skip("read without bases (5D): Read construction itself is outside the finder")
    rd = orc.make_read(start, case["read"], cigar=ops, quals=case["quals"])
    got = sorted(orc.find_candidates(rd, ref, min_bq=_FINDER["min_base_call_quality"], max_mnv=case["max_mnv_length"],
                                     max_gap=case["max_gap"], call_mnvs=_FINDER["call_mnvs"]), key=lambda c: c.position)
    assert len(got) == case["expected_count"]
    if not got:
        return
    assert len(got) == len(case["expected"])
    for c, e in zip(got, case["expected"]):
        assert (c.position - start, c.ref.decode(), c.alt.decode(), c.category) == (e["coord"], e["ref"], e["alt"], _TYPE[e["type"]])
        if e["open_left"] is not None:
            assert bool(c.open_left) == e["open_left"]
        if e["open_right"] is not None:
            assert bool(c.open_right) == e["open_right"]


# ---------------------------------------------------------------- VariantCollapser
@pytest.mark.parametrize("case", load("collapser_cases.json")["cases"], ids=lambda c: c["name"])
def test_variant_collapser_reference_cases(case):
    st = orc.State(1, 64)
    for pos in range(1, 40):                       # the mock allele source: every count is 1
        for a in range(6):
            for d in range(3):
                for anchor in range(11):
                    st.set_count(pos, a, d, anchor, 0)
                st.set_count(pos, a, d, 5, 1)
    def run(order):
        cands = [orc.make_candidate(c["pos"], _CAT[c["category"]], c["ref"], c["alt"], support=(1, 0, 0), open_left=c["open_left"],
                                    open_right=c["open_right"]) for c in order]
        out, n_collapsed, _ = orc.collapse(st, cands)
        assert len(out) == case["expected_count"]
        assert n_collapsed == len(order) - case["expected_count"]
        if case["expected_support_first"] is not None:
            assert sum(out[0].support_by_dir) == case["expected_support_first"]
    run(case["candidates"])
    run(list(reversed(case["candidates"])))


def test_variant_collapser_known_variants():
    """VariantCollapser.cs:178-190 (AnnotateKnown) and :216-218 (Compare returns the known one first — VariantCollapserTests.cs:765-766: a
    known candidate sorts before a fully anchored, longer, more frequent one).  On the mock allele source of the cases above."""
    st = orc.State(1, 64)
    for pos in range(1, 40):
        for a in range(6):
            for d in range(3):
                for anchor in range(11):
                    st.set_count(pos, a, d, anchor, 0)
                st.set_count(pos, a, d, 5, 1)
    ins = _CAT["Insertion"] if "Insertion" in _CAT else 1
    def cands():
        return [orc.make_candidate(10, ins, "A", "AACGTTGCA", support=(3, 0, 0)),                      # long, anchored
                orc.make_candidate(10, ins, "A", "AACGTA", support=(2, 0, 0)),                         # short, anchored
                orc.make_candidate(10, ins, "A", "AACG", support=(1, 0, 0), open_right=True)]          # ends inside the insertion: matches both
    out, n, _ = orc.collapse(st, cands())
    assert n == 1 and [(c.alt.decode(), sum(c.support_by_dir)) for c in out] == [("AACGTTGCA", 4), ("AACGTA", 2)]   # the longer one takes it
    keep = orc.set_known_variants([(10, ins, "A", "AACGTA")])
    try:
        out, n, _ = orc.collapse(st, cands())
        assert n == 1 and [(c.alt.decode(), sum(c.support_by_dir)) for c in out] == [("AACGTTGCA", 3), ("AACGTA", 3)]   # the known one does
        # a candidate that IS a known variant is anchored on both sides (it is no longer collapsed away, others may join it)
        mine = cands()
        mine[1].open_left = 1
        out, n, _ = orc.collapse(st, mine)
        assert n == 1 and [(c.alt.decode(), sum(c.support_by_dir), c.open_left, c.open_right) for c in out] == [("AACGTTGCA", 3, 0, 0), ("AACGTA", 3, 0, 0)]
    finally:
        orc.set_known_variants([])
    del keep


def test_variant_collapser_ignores_mnvs_when_asked():
    """VariantCollapserTests.cs:383-425 (Collapse_IgnoreMNVs): with excludeMNVs the MNV AC>GT (open on the left, support 3047) stays as it
    is and the SNV A>G that is open on both sides (30) joins the SNV A>G that is open on the left (16); without it
    (Collapse_CandidateOrderIndependent :428-480) the one open on both sides joins the MNV (3077) and the other SNV keeps its 16.  On the
    reference's mock allele source (every GetAlleleCount is 1, :948-949)."""
    st = orc.State(1, 64)
    for pos in range(1, 40):
        for a in range(6):
            for d in range(3):
                for anchor in range(11):
                    st.set_count(pos, a, d, anchor, 0)
                st.set_count(pos, a, d, 5, 1)
    mnv, snv = _CAT["Mnv"], _CAT["Snv"]
    def cands():
        return [orc.make_candidate(20, snv, "A", "G", support=(16, 0, 0), open_left=True),
                orc.make_candidate(20, snv, "A", "G", support=(30, 0, 0), open_left=True, open_right=True),
                orc.make_candidate(20, mnv, "AC", "GT", support=(3047, 0, 0), open_left=True)]
    out, n, _ = orc.collapse(st, cands(), exclude_mnvs=True)
    assert sorted((c.alt.decode(), sum(c.support_by_dir)) for c in out) == [("G", 16 + 30), ("GT", 3047)] and n == 1
    out, n, _ = orc.collapse(st, cands(), exclude_mnvs=False)
    assert sorted((c.alt.decode(), sum(c.support_by_dir)) for c in out) == [("G", 16), ("GT", 3047 + 30)] and n == 1


# ---- end to end: the reference's own BAMs -> the VCF rows Pisces wrote for them -----------------------------------------------
@pytest.mark.parametrize("name", ["bam_chr19", "bam_chr17_again", "bam_chr17_int", "bam_chr17_vcf", "bam_phix", "bam_edge_ins", "bam_edge_del", "bam_small_s1"])
def test_reference_bams_give_the_vcf_rows_pisces_wrote(name):
    """Reads decoded from the reference's test BAMs (filtered as AlignmentSource does), run through the oracle with the options of
    the functional test that owns the BAM, formatted by pisces_hip_format_vcf: the body lines must be the ones Pisces left in its
    test-data VCFs / quotes in its tests, byte for byte (tests/bam_fixtures.py names each source)."""
    from pisces_amd import engine
    from tests import bam_fixtures
    case = bam_fixtures.CASES[name]
    z, batch = bam_fixtures.load(name)
    off = int(z["offset"])
    cfg = _abi.default_config(**case["cfg"])
    regions = [(a - off, b - a + 1) for a, b in case["intervals"]] if case["intervals"] else [(1, len(z["ref"]))]
    lines = []
    for start, loci in regions:
        recs, alleles, _, _ = orc.run_reads_full(batch, z["ref"], start, loci, cfg)
        recs = recs.copy()
        recs["position"] += off
        text = engine.format_vcf(case["chrom"], recs, alleles=alleles, noise_level_from_records=1, **case["vcf"])
        lines += text.rstrip("\n").split("\n") if text else []
    bam_fixtures.check_lines(case, lines, bam_fixtures.expected_lines(name, z))


@pytest.mark.parametrize("name", ["bam_chr19", "bam_chr17_again", "bam_chr17_int", "bam_chr17_vcf"])
def test_reference_bams_through_the_oracle_s_interval_set(name):
    """The same rows from ONE run of the oracle's block schedule over the whole window with the run's ChrIntervalSet
    (orc_run_reads_schedule_intervals: Reference candidates inside the intervals only, callable alleles outside them counted and not
    reported) — what the GPU fuzz's interval draws are checked against, pinned here to the rows Pisces wrote."""
    from pisces_amd import engine
    from tests import bam_fixtures
    case = bam_fixtures.CASES[name]
    z, batch = bam_fixtures.load(name)
    off = int(z["offset"])
    cfg = _abi.default_config(**case["cfg"])
    intervals = [(a - off, b - off) for a, b in case["intervals"]]
    recs, alleles, _ = orc.run_reads_schedule(batch, z["ref"], 1, len(z["ref"]), cfg, [], intervals=intervals)
    recs = recs.copy()
    recs["position"] += off
    text = engine.format_vcf(case["chrom"], recs, alleles=alleles, noise_level_from_records=1, **case["vcf"])
    bam_fixtures.check_lines(case, text.rstrip("\n").split("\n") if text else [], bam_fixtures.expected_lines(name, z))


# ---- MnvReallocator ------------------------------------------------------------------------------------
def _norm(rows):
    return sorted((r["position"], r["ref"], r["alt"], r["support"], tuple(r["dirs"]), r["category"]) for r in rows)


@pytest.mark.parametrize("case", json.load(open(os.path.join(G, "mnv_reallocator_cases.json")))["cases"], ids=lambda c: c["name"][:40])
def test_mnv_reallocator_cases(case):
    got_callable, got_outside = orc.reallocate_failed_mnvs(case["failed"], case["callable"], case["max"])
    if "expect_callable" in case:
        assert _norm(got_callable) == _norm(case["expect_callable"])
    for want in case.get("expect_callable_contains", []):
        assert _norm(got_callable).count(_norm([want])[0]) == 1
    assert _norm(got_outside) == _norm(case["expect_outside"])


# ---- NoiseModel.Window ---------------------------------------------------------------------------------
def test_window_noise_model_uses_the_mean_base_error_of_the_locus():
    """AlleleCaller.cs:215-218 + RegionStateManager.cs:191: with NoiseModel.Window the q-score of an allele is computed at noise level
    (int)PtoQ(sum of 10^(-(int)q/10f) over the passing A/C/G/T bases / TotalCoverage).  200 reads of Q30 bases, 14 of them with an SNV:
    the mean error is 10^-3 -> noise level 29 or 30 (the quotient sits on the integer edge), well above the flat level of 20, so the
    window q-score must equal the flat q-score computed at that noise level and exceed the flat-20 one."""
    ref = b"ACGTACGTACGTACGTACGT" * 5
    reads = []
    for i in range(200):
        seq = bytearray(ref[10:60])
        if i < 14:
            seq[20] = ord("T") if ref[30] != ord("T") else ord("G")
        reads.append({"pos": 11, "cigar": [("M", 50)], "seq": bytes(seq).decode(), "quals": [30] * 50, "reverse": bool(i % 2)})
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(ref, dtype=np.uint8)
    def run(**kw):
        recs, _ = orc.run_reads(batch, refa, 1, len(ref), _abi.default_config(max_variant_qscore=1000, **kw))
        snv = recs[((recs["info"] >> 4) & 7) == _abi.CAT_SNV]
        assert len(snv) == 1 and snv["position"][0] == 31
        return int(snv["variant_qscore"][0])
    flat20, window = run(), run(noise_model=1)
    assert window in (run(noise_level=29), run(noise_level=30)) and window > flat20


# ---- diploid (germline) genotyping, SURVEY section 8 row f4 ----------------------------------------------------------------------
_DIPLOID = load("diploid_cases.json")
_GT_CODE = {"HeterozygousAlt1Alt2": 0, "Alt12LikeNoCall": 1, "HeterozygousAltRef": 2, "HomozygousAlt": 3, "HomozygousRef": 4,
            "RefLikeNoCall": 5, "AltLikeNoCall": 6, "RefAndNoCall": 7, "AltAndNoCall": 8}


@pytest.mark.parametrize("case", _DIPLOID["genotype_scenarios"], ids=lambda c: "%s-%s-%s" % (c["genotype"], c["ref_freqs"], c["alt_freqs"]))
def test_diploid_genotype_scenarios(case):
    """GenotypeCalculatorTest.DiploidGenotypeScenarios through its harness (:107-147): float32 frequencies x coverage truncated to int."""
    cov = case["coverage"]
    alleles = []
    ref_freq = 0.0
    for rf in case["ref_freqs"]:
        sup = int(np.float32(rf) * np.float32(cov))
        alleles.append({"category": _abi.CAT_REFERENCE, "ref": "A", "alt": "A", "support": sup, "coverage": cov, "ref_support": sup})
        ref_freq = float(np.float32(rf))
    if ref_freq == 0:
        ref_freq = 1.0 - float(np.sum(np.array(case["alt_freqs"], dtype=np.float32), dtype=np.float32))   # List<float>.Sum() is a float
    for vf in case["alt_freqs"]:
        alleles.append({"category": _abi.CAT_SNV, "ref": "A", "alt": "T", "support": int(np.float32(vf) * np.float32(cov)), "coverage": cov,
                        "ref_support": int(ref_freq * cov)})
    gt, prune, per = orc.diploid_set_genotypes(alleles, min_depth=_DIPLOID["min_depth_to_genotype"])
    assert gt == _GT_CODE[case["genotype"]] and sum(prune) == case["prune"]
    assert all(p[0] == gt for p in per)


@pytest.mark.parametrize("table", _DIPLOID["genotype_qscores"], ids=lambda t: "%s-%d" % (t["genotype"], t["depth"]))
def test_diploid_genotype_qscores(table):
    """DiploidGenotypeQualityCalculatorTests (:16-96, :103-117) through TestCalculation (:124-134)."""
    gt = _GT_CODE[table["genotype"]]
    for f, want in zip(table["frequencies"], table["expected"]):
        depth = float(table["depth"])
        support = int(depth * f)
        if table["genotype"] == "HomozygousRef":
            support = int(depth * (1.0 - f))
        assert orc.diploid_gq(gt, int(depth), support) == want, (table["genotype"], depth, f)


def test_diploid_strand_bias_stats():
    """StrandBiasCalculatorTests PopulateDiploidStats cases (:185-285), three decimals as the test asserts them."""
    for c in _DIPLOID["diploid_sb_stats"]:
        fn, fp, pv = orc.diploid_sb_stats(c["support"], c["coverage"], _DIPLOID["sb_threshold"])
        for name, got in (("ChanceFalseNeg", fn), ("ChanceFalsePos", fp), ("ChanceVarFreqGreaterThanZero", pv)):
            if name in c:
                assert abs(got - c[name]) < 0.0005 + 1e-12, (c, name, got)


@pytest.mark.parametrize("want,prune,ref_freq,alt_freqs,coverage", [
    (9, 2, 0.80, [0.01, 0.01], 1000),     # HemizygousRefTest
    (11, 2, 0.70, [0.01, 0.01], 1000),    # NoCallDueToRefMajorVf
    (11, 2, 0.22, [0.75, 0.01], 1000),    # NoCallDueToRefMinorVf
    (11, 2, 0.80, [0.01, 0.01], 10),      # NoCallDueToCoverge
    (10, 1, 0.10, [0.75, 0.01], 1000),    # HemizygousAlt
])
def test_haploid_genotype_scenarios(want, prune, ref_freq, alt_freqs, coverage):
    """HaploidGenotypeCalculatorTests.cs:59-96 through its harness (:20-57): minor / major VF 0.20 / 0.70, minimum depth 100; genotype
    codes 9 / 10 / 11 = HemizygousRef / HemizygousAlt / HemizygousNoCall."""
    sup = int(np.float32(ref_freq) * np.float32(coverage))
    alleles = [{"category": _abi.CAT_REFERENCE, "ref": "A", "alt": "A", "support": sup, "coverage": coverage, "ref_support": sup}]
    for vf in alt_freqs:
        alleles.append({"category": _abi.CAT_SNV, "ref": "A", "alt": "T", "support": int(np.float32(vf) * np.float32(coverage)),
                        "coverage": coverage, "ref_support": int(float(np.float32(ref_freq)) * coverage)})
    gt, pr, per = orc.haploid_set_genotypes(alleles)
    assert gt == want and sum(pr) == prune and all(p[0] == gt for p in per)


def test_stitched_deletion_support_direction_scenarios():
    """GetSupportDirection for a deletion inside a stitched read (CigarDirections != null -> GetDeletionDirectionForStitchedRead,
    CandidateVariantFinder.cs:417-420, 468-487): the reference's 14 RunDeletionScenarios."""
    doc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "support_direction_deletion_cases.json")))
    code = {"Forward": _abi.DIR_FORWARD, "Reverse": _abi.DIR_REVERSE, "Stitched": _abi.DIR_STITCHED}
    rd = doc["read"]
    start, dl = rd["variant_start_in_read"], rd["deletion_length"]
    ref = "ATCG" * 5
    old_method_differs = 0
    for case in doc["cases"]:
        expanded = ([_abi.DIR_FORWARD] * case["num_forward"] + [_abi.DIR_STITCHED] * case["num_stitched"] + [_abi.DIR_REVERSE] * case["num_reverse"])
        sequenced = expanded[:start] + expanded[start + dl:]   # PiscesSupportDirectionTestSetup.GetCoverageDirections :45-59
        read = orc.make_read(rd["position"], rd["sequence"], cigar=rd["cigar"], dirs=sequenced, expanded_dirs=expanded)
        assert orc.lib.orc_deletion_direction_for_stitched_read(read, start - 1, start) == code[case["expected"]], case["name"]
        dels = [c for c in orc.find_candidates(read, ref) if c.category == _abi.CAT_DELETION]
        assert len(dels) == 1 and dels[0].position == 3
        want = [0, 0, 0]
        want[code[case["expected"]]] = 1
        assert list(dels[0].support_by_dir) == want, case["name"]
        # without the expanded map the same read takes the anchor-direction fallback (:422-428)
        plain = orc.make_read(rd["position"], rd["sequence"], cigar=rd["cigar"], dirs=sequenced)
        old = [c for c in orc.find_candidates(plain, ref) if c.category == _abi.CAT_DELETION][0]
        old_method_differs += list(old.support_by_dir) != want
    assert old_method_differs >= 2   # the scenarios do tell the two branches apart


@pytest.mark.parametrize("track_open_ended", [True, False])
def test_batches_and_collapsable_candidates_of_later_blocks(track_open_ended):
    """RegionStateManagerTests.AddAndGetCandidates (Pisces.Processing.Tests/UnitTests/RegionStateManagerTests.cs:27-122), the same
    candidates and the same sequence of GetCandidatesToProcess calls: a batch only when upTo has moved onto another block, only blocks
    that lie wholly below upTo, a block held while one of its alleles reaches past upTo, and — with open-ended tracking on — the
    collapsable SNV / MNV candidates of the following blocks pulled into a batch whose alleles reach past its last position."""
    SNV, MNV, DEL = _abi.CAT_SNV, _abi.CAT_MNV, _abi.CAT_DELETION
    st = orc.State(1, 6000, track_open_ended=track_open_ended)
    st.track_blocks(1000)
    cands = [
        (1, SNV, "A", "T", False), (998, DEL, "AT", "A", False), (1000, SNV, "A", "T", False),
        (1001, SNV, "A", "T", False), (1001, SNV, "A", "G", False),
        (3000, MNV, "ATCC", "GAGG", False),            # spans blocks
        (3001, DEL, "AT", "A", False),                 # not collapsable
        (3002, SNV, "T", "A", False),                  # collapsable
        (3003, SNV, "G", "C", True),                   # open on the right: not collapsable
        (3002, MNV, "TA", "GA", False),                # collapsable
        (3001, MNV, "TACGG", "GAGAA", False),          # ends past upTo
        (5005, MNV, "AC", "TT", False),
    ]
    for (p, cat, r, a, open_right) in cands:
        assert st.add_candidate(orc.make_candidate(p, cat, r, a, support=(1, 0, 0), open_right=open_right)) == 0
    key = lambda c: (c.position, c.category, c.ref.decode(), c.alt.decode())
    def batch(up_to):
        b = st.next_batch(up_to)
        if not b:
            return b, None
        got, _ = st.batch_candidates(b[0], b[1], up_to)
        return b, sorted(key(c) for c in got)
    want = lambda pred: sorted((p, cat, r, a) for (p, cat, r, a, o) in cands if pred(p, cat, r, a, o))
    collapsable = lambda p, cat, r, a, o: cat in (SNV, MNV) and p + len(a) - 1 <= 3003 and not o

    assert batch(1) == ((), None)                       # first time: a batch, nothing cleared
    assert batch(1000) == (None, None)                  # upTo has not left its block: no batch
    b, got = batch(1002)
    assert b == (1, 1000) and got == want(lambda p, *_: p <= 1000)
    st.done_processing(b[1])
    b, got = batch(2001)
    assert b == (1001, 2000) and got == want(lambda p, *_: p == 1001)
    st.done_processing(b[1])
    b, got = batch(3003)                                # the MNV at 3000 ends at 3003: block 3 clears and reaches into block 4
    assert b == (2001, 3000)
    assert got == want(lambda p, cat, r, a, o: p > 1001 and (p <= 3000 or (track_open_ended and collapsable(p, cat, r, a, o))))
    # not done: the next batch holds the same blocks again, without what was extracted
    b, got = batch(4001)
    assert b == (2001, 4000)
    assert got == want(lambda p, cat, r, a, o: 1001 < p < 4000 and (p != 3002 or not track_open_ended))
    b, got = batch(None)
    assert b == (2001, 6000)
    assert got == want(lambda p, cat, r, a, o: p > 1001 and (p != 3002 or not track_open_ended))
    st.done_processing(b[1])
    assert batch(None) == ((), None)                    # an empty state is fine


def test_schedule_collapses_the_open_left_base_of_the_next_block_into_the_mnv():
    """The oracle's upTo schedule on the cross-block case of the GPU test: an MNV that starts in a cleared block takes the support of
    the open-left SNV that is its last base and lives in the next block (VariantCollapser's end-anchored match); with one batch per
    block and no look-ahead that SNV is called on its own."""
    from tests.test_gpu_parity import _cross_block_collapse_case
    ref, reads, planted = _cross_block_collapse_case()
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    cfg = _abi.default_config(call_mnvs=1, collapse=1)
    ahead = orc.run_reads_schedule(batch, refa, 1, len(ref), cfg, [1500, 2600])
    plain = orc.run_reads_blocks(batch, refa, 1, len(ref), cfg)
    rows = lambda x: {(int(r["position"]), a): int(r["allele_support"]) for r, a in zip(x[0], x[1]) if a[0] != a[1]}
    ra, rp = rows(ahead), rows(plain)
    for p in (999, 1999):
        mnv = (p, (bytes(ref[p - 1:p + 2]).decode(), planted[0 if p == 999 else 1][1]))
        tail = (p + 2, (chr(ref[p + 1]), mnv[1][1][2]))
        assert tail in rp and tail not in ra
        assert ra[mnv] == rp[mnv] + rp[tail]
    # candidates that were looked at and did not collapse are called with their own block, unchanged
    for p in (1020, 1050, 1600, 2040):
        same = [k for k in ra if k[0] == p]
        assert same and all(ra[k] == rp[k] for k in same)
    # a schedule that never looks ahead (upTo at the block ends) gives the per-block result
    flat = orc.run_reads_schedule(batch, refa, 1, len(ref), _abi.default_config(call_mnvs=1, collapse=0), [1500, 2600])
    flat_blocks = orc.run_reads_blocks(batch, refa, 1, len(ref), _abi.default_config(call_mnvs=1, collapse=0))
    assert rows(flat) == rows(flat_blocks)


# ---- forced genotyping (-forcedalleles): ForcedGTFxnlTest.RunForcedGT ------------------------------------------------------------
FORCED_GT = load("forced_gt.json")


@pytest.mark.parametrize("run", ["noisy", "forced1", "forced2"])
def test_forced_gt_functional_test_vcfs(run):
    """ForcedGTFxnlTest.RunForcedGT (ForcedGTFxnlTest.cs:10-124) on PhiX_S3.bam: -c 2 -minbq 10 -minvf 0.00001 -nl 40 -callMNVs
    -maxmnvlength 10 -maxgapbetweenmnv 5 -ncfilter 1, first without forced alleles (-minvq 1), then with the nine alleles of
    PhiX_S3.forcedGTInput.vcf (-minvq 1: three of them are not in the reads and come out as ForcedReport rows without support), then
    with -minvq 20 (the noise-level MNVs among them fail, are reallocated AND reported; Reference rows stay beside forced rows).
    The oracle runs the reads of the BAM through the block schedule; pisces_hip_format_vcf writes the rows: byte for byte the body
    lines of PhiX_S3.noisy.vcf / Forced1.vcf / Forced2.vcf (the files hold the first 76 positions)."""
    from pisces_amd import engine
    from tests import bam_fixtures
    r = FORCED_GT["runs"][run]
    z, batch = bam_fixtures.load("bam_phix")
    cfg = _abi.default_config(**forced_gt_config(r["min_variant_qscore"]))
    forced = [tuple(f) for f in FORCED_GT["forced"]] if r["forced"] else []
    recs, alleles, _ = orc.run_reads_schedule(batch, z["ref"], 1, len(z["ref"]), cfg, [1500, 2500, 3500, 4500], forced=forced)
    text = engine.format_vcf("phix", recs, alleles=alleles, noise_level_from_records=1, noise_level=40, min_frequency_threshold=0.00001)
    last = int(r["lines"][-1].split("\t")[1])
    got = [l for l in text.rstrip("\n").split("\n") if int(l.split("\t")[1]) <= last]
    assert got == r["lines"]


def forced_gt_config(min_variant_qscore):
    # (-minvf also sets the frequency filter, the genotyper's frequency and the LOD target: VariantCallingParameters.cs:134-156; the
    # functional-test harness skips Validate(), which leaves LowDepthFilter null: see tests/bam_fixtures.py)
    return dict(low_depth_filter=-1, min_coverage=2, min_base_call_quality=10, min_variant_qscore=min_variant_qscore, min_frequency=0.00001,
                variant_freq_filter=0.00001, genotype_min_freq_filter=0.00001, target_lod_frequency=0.00001, noise_level=40, call_mnvs=1,
                max_mnv_length=10, max_gap_between_mnv=5, no_call_filter_threshold=1.0)


def test_diploid_locus_processor_cases():
    """DiploidLocusProcessorTests.cs:11-125, the four cases: a forced allele at a reference site, at a no-call site, beside a
    heterozygous call, and the genotype q-score of the whole position = the smallest of the alleles that were not forced."""
    SNV, INS, REF = _abi.CAT_SNV, _abi.CAT_INSERTION, _abi.CAT_REFERENCE
    forced = dict(category=SNV, genotype=_abi.GT_ALT_LIKE_NOCALL, gq=10, forced=True)
    got = orc.diploid_locus_process([forced, dict(category=REF, genotype=_abi.GT_HOM_REF, gq=100)])
    assert got[0] == (_abi.GT_HOM_REF, 100)
    got = orc.diploid_locus_process([forced, dict(category=INS, genotype=_abi.GT_ALT_LIKE_NOCALL, gq=20)])
    assert got[0] == (_abi.GT_ALT_LIKE_NOCALL, 20)
    got = orc.diploid_locus_process([forced, dict(category=INS, genotype=_abi.GT_HET_ALT_REF, gq=40)])
    assert got[0] == (_abi.GT_OTHERS, 40)
    got = orc.diploid_locus_process([forced, dict(category=INS, genotype=_abi.GT_HET_ALT1_ALT2, gq=40),
                                     dict(category=INS, genotype=_abi.GT_HET_ALT1_ALT2, gq=100)])
    assert [g[1] for g in got] == [40, 40, 40] and got[0][0] == _abi.GT_OTHERS
    # no forced allele: nothing changes (Process returns early)
    assert orc.diploid_locus_process([dict(category=INS, genotype=_abi.GT_HET_ALT_REF, gq=40), dict(category=SNV, genotype=_abi.GT_HOM_ALT, gq=7)]) == \
        [(_abi.GT_HET_ALT_REF, 40), (_abi.GT_HOM_ALT, 7)]


# ---- the reference's tables on the caller / region-state / MNV path (tests/golden/README.md: file:line of each) --------------------
@pytest.mark.parametrize("sc", load("region_state.json")["deletions"]["scenarios"], ids=lambda s: s["name"])
def test_add_and_get_allele_counts_deletions(sc):
    """RegionStateManagerTests.AddAndGetAlleleCounts_Deletions (:597-704): deletions are counted at every position they span — inside a
    read, behind a soft clip at its start, at its end — with the bases at the minimum quality; every asserted cell, the zeros included."""
    g = load("region_state.json")["deletions"]
    st = orc.State(900, 300, min_bq=g["min_quality"])
    for rd in sc["reads"]:
        assert st.add_allele_counts(_mk(rd, g["min_quality"])) == 0
    for pos, a, d, n in sc["expect"]:
        assert st.get_allele_count(pos, ALLELE[a], DIR[d]) == n, (pos, a, d)


def test_done_processing_clears_blocks_and_holds_the_spanned_ones():
    """RegionStateManagerTests.DoneProcessing (:707-781): GetCandidatesToProcess(upTo) + DoneProcessing per upTo; a cleared block's
    counts read 0, the block whose deletion ends past upTo and the block behind it keep theirs."""
    g = load("done_processing.json")
    st = orc.State(1, 9000)
    st.track_blocks(g["block_size"])
    for rd in g["reads"]:
        assert st.add_allele_counts(_mk(rd, 30)) == 0
    for pos, a, d, n in g["expect_before"]:
        assert st.get_allele_count(pos, ALLELE[a], DIR[d]) == n, (pos, a, d)
    for c in g["candidates"]:
        if "ref_length" in c:
            cand = orc.make_candidate(c["pos"], _CAT[c["category"]], c["ref_base"] * (orc.ORC_MAX_ALLELE - 1), c["alt"], support=tuple(c["support"]))
            assert st.add_candidate(cand, ref_length=c["ref_length"]) == 0
        else:
            assert st.add_candidate(orc.make_candidate(c["pos"], _CAT[c["category"]], c["ref"], c["alt"], support=tuple(c["support"]))) == 0
    for step in g["steps"]:
        b = st.next_batch(step["up_to"])
        assert b is not None, step        # every upTo of the test lies in another block than the one before: a batch each time
        if b:
            st.done_processing(b[1])
        for pos, a, d, n in step["expect"]:
            assert st.get_allele_count(pos, ALLELE[a], DIR[d]) == n, (step["up_to"], pos)


def test_gapped_mnv_ref_counts_add_and_get():
    """RegionStateManagerTests.AddAndGetGappedMnvRefCount (:136-169) and RegionStateTests.AddAndGetGappedMnvReferenceCounts (+ _Errors)
    (:282-325): counts add up per position, an add of 0 and positions not named change nothing, an add outside the region is dropped and
    a get outside it throws."""
    g = load("gapped_mnv_ref.json")
    st = orc.State(1, 25000)
    for step in g["manager"]["steps"]:
        for pos, n in step["add"]:
            st.add_gapped_mnv_ref(pos, n)
        for pos, n in step["expect"]:
            assert st.get_gapped_mnv_ref(pos) == n, pos
    r = g["region"]
    st = orc.State(r["start"], r["end"] - r["start"] + 1)
    for step in r["steps"]:
        for pos, n in step["add"]:
            st.add_gapped_mnv_ref(pos, n)
        for pos, n in step["expect"]:
            assert st.get_gapped_mnv_ref(pos) == n, pos
    e = g["region_errors"]
    st = orc.State(e["start"], e["end"] - e["start"] + 1)
    for pos, n in e["add"]:
        st.add_gapped_mnv_ref(pos, n)
    everything = lambda: [st.get_gapped_mnv_ref(p) for p in range(e["start"], e["end"] + 1)]
    before = everything()
    st.add_gapped_mnv_ref(*e["add_outside"])
    assert everything() == before
    nonzero = dict(map(tuple, e["expect_all_after"]["nonzero"]))
    assert before == [nonzero.get(p, 0) for p in range(e["start"], e["end"] + 1)]
    with pytest.raises(ValueError):
        st.get_gapped_mnv_ref(e["get_throws"])


def _region_candidates_state(g, with_intervals):
    st = orc.State(g["region"][0], g["region"][1] - g["region"][0] + 1)
    for c in g["candidates"]:
        assert st.add_candidate(orc.make_candidate(c["pos"], _CAT[c["category"]], c["ref"], c["alt"], support=tuple(c["support"]))) == 0
    for row in g["counts"]:
        st.set_count(row["pos"], ALLELE[row["allele"]], DIR[row["dir"]], g["anchor_index"], row["n"])
    if with_intervals:
        st.set_intervals([tuple(iv) for iv in g["intervals"]])
    return st


def _region_candidates_config(v, **kw):
    # (emit_zero_coverage_refs: "1 when an interval set is supplied", include/pisces_hip.h — RegionState.cs:446)
    return _abi.default_config(include_reference_calls=1 if v["with_reference"] else 0, emit_zero_coverage_refs=1 if v["with_intervals"] else 0, **kw)


_REGION_CANDIDATES = load("region_candidates.json")


@pytest.mark.parametrize("v", _REGION_CANDIDATES["variants"], ids=lambda v: v["name"])
def test_get_all_candidates_reference_cases(v):
    """RegionStateTests.ExecuteTest_GetCandidates (:339-437), all four of :258-279: the list GetAllCandidates returns — the candidates as
    added (the SNV at 15 too, outside the intervals: intervals limit Reference candidates only), a Reference candidate with the reference
    base's support by direction where there is coverage, and inside an interval set also where there is none."""
    g = _REGION_CANDIDATES
    st = _region_candidates_state(g, v["with_intervals"])
    got = st.all_candidates(g["reference"], _region_candidates_config(v))
    key = lambda c: (c["pos"], c["category"], c["ref"], c["alt"], tuple(c["support"]))
    assert sorted((c.position, c.category, c.ref.decode(), c.alt.decode(), tuple(c.support_by_dir)) for c in got) == \
        sorted((c["pos"], _CAT[c["category"]], c["ref"], c["alt"], tuple(c["support"])) for c in v["expect"])


_CALLER_MNV = load("caller_mnv_cases.json")


def caller_mnv_config(sc, **kw):
    c = sc["config"]
    freq = float(np.float32(c["min_frequency_num"]) / np.float32(c["min_frequency_den"])) if "min_frequency_num" in c else c["min_frequency"]
    return _abi.default_config(rmxn_max_repeat_length=-1, variant_qscore_filter=-1, low_depth_filter=-1, variant_freq_filter=-1.0, no_call_filter_threshold=-1.0,
                               max_variant_qscore=c["max_variant_qscore"], noise_level=c["noise_level"], min_coverage=c["min_coverage"],
                               min_variant_qscore=c["min_variant_qscore"], include_reference_calls=c["include_reference_calls"], min_frequency=freq,
                               call_mnvs=1, collapse=0, max_mnv_length=8, **kw)


def caller_mnv_multiplier(sc, position):
    m = _CALLER_MNV["multipliers"]
    return m["high"] if position == sc["high_coverage_coordinate"] else m["low"] if position == sc["low_coverage_coordinate"] else m["normal"]


@pytest.mark.parametrize("sc", _CALLER_MNV["scenarios"], ids=lambda s: s["name"])
def test_allele_caller_mnv_reallocation_cases(sc):
    """VariantCallerTests.CallVariants_MnvReallocation / _MnvTakingRefSupport / _MnvReallocatesToDifferentBlock /
    _MnvReallocatesToSnvOutsideInterval (:307-656): MNV reallocation as AlleleCaller.Call drives it — who gains the failed MNVs' support,
    what is handed to the next block past MaxClearedPosition, the reference support a gapped MNV takes, and the interval set applied to
    what reallocation makes."""
    lo, hi = sc["positions_touched"]
    st = orc.State(1, 2100)
    for p in range(lo, hi + 1):
        for a in range(6):
            for d in range(3):
                st.set_count(p, a, d, 5, caller_mnv_multiplier(sc, p))
    if sc["intervals"]:
        st.set_intervals([tuple(iv) for iv in sc["intervals"]])
    cands = [orc.make_candidate(c["pos"], _CAT[c["category"]], c["ref"], c["alt"], support=tuple(c["support"])) for c in sc["candidates"]]
    _, full, _ = orc.call_candidates(st, cands, caller_mnv_config(sc), max_cleared_position=sc["max_cleared_position"])
    same = lambda f, e: (f.position, f.category, f.ref.decode(), f.alt.decode()) == (e["pos"], _CAT[e["category"]], e["ref"], e["alt"])
    for e in sc["expect_called"]:
        rows = [f for f in full if same(f, e)]
        assert len(rows) == 1, e
        for field in ("allele_support", "total_coverage", "reference_support"):
            if field in e:
                assert getattr(rows[0], field) == e[field], (e, field)
        if "frequency" in e:   # CalledAllele.Frequency, float: AlleleSupport / TotalCoverage
            assert np.float32(rows[0].allele_support) / np.float32(rows[0].total_coverage) == np.float32(e["frequency"])
    for e in sc["expect_absent"]:
        assert not [f for f in full if same(f, e)], e
    for e in sc["expect_no_reference_row"]:
        for f in full:
            if f.position == e["pos"] and f.category == _abi.CAT_REFERENCE:
                assert "allele_support" in e or "allele_support_above" in e, e
                assert f.allele_support != e.get("allele_support") and not f.allele_support > e.get("allele_support_above", 1 << 30), e
    if "expect_called_count" in sc:
        assert len(full) == sc["expect_called_count"], [(f.position, f.ref, f.alt) for f in full]
    if "expect_gapped_mnv_ref" in sc:   # what AddGappedMnvRefCount was given: these and nothing else
        want = dict(map(tuple, sc["expect_gapped_mnv_ref"]))
        assert {p: st.get_gapped_mnv_ref(p) for p in range(1, 2101) if st.get_gapped_mnv_ref(p)} == want
    # IAlleleSource.AddCandidates: the batch was an explicit list, so what the state holds now is what the call handed to the next block
    handed = sorted((c.position, c.category, c.ref.decode(), c.alt.decode(), tuple(c.support_by_dir)) for c in st.candidates())
    assert handed == sorted((c["pos"], _CAT[c["category"]], c["ref"], c["alt"], tuple(c["support"])) for c in sc.get("expect_handed_to_next_block", []))


def test_ref_support_taken_by_gapped_mnvs():
    """VariantCallerTests.GetRefSupportFromGappedMnvs (:658-763): the eight alleles as one callable batch (nothing fails: no thresholds);
    the map AlleleCaller registers with the state is {13: 15, 124: 36, 78901: 25, 78903: 25} and has none of the keys the test asserts
    absent — nor any other."""
    g = load("gapped_mnv_ref_support.json")
    st = orc.State(1, g["reference_length"])
    cands = [orc.make_candidate(a["pos"], _CAT[a["category"]], a["ref"], a["alt"], support=(a["allele_support"], 0, 0)) for a in g["alleles"]]
    cfg = _abi.default_config(rmxn_max_repeat_length=-1, variant_qscore_filter=-1, low_depth_filter=-1, variant_freq_filter=-1.0, no_call_filter_threshold=-1.0,
                              min_coverage=0, min_variant_qscore=0, min_frequency=0.0, call_mnvs=1, collapse=0, max_mnv_length=8)
    _, full, _ = orc.call_candidates(st, cands, cfg)
    assert len(full) == len(g["alleles"])
    for p in g["expect_absent"]:
        assert st.get_gapped_mnv_ref(p) == 0, p
    gapped = np.array([st.get_gapped_mnv_ref(p) for p in range(1, g["reference_length"] + 1)])
    assert {int(i) + 1: int(gapped[i]) for i in np.nonzero(gapped)[0]} == dict(map(tuple, g["expect"]))
