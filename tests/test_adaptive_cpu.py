"""PloidyModel.DiploidByAdaptiveGT without a device: the host-only entries of the library (pisces_hip_adaptive_genotype_qscore,
pisces_hip_set_genotypes_adaptive, pisces_hip_format_vcf[_padded]_ex) against the reference's own tables
(tests/golden/adaptive_cases.json) and against tests/adaptive_ref.py, which is itself held to those tables first."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import adaptive_ref as R
from tests import orc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "adaptive_cases.json")))
GT_OF_NAME = {"HeterozygousAlt1Alt2": 0, "Alt12LikeNoCall": 1, "HeterozygousAltRef": 2, "HomozygousAlt": 3, "HomozygousRef": 4, "RefLikeNoCall": 5,
              "AltLikeNoCall": 6, "RefAndNoCall": 7, "AltAndNoCall": 8}
CAT_OF_NAME = {"Snv": 0, "Insertion": 1, "Deletion": 2, "Mnv": 3, "Reference": 4}
F = np.float32

# the five (means, priors) pairs of the exhaustive check: default SNV, default indel, the reference's test pair, both pairs of example.model
PAIRS = [
    (R.DEFAULT_PARAMS["snv_model"], R.DEFAULT_PARAMS["snv_prior"]),
    (R.DEFAULT_PARAMS["indel_model"], R.DEFAULT_PARAMS["indel_prior"]),
    (tuple(CASES["means"]), tuple(CASES["priors"])),
    (tuple(CASES["model"]["snv_model"]), tuple(CASES["model"]["snv_prior"])),
    (tuple(CASES["model"]["indel_model"]), tuple(CASES["model"]["indel_prior"])),
]


def lib_params(means=None, priors=None, **kw):
    """engine.adaptive_params with one pair standing for SNVs and indels alike when given"""
    return engine.adaptive_params(snv_model=means, indel_model=means, snv_prior=priors, indel_prior=priors, **kw)


def ref_params(means=None, priors=None):
    p = dict(R.DEFAULT_PARAMS)
    if means is not None:
        p.update(snv_model=tuple(means), indel_model=tuple(means), snv_prior=tuple(priors), indel_prior=tuple(priors))
    return p


def gp_close(got, want):
    """|gp - ref| <= max(one float32 step of ref, 1e-9); NaN only where the reference has NaN"""
    got = np.asarray(got, dtype=F)
    want = np.asarray(want, dtype=F)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        tol = np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-9)
        ok = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol
    return bool(np.all(ok | both_nan))


# ---- 1. the reference's tables ------------------------------------------------------------------------------------------------------
def _table_cases():
    for t in CASES["qscores"]:
        for f, want in zip(t["frequencies"], t["expected"]):
            depth = t["depth"]
            support = int(depth * (1.0 - f)) if t["reference_allele"] else int(depth * f)   # the harness of the reference's test
            yield t["reference_allele"], support, int(depth), want


def test_qscore_table_from_r_on_the_transcription():
    cases = list(_table_cases())
    assert len(cases) == 30
    for is_ref, support, depth, want in cases:
        ad, dp = R.preprocess(is_ref, support, depth)
        assert R.qscore_and_posteriors(ad, dp, CASES["means"], CASES["priors"])[1] == want, (is_ref, support, depth)


def test_qscore_table_from_r():
    par = lib_params(CASES["means"], CASES["priors"])
    for is_ref, support, depth, want in _table_cases():
        _, q, _ = engine.adaptive_genotype_qscore(support, depth, _abi.CAT_REFERENCE if is_ref else _abi.CAT_SNV, is_ref, par)
        assert q == want, (is_ref, support, depth, q, want)


def _scenario_alleles(s):
    cov = s["coverage"]
    alleles = [dict(category=_abi.CAT_REFERENCE, ref="A", alt="A", support=int(F(s["ref_frequency"]) * F(cov)), coverage=cov)]
    alleles += [dict(category=_abi.CAT_SNV, ref="A", alt="C", support=int(F(v) * F(cov)), coverage=cov) for v in s["alt_frequencies"]]
    return alleles


@pytest.mark.parametrize("s", CASES["scenarios"], ids=lambda s: s["name"])
def test_genotype_scenarios_on_the_transcription(s):
    h = CASES["harness"]
    gt, out = R.set_genotypes(_scenario_alleles(s), None, h["min_depth"], h["min_gq"], h["max_gq"])
    assert [o["genotype"] for o in out] == [GT_OF_NAME[s["genotype"]]] * len(out) and gt == GT_OF_NAME[s["genotype"]]
    assert sum(o["prune"] for o in out) == s["prune"]


@pytest.mark.parametrize("s", CASES["scenarios"], ids=lambda s: s["name"])
def test_genotype_scenarios(s):
    h = CASES["harness"]
    cfg = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE, min_coverage=h["min_depth"], min_genotype_qscore=h["min_gq"], max_genotype_qscore=h["max_gq"])
    gt, out, post = engine.set_genotypes_adaptive(_scenario_alleles(s), cfg)
    assert [o["genotype"] for o in out] == [GT_OF_NAME[s["genotype"]]] * len(out) and gt == GT_OF_NAME[s["genotype"]]
    assert sum(o["prune"] for o in out) == s["prune"]
    assert (post["n"] == (6 if s["genotype"] == "HeterozygousAlt1Alt2" else 3)).all()


def test_multi_allelic_property_and_recalibrated_rows():
    m = CASES["multi_allelic"]
    a1, a2 = m["alleles"]
    q, gp = R.multinomial_qscores(a1["support"], a2["support"], a1["depth"], CASES["means"], CASES["means"])
    assert int(np.argmin(gp)) == m["smallest_posterior_index"]
    # Through the library.  The reference's test calls the calculator directly; the library reaches the multinomial only through a locus
    # that genotypes as 1/2, and 12 + 11 of 30 reads leave 23 % for the reference (a multi-allelic no-call).  So: the same two SNVs with
    # 15 and 14 of 30 reads, the property there, and the values against the transcription, which holds the reference's own case above.
    cfg = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE, min_coverage=10)
    alleles = [dict(category=_abi.CAT_SNV, ref=a["ref"], alt=a["alt"], support=a["support"] + 3, coverage=a["depth"]) for a in (a1, a2)]
    gt, out, post = engine.set_genotypes_adaptive(alleles, cfg, lib_params(CASES["means"], CASES["priors"]))
    q, gp = R.multinomial_qscores(a1["support"] + 3, a2["support"] + 3, a1["depth"], CASES["means"], CASES["means"])
    assert gt == _abi.GT_HET_ALT1_ALT2 and (post["n"] == 6).all()
    assert int(np.argmin(post["gp"][0])) == m["smallest_posterior_index"] and gp_close(post["gp"][0], gp) and out[0]["genotype_qscore"] == q
    # the two 1/2 rows of the recalibration tool's test VCF, with the models of example.model
    mod = CASES["model"]
    par = engine.adaptive_params(mod["snv_model"], mod["indel_model"], mod["snv_prior"], mod["indel_prior"])
    rp = dict(R.DEFAULT_PARAMS, **{k: tuple(v) for k, v in mod.items()})
    through_library = []
    for row in CASES["recal_rows"]:
        cats = [CAT_OF_NAME[t] for t in row["types"]]
        q, gp = R.multinomial_qscores(row["ad"][0], row["ad"][1], row["dp"], R.model_of(rp, cats[0])[0], R.model_of(rp, cats[1])[0])
        assert q == row["gq"] and ",".join("%.2f" % abs(v) for v in gp) == row["gp"]
        alleles = [dict(category=c, ref=row["ref"], alt=alt, support=ad, coverage=row["dp"]) for c, alt, ad in zip(cats, row["alts"], row["ad"])]
        gt, out, post = engine.set_genotypes_adaptive(alleles, cfg, par)
        if gt != _abi.GT_HET_ALT1_ALT2:
            # (the second row: 26 % of the reads are neither allele, the caller's genotyper sees a reference there and says 0/1; the
            # recalibration tool applied the multinomial because the input VCF said 1/2.  The library's multinomial with an insertion
            # and an SNV model is held to the transcription by test_whole_loci_equal_the_transcription)
            through_library.append(False)
            post = np.zeros(2, dtype=_abi.POSTERIORS_DTYPE)
            post["n"], post["gp"] = 6, gp
        else:
            through_library.append(True)
            assert [o["genotype_qscore"] for o in out] == [row["gq"]] * 2 and gp_close(post["gp"][0], gp)
        recs = np.concatenate([_record(row["position"], row["ref"], alt, _abi.GT_HET_ALT1_ALT2, c, row["dp"], ad, 0, 100, row["gq"])
                               for c, alt, ad in zip(cats, row["alts"], row["ad"])])
        line = engine.format_vcf("chr1", recs, alleles=[(row["ref"], alt) for alt in row["alts"]], posteriors=post, crush=1).rstrip("\n").split("\t")
        assert line[8].endswith(":GP") and line[9].split(":")[-1] == row["gp"]   # (-0.0 for the certain genotype prints 0.00)
    assert any(through_library)


# ---- 2. exhaustive: every (support, coverage) up to 1000, and the downsampling branch ---------------------------------------------------
def _library_table(par, category, is_ref, supports, coverages):
    cat, q = C.c_int32(0), C.c_int32(0)
    gp = (C.c_float * 3)()
    f = engine.lib.pisces_hip_adaptive_genotype_qscore
    pp, pc, pq = C.byref(par), C.byref(cat), C.byref(q)
    cats = np.zeros(len(supports), dtype=np.int64)
    qs = np.zeros(len(supports), dtype=np.int64)
    gps = np.zeros((len(supports), 3), dtype=F)
    for i, (s, c) in enumerate(zip(supports.tolist(), coverages.tolist())):
        assert f(pp, category, is_ref, s, c, pc, pq, gp) == 0
        cats[i], qs[i] = cat.value, q.value
        gps[i] = gp[:]
    return cats, qs, gps


def _preprocess_arrays(is_ref, support, coverage):
    ad = np.where(is_ref, np.maximum(coverage - support, 0), support).astype(np.int64)
    dp = coverage.astype(np.int64)
    big = dp > 1000
    ad = np.where(big, (ad.astype(np.float64) / np.maximum(dp, 1) * 1000).astype(np.int64), ad)
    dp = np.where(big, 1000, dp)
    return np.minimum(ad, dp), dp


@pytest.mark.parametrize("pair", range(len(PAIRS)), ids=["snv", "indel", "test pair", "model snv", "model indel"])
def test_every_support_and_coverage_equals_the_transcription(pair):
    means, priors = PAIRS[pair]
    par = lib_params(means, priors)
    cov = np.repeat(np.arange(1, 1001), np.arange(2, 1002))
    sup = np.concatenate([np.arange(0, c + 1) for c in range(1, 1001)])
    assert len(cov) == 501500
    rng = np.random.default_rng(20 + pair)
    big_cov = rng.integers(1001, 200001, 20000)
    big_sup = (rng.random(20000) * (big_cov + 1)).astype(np.int64)
    cov = np.concatenate([cov, big_cov])
    sup = np.concatenate([sup, big_sup])
    # the vectorised table against the scalar transcription on a sample, so that it may stand for it
    for i in rng.integers(0, len(cov), 400).tolist():
        ad, dp = R.preprocess(False, int(sup[i]), int(cov[i]))
        c1, q1, g1 = R.qscore_and_posteriors(ad, dp, means, priors)
        c2, q2, g2 = R.qscore_table([ad], [dp], means, priors)
        assert (c1, q1) == (int(c2[0]), int(q2[0])) and gp_close(g2[0], g1)
    for is_ref in (0, 1):
        ad, dp = _preprocess_arrays(bool(is_ref), sup, cov)
        want_cat, want_q, want_gp = R.qscore_table(ad, dp, means, priors)
        cat, q, gp = _library_table(par, _abi.CAT_REFERENCE if is_ref else _abi.CAT_SNV, is_ref, sup, cov)
        bad = np.nonzero((cat != want_cat) | (q != want_q))[0]
        assert len(bad) == 0, [(int(sup[i]), int(cov[i]), int(cat[i]), int(want_cat[i]), int(q[i]), int(want_q[i])) for i in bad[:10]]
        tol = np.maximum(np.spacing(np.abs(want_gp)).astype(np.float64), 1e-9)
        off = np.nonzero((np.abs(gp.astype(np.float64) - want_gp.astype(np.float64)) > tol).any(axis=1))[0]
        assert len(off) == 0, [(int(sup[i]), int(cov[i]), gp[i].tolist(), want_gp[i].tolist()) for i in off[:10]]


# ---- 3. whole loci ---------------------------------------------------------------------------------------------------------------------
def random_locus(rng, kind=None):
    """1-5 alleles of one locus in (ref, alt) order unless the case says otherwise"""
    depth = int(rng.choice([0, int(rng.integers(1, 10)), int(rng.integers(10, 100)), int(rng.integers(100, 500)), int(rng.integers(501, 1000)),
                            int(rng.integers(1001, 60000))], p=[0.05, 0.1, 0.25, 0.3, 0.15, 0.15]))
    kind = kind or rng.choice(["mixed", "reference", "equal", "least first", "two"], p=[0.45, 0.15, 0.1, 0.15, 0.15])
    ref_base = "A"

    def variant(cat, k):
        if cat == _abi.CAT_SNV:
            return (ref_base, "CGT"[k % 3])
        if cat == _abi.CAT_INSERTION:
            return (ref_base, ref_base + "CGT"[k % 3] * (1 + k % 2))
        if cat == _abi.CAT_DELETION:
            return (ref_base + "CG"[: 1 + k % 2], ref_base)
        return (ref_base + "C", "GT" if k % 2 else "TG")
    if kind == "reference":
        n_alt = int(rng.integers(0, 3))
        cats = [_abi.CAT_REFERENCE] + [int(rng.choice([0, 1, 2, 3])) for _ in range(n_alt)]
    elif kind == "least first":
        cats = [_abi.CAT_SNV] * 3
    elif kind == "two":
        cats = [int(rng.choice([0, 0, 1, 2, 3])) for _ in range(2)]
    else:
        cats = [int(rng.choice([0, 0, 0, 1, 2, 3])) for _ in range(int(rng.integers(1, 6)))]
    n = len(cats)
    if kind == "equal":
        fr = np.full(n, rng.choice([0.1, 0.2, 0.3, 0.45]) if n > 1 else 0.5)
    elif kind == "least first":
        fr = np.array([0.06, 0.44, 0.5]) * rng.uniform(0.9, 1.0)
    elif kind == "two":
        fr = np.array([rng.uniform(0.3, 0.6), rng.uniform(0.3, 0.6)])
        fr = fr / max(1.0, fr.sum())
    else:
        fr = rng.dirichlet(np.ones(n + 1) * rng.choice([0.3, 1.0, 3.0]))[:n]
    alleles = []
    for k, (cat, f) in enumerate(zip(cats, fr)):
        cov = depth if rng.random() < 0.85 else max(0, depth + int(rng.integers(-20, 21)))
        ref, alt = (ref_base, ref_base) if cat == _abi.CAT_REFERENCE else variant(cat, k)
        alleles.append(dict(category=cat, ref=ref, alt=alt, support=min(cov, int(f * cov + rng.random())), coverage=cov, reference_support=0))
    if kind not in ("reference", "least first"):
        alleles.sort(key=lambda a: (a["ref"], a["alt"]))
    if kind == "reference" and rng.random() < 0.2:   # (the host-only entry takes a Reference row anywhere)
        alleles.append(alleles.pop(0))
    return alleles


def test_whole_loci_equal_the_transcription():
    rng = np.random.default_rng(4242)
    seen = set()
    for it in range(5000):
        alleles = random_locus(rng)
        low_depth = it % 2 == 0
        cfg = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE, min_coverage=100 if low_depth else 10, min_genotype_qscore=0 if it % 3 else 5,
                                  max_genotype_qscore=100 if it % 5 else 60)
        gt, out, post = engine.set_genotypes_adaptive(alleles, cfg)
        want_gt, want = R.set_genotypes(alleles, None, cfg.min_coverage, cfg.min_genotype_qscore, cfg.max_genotype_qscore)
        assert gt == want_gt, (alleles, gt, want_gt)
        for a, o, w, p in zip(alleles, out, want, post):
            assert {k: o[k] for k in o} == {k: w[k] for k in o}, (alleles, o, w)
            assert p["n"] == len(w["gp"]) and gp_close(p["gp"][: p["n"]], w["gp"]), (alleles, p, w["gp"])
        seen.add(gt)
        if gt == _abi.GT_HET_ALT1_ALT2:
            seen.add("1/2 over 500" if alleles[0]["coverage"] > 500 else "1/2")
    assert set(range(9)) <= seen and {"1/2", "1/2 over 500"} <= seen, seen


# ---- 4. the method the GPU tests rest on: somatic oracle rows + a per-locus genotyper = the reference's germline rows ------------------
def genotype_oracle_rows(rows, alleles, low_gq_filter, set_locus, forced_keys=()):
    """What the host pass of a flush does with the merged rows (AlleleCaller.ComputeGenotypeAndFilterAllele :143-177): per position, the rows
    that are not forced-report rows go to set_locus(list of allele dicts) -> list of dicts(genotype, genotype_qscore, phase_set_index,
    multi_allelic, prune[, gp]); pruned rows leave unless they are forced alleles.  Returns (rows, alleles, posteriors per row or None)."""
    out_rows, out_alleles, out_gp = [], [], []
    n = len(rows)
    i = 0
    while i < n:
        j = i
        while j < n and rows["position"][j] == rows["position"][i]:
            j += 1
        shown = [k for k in range(i, j) if not (int(rows["filter_bits"][k]) >> _abi.FILTER_FORCED_REPORT) & 1]
        res = set_locus([dict(category=(int(rows["info"][k]) >> 4) & 7, ref=alleles[k][0], alt=alleles[k][1], support=int(rows["allele_support"][k]),
                              coverage=int(rows["total_coverage"][k]), reference_support=int(rows["reference_support"][k])) for k in shown]) if shown else []
        for k in range(i, j):
            r = rows[k: k + 1].copy()
            gp = None
            if k in shown:
                a = res[shown.index(k)]
                if a["prune"] and (int(rows["position"][k]), alleles[k][0], alleles[k][1]) not in forced_keys:
                    continue
                gp = a.get("gp")
                r["info"] = (int(r["info"][0]) & ~0xF) | a["genotype"]
                r["genotype_qscore"] = a["genotype_qscore"]
                fb = int(r["filter_bits"][0]) & ~(1 << _abi.FILTER_LOW_GENOTYPE_QUALITY) & 0x3FFF
                if a["multi_allelic"]:
                    fb |= 1 << _abi.FILTER_MULTI_ALLELIC_SITE
                if low_gq_filter >= 0 and a["genotype_qscore"] < low_gq_filter:
                    fb |= 1 << _abi.FILTER_LOW_GENOTYPE_QUALITY
                r["filter_bits"] = fb | ((a["phase_set_index"] & 3) << 14)
            out_rows.append(r)
            out_alleles.append(alleles[k])
            out_gp.append(gp)
        i = j
    return (np.concatenate(out_rows) if out_rows else rows[:0]), out_alleles, out_gp


def adaptive_expected(rows, alleles, cfg, params=None, forced_keys=()):
    """Expected rows of an adaptive handle: somatic oracle rows genotyped locus by locus by tests/adaptive_ref.py"""
    return genotype_oracle_rows(rows, alleles, cfg.low_gq_filter,
                                lambda als: R.set_genotypes(als, params, cfg.min_coverage, cfg.min_genotype_qscore, cfg.max_genotype_qscore)[1], forced_keys)


def _thresholding_locus(cfg):
    def set_locus(als):
        n = len(als)
        arr = (_abi.PiscesGenotypeAllele * max(n, 1))()
        pool = bytearray()
        for i, a in enumerate(als):
            arr[i].category, arr[i].ref_len, arr[i].alt_len = a["category"], len(a["ref"]), len(a["alt"])
            arr[i].support, arr[i].coverage, arr[i].reference_support, arr[i].allele_offset = a["support"], a["coverage"], a["reference_support"], len(pool)
            pool += a["ref"].encode() + a["alt"].encode()
        pool_arr = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy()
        assert engine.lib.pisces_hip_set_genotypes(C.byref(cfg), arr, n, pool_arr.ctypes.data, len(pool)) >= 0
        return [dict(genotype=arr[i].genotype, genotype_qscore=arr[i].genotype_qscore, phase_set_index=arr[i].phase_set_index,
                     multi_allelic=bool(arr[i].multi_allelic), prune=bool(arr[i].prune)) for i in range(n)]
    return set_locus


@pytest.mark.parametrize("seed,with_deletion", [(501, True), (641, False)])
def test_somatic_oracle_rows_plus_a_locus_genotyper_are_the_germline_rows(seed, with_deletion):
    from tests.test_gpu_parity import _germline_reads, assert_records_match
    ref, reads = _germline_reads(seed, with_deletion=with_deletion)
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    kw = dict(min_frequency=0.2, variant_freq_filter=0.2, max_genotype_qscore=1000, block_size=2000)
    germ = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID, low_gq_filter=30, **kw)
    som = _abi.default_config(ploidy=_abi.PLOIDY_SOMATIC, low_gq_filter=-1, **kw)
    exp, exp_alleles, _, _ = orc.run_reads_full(batch, refa, 1, len(ref), germ)
    rows, alleles, _, _ = orc.run_reads_full(batch, refa, 1, len(ref), som)
    got, got_alleles, _ = genotype_oracle_rows(rows, alleles, germ.low_gq_filter, _thresholding_locus(germ))
    assert len(exp) > 1000 and {0, 2, 3, 4} <= set((exp["info"] & 15).tolist())
    assert got_alleles == exp_alleles
    assert_records_match(got, exp)
    assert (got["genotype_qscore"] == exp["genotype_qscore"]).all() and (got["filter_bits"] == exp["filter_bits"]).all()


# ---- 5. VCF ----------------------------------------------------------------------------------------------------------------------------
def _record(pos, ref, alt, gt, cat, cov, support, ref_support, q, gq, **kw):
    from tests.test_vcf_format import record
    return record(pos, ref, alt, gt, cat, cov, support, ref_support, q, gq, **kw)


def test_vcf_without_posteriors_is_the_existing_text():
    from tests import test_vcf_format as T
    checked = 0
    for spec in json.load(open(os.path.join(GOLDEN, "vcf_lines.json"))):
        for line in spec["lines"]:
            p = T._parse(line, spec)
            if p is None:
                continue
            r, alleles, f, decimals = p
            cfg = _abi.PiscesVcfConfig()
            assert engine.lib.pisces_hip_vcf_default_config(C.byref(cfg)) == 0
            cfg.variant_quality_filter = spec["q"] if spec["q"] is not None else 30
            cfg.min_frequency_threshold = 10.0 ** -(decimals - 1)
            cfg.output_no_call_fraction = int("NC" in f)
            cand = _abi.PiscesCandidate()
            cand.ref_len, cand.alt_len, cand.allele_offset = len(alleles[0]), len(alleles[1]), 0
            pool = np.frombuffer((alleles[0] + alleles[1]).encode() + b"\0", dtype=np.uint8).copy()
            idx = np.zeros(1, dtype=np.int32)
            a, b = C.create_string_buffer(4096), C.create_string_buffer(4096)
            chrom = line.split("\t")[0].encode()
            na = engine.lib.pisces_hip_format_vcf(C.byref(cfg), chrom, r.ctypes.data, 1, idx.ctypes.data, C.byref(cand), pool.ctypes.data, a, 4096)
            nb = engine.lib.pisces_hip_format_vcf_ex(C.byref(cfg), chrom, r.ctypes.data, 1, idx.ctypes.data, C.byref(cand), pool.ctypes.data, b, 4096, None)
            assert na == nb and na != 0 and (na < 0 or a.raw[:na] == b.raw[:nb]), line
            checked += 1
    assert checked > 300


def test_vcf_line_with_gp_of_the_writer_test():
    v = CASES["vcf_gp"]
    recs, alleles, post = [], [], np.zeros(len(v["alleles"]), dtype=_abi.POSTERIORS_DTYPE)
    for i, a in enumerate(v["alleles"]):
        recs.append(_record(a["ReferencePosition"], a["ReferenceAllele"], a["AlternateAllele"], GT_OF_NAME[a["Genotype"]], CAT_OF_NAME[a["category"]],
                            a["TotalCoverage"], a["AlleleSupport"], a["ReferenceSupport"], 0, 0, no_calls=a["NumNoCalls"]))
        alleles.append((a["ReferenceAllele"], a["AlternateAllele"]))
        post["n"][i] = len(a["GenotypePosteriors"])
        post["gp"][i][: post["n"][i]] = a["GenotypePosteriors"]
    c = v["config"]
    kw = dict(variant_quality_filter=int(c["VariantQualityFilterThreshold"]), min_frequency_threshold=float(c["MinFrequencyThreshold"]),
              frequency_filter_threshold=float(c["FrequencyFilterThreshold"]), noise_level=int(c["EstimatedBaseCallQuality"]),
              output_no_call_fraction=int(c["ShouldOutputNoCallFraction"] == "true"), crush=int(c["AllowMultipleVcfLinesPerLoci"] == "false"))
    assert engine.format_vcf(v["alleles"][0]["Chromosome"], np.concatenate(recs), alleles=alleles, posteriors=post, **kw) == v["line"] + "\n"
    # a first allele without posteriors: the line as it was
    post["n"][0] = 0
    assert engine.format_vcf("chr4", np.concatenate(recs), alleles=alleles, posteriors=post, **kw) == v["line"].replace(":GP", "").rsplit(":", 1)[0] + "\n"


def test_vcf_padding_rows_have_no_gp():
    a = _record(7, "C", "A", _abi.GT_HOM_ALT, _abi.CAT_SNV, cov=5394, support=2387, ref_support=7, q=0, gq=0)
    post = np.zeros(1, dtype=_abi.POSTERIORS_DTYPE)
    post["n"], post["gp"] = 3, [[100.0, 12.345, -0.0, 0, 0, 0]]
    kw = dict(variant_quality_filter=20, min_frequency_threshold=0.007, frequency_filter_threshold=0.007, noise_level=23, output_no_call_fraction=1)
    pad = dict(state=engine.new_pad_state(), reference=b"C" * 15, intervals=[(6, 8)], finish=True)
    lines = engine.format_vcf("chr4", a, alleles=[("C", "A")], pad=pad, posteriors=post, **kw).rstrip("\n").split("\n")
    assert [ln.split("\t")[1] for ln in lines] == ["6", "7", "8"]
    assert [ln.split("\t")[8].endswith(":GP") for ln in lines] == [False, True, False]
    assert lines[1].split("\t")[9].endswith(":0.0000:100.00,12.35,0.00") and lines[0].split("\t")[9].endswith(":0.0000")
    # and the same text as the entries without posteriors give when none are handed in
    pad2 = dict(state=engine.new_pad_state(), reference=b"C" * 15, intervals=[(6, 8)], finish=True)
    plain = engine.format_vcf("chr4", a, alleles=[("C", "A")], pad=pad2, **kw).rstrip("\n").split("\n")
    assert plain[0] == lines[0] and plain[2] == lines[2] and plain[1] == lines[1].replace(":GP", "").rsplit(":", 1)[0]


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
def test_create_takes_the_adaptive_ploidy():
    import torch
    h = C.c_void_p()
    cfg = _abi.default_config(ploidy=3, min_frequency=0.0)   # PISCES_PLOIDY_DIPLOID_ADAPTIVE
    rc = engine.lib.pisces_hip_create(C.byref(cfg), 0, C.byref(h))
    assert rc == (_abi.OK if torch.cuda.is_available() else _abi.E_DEVICE), rc
    if h.value:
        assert engine.lib.pisces_hip_destroy(h) == 0
    assert _abi.PLOIDY_DIPLOID_ADAPTIVE == 3
    cfg = _abi.default_config(ploidy=4)
    assert engine.lib.pisces_hip_create(C.byref(cfg), 0, C.byref(h)) == _abi.E_INVALID_ARG and not h.value


def test_parameter_validation():
    d = engine.adaptive_params()
    assert list(d.snv_model) == [0.037, 0.439, 0.976] and list(d.indel_model) == [0.037, 0.443, 0.905]
    assert list(d.snv_prior) == [0.755, 0.154, 0.0919] and list(d.indel_prior) == [0.962, 0.0266, 0.0114]
    assert F(d.sum_vf_for_multi_allelic_site) == F(0.80) and d.max_genotype_posteriors == 3000
    assert C.sizeof(_abi.PiscesAdaptiveParams) == 104 and C.sizeof(_abi.PiscesGenotypePosteriors) == 32 == _abi.POSTERIORS_DTYPE.itemsize
    assert engine.lib.pisces_hip_adaptive_default_params(None) == _abi.E_INVALID_ARG
    cfg = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE)
    one = [dict(category=_abi.CAT_SNV, ref="A", alt="C", support=40, coverage=100)]
    for bad in (dict(snv_model=(0.0, 0.5, 0.9)), dict(indel_model=(0.1, 0.5, 1.0)), dict(snv_model=(0.5, 0.4, 0.9)), dict(indel_model=(0.1, 0.9, 0.9)),
                dict(snv_prior=(0.9, 0.1, 0.0)), dict(indel_prior=(1.5, 0.1, 0.1)), dict(snv_model=(float("nan"), 0.5, 0.9))):
        with pytest.raises(engine.PiscesHipError) as e:
            engine.set_genotypes_adaptive(one, cfg, engine.adaptive_params(**bad))
        assert e.value.code == _abi.E_INVALID_ARG
        with pytest.raises(engine.PiscesHipError) as e:
            engine.adaptive_genotype_qscore(40, 100, params=engine.adaptive_params(**bad))
        assert e.value.code == _abi.E_INVALID_ARG
    with pytest.raises(engine.PiscesHipError):   # no alleles: alleles.First() of the reference throws
        engine.set_genotypes_adaptive([], cfg)
    with pytest.raises(engine.PiscesHipError):
        engine.adaptive_genotype_qscore(1, 0)
    assert engine.set_genotypes_adaptive(one, cfg)[0] == _abi.GT_HET_ALT_REF
