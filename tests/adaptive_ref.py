"""PloidyModel.DiploidByAdaptiveGT in plain Python: the yardstick of tests/test_adaptive_cpu.py and tests/test_adaptive_gpu.py.

A statement, formula by formula, of
  src/lib/Pisces.Genotyping/Adaptive/DiploidAdaptiveGenotyper.cs:45-176   SetGenotypes, CalculateDiploidGenotypeFromBinomialModel
  src/lib/Pisces.Genotyping/Adaptive/AdaptiveGenotyperCalculator.cs:18-82 PreprocessCalledAllele, GetMultiAllelicQScores
  src/lib/Pisces.Genotyping/Adaptive/MixtureModel.cs:281-346,378-406,449-518
  src/lib/Pisces.Genotyping/GenotypeCalculatorUtilities.cs:11-234         ordering, tri-allelic test, simple -> complex genotype, pruning
  src/lib/Pisces.Calculators/stats/MathOperations.cs:17-23                PToQ_CapAt300
with MathNet.Numerics 4.5.1's Binomial.PMF, Normal.PDF, Multinomial.Probability, FactorialLn and GammaLn restated (the package's source
is not part of the reference tree).  double where the C# has double, numpy.float32 where it has float.  It shares no code with the
library; tests/test_adaptive_cpu.py first holds it to the reference's own tables (tests/golden/adaptive_cases.json)."""
import math

import numpy as np

F = np.float32
CAT_SNV, CAT_INSERTION, CAT_DELETION, CAT_MNV, CAT_REFERENCE = range(5)
(GT_HET_ALT1_ALT2, GT_ALT12_LIKE_NOCALL, GT_HET_ALT_REF, GT_HOM_ALT, GT_HOM_REF, GT_REF_LIKE_NOCALL, GT_ALT_LIKE_NOCALL, GT_REF_AND_NOCALL,
 GT_ALT_AND_NOCALL) = range(9)
INT_MIN = -2 ** 31

DEFAULT_PARAMS = dict(snv_model=(0.037, 0.439, 0.976), indel_model=(0.037, 0.443, 0.905), snv_prior=(0.755, 0.154, 0.0919),
                      indel_prior=(0.962, 0.0266, 0.0114), sum_vf=F(0.80), max_gp=3000)

_DK = (2.48574089138753565546e-5, 1.05142378581721974210, -3.45687097222016235469, 4.51227709466894823700, -2.98285225323576655721,
       1.05639711577126713077, -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
       4.63399473359905636708e-6, -2.71994908488607703910e-9)


def gamma_ln(z):   # SpecialFunctions.GammaLn, z >= 0.5
    s = _DK[0]
    for i in range(1, 11):
        s += _DK[i] / (z + i - 1.0)
    return math.log(s) + 0.6207822376352452223455184457816472122518527279025978 + ((z - 0.5) * math.log((z - 0.5 + 10.900511) / 2.7182818284590452354))


_FACT_LN = {}


def factorial_ln(x):   # SpecialFunctions.FactorialLn: log of the cached factorial below 171
    if x <= 1:
        return 0.0
    v = _FACT_LN.get(x)
    if v is None:
        if x < 171:
            c = 1.0
            for i in range(2, x + 1):
                c = c * i
            v = math.log(c)
        else:
            v = gamma_ln(x + 1.0)
        _FACT_LN[x] = v
    return v


def binomial_pmf(p, n, k):   # Binomial.PMF
    if k < 0 or k > n:
        return 0.0
    if p == 0.0:
        return 1.0 if k == 0 else 0.0
    if p == 1.0:
        return 1.0 if k == n else 0.0
    return math.exp((factorial_ln(n) - factorial_ln(k) - factorial_ln(n - k)) + (k * math.log(p)) + ((n - k) * math.log(1.0 - p)))


def normal_pdf(mean, sd, x):   # Normal.PDF
    d = (x - mean) / sd
    return math.exp(-0.5 * d * d) / (2.5066282746310005024 * sd)


def multinomial_probability(p, n, x):   # Multinomial(p, n).Probability(x); p as given
    if sum(x) != n:
        return 0.0
    coef = math.floor(0.5 + math.exp(factorial_ln(n) - sum(factorial_ln(v) for v in x)))
    num = 1.0
    for pi, xi in zip(p, x):
        num *= math.pow(pi, float(xi))
    return coef * num


def p_to_q_cap_at_300(p):   # MathOperations.PToQ_CapAt300: a float
    if p < 1e-300:
        return F(3000.0)
    return F(-10 * math.log10(p))


def _int_of(v):   # (int) of a double in C#
    if v != v or v >= 2147483648.0 or v <= -2147483649.0:
        return INT_MIN
    return int(v)


def _q_of(p_wrong):   # Math.Min(100, (int)Math.Round(PToQ_CapAt300(p)))
    q = float(p_to_q_cap_at_300(p_wrong))
    q = _int_of(float(round(q))) if q == q else INT_MIN   # round(): half to even, as Math.Round
    return min(100, q)


def _min_f(a, b):   # Math.Min(float, float): NaN if either is
    if a != a or b != b:
        return F(np.nan)
    return a if a < b else b


def frequency(support, coverage):   # CalledAllele.Frequency
    if coverage == 0:
        return F(0.0)
    f = F(support) / F(coverage)
    return f if f < F(1.0) else F(1.0)


def min_var_frequency(n, model, priors):   # DiploidAdaptiveGenotyper.GetMinVarFrequency: (float) of a double; n = 0 divides by zero
    mu1, mu2, prior1, prior2 = model[0], model[1], priors[0], priors[1]
    with np.errstate(all="ignore"):
        v = (np.float64(math.log(prior2) - math.log(prior1) - n * math.log(1 - mu1) + n * math.log(1 - mu2)) /
             np.float64(math.log(mu1) - math.log(1 - mu1) - math.log(mu2) + math.log(1 - mu2))) / np.float64(n)
        return F(v)


def preprocess(is_reference, support, coverage):   # AdaptiveGenotyperCalculator.PreprocessCalledAllele
    dp = coverage
    ad = max(dp - support, 0) if is_reference else support
    if dp > 1000:
        ad = int(float(ad) / dp * 1000)
        dp = 1000
    if ad > dp:
        ad = dp
    return ad, dp


def posteriors(ks, ns, means, priors):   # MixtureModel.CalculatePosteriors :319-346
    temp = [0.0, 0.0, 0.0]
    total = 0.0
    for i in range(3):
        temp[i] = binomial_pmf(means[i], ns[i], ks[i]) * priors[i]
        total += temp[i]
        if i == 2 and total == 0:
            for ii in range(3):
                temp[ii] = normal_pdf(means[ii], math.sqrt(ns[i] * means[ii] * (1 - means[ii])), float(ks[i]) / ns[i])
                total += temp[ii]
    with np.errstate(all="ignore"):
        return [float(np.float64(t) / np.float64(total)) for t in temp]


def category(ad, dp, means, priors):   # MixtureModel.GetSimplifiedGenotype: first index of the largest posterior
    post = posteriors([ad] * 3, [dp] * 3, means, priors)
    real = [p for p in post if p == p]
    if not real:
        return 0
    return post.index(max(real))


def qscore_and_posteriors(ad, dp, means, priors):   # MixtureModel.CalculateQScoreAndGenotypePosteriors, effective depths {25, 25, 10}
    cat = category(ad, dp, means, priors)
    ks, ns = [], []
    for max_n in (25, 25, 10):
        if dp > max_n:
            vf = float(ad) / dp
            ks.append(int(round(vf * max_n)))
            ns.append(max_n)
        else:
            ks.append(ad)
            ns.append(dp)
    post = posteriors(ks, ns, means, priors)
    gp = np.array([_min_f(F(100.0), p_to_q_cap_at_300(p)) for p in post], dtype=F)
    return cat, _q_of(1 - post[cat]), gp


def multinomial_qscores(support1, support2, total_coverage, means1, means2):   # GetMultiAllelicQScores + GetMultinomialQScores
    dp = total_coverage
    ad = [max(dp - support1 - support2, 0), support1, support2]
    if dp > 500:
        return 100, np.array([100, 100, 100, 100, 0, 100], dtype=F)
    temp = []
    norm = 0.0
    for m2 in range(3):
        for m1 in range(3):
            if (m1 == 2 and m2 != 0) or (m2 == 2 and m1 != 0):
                continue
            p = [0.0, means1[m1], means2[m2]]
            p[0] = 1 - p[1] - p[2]
            if p[0] <= 0:
                if m1 == 2:
                    p[0] = 1 - p[1]
                elif m2 == 2:
                    p[0] = 1 - p[2]
                elif m1 == 1 and m2 == 1:
                    p[0] = 1 - means1[2]
            prior = 0.99 if (m1 == 0 and m2 == 0) else 0.01 / 5
            temp.append(multinomial_probability(p, dp, ad) * prior)
            norm = norm + temp[-1]
    with np.errstate(all="ignore"):
        ratio = [float(np.float64(t) / np.float64(norm)) for t in temp]
    gp = np.array([_min_f(F(100.0), p_to_q_cap_at_300(r)) for r in ratio], dtype=F)
    return _q_of(1 - ratio[4]), gp


def model_of(params, cat):
    indel = cat in (CAT_INSERTION, CAT_DELETION)
    return (params["indel_model"], params["indel_prior"]) if indel else (params["snv_model"], params["snv_prior"])


def set_genotypes(alleles, params=None, min_depth=10, min_gq=0, max_gq=100):
    """DiploidAdaptiveGenotyper.SetGenotypes.  alleles: list of dicts(category, ref, alt, support, coverage), at least one, in input order.
    Returns (locus genotype, [dict(genotype, genotype_qscore, phase_set_index, multi_allelic, prune, gp = float32 array of 3 or 6)])."""
    A = params or DEFAULT_PARAMS
    n = len(alleles)
    freq = [frequency(a["support"], a["coverage"]) for a in alleles]
    min_vf = min_var_frequency(alleles[0]["coverage"], A["snv_model"], A["snv_prior"])
    # the genotyper's own GetReferenceFrequency
    ref_freq = 1.0
    saw_ref = False
    for a, f in zip(alleles, freq):
        if a["category"] == CAT_REFERENCE:
            ref_freq = float(f)
            saw_ref = True
            break
        ref_freq = ref_freq - float(f)
    if not saw_ref:
        ref_freq = max(ref_freq, 0)
    depth_issue = any(a["coverage"] < min_depth for a in alleles)
    ref_exists = ref_freq > float(min_vf)
    # FilterAndOrderAllelesByFrequency
    prune = [False] * n
    variants = []
    for i, a in enumerate(alleles):
        if a["category"] == CAT_REFERENCE:
            continue
        if float(freq[i]) >= float(min_vf):
            variants.append(i)
        else:
            prune[i] = True
    variants.sort(key=lambda i: (-float(freq[i]), alleles[i]["ref"], alleles[i]["alt"]))
    ref_call = not variants
    prelim = 0
    if not ref_call:
        d = alleles[variants[0]]
        model, priors = model_of(A, d["category"])
        ad, dp = preprocess(d["category"] == CAT_REFERENCE, d["support"], d["coverage"])
        prelim = category(ad, dp, model, priors)
        min_vf = min_var_frequency(d["coverage"], model, priors)
    # ConvertSimpleGenotypeToComplexGenotype
    multi = False
    if depth_issue:
        gt = GT_REF_LIKE_NOCALL if ref_call else GT_ALT_LIKE_NOCALL
    elif prelim == 0:
        if not ref_exists:
            gt = GT_REF_LIKE_NOCALL
        elif alleles[0]["category"] == CAT_REFERENCE and (F(1) - freq[0]) > min_vf:
            gt = GT_REF_AND_NOCALL
        else:
            gt = GT_HOM_REF
    elif prelim == 1:
        sum_vf = F(A["sum_vf"])
        fail = False
        if len(variants) > 1:   # CheckForTriAllelicIssue
            f0 = freq[variants[0]]
            if alleles[variants[-1]]["category"] != CAT_SNV:
                fail = False
            elif ref_exists and (float(f0) + ref_freq) < float(sum_vf):
                fail = True
            else:
                fail = bool(F(f0 + freq[variants[1]]) < sum_vf)
        if len(variants) == 1:
            gt = GT_HET_ALT_REF if ref_exists else GT_ALT_AND_NOCALL
        elif fail:
            multi = True
            gt = GT_ALT_LIKE_NOCALL if ref_exists else GT_ALT12_LIKE_NOCALL
        else:
            gt = GT_HET_ALT_REF if ref_exists else GT_HET_ALT1_ALT2
    else:
        gt = GT_HOM_ALT
    allowed = 1 if gt in (GT_ALT_AND_NOCALL, GT_ALT_LIKE_NOCALL, GT_HOM_ALT, GT_HET_ALT_REF) else 2 if gt in (GT_ALT12_LIKE_NOCALL, GT_HET_ALT1_ALT2) else 0
    for i in variants[allowed:]:
        prune[i] = True
    out = []
    phase = 1
    for i, a in enumerate(alleles):
        if a["coverage"] == 0:
            q = min_gq
            gp = np.array([A["max_gp"]] * 3, dtype=F)
        else:
            model, priors = model_of(A, a["category"])
            ad, dp = preprocess(a["category"] == CAT_REFERENCE, a["support"], a["coverage"])
            _, q, gp = qscore_and_posteriors(ad, dp, model, priors)
            q = max(min(q, max_gq), min_gq)
        if a["category"] == CAT_REFERENCE:
            ps = 0
        else:
            ps = phase
            phase += 1
        out.append(dict(genotype=gt, genotype_qscore=q, phase_set_index=ps, multi_allelic=multi or bool(a.get("multi_allelic", False)), prune=prune[i], gp=gp))
    if gt == GT_HET_ALT1_ALT2:
        a1, a2 = alleles[0], alleles[1]
        q, gp = multinomial_qscores(a1["support"], a2["support"], a1["coverage"], model_of(A, a1["category"])[0], model_of(A, a2["category"])[0])
        for o in out:
            o["genotype_qscore"] = max(min(q, max_gq), min_gq)
            o["gp"] = gp
    return gt, out


def qscore_table(ad, dp, means, priors):
    """qscore_and_posteriors over arrays of (allele depth, depth) after preprocess (depth 1..1000): the same operations on numpy float64
    vectors (numpy's exp / log10 where the scalar form has math's); an entry whose posterior sum is zero takes the scalar form.  Returns
    (category, q-score, posteriors [n][3] float32)."""
    ad = np.asarray(ad, dtype=np.int64)
    dp = np.asarray(dp, dtype=np.int64)
    fl = np.array([factorial_ln(i) for i in range(1001)])
    lp = [math.log(m) for m in means]
    lq = [math.log(1.0 - m) for m in means]

    def post_of(ks, ns):
        temp = []
        for i in range(3):
            k, n = ks[i], ns[i]
            temp.append(np.exp((fl[n] - fl[k] - fl[n - k]) + (k * lp[i]) + ((n - k) * lq[i])) * priors[i])
        total = (temp[0] + temp[1]) + temp[2]
        with np.errstate(all="ignore"):
            return np.stack([t / total for t in temp], axis=1), total == 0

    p1, z1 = post_of([ad] * 3, [dp] * 3)
    cat = np.argmax(p1, axis=1)
    ks, ns = [], []
    for max_n in (25, 25, 10):
        big = dp > max_n
        ks.append(np.where(big, np.rint(ad.astype(np.float64) / dp * max_n).astype(np.int64), ad))
        ns.append(np.where(big, max_n, dp))
    p2, z2 = post_of(ks, ns)
    wrong = 1 - p2[np.arange(len(ad)), cat]
    with np.errstate(all="ignore"):
        def ptoq(p):
            return np.where(p < 1e-300, F(3000.0), (-10 * np.log10(np.where(p < 1e-300, 1.0, p))).astype(F)).astype(F)
        q = np.minimum(100, np.rint(ptoq(wrong).astype(np.float64)).astype(np.int64))
        gp = np.minimum(F(100.0), ptoq(p2)).astype(F)
    for i in np.nonzero(z1 | z2)[0].tolist():
        cat[i], q[i], gp[i] = qscore_and_posteriors(int(ad[i]), int(dp[i]), means, priors)
    return cat, q, gp
