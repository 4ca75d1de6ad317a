// genotype_core.h — PloidyModel.DiploidByThresholding / Haploid / DiploidByAdaptiveGT for the alleles of ONE locus, one source for the host and the device
// (src/lib/Pisces.Genotyping/Thresholding/DiploidThresholdingGenotyper.cs:54-141, GenotypeCalculatorUtilities.cs:11-237, Adaptive/*.cs,
// DiploidGenotypeQualityCalculator.cs:12-105, Haploid/HaploidGenotyper.cs:36-83, HaploidGenotypeQualityCalculator.cs:10-59; the ln PMFs are
// MathNet.Numerics 4.5.1's Poisson.ProbabilityLn / Binomial.ProbabilityLn with its GammaLn / FactorialLn).
//   diploid.cpp                 the host form: the per-locus pass of a flush whose rows come from two kernels, pisces_hip_set_genotypes
//   genotype_loci_kernel,       (kernels.hip.h) lane = locus over the tile kernels' record slots: the device-resident surface and the
//   genotype_loci_adaptive_kernel flushes that have no candidate rows
// The alleles are plain records; the order of two alleles of equal frequency (ordinal order of their REF, then ALT strings) comes from the
// caller: strings on the host, the slot rank (A C G T) on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pisces_hip.h"

#if defined(__HIPCC__)
#define PISCES_GHD __host__ __device__
#else
#define PISCES_GHD
#endif

namespace pisces {
namespace genotype {

struct Allele {
    int32_t category;            // PISCES_CAT_*
    int32_t support, coverage, ref_support;
    // results
    int32_t genotype, genotype_qscore, phase_set_index;
    bool multi_allelic;          // FilterType.MultiAllelicSite
    bool prune;                  // the genotyper asks the caller to drop this allele
};

// MathNet.Numerics 4.5.1 SpecialFunctions.GammaLn (Lanczos, g = 10.900511) for z >= 0.5 (arguments here are counts + 1)
PISCES_GHD inline double gamma_ln(double z)
{
    const double dk[11] = {2.48574089138753565546e-5,  1.05142378581721974210,    -3.45687097222016235469,
                           4.51227709466894823700,     -2.98285225323576655721,   1.05639711577126713077,
                           -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
                           4.63399473359905636708e-6,  -2.71994908488607703910e-9};
    const double r = 10.900511, log_two_sqrt_e_over_pi = 0.6207822376352452223455184457816472122518527279025978, e = 2.7182818284590452354;
    double s = dk[0];
    for (int i = 1; i <= 10; i++) s += dk[i] / (z + i - 1.0);
    return log(s) + log_two_sqrt_e_over_pi + ((z - 0.5) * log((z - 0.5 + r) / e));
}
// SpecialFunctions.FactorialLn: the log of the cached factorial below 171, GammaLn(x + 1) from there
PISCES_GHD inline double factorial_ln(int x)
{
    if (x <= 1) return 0.0;
    if (x < 171) {
        double c = 1.0;
        for (int i = 2; i <= x; i++) c = c * i;
        return log(c);
    }
    return gamma_ln(x + 1.0);
}
PISCES_GHD inline double poisson_ln_pmf(double lambda, int k) { return -lambda + (k * log(lambda)) - factorial_ln(k); }   // Poisson.ProbabilityLn
PISCES_GHD inline double binomial_ln_pmf(double p, int n, int k)   // Binomial.ProbabilityLn
{
    const double ninf = -INFINITY;
    if (k < 0 || k > n) return ninf;
    if (p == 0.0) return k == 0 ? 0.0 : ninf;
    if (p == 1.0) return k == n ? 0.0 : ninf;
    return (factorial_ln(n) - factorial_ln(k) - factorial_ln(n - k)) + (k * log(p)) + ((n - k) * log(1.0 - p));
}
// CalledAllele.Frequency / RefFrequency (CalledAllele.cs:49-52,121-124)
PISCES_GHD inline float frequency_of(int32_t support, int32_t coverage)
{
    if (coverage == 0) return 0.0f;
    const float f = (float)support / (float)coverage;
    return f < 1.0f ? f : 1.0f;
}
PISCES_GHD inline int32_t clamp_q(double v, int32_t lo, int32_t hi)   // C#: (int) of a double, then Math.Max(Math.Min(q, max), min)
{
    const int32_t q = (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;
    const int32_t a = q < hi ? q : hi;
    return a > lo ? a : lo;
}

// DiploidGenotypeQualityCalculator.Compute
PISCES_GHD inline int32_t diploid_qscore(int32_t calledGT, int32_t totalCoverage, int32_t alleleSupport, int32_t minQScore, int32_t maxQScore)
{
    if (totalCoverage == 0) return minQScore;
    const float noiseHomRef = 0.05f, noiseHomAlt = 0.075f, noiseHetAlt = 0.10f, expectedHetFreq = 0.40f;
    const float depth = (float)totalCoverage;
    const float frequency = frequency_of(alleleSupport, totalCoverage);
    const int nonAlleleCalls = totalCoverage - alleleSupport > 0 ? totalCoverage - alleleSupport : 0;
    double h0 = 0, h1 = 0;
    switch (calledGT) {
    case PISCES_GT_HOM_REF:
        h0 = poisson_ln_pmf((double)(noiseHomRef * depth), nonAlleleCalls);
        h1 = binomial_ln_pmf((double)expectedHetFreq, totalCoverage, nonAlleleCalls);
        break;
    case PISCES_GT_HOM_ALT:
        h0 = poisson_ln_pmf((double)(noiseHomAlt * depth), nonAlleleCalls);
        h1 = binomial_ln_pmf((double)expectedHetFreq, totalCoverage, alleleSupport);
        break;
    case PISCES_GT_HET_ALT1_ALT2:
    case PISCES_GT_HET_ALT_REF: {
        const int k = (int)(depth * frequency);
        h0 = binomial_ln_pmf((double)expectedHetFreq, totalCoverage, k);
        h1 = frequency >= 0.50 ? binomial_ln_pmf((double)(1 - noiseHetAlt), totalCoverage, k) : binomial_ln_pmf((double)noiseHetAlt, totalCoverage, k);
        break;
    }
    default: return minQScore;
    }
    const double v = floor(10.0 * 0.4342944819032518 * (h0 - h1));   // Math.Log10(Math.E)
    if (h1 <= (double)INT32_MIN && h0 > h1) return maxQScore;
    if (h0 <= (double)INT32_MIN && h0 < h1) return minQScore;
    return clamp_q(v, minQScore, maxQScore);
}

// FilterAndOrderAllelesByFrequency: the variant alleles at or above the minor frequency, by descending frequency; `order` has room for n
// indices; before(x, y): allele x goes before allele y among equals (ordinal order of REF, then ALT).  Returns how many.
template <typename Before>
PISCES_GHD inline int order_by_frequency(Allele* a, int n, int* order, float minorVF, Before before)
{
    int nv = 0;
    for (int i = 0; i < n; i++) {
        a[i].prune = false;
        if (a[i].category == PISCES_CAT_REFERENCE) continue;
        const float fi = frequency_of(a[i].support, a[i].coverage);
        if (!((double)fi >= (double)minorVF)) { a[i].prune = true; continue; }
        int at = nv;   // insertion behind every allele that goes before this one (a stable sort of the arrival order)
        while (at > 0) {
            const int j = order[at - 1];
            const float fj = frequency_of(a[j].support, a[j].coverage);
            const bool j_first = fj != fi ? fj > fi : !before(i, j);
            if (j_first) break;
            order[at] = j;
            at--;
        }
        order[at] = i;
        nv++;
    }
    return nv;
}
// GetReferenceFrequency
PISCES_GHD inline double reference_frequency(const Allele* a, int n)
{
    if (n == 1) return frequency_of(a[0].ref_support, a[0].coverage);
    double refBySNP = 0, indelCount = 0;
    for (int i = 0; i < n; i++) {
        if (a[i].category == PISCES_CAT_REFERENCE) return frequency_of(a[i].support, a[i].coverage);
        if (a[i].category == PISCES_CAT_SNV) refBySNP = frequency_of(a[i].ref_support, a[i].coverage);
        else indelCount += frequency_of(a[i].support, a[i].coverage);
    }
    if (n < 1) return 0.0;
    return refBySNP - indelCount > 0.0 ? refBySNP - indelCount : 0.0;
}

// ConvertSimpleGenotypeToComplexGenotype with CheckForTriAllelicIssue and SetMultiAllelicFilter (GenotypeCalculatorUtilities.cs:135-234);
// prelim: 0 HomozygousRef, 1 HeterozygousAltRef, 2 HomozygousAlt; order[0..nv) = the variants by descending frequency
PISCES_GHD inline int32_t complex_genotype(Allele* a, int n, const int* order, int nv, double referenceFrequency, bool refExists, bool depthIssue, bool refCall,
                                           float minVarFrequency, float sumVFforMultiAllelicSite, int prelim)
{
    if (depthIssue) return refCall ? PISCES_GT_REF_LIKE_NOCALL : PISCES_GT_ALT_LIKE_NOCALL;
    if (prelim == 0) {
        if (!refExists) return PISCES_GT_REF_LIKE_NOCALL;
        return (n > 0 && a[0].category == PISCES_CAT_REFERENCE && (1 - frequency_of(a[0].support, a[0].coverage)) > minVarFrequency) ? PISCES_GT_REF_AND_NOCALL
                                                                                                                                   : PISCES_GT_HOM_REF;
    }
    if (prelim == 1) {
        if (nv == 1) return refExists ? PISCES_GT_HET_ALT_REF : PISCES_GT_ALT_AND_NOCALL;
        const float f0 = frequency_of(a[order[0]].support, a[order[0]].coverage);
        bool fail;   // CheckForTriAllelicIssue
        if (a[order[nv - 1]].category != PISCES_CAT_SNV) fail = false;
        else if (refExists && ((double)f0 + referenceFrequency) < (double)sumVFforMultiAllelicSite) fail = true;
        else fail = (f0 + frequency_of(a[order[1]].support, a[order[1]].coverage)) < sumVFforMultiAllelicSite;
        if (fail) {
            for (int i = 0; i < n; i++) a[i].multi_allelic = true;
            return refExists ? PISCES_GT_ALT_LIKE_NOCALL : PISCES_GT_ALT12_LIKE_NOCALL;
        }
        return refExists ? PISCES_GT_HET_ALT_REF : PISCES_GT_HET_ALT1_ALT2;
    }
    return PISCES_GT_HOM_ALT;
}
// GetAllelesToPruneBasedOnGTCall (GenotypeCalculatorUtilities.cs:11-47)
PISCES_GHD inline void prune_beyond_genotype(Allele* a, const int* order, int nv, int32_t gt)
{
    int allowed = 0;
    if (gt == PISCES_GT_ALT_AND_NOCALL || gt == PISCES_GT_ALT_LIKE_NOCALL || gt == PISCES_GT_HOM_ALT || gt == PISCES_GT_HET_ALT_REF) allowed = 1;
    else if (gt == PISCES_GT_ALT12_LIKE_NOCALL || gt == PISCES_GT_HET_ALT1_ALT2) allowed = 2;
    for (int k = allowed; k < nv; k++) a[order[k]].prune = true;
}

// DiploidThresholdingGenotyper.SetGenotypes over the alleles of one locus (Reference rows already gone when a variant is there);
// snv / indel = {MinorVF, MajorVF, SumVFforMultiAllelicSite}.  Returns the locus genotype.
template <typename Before>
PISCES_GHD inline int32_t diploid_set(Allele* a, int n, int* order, const float snv[3], const float indel[3], int32_t minDepthToGenotype, int32_t minGQ,
                                      int32_t maxGQ, Before before)
{
    const int nv = order_by_frequency(a, n, order, snv[0], before);
    const double referenceFrequency = reference_frequency(a, n);
    const bool refExists = referenceFrequency >= (double)snv[0];
    bool depthIssue = false;
    for (int i = 0; i < n; i++) depthIssue |= a[i].coverage < minDepthToGenotype;
    const float f0 = nv ? frequency_of(a[order[0]].support, a[order[0]].coverage) : 0.0f;
    const bool refCall = nv == 0 || f0 < snv[0];
    const float* par = (!refCall && a[order[0]].category != PISCES_CAT_SNV) ? indel : snv;   // SelectParameters
    int prelim = 0;   // GetPreliminaryGenotype: 0 HomozygousRef, 1 HeterozygousAltRef, 2 HomozygousAlt
    if (!refCall) prelim = (f0 >= par[0] && f0 <= par[1]) ? 1 : (f0 > par[1]) ? 2 : 0;
    const int32_t gt = complex_genotype(a, n, order, nv, referenceFrequency, refExists, depthIssue, refCall, par[0], par[2], prelim);
    prune_beyond_genotype(a, order, nv, gt);
    // SetGenotypes
    int phase = 1;
    for (int i = 0; i < n; i++) {
        a[i].genotype = gt;
        a[i].genotype_qscore = diploid_qscore(gt, a[i].coverage, a[i].support, minGQ, maxGQ);
        a[i].phase_set_index = a[i].category == PISCES_CAT_REFERENCE ? 0 : phase++;
    }
    return gt;
}

// HaploidGenotyper.SetGenotypes with HaploidGenotypeQualityCalculator; minorVF / majorVF are the SNV thresholding parameters
// (GenotypeCreator.cs:21-22)
template <typename Before>
PISCES_GHD inline int32_t haploid_set(Allele* a, int n, int* order, float minorVF, float majorVF, int32_t minDepthToGenotype, int32_t minGQ, int32_t maxGQ,
                                      Before before)
{
    const int nv = order_by_frequency(a, n, order, minorVF, before);
    const double referenceFrequency = reference_frequency(a, n);
    const bool refExists = referenceFrequency >= (double)minorVF;
    bool depthIssue = false;
    for (int i = 0; i < n; i++) depthIssue |= a[i].coverage < minDepthToGenotype;
    const float f0 = nv ? frequency_of(a[order[0]].support, a[order[0]].coverage) : 0.0f;
    const bool refCall = nv == 0 || f0 < minorVF;
    int32_t gt = PISCES_GT_HEMI_NOCALL;
    if (!depthIssue && refCall && refExists && referenceFrequency > (double)majorVF) gt = PISCES_GT_HEMI_REF;
    if (!depthIssue && !refCall && !refExists && f0 > majorVF) gt = PISCES_GT_HEMI_ALT;
    for (int k = gt == PISCES_GT_HEMI_ALT ? 1 : 0; k < nv; k++) a[order[k]].prune = true;
    for (int i = 0; i < n; i++) {
        a[i].genotype = gt;
        a[i].phase_set_index = 0;
        a[i].multi_allelic = false;
        // HaploidGenotypeQualityCalculator.Compute
        int32_t gq = minGQ;
        if (a[i].coverage != 0 && (gt == PISCES_GT_HEMI_REF || gt == PISCES_GT_HEMI_ALT)) {
            const float depth = (float)a[i].coverage;
            const int nonAlleleCalls = a[i].coverage - a[i].support > 0 ? a[i].coverage - a[i].support : 0;
            const double h0 = poisson_ln_pmf((double)((gt == PISCES_GT_HEMI_REF ? 0.05f : 0.075f) * depth), nonAlleleCalls);
            const double h1 = binomial_ln_pmf((double)0.40f, a[i].coverage, gt == PISCES_GT_HEMI_REF ? nonAlleleCalls : a[i].support);
            gq = clamp_q(floor(10.0 * 0.4342944819032518 * (h0 - h1)), minGQ, maxGQ);
        }
        a[i].genotype_qscore = gq;
    }
    return gt;
}

// ---- PloidyModel.DiploidByAdaptiveGT (Adaptive/DiploidAdaptiveGenotyper.cs:45-176, AdaptiveGenotyperCalculator.cs:18-82, MixtureModel.cs:281-346,
// 378-406, 449-518; MathNet.Numerics 4.5.1's Binomial.PMF, Normal.PDF and Multinomial.Probability restated) -----------------------------------
PISCES_GHD inline double binomial_pmf(double p, int n, int k) { return exp(binomial_ln_pmf(p, n, k)); }   // Binomial.PMF
PISCES_GHD inline double normal_pdf(double mean, double sd, double x)                                      // Normal.PDF
{
    const double d = (x - mean) / sd;
    return exp(-0.5 * d * d) / (2.5066282746310005024 * sd);
}
// Multinomial(p, n).Probability(x) over three classes: the rounded coefficient times the product of powers; p as given (not normalised)
PISCES_GHD inline double multinomial_probability(const double p[3], int n, const int x[3])
{
    if (x[0] + x[1] + x[2] != n) return 0.0;
    const double coef = floor(0.5 + exp(factorial_ln(n) - (factorial_ln(x[0]) + factorial_ln(x[1]) + factorial_ln(x[2]))));
    double num = 1.0;
    for (int i = 0; i < 3; i++) num *= pow(p[i], (double)x[i]);
    return coef * num;
}
// MathOperations.PToQ_CapAt300 (a float), and C#'s Math.Min(float, float) / (int) of a double
PISCES_GHD inline float p_to_q_cap_at_300(double p) { return p < 1e-300 ? 3000.0f : (float)(-10 * log10(p)); }
PISCES_GHD inline float min_f(float a, float b) { return (a < b || a != a) ? a : b; }
PISCES_GHD inline int32_t int_of(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; }
PISCES_GHD inline int32_t adaptive_q_of(double pWrong)   // Math.Min((int)_maxQScore, (int)Math.Round(PToQ_CapAt300(1 - posterior)))
{
    const int32_t q = int_of(rint((double)p_to_q_cap_at_300(pWrong)));
    return q < 100 ? q : 100;
}
// DiploidAdaptiveGenotyper.GetMinVarFrequency: the analytic frequency threshold at depth n (infinite or NaN at n = 0, as in the C#)
PISCES_GHD inline float adaptive_min_var_frequency(int n, const double model[3], const double priors[3])
{
    const double mu1 = model[0], mu2 = model[1], prior1 = priors[0], prior2 = priors[1];
    const double minVq = (log(prior2) - log(prior1) - n * log(1 - mu1) + n * log(1 - mu2)) / (log(mu1) - log(1 - mu1) - log(mu2) + log(1 - mu2)) / n;
    return (float)minVq;
}
// AdaptiveGenotyperCalculator.PreprocessCalledAllele: allele depth and depth as the mixture sees them (at most 1000)
PISCES_GHD inline void adaptive_preprocess(bool isReference, int32_t support, int32_t coverage, int& ad, int& dp)
{
    dp = coverage;
    ad = isReference ? (dp - support > 0 ? dp - support : 0) : support;
    if (dp > 1000) {
        ad = (int)((double)ad / dp * 1000);
        dp = 1000;
    }
    if (ad > dp) ad = dp;
}
// MixtureModel.CalculatePosteriors (:319-346), the Normal.PDF fallback as written
PISCES_GHD inline void adaptive_posteriors(const int k[3], const int n[3], const double means[3], const double priors[3], double post[3])
{
    double temp[3], sum = 0;
    for (int i = 0; i < 3; i++) {
        temp[i] = binomial_pmf(means[i], n[i], k[i]) * priors[i];
        sum += temp[i];
        if (i == 2 && sum == 0) {
            for (int ii = 0; ii < 3; ii++) {
                temp[ii] = normal_pdf(means[ii], sqrt(n[i] * means[ii] * (1 - means[ii])), (double)k[i] / n[i]);
                sum += temp[ii];
            }
        }
    }
    for (int i = 0; i < 3; i++) post[i] = temp[i] / sum;
}
// MixtureModel.GetSimplifiedGenotype: the first index of the largest posterior (Enumerable.Max passes over NaN; Array.IndexOf)
PISCES_GHD inline int adaptive_category(int ad, int dp, const double means[3], const double priors[3])
{
    const int k[3] = {ad, ad, ad}, n[3] = {dp, dp, dp};
    double post[3];
    adaptive_posteriors(k, n, means, priors, post);
    int cat = 0;
    for (int i = 1; i < 3; i++)
        if (post[i] > post[cat] || (post[cat] != post[cat] && post[i] == post[i])) cat = i;
    return cat;
}
// MixtureModel.CalculateQScoreAndGenotypePosteriors (:281-317, 389-406) with the default effective depths {25, 25, 10}: the category, the
// unclamped q-score, three phred-scaled posteriors
PISCES_GHD inline int adaptive_qscore_and_posteriors(int ad, int dp, const double means[3], const double priors[3], int32_t& qscore, float gp[3])
{
    const int cat = adaptive_category(ad, dp, means, priors);
    const int maxN[3] = {25, 25, 10};
    int k[3], n[3];
    for (int i = 0; i < 3; i++) {
        if (dp > maxN[i]) {
            const double vf = (double)ad / dp;
            k[i] = int_of(rint(vf * maxN[i]));
            n[i] = maxN[i];
        } else {
            k[i] = ad;
            n[i] = dp;
        }
    }
    double post[3];
    adaptive_posteriors(k, n, means, priors, post);
    for (int i = 0; i < 3; i++) gp[i] = min_f(100.0f, p_to_q_cap_at_300(post[i]));
    qscore = adaptive_q_of(1 - post[cat]);
    return cat;
}
// AdaptiveGenotyperCalculator.GetMultiAllelicQScores + MixtureModel.GetMultinomialQScores: six posteriors and the q-score of a 1/2 locus
// from its first two alleles (in input order); means1 / means2 are their models
PISCES_GHD inline void adaptive_multinomial(int32_t support1, int32_t support2, int32_t totalCoverage, const double means1[3], const double means2[3],
                                            int32_t& qscore, float gp[6])
{
    const int dp = totalCoverage;
    int ad[3];
    ad[2] = support2;
    ad[1] = support1;
    ad[0] = dp - ad[1] - ad[2] > 0 ? dp - ad[1] - ad[2] : 0;
    if (dp > 500) {   // "Can't be calculated"
        for (int i = 0; i < 6; i++) gp[i] = i == 4 ? 0.0f : 100.0f;
        qscore = 100;
        return;
    }
    double temp[6], norm = 0;
    int count = 0;
    for (int m2 = 0; m2 < 3; m2++) {
        for (int m1 = 0; m1 < 3; m1++) {
            if ((m1 == 2 && m2 != 0) || (m2 == 2 && m1 != 0)) continue;   // either allele hom-alt and the other not hom-ref
            double p[3];
            p[1] = means1[m1];
            p[2] = means2[m2];
            p[0] = 1 - p[1] - p[2];
            if (p[0] <= 0) {
                if (m1 == 2) p[0] = 1 - p[1];
                else if (m2 == 2) p[0] = 1 - p[2];
                else if (m1 == 1 && m2 == 1) p[0] = 1 - means1[2];
            }
            const double prior = (m1 == 0 && m2 == 0) ? 0.99 : 0.01 / 5;
            temp[count] = multinomial_probability(p, dp, ad) * prior;
            norm = norm + temp[count];
            count++;
        }
    }
    for (int i = 0; i < 6; i++) gp[i] = min_f(100.0f, p_to_q_cap_at_300(temp[i] / norm));
    qscore = adaptive_q_of(1 - temp[4] / norm);
}
// AdaptiveGenotypingParameters.GetModelsAndPriors: SNV / Reference / MNV the SNV pair, insertions / deletions the indel pair
PISCES_GHD inline const double* adaptive_model_of(const PiscesAdaptiveParams& A, int32_t category)
{
    return (category == PISCES_CAT_INSERTION || category == PISCES_CAT_DELETION) ? A.indel_model : A.snv_model;
}
PISCES_GHD inline const double* adaptive_prior_of(const PiscesAdaptiveParams& A, int32_t category)
{
    return (category == PISCES_CAT_INSERTION || category == PISCES_CAT_DELETION) ? A.indel_prior : A.snv_prior;
}
PISCES_GHD inline int32_t clamp_gq(int32_t q, int32_t lo, int32_t hi)   // Math.Max(Math.Min(q, max), min)
{
    const int32_t v = q < hi ? q : hi;
    return v > lo ? v : lo;
}

// DiploidAdaptiveGenotyper.SetGenotypes over the alleles of one locus, n >= 1, in input order; out[i] receives allele i's posteriors (every
// allele's, the pruned ones included).  Returns the locus genotype.
template <typename Before>
PISCES_GHD inline int32_t adaptive_set(Allele* a, int n, int* order, const PiscesAdaptiveParams& A, int32_t minDepthToGenotype, int32_t minGQ, int32_t maxGQ,
                                       Before before, PiscesGenotypePosteriors* out)
{
    // CalculateDiploidGenotypeFromBinomialModel
    float minVariantFrequency = adaptive_min_var_frequency(a[0].coverage, A.snv_model, A.snv_prior);
    double referenceFrequency = 1;   // the genotyper's own GetReferenceFrequency (:146-159)
    bool sawReference = false;
    for (int i = 0; i < n && !sawReference; i++) {
        if (a[i].category == PISCES_CAT_REFERENCE) {
            referenceFrequency = frequency_of(a[i].support, a[i].coverage);
            sawReference = true;
        } else referenceFrequency = referenceFrequency - frequency_of(a[i].support, a[i].coverage);
    }
    if (!sawReference) referenceFrequency = referenceFrequency > 0 ? referenceFrequency : 0;
    bool depthIssue = false;
    for (int i = 0; i < n; i++) depthIssue |= a[i].coverage < minDepthToGenotype;
    const bool refExists = referenceFrequency > (double)minVariantFrequency;
    const int nv = order_by_frequency(a, n, order, minVariantFrequency, before);
    const bool refCall = nv == 0;
    int prelim = 0;
    if (!refCall) {
        const Allele& d = a[order[0]];
        const double* model = adaptive_model_of(A, d.category);
        const double* priors = adaptive_prior_of(A, d.category);
        int ad, dp;
        adaptive_preprocess(d.category == PISCES_CAT_REFERENCE, d.support, d.coverage, ad, dp);
        prelim = adaptive_category(ad, dp, model, priors);
        minVariantFrequency = adaptive_min_var_frequency(d.coverage, model, priors);
    }
    const int32_t gt = complex_genotype(a, n, order, nv, referenceFrequency, refExists, depthIssue, refCall, minVariantFrequency,
                                        A.sum_vf_for_multi_allelic_site, prelim);
    prune_beyond_genotype(a, order, nv, gt);
    // SetGenotypes
    int phase = 1;
    for (int i = 0; i < n; i++) {
        a[i].genotype = gt;
        PiscesGenotypePosteriors& o = out[i];
        o.n = 3;
        o.reserved = 0;
        o.gp[3] = o.gp[4] = o.gp[5] = 0.0f;
        if (a[i].coverage == 0) {
            a[i].genotype_qscore = minGQ;
            o.gp[0] = o.gp[1] = o.gp[2] = (float)A.max_genotype_posteriors;
        } else {
            int ad, dp;
            adaptive_preprocess(a[i].category == PISCES_CAT_REFERENCE, a[i].support, a[i].coverage, ad, dp);
            int32_t q;
            (void)adaptive_qscore_and_posteriors(ad, dp, adaptive_model_of(A, a[i].category), adaptive_prior_of(A, a[i].category), q, o.gp);
            a[i].genotype_qscore = clamp_gq(q, minGQ, maxGQ);
        }
        a[i].phase_set_index = a[i].category == PISCES_CAT_REFERENCE ? 0 : phase++;
    }
    if (gt == PISCES_GT_HET_ALT1_ALT2) {   // the multinomial over alleles.First() and alleles.ElementAt(1), for every allele of the locus
        int32_t q;
        float gp[6];
        adaptive_multinomial(a[0].support, a[1].support, a[0].coverage, adaptive_model_of(A, a[0].category), adaptive_model_of(A, a[1].category), q, gp);
        for (int i = 0; i < n; i++) {
            a[i].genotype_qscore = clamp_gq(q, minGQ, maxGQ);
            out[i].n = 6;
            for (int j = 0; j < 6; j++) out[i].gp[j] = gp[j];
        }
    }
    return gt;
}

}  // namespace genotype
}  // namespace pisces
