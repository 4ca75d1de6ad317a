// diploid.cpp — see diploid.h: the host form of genotype_core.h (alleles with their strings; the order among equal frequencies is the
// ordinal order of REF, then ALT).
#include "diploid.h"

#include <vector>

#include "genotype_core.h"

namespace pisces {
namespace {

struct Scratch {
    std::vector<genotype::Allele> a;
    std::vector<int> order;
    explicit Scratch(const std::vector<DiploidAllele>& in) : a(in.size()), order(in.size() + 1)
    {
        for (size_t i = 0; i < in.size(); i++) {
            genotype::Allele& g = a[i];
            g.category = in[i].category; g.support = in[i].support; g.coverage = in[i].coverage; g.ref_support = in[i].ref_support;
            g.genotype = 0; g.genotype_qscore = 0; g.phase_set_index = 0;
            g.multi_allelic = in[i].multi_allelic; g.prune = false;
        }
    }
    void back(std::vector<DiploidAllele>& out) const
    {
        for (size_t i = 0; i < out.size(); i++) {
            out[i].genotype = a[i].genotype; out[i].genotype_qscore = a[i].genotype_qscore; out[i].phase_set_index = a[i].phase_set_index;
            out[i].multi_allelic = a[i].multi_allelic; out[i].prune = a[i].prune;
        }
    }
};

}  // namespace

int32_t diploid_genotype_qscore(int32_t calledGT, int32_t totalCoverage, int32_t alleleSupport, int32_t minQScore, int32_t maxQScore)
{
    return genotype::diploid_qscore(calledGT, totalCoverage, alleleSupport, minQScore, maxQScore);
}

int32_t diploid_set_genotypes(std::vector<DiploidAllele>& alleles, const float snv[3], const float indel[3], int32_t minDepthToGenotype,
                              int32_t minGQ, int32_t maxGQ)
{
    Scratch s(alleles);
    auto before = [&](int x, int y) {
        if (alleles[(size_t)x].ref != alleles[(size_t)y].ref) return alleles[(size_t)x].ref < alleles[(size_t)y].ref;
        return alleles[(size_t)x].alt < alleles[(size_t)y].alt;
    };
    const int32_t gt = genotype::diploid_set(s.a.data(), (int)alleles.size(), s.order.data(), snv, indel, minDepthToGenotype, minGQ, maxGQ, before);
    s.back(alleles);
    return gt;
}

int32_t haploid_set_genotypes(std::vector<DiploidAllele>& alleles, float minorVF, float majorVF, int32_t minDepthToGenotype, int32_t minGQ,
                              int32_t maxGQ)
{
    Scratch s(alleles);
    auto before = [&](int x, int y) {
        if (alleles[(size_t)x].ref != alleles[(size_t)y].ref) return alleles[(size_t)x].ref < alleles[(size_t)y].ref;
        return alleles[(size_t)x].alt < alleles[(size_t)y].alt;
    };
    const int32_t gt = genotype::haploid_set(s.a.data(), (int)alleles.size(), s.order.data(), minorVF, majorVF, minDepthToGenotype, minGQ, maxGQ, before);
    s.back(alleles);
    return gt;
}

int32_t adaptive_set_genotypes(std::vector<DiploidAllele>& alleles, const PiscesAdaptiveParams& params, int32_t minDepthToGenotype, int32_t minGQ,
                               int32_t maxGQ, std::vector<PiscesGenotypePosteriors>& posteriors)
{
    Scratch s(alleles);
    auto before = [&](int x, int y) {
        if (alleles[(size_t)x].ref != alleles[(size_t)y].ref) return alleles[(size_t)x].ref < alleles[(size_t)y].ref;
        return alleles[(size_t)x].alt < alleles[(size_t)y].alt;
    };
    posteriors.assign(alleles.size(), PiscesGenotypePosteriors{});
    const int32_t gt = genotype::adaptive_set(s.a.data(), (int)alleles.size(), s.order.data(), params, minDepthToGenotype, minGQ, maxGQ, before, posteriors.data());
    s.back(alleles);
    return gt;
}

int32_t adaptive_genotype_qscore(const PiscesAdaptiveParams& params, int32_t category, bool is_reference, int32_t allele_support, int32_t total_coverage,
                                 int32_t* qscore, float gp[3])
{
    int ad, dp;
    genotype::adaptive_preprocess(is_reference, allele_support, total_coverage, ad, dp);
    return genotype::adaptive_qscore_and_posteriors(ad, dp, genotype::adaptive_model_of(params, category), genotype::adaptive_prior_of(params, category), *qscore, gp);
}

void adaptive_default_params(PiscesAdaptiveParams& p)
{
    const double snv_model[3] = {0.037, 0.439, 0.976}, indel_model[3] = {0.037, 0.443, 0.905};
    const double snv_prior[3] = {0.755, 0.154, 0.0919}, indel_prior[3] = {0.962, 0.0266, 0.0114};
    for (int i = 0; i < 3; i++) {
        p.snv_model[i] = snv_model[i]; p.indel_model[i] = indel_model[i];
        p.snv_prior[i] = snv_prior[i]; p.indel_prior[i] = indel_prior[i];
    }
    p.sum_vf_for_multi_allelic_site = 0.80f;
    p.max_genotype_posteriors = 3000;
}

bool adaptive_params_valid(const PiscesAdaptiveParams& p)
{
    const double* sets[4] = {p.snv_model, p.indel_model, p.snv_prior, p.indel_prior};
    for (int s = 0; s < 4; s++)
        for (int i = 0; i < 3; i++)
            if (!(sets[s][i] > 0.0 && sets[s][i] < 1.0)) return false;
    for (int s = 0; s < 2; s++)
        if (!(sets[s][0] < sets[s][1] && sets[s][1] < sets[s][2])) return false;
    return true;
}

}  // namespace pisces
