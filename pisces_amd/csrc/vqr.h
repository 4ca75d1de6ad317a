// vqr.h — VariantQualityRecalibration (src/exe/VariantQualityRecalibration/) over the 64-byte rows: the decisions of its three passes,
// one source for the host and the device, as indel_repeat.h, amplicon_bias.h and exact_span.h are for theirs.
//   surface_vqr.inc.h     the host forms: pisces_hip_vqr_count, pisces_hip_vqr_tables
//   vqr_kernels.hip.h     the device forms: vqr_count_kernel, vqr_apply_kernel
// What is restated:
//   count_category    MutationCategoryUtil.GetMutationCategory (MutationCategory.cs:41-81), what CountData.Add (CountData.cs:59-76) and
//                     EdgeIssueCountData.Add (EdgeIssueCountData.cs:30-57) count by: the alleles alone, no filter is looked at
//   update_category   MutationCounter.GetMutationCategory(CalledAllele) (MutationCounter.cs:133-172): a ForcedReport row is Other
//   at_edge           EdgeIssueCountData.DidWeDetectAnEdge (EdgeIssueCountData.cs:67-118) over the E rows before and after a row
//   rates / edge_risk GetPhredScaledCalibratedRates / GetPhredScaledCalibratedRatesForEdges (QualityRecalibration.cs:276-381)
//   update_row        UpdateAllele + UpdateVariantQScoreAndRefilter + InsertNewQ + HaveInfoToUpdateQ (QualityRecalibration.cs:131-155, 197-274),
//                     VariantQualityCalculator.AssignPoissonQScore passed in as a callable (the device has poisson_qscore_core, the host has none)
// A row is read through its words: w60 = the dword at byte 60, filter_bits in the low half, info in the high half.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pisces_hip.h"

#if defined(__HIPCC__)
#define PISCES_VHD __host__ __device__
#else
#define PISCES_VHD
#endif

namespace pisces {
namespace vqr {

// MutationCategory (MutationCategory.cs:12-30), index = enum value - 1: AtoC AtoG AtoT CtoA CtoG CtoT GtoA GtoC GtoT TtoA TtoC TtoG, then
constexpr int32_t kInsertion = 12, kDeletion = 13, kReference = 14, kOther = 15, kCategories = 16, kSnvCategories = 12;
constexpr int32_t kIntMin = (int32_t)0x80000000;   // what the C# (int) cast makes of NaN and of the infinities
constexpr int32_t kMaxExtent = 64;                 // extent_of_edge_region the entries accept

PISCES_VHD inline uint32_t w60_of(uint16_t filter_bits, uint16_t info) { return (uint32_t)filter_bits | ((uint32_t)info << 16); }

// AlleleType codes are A G C T (pisces_hip.h); the enum's order is alphabetical
PISCES_VHD inline int32_t alphabetical(int32_t code) { return code == PISCES_ALLELE_A ? 0 : code == PISCES_ALLELE_C ? 1 : code == PISCES_ALLELE_G ? 2 : code == PISCES_ALLELE_T ? 3 : -1; }

PISCES_VHD inline int32_t count_category(uint32_t w60)
{
    const uint32_t info = w60 >> 16;
    const int32_t cat = (int32_t)PISCES_INFO_CATEGORY(info);
    if (cat == PISCES_CAT_REFERENCE) return kReference;   // :45
    if (cat == PISCES_CAT_DELETION) return kDeletion;     // refLength > altLength (:59)
    if (cat == PISCES_CAT_INSERTION) return kInsertion;   // :62
    if (cat != PISCES_CAT_SNV) return kOther;             // an MNV: equal lengths above 1 (:65)
    const int32_t r = (int32_t)PISCES_INFO_REF(info), a = (int32_t)PISCES_INFO_ALT(info);
    if (r == a) return kReference;                        // :68-70
    const int32_t ri = alphabetical(r), ai = alphabetical(a);
    if (ri < 0 || ai < 0) return kOther;                  // N: no enum name matches (:80)
    return ri * 3 + ai - (ai > ri ? 1 : 0);
}

PISCES_VHD inline int32_t update_category(uint32_t w60)
{
    if (w60 & (1u << PISCES_FILTER_FORCED_REPORT)) return kOther;   // :139-140
    return count_category(w60);   // :142-171 — the same answers from CalledAllele.Type and the two strings
}

// DidWeDetectAnEdge for row i (position, coverage) with neighbour(j, &position, &coverage) = false for a row that is not there.
template <typename Neighbour>
PISCES_VHD inline bool at_edge(int64_t i, int32_t position, int32_t coverage, int32_t extent, Neighbour neighbour)
{
    if (coverage == 0) return false;   // :74
    const double half = 0.5 * (double)coverage;
    for (int32_t k = 1; k <= extent; k++) {
        int32_t p = 0, c = 0;
        // in front of the test row (:103-107): distance = test - buffer, allowed = k
        if (!neighbour(i - k, &p, &c)) return true;                        // :87
        if ((double)c < half) return true;                                 // :91
        if ((int64_t)position - (int64_t)p > (int64_t)k) return true;      // :105
        // behind it (:108-112): distance < -k
        if (!neighbour(i + k, &p, &c)) return true;
        if ((double)c < half) return true;
        if ((int64_t)position - (int64_t)p < -(int64_t)k) return true;     // :110
    }
    return false;
}

// MathOperations.QtoP / PtoQ (stats/MathOperations.cs:7-15) and the C# (int) cast of a Double
inline double q_to_p(double q) { return pow(10.0, -1 * q / 10.0); }
inline double p_to_q(double p) { return -10 * log10(p); }
inline int32_t cs_int(double d) { return (d > -2147483649.0 && d < 2147483648.0) ? (int32_t)d : kIntMin; }

// One CountData: the 16 counts as Doubles and NumPossibleVariants.  remove_non_snv is what GetPhredScaledCalibratedRates does to the
// dictionary it is handed (:331-334), in place: every TotalMutations read afterwards is over the 12.
struct Counts {
    double by_category[kCategories];
    double num_possible;
    bool removed;
    double total() const   // CountData.TotalMutations (:25-36)
    {
        double t = 0;
        for (int32_t c = 0; c < (removed ? kSnvCategories : kCategories); c++) t += by_category[c];
        return t;
    }
    double rate() const { return num_possible == 0 ? 0 : total() / num_possible; }   // ObservedMutationRate (:39-48)
};

// GetPhredScaledCalibratedRates (:323-381): the categories above mean + z * sigma of the sorted counts [2..9] get (int)PtoQ(rate + QtoP(base))
inline uint32_t rates(Counts& counts, int32_t base_q_noise, double z_factor, int32_t table[kSnvCategories])
{
    const double base = q_to_p((double)base_q_noise);
    counts.removed = true;
    double sorted[kSnvCategories];
    for (int32_t c = 0; c < kSnvCategories; c++) sorted[c] = counts.by_category[c];
    for (int32_t a = 1; a < kSnvCategories; a++)   // OrderBy (:336)
        for (int32_t b = a; b > 0 && sorted[b - 1] > sorted[b]; b--) { const double t = sorted[b]; sorted[b] = sorted[b - 1]; sorted[b - 1] = t; }
    const double points = 8;
    double avg = 0;
    for (int32_t i = 2; i < 10; i++) avg += (sorted[i] / points);
    double variance = 0;
    for (int32_t i = 2; i < 10; i++) variance += ((avg - sorted[i]) * (avg - sorted[i]) / points);
    const double threshold = avg + z_factor * sqrt(variance);
    uint32_t mask = 0;
    for (int32_t c = 0; c < kSnvCategories; c++) {
        table[c] = 0;
        const double n = counts.by_category[c];
        if (n > threshold) {   // :360
            double observed = 0;
            if (counts.num_possible > 0) observed = n / counts.num_possible;
            table[c] = cs_int(p_to_q(observed + base));   // :374 "deliberately taking floor"
            mask |= 1u << c;
        }
    }
    return mask;
}

// GetPhredScaledCalibratedRatesForEdges (:276-321), after both CountData have been through rates()
inline double edge_risk(const Counts& basic, const Counts& edge, int32_t table[kSnvCategories])
{
    const double increase = edge.rate() / basic.rate();   // GeneralEdgeRiskIncrease (:281)
    const double not_in_edge = basic.total() - edge.total();
    const double loci_not_in_edge = basic.num_possible - edge.num_possible;
    const double rate_not_in_edge = not_in_edge / loci_not_in_edge;
    const double expected = rate_not_in_edge * edge.num_possible;
    const double probably_wrong = edge.total() - expected;
    const double error_rate = probably_wrong / edge.total();
    for (int32_t c = 0; c < kSnvCategories; c++) {
        const double proportion = edge.by_category[c] / edge.total();
        table[c] = cs_int(p_to_q(proportion * error_rate));   // :312-316
    }
    return increase;
}

// The fields of a row the update reads and writes
struct RowQ {
    int32_t variant_qscore;
    int32_t genotype_qscore;
    int32_t noise_level;     // kIntMin for int.MinValue
    uint32_t filter_bits;
    bool changed;            // InsertNewQ ran
};

// UpdateVariantQScoreAndRefilter (:197-246).  err = QtoP(rate), evaluated by whoever made the table.  qscore(callCount, depth, err, cap)
// is AssignPoissonQScore for callCount > 0 and depth > 0; it is not asked otherwise (:57-58 returns 0), so a rate of int.MinValue under
// subsampling — err = +inf, subSampleToThis = 0 — never reaches it.
template <typename QScore>
PISCES_VHD inline void update_q(RowQ& r, int32_t rate, double err, bool subsample, int32_t total_coverage, int32_t allele_support, int32_t max_qscore,
                                int32_t filter_qscore, QScore qscore)
{
    const double sub_sample_to_this = 1.0 / err;
    if (rate == 0 || err == 0) subsample = false;   // :218-219
    if (r.variant_qscore < 1) return;               // HaveInfoToUpdateQ (:263-264)
    double depth = (double)total_coverage, call_count = (double)allele_support;
    if (subsample && depth > sub_sample_to_this) {  // :223-227
        call_count = call_count * sub_sample_to_this / depth;
        depth = sub_sample_to_this;
    }
    const int32_t k = (int32_t)call_count, n = (int32_t)depth;   // both within int32: depth only ever shrinks
    const int32_t cap = r.variant_qscore < max_qscore ? r.variant_qscore : max_qscore;   // :232
    // a rate whose QtoP is not finite (int.MinValue without subsampling): MathNet's Poisson(+inf).CumulativeDistribution is 0, p = 1, Q = 0
    // (oracle/pisces_oracle.c says the same of NoiseModel.Window's int.MinValue level)
    const int32_t new_q = (k <= 0 || n <= 0 || !(err < INFINITY)) ? 0 : qscore(k, n, err, cap);
    r.variant_qscore = new_q;      // InsertNewQ (:248-255), isSomatic = true at the only call site
    r.noise_level = rate;
    r.genotype_qscore = new_q;
    r.changed = true;
    if (new_q < filter_qscore) r.filter_bits |= 1u << PISCES_FILTER_LOW_VARIANT_QSCORE;   // :237-244, never cleared
}

// What the update pass needs of PiscesVqrOptions and PiscesVqrTables, with QtoP of every rate evaluated on the host (as DeviceParams.err_q is)
struct ApplyTables {
    int32_t basic[kSnvCategories], edge_risk[kSnvCategories];
    double basic_err[kSnvCategories], edge_risk_err[kSnvCategories];
    uint32_t basic_mask, edge_mask;     // BasicLookupTable / AmpliconEdgeVariantsLookupTable .ContainsKey; 0 with the check switched off
    int32_t max_qscore, filter_qscore;
    double ln10;
};

// UpdateAllele (:131-155): is this row's category in either table at all?
PISCES_VHD inline bool in_a_table(const ApplyTables& T, int32_t cat) { return cat < kSnvCategories && (((T.basic_mask | T.edge_mask) >> cat) & 1u); }
PISCES_VHD inline bool in_edge_table(const ApplyTables& T, int32_t cat) { return cat < kSnvCategories && ((T.edge_mask >> cat) & 1u); }

// UpdateAllele for one row: the basic table first, then — for a category of the edge table at a position that holds a suspect — the
// edge-risk rate with subsampling.
template <typename QScore>
PISCES_VHD inline void update_row(RowQ& r, const ApplyTables& T, int32_t cat, bool suspect_at_position, int32_t total_coverage, int32_t allele_support,
                                  QScore qscore)
{
    if (cat >= kSnvCategories) return;
    if ((T.basic_mask >> cat) & 1u)
        update_q(r, T.basic[cat], T.basic_err[cat], false, total_coverage, allele_support, T.max_qscore, T.filter_qscore, qscore);
    if (((T.edge_mask >> cat) & 1u) && suspect_at_position)
        update_q(r, T.edge_risk[cat], T.edge_risk_err[cat], true, total_coverage, allele_support, T.max_qscore, T.filter_qscore, qscore);
}

// CalledAllele.NoiseLevelApplied as the row carries it
PISCES_VHD inline int16_t noise_level_field_of(int32_t level) { return level == kIntMin ? (int16_t)-32768 : (int16_t)level; }

}  // namespace vqr
}  // namespace pisces
