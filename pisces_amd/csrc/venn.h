// venn.h — VennVcf (src/exe/VennVcf/) over the 64-byte rows: the consensus of two probe pools' call sets and the probe-pool-bias filter
// (PB, FilterType.PoolBias).  One source for the host (surface_venn.inc.h) and the device (venn_kernels.hip.h), as vqr.h is.  Restated:
//   same_allele / select_pairs / comparison_case   VennVcf.cs:420-537, CalledAllele.cs:204-210
//   combine            ConsensusBuilder.CombineVariants (ConsensusBuilder.cs:36-488) with everything below it
//   merge_reference    several HomozygousRef consensus calls of one position (VennVcf.cs:209-243)
//   walk_group         one turn of DoPairwiseVenn's loop (VennVcf.cs:180-252) behind a Sink: count, emit and the host entry are this code
//   venn_class         WriteVarsToVennFiles (VennVcf.cs:329-350): 1 = "and", 2 = "not", 0 = in no file
// The two scores come in as a Math object (venn_kernels.hip.h: VennMath, over poisson_qscore_core and the strand-bias statistics).
// This library's choice where the reference's consensus defines nothing (no column of VennVcf reads them): coverage_by_dir, support_by_dir
// and num_no_calls are the components' sums, the three bias bits of info and filter_bits their ORs; strand_bias_score is the larger
// component's, copied (the maximum of the GATK scores, ConsensusBuilder.cs:287, is the maximum of the scores).
// Out of scope: reading VCFs, output file names, the sample-name regex and header lines; chromosome ordering across calls (a call sees ONE
// chromosome); the PB and VF0..DP1 columns of the VCF formatters; crushed diploid inputs.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pisces_hip.h"

#if defined(__HIPCC__)
#define PISCES_NHD __host__ __device__
#else
#define PISCES_NHD
#endif

namespace pisces {
namespace venn {

constexpr int32_t kIntMin = (int32_t)0x80000000;
// VariantComparisonCase (VennVcf.cs:15-21)
constexpr int32_t kAgreedOnReference = 0, kAgreedOnAlternate = 1, kOneReferenceOneAlternate = 2, kCanNotCombine = 3;
constexpr uint8_t kVennNone = 0, kVennAnd = 1, kVennNot = 2;

// One pool's rows as a flush gives them out
struct Pool {
    const PiscesCalledAllele* recs;
    int64_t n;                        // rows there: min(n, *d_count) on the device
    const int32_t* cand_index;        // optional
    const PiscesCandidate* cands;
    const uint8_t* alleles;
};

// a row, whole: four 16-byte loads on the device (the entries refuse a row pointer that is not 16-byte aligned), memcpy on the host
struct alignas(16) Quad { uint32_t x, y, z, w; };
PISCES_NHD inline PiscesCalledAllele load_row(const PiscesCalledAllele* p)
{
    PiscesCalledAllele r;
#if defined(__HIP_DEVICE_COMPILE__)
    const Quad* s = reinterpret_cast<const Quad*>(p);
    Quad q[4] = {s[0], s[1], s[2], s[3]};
    memcpy(&r, q, sizeof(r));
#else
    memcpy(&r, p, sizeof(r));
#endif
    return r;
}
PISCES_NHD inline void store_row(PiscesCalledAllele* p, const PiscesCalledAllele& r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    Quad q[4];
    memcpy(q, &r, sizeof(r));
    Quad* d = reinterpret_cast<Quad*>(p);
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; d[3] = q[3];
#else
    memcpy(p, &r, sizeof(r));
#endif
}

PISCES_NHD inline uint8_t base_of(int32_t code) { return code == PISCES_ALLELE_A ? 'A' : code == PISCES_ALLELE_G ? 'G' : code == PISCES_ALLELE_C ? 'C' : code == PISCES_ALLELE_T ? 'T' : 'N'; }
PISCES_NHD inline int32_t code_of(uint8_t base)
{
    return (base == 'A' || base == 'a') ? PISCES_ALLELE_A : (base == 'G' || base == 'g') ? PISCES_ALLELE_G : (base == 'C' || base == 'c') ? PISCES_ALLELE_C
           : (base == 'T' || base == 't') ? PISCES_ALLELE_T : PISCES_ALLELE_N;
}

// The allele strings of row i of a pool.  A Reference row's AlternateAllele is "." (AlleleReader), whatever its alt code says.
struct AlleleView {
    const uint8_t* ref;   // null: one base, ref1
    const uint8_t* alt;
    int32_t ref_len, alt_len;
    uint8_t ref1, alt1;
    bool dot;             // AlternateAllele == "."
    int32_t cand;         // cand_index, or -1
    PISCES_NHD uint8_t ref_at(int32_t k) const { return ref ? ref[k] : ref1; }
    PISCES_NHD uint8_t alt_at(int32_t k) const { return alt ? alt[k] : alt1; }
};
PISCES_NHD inline AlleleView allele_view(const Pool& P, int64_t i, uint32_t info)
{
    AlleleView v;
    v.cand = P.cand_index ? P.cand_index[i] : -1;
    v.dot = (int32_t)PISCES_INFO_CATEGORY(info) == PISCES_CAT_REFERENCE;
    if (v.cand >= 0) {
        const PiscesCandidate& c = P.cands[v.cand];
        v.ref = P.alleles + c.allele_offset;
        v.alt = v.ref + c.ref_len;
        v.ref_len = c.ref_len;
        v.alt_len = c.alt_len;
        v.ref1 = v.alt1 = 0;
    } else {
        v.ref = v.alt = nullptr;
        v.ref_len = v.alt_len = 1;
        v.ref1 = base_of((int32_t)PISCES_INFO_REF(info));
        v.alt1 = base_of((int32_t)PISCES_INFO_ALT(info));
    }
    if (v.dot) { v.alt = nullptr; v.alt_len = 1; v.alt1 = '.'; }
    return v;
}
// ReferenceAllele == ReferenceAllele && AlternateAllele == AlternateAllele: lengths, then bytes
PISCES_NHD inline bool same_allele(const AlleleView& a, const AlleleView& b)
{
    if (a.ref_len != b.ref_len || a.alt_len != b.alt_len) return false;
    for (int32_t k = 0; k < a.ref_len; k++)
        if (a.ref_at(k) != b.ref_at(k)) return false;
    for (int32_t k = 0; k < a.alt_len; k++)
        if (a.alt_at(k) != b.alt_at(k)) return false;
    return true;
}
PISCES_NHD inline uint32_t info_of(const Pool& P, int64_t i) { return (uint32_t)P.recs[i].info; }
PISCES_NHD inline bool same_allele(const Pool& A, int64_t i, const Pool& B, int64_t j)
{
    return same_allele(allele_view(A, i, info_of(A, i)), allele_view(B, j, info_of(B, j)));
}
PISCES_NHD inline bool is_dot(const Pool& P, int64_t i) { return (int32_t)PISCES_INFO_CATEGORY(info_of(P, i)) == PISCES_CAT_REFERENCE; }

// SelectPairs over A[a0, a1) and B[b0, b1): pair(ia, ib) in the reference's order, -1 for a missing member.  The loops have no cap;
// nothing is remembered between them: B[j] was matched exactly when it is the first equal of some A[i] (the reference breaks at the first).
template <typename Pair>
PISCES_NHD inline void select_pairs(const Pool& A, int64_t a0, int64_t a1, const Pool& B, int64_t b0, int64_t b1, Pair pair)
{
    if (a1 - a0 == 1 && is_dot(A, a0)) {               // ref + ref, ref + {alt, alt', ...} (:425-435)
        for (int64_t j = b0; j < b1; j++) pair(a0, j);
        if (b1 == b0) pair(a0, (int64_t)-1);
    } else if (b1 - b0 == 1 && is_dot(B, b0)) {        // :436-446
        for (int64_t i = a0; i < a1; i++) pair(i, b0);
        if (a1 == a0) pair((int64_t)-1, b0);
    } else {                                           // :448-485
        for (int64_t i = a0; i < a1; i++) {
            int64_t found = -1;
            for (int64_t j = b0; j < b1 && found < 0; j++)
                if (same_allele(A, i, B, j)) found = j;
            pair(i, found);
        }
        for (int64_t j = b0; j < b1; j++) {
            bool matched = false;
            for (int64_t i = a0; i < a1 && !matched; i++) {
                int64_t first = -1;
                for (int64_t k = b0; k <= j && first < 0; k++)
                    if (same_allele(A, i, B, k)) first = k;
                matched = first == j;
            }
            if (!matched) pair((int64_t)-1, j);
        }
    }
}

PISCES_NHD inline bool is_ref_type(uint32_t info) { return (int32_t)PISCES_INFO_CATEGORY(info) == PISCES_CAT_REFERENCE; }

// GetComparisonCase (:489-537).  Two alternates that differ never arrive here: SelectPairs pairs equal alleles only.
PISCES_NHD inline int32_t comparison_case(bool has_a, uint32_t info_a, bool has_b, uint32_t info_b)
{
    if (!has_a || !has_b) return kCanNotCombine;
    const bool ra = is_ref_type(info_a), rb = is_ref_type(info_b);
    if (ra && rb) return kAgreedOnReference;
    if (ra != rb) return kOneReferenceOneAlternate;
    return kAgreedOnAlternate;
}

// DoDefensiveGenotyping (ConsensusBuilder.cs:82-95)
PISCES_NHD inline int32_t defensive_genotype(int32_t gt)
{
    if (gt == PISCES_GT_ALT_AND_NOCALL || gt == PISCES_GT_HEMI_ALT) return PISCES_GT_HOM_ALT;
    if (gt == PISCES_GT_REF_AND_NOCALL || gt == PISCES_GT_HEMI_REF) return PISCES_GT_HOM_REF;
    if (gt == PISCES_GT_HEMI_NOCALL) return PISCES_GT_REF_LIKE_NOCALL;
    return gt;
}
// CalledAllele.HasARefAllele / HasAnAltAllele (CalledAllele.cs:80-100)
PISCES_NHD inline bool has_a_ref_allele(int32_t gt) { return gt == PISCES_GT_REF_AND_NOCALL || gt == PISCES_GT_HOM_REF || gt == PISCES_GT_HEMI_REF || gt == PISCES_GT_HET_ALT_REF; }
PISCES_NHD inline bool has_an_alt_allele(int32_t gt) { return gt == PISCES_GT_ALT_AND_NOCALL || gt == PISCES_GT_HOM_ALT || gt == PISCES_GT_HET_ALT1_ALT2 || gt == PISCES_GT_HET_ALT_REF; }

PISCES_NHD inline int32_t level_of(int16_t field) { return field == (int16_t)-32768 ? kIntMin : (int32_t)field; }
PISCES_NHD inline int16_t level_field_of(int32_t level) { return level == kIntMin ? (int16_t)-32768 : (int16_t)level; }

// CombineNoiseLevelsByTakingAvgP (:458-467).  QtoP(int.MinValue) is +infinity, PtoQ of it -infinity, and the C# cast of that int.MinValue.
PISCES_NHD inline int32_t average_noise_level(int32_t nl1, int32_t nl2)
{
    if (nl1 == nl2) return nl1;
    if (nl1 == kIntMin || nl2 == kIntMin) return kIntMin;
    const double p1 = pow(10.0, -1 * (double)nl1 / 10.0), p2 = pow(10.0, -1 * (double)nl2 / 10.0);
    return (int32_t)rint(-10 * log10((p1 + p2) / 2.0));
}

// GetGenotype (:304-398).  min_frequency and min_frequency_filter are Singles in the reference: the comparisons widen them.
PISCES_NHD inline int32_t consensus_genotype(bool has_a, int32_t gt_a, bool has_b, int32_t gt_b, int32_t cmp, int32_t total_depth, double vf, double vf_a,
                                            double vf_b, const PiscesVennOptions& O)
{
    const bool ref_present = (has_a && has_a_ref_allele(gt_a)) || (has_b && has_a_ref_allele(gt_b));
    const bool alt_present = (has_a && has_an_alt_allele(gt_a)) || (has_b && has_an_alt_allele(gt_b));
    int32_t gt;
    if (!alt_present && ref_present) gt = PISCES_GT_HOM_REF;
    else if (alt_present && ref_present) gt = PISCES_GT_HET_ALT_REF;
    else if (alt_present && !ref_present) gt = PISCES_GT_HOM_ALT;
    else return PISCES_GT_REF_LIKE_NOCALL;                                    // :344-345
    if (cmp != kAgreedOnReference) {
        if (vf < (double)O.min_frequency) {                                   // :365
            if (vf_a < (double)O.min_frequency_filter && vf_b < (double)O.min_frequency_filter) gt = PISCES_GT_HOM_REF;
            else gt = PISCES_GT_ALT_LIKE_NOCALL;
        } else if (vf < (double)O.min_frequency_filter) {                     // :378
            gt = PISCES_GT_ALT_LIKE_NOCALL;
        }
    } else if (total_depth < O.min_coverage) {                                // :391
        gt = PISCES_GT_REF_LIKE_NOCALL;
    }
    return gt;
}

// What combine gives back beside the row: whose alleles the consensus carries, and whether they were cut down to the reference's
struct Combined {
    PiscesCalledAllele row;
    PiscesConsensusInfo info;
    int32_t source;           // 0: pool A's member, 1: pool B's
    int32_t vq_a, vq_b;       // VariantA / VariantB .VariantQscore as PushThroughRamificationsOfGTChange leaves them
};

// CombineVariants.  a / b: the members (null = absent), whose variant_qscore the caller may have replaced by what an earlier pair of this
// position left there (PushThroughRamificationsOfGTChange writes into its inputs).  ref_code: the code of the first base of the source's
// ReferenceAllele, for a consensus cut down to "ref ."
template <typename Math>
PISCES_NHD inline Combined combine(const PiscesCalledAllele* a, const PiscesCalledAllele* b, int32_t cmp, const PiscesVennOptions& O, const Math& math,
                                   int32_t ref_code_a, int32_t ref_code_b)
{
    Combined c;
    memset(&c, 0, sizeof(c));
    const bool has_a = a != nullptr, has_b = b != nullptr;
    const uint32_t info_a = has_a ? a->info : 0u, info_b = has_b ? b->info : 0u;
    const int32_t gt_a = has_a ? defensive_genotype((int32_t)PISCES_INFO_GENOTYPE(info_a)) : PISCES_GT_REF_LIKE_NOCALL;
    const int32_t gt_b = has_b ? defensive_genotype((int32_t)PISCES_INFO_GENOTYPE(info_b)) : PISCES_GT_REF_LIKE_NOCALL;
    // CombineReferenceAlleles / CombineVariantAlleles (:99-156): whose strings
    if (cmp == kAgreedOnReference || cmp == kAgreedOnAlternate) c.source = 0;
    else if (cmp == kOneReferenceOneAlternate) c.source = is_ref_type(info_a) ? 1 : 0;
    else c.source = has_b ? 1 : 0;
    const PiscesCalledAllele* src = c.source ? b : a;

    // RecalculateScoring (:158-245)
    const int32_t ref_count_a = has_a ? a->reference_support : 0, ref_count_b = has_b ? b->reference_support : 0;
    const int32_t alt_count_a = has_a ? (is_ref_type(info_a) ? 0 : a->allele_support) : 0;
    const int32_t alt_count_b = has_b ? (is_ref_type(info_b) ? 0 : b->allele_support) : 0;
    const int32_t depth_a = has_a ? a->total_coverage : 0, depth_b = has_b ? b->total_coverage : 0;
    const int32_t total_depth = depth_a + depth_b, reference_depth = ref_count_a + ref_count_b, alt_depth = alt_count_a + alt_count_b;
    const double vf = (alt_depth == 0 || total_depth == 0) ? 0.0 : (double)alt_depth / (double)total_depth;
    const double vf_a = (alt_count_a == 0 || depth_a == 0) ? 0.0 : (double)alt_count_a / (double)depth_a;
    const double vf_b = (alt_count_b == 0 || depth_b == 0) ? 0.0 : (double)alt_count_b / (double)depth_b;
    const int32_t gt = consensus_genotype(has_a, gt_a, has_b, gt_b, cmp, total_depth, vf, vf_a, vf_b, O);
    const bool take_min = O.combine_qscore_method == 1;
    // GetCombinedNLValue (:290-302), GetCombinedSBValue (:277-289)
    int32_t nl;
    double sb;
    if (!has_a) { nl = level_of(b->noise_level); sb = b->strand_bias_score; }
    else if (!has_b) { nl = level_of(a->noise_level); sb = a->strand_bias_score; }
    else {
        const int32_t la = level_of(a->noise_level), lb = level_of(b->noise_level);
        nl = take_min ? (la < lb ? la : lb) : average_noise_level(la, lb);
        sb = a->strand_bias_score > b->strand_bias_score ? a->strand_bias_score : b->strand_bias_score;   // a NaN on either side: b's, as Math.Max gives a NaN there
        if (a->strand_bias_score != a->strand_bias_score) sb = a->strand_bias_score;
    }
    // PushThroughRamificationsOfGTChange (:247-275)
    c.vq_a = has_a ? a->variant_qscore : 0;
    c.vq_b = has_b ? b->variant_qscore : 0;
    const bool changed = (gt == PISCES_GT_HOM_REF || gt == PISCES_GT_REF_LIKE_NOCALL) && cmp == kOneReferenceOneAlternate;
    if (changed) {
        if (has_a) c.vq_a = math.qscore(ref_count_a, depth_a, nl, O.max_variant_qscore);
        if (has_b) c.vq_b = math.qscore(ref_count_b, depth_b, nl, O.max_variant_qscore);
    }
    // GetProbePoolBiasScore (:401-455)
    uint32_t filters = (has_a ? a->filter_bits : 0u) | (has_b ? b->filter_bits : 0u);   // CombineFilters (:485-488)
    double pb_score = 0, pb_gatk = -100;
    if (changed || cmp == kAgreedOnReference) {
    } else if (cmp == kOneReferenceOneAlternate || cmp == kCanNotCombine) {
        filters |= 1u << PISCES_FILTER_POOL_BIAS;
        pb_gatk = 0;
        pb_score = 1;
    } else {
        double score, gatk;
        bool acceptable;
        math.pool_bias(depth_a, depth_b, alt_count_a, alt_count_b, nl, (double)O.min_frequency, (double)O.pool_bias_threshold, &score, &gatk, &acceptable);
        pb_gatk = gatk < 0 ? gatk : 0;                 // Math.Min(0, x): a NaN stays a NaN in C#
        if (gatk != gatk) pb_gatk = gatk;
        pb_gatk = pb_gatk > -100 ? pb_gatk : -100;     // Math.Max(-100, x)
        if (gatk != gatk) pb_gatk = gatk;
        pb_score = score < 1 ? score : 1;
        if (score != score) pb_score = score;
        if (!acceptable) filters |= 1u << PISCES_FILTER_POOL_BIAS;
    }
    // the q-score (:215-237)
    int32_t vq;
    if (take_min) vq = !has_b ? c.vq_a : !has_a ? c.vq_b : (c.vq_a < c.vq_b ? c.vq_a : c.vq_b);
    else if (cmp == kAgreedOnReference || (cmp == kOneReferenceOneAlternate && changed) || (cmp == kCanNotCombine && alt_depth == 0))
        vq = math.qscore(reference_depth, total_depth, nl, O.max_variant_qscore);
    else
        vq = math.qscore(alt_depth, total_depth, nl, O.max_variant_qscore);
    // SetType (BaseAllele.cs:45-76) on the consensus strings: the source's, or "ref ." once the alternate is gone
    const uint32_t src_info = src->info;
    const bool ref_typed = changed || is_ref_type(src_info);
    const int32_t ref_code = changed ? (c.source ? ref_code_b : ref_code_a) : (int32_t)PISCES_INFO_REF(src_info);
    PiscesCalledAllele& r = c.row;
    r.position = src->position;
    r.total_coverage = total_depth;
    r.allele_support = ref_typed ? reference_depth : alt_depth;   // :243-244, :270
    r.reference_support = reference_depth;
    r.variant_qscore = vq;
    r.genotype_qscore = (int16_t)vq;                               // :240
    r.noise_level = level_field_of(nl);
    r.strand_bias_score = sb;
    r.filter_bits = (uint16_t)filters;
    uint32_t both = 0;
    for (int32_t k = 0; k < 2; k++) {
        const PiscesCalledAllele* m = k ? b : a;
        if (!m) continue;
        r.num_no_calls += m->num_no_calls;
        for (int32_t d = 0; d < 3; d++) { r.coverage_by_dir[d] += m->coverage_by_dir[d]; r.support_by_dir[d] += m->support_by_dir[d]; }
        both |= (uint32_t)m->info & 0xe000u;
    }
    const int32_t cat = ref_typed ? PISCES_CAT_REFERENCE : (int32_t)PISCES_INFO_CATEGORY(src_info);
    const int32_t alt_code = ref_typed ? ref_code : (int32_t)PISCES_INFO_ALT(src_info);
    r.info = (uint16_t)((uint32_t)gt | ((uint32_t)cat << 4) | ((uint32_t)ref_code << 7) | ((uint32_t)alt_code << 10) | both);
    c.info.row_a = c.info.row_b = -1;
    c.info.comparison_case = cmp;
    c.info.alt_changed_to_ref = changed ? 1 : 0;
    c.info.pool_bias_score = pb_score;
    c.info.pool_bias_gatk = pb_gatk;
    return c;
}

// The merge of a later HomozygousRef consensus into the position's first (VennVcf.cs:225-241).  Both bias results are replaced by new
// objects that hold a GATK score alone: pool_bias_score is 0 afterwards, as BiasResults.BiasScore is.
PISCES_NHD inline void merge_reference(Combined& last, const Combined& c)
{
    last.row.filter_bits |= c.row.filter_bits;
    if (c.row.strand_bias_score > last.row.strand_bias_score) last.row.strand_bias_score = c.row.strand_bias_score;
    if (c.info.pool_bias_gatk > last.info.pool_bias_gatk) last.info.pool_bias_gatk = c.info.pool_bias_gatk;
    last.info.pool_bias_score = 0;
    const int32_t la = level_of(last.row.noise_level), lb = level_of(c.row.noise_level);
    last.row.noise_level = level_field_of(la < lb ? la : lb);
    if (c.row.genotype_qscore < last.row.genotype_qscore) last.row.genotype_qscore = c.row.genotype_qscore;
    if ((int32_t)c.row.genotype_qscore < last.row.variant_qscore) last.row.variant_qscore = c.row.genotype_qscore;   // :239 reads GenotypeQscore
}

// WriteVarsToVennFiles (:329-350): the class of a pair's member
PISCES_NHD inline uint8_t venn_class(int32_t cmp, uint32_t member_info)
{
    if (cmp == kAgreedOnAlternate) return kVennAnd;
    if ((cmp == kOneReferenceOneAlternate || cmp == kCanNotCombine) && !is_ref_type(member_info)) return kVennNot;
    return kVennNone;
}

struct GroupCounts { int64_t rows, cands, bytes; };

// One position: the rows A[a0, a1) and B[b0, b1) of it (either may be empty).  Sink:
//   row(slot, row, info)                       consensus row `slot` of the group (a merged reference is stored once, after its last merge)
//   cand(slot, cslot, byte_off, candidate, bytes)   the row's candidate, the group's cslot-th, with its ref_len + alt_len bytes at byte_off of the group's
//   venn(pool, index, class)                   an input row's Venn class (each row of the group is set to 0 first)
// A row is in at most one pair that can class it: the single Reference row of SelectPairs' first two arms is in many pairs and is never
// classed (venn_class), every other row of those arms is in one; in the third arm an A row is in one pair, a B row in several only beside
// duplicate A alleles, all AgreedOnAlternate.
template <typename Math, typename Sink>
PISCES_NHD inline GroupCounts walk_group(const Pool& A, int64_t a0, int64_t a1, const Pool& B, int64_t b0, int64_t b1, const PiscesVennOptions& O, const Math& math,
                                         Sink& sink)
{
    GroupCounts n = {0, 0, 0};
    for (int64_t i = a0; i < a1; i++) sink.venn(0, i, kVennNone);
    for (int64_t j = b0; j < b1; j++) sink.venn(1, j, kVennNone);
    // the q-score PushThroughRamificationsOfGTChange left in the one row that several pairs share (the lone Reference row of the first two arms)
    const bool share_a = a1 - a0 == 1 && is_dot(A, a0);
    const bool share_b = !share_a && b1 - b0 == 1 && is_dot(B, b0);
    bool have_shared_vq = false;
    int32_t shared_vq = 0;
    bool have_last = false;
    Combined last;
    int64_t last_slot = 0;
    select_pairs(A, a0, a1, B, b0, b1, [&](int64_t ia, int64_t ib) {
        PiscesCalledAllele ra, rb;
        const bool has_a = ia >= 0, has_b = ib >= 0;
        AlleleView va, vb;
        if (has_a) { ra = load_row(A.recs + ia); va = allele_view(A, ia, ra.info); }
        if (has_b) { rb = load_row(B.recs + ib); vb = allele_view(B, ib, rb.info); }
        if (have_shared_vq && share_a && has_a) ra.variant_qscore = shared_vq;
        if (have_shared_vq && share_b && has_b) rb.variant_qscore = shared_vq;
        const int32_t cmp = comparison_case(has_a, has_a ? ra.info : 0u, has_b, has_b ? rb.info : 0u);
        if (has_a) { const uint8_t k = venn_class(cmp, ra.info); if (k) sink.venn(0, ia, k); }
        if (has_b) { const uint8_t k = venn_class(cmp, rb.info); if (k) sink.venn(1, ib, k); }
        Combined c = combine(has_a ? &ra : nullptr, has_b ? &rb : nullptr, cmp, O, math, has_a ? code_of(va.ref_at(0)) : 0, has_b ? code_of(vb.ref_at(0)) : 0);
        c.info.row_a = (int32_t)ia;
        c.info.row_b = (int32_t)ib;
        if (share_a && has_a) { shared_vq = c.vq_a; have_shared_vq = true; }
        if (share_b && has_b) { shared_vq = c.vq_b; have_shared_vq = true; }
        const bool hom_ref = (int32_t)PISCES_INFO_GENOTYPE(c.row.info) == PISCES_GT_HOM_REF;
        if (hom_ref && have_last) {   // :223-242
            merge_reference(last, c);
            return;
        }
        const int64_t slot = n.rows++;
        const AlleleView& sv = c.source ? vb : va;
        if (sv.cand >= 0 && !c.info.alt_changed_to_ref) {
            const PiscesCandidate& cand = (c.source ? B : A).cands[sv.cand];
            sink.cand(slot, n.cands, n.bytes, cand, sv.ref);
            n.cands++;
            n.bytes += (int64_t)cand.ref_len + (int64_t)cand.alt_len;
        } else {
            sink.no_cand(slot);
        }
        if (hom_ref) { last = c; last_slot = slot; have_last = true; }   // :213-217
        else sink.row(slot, c.row, c.info);
    });
    if (have_last) sink.row(last_slot, last.row, last.info);
    return n;
}

// first index in [0, n) whose position is >= position (rows sorted by position)
PISCES_NHD inline int64_t lower_bound(const PiscesCalledAllele* recs, int64_t n, int32_t position)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (recs[mid].position < position) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
PISCES_NHD inline int64_t group_end(const PiscesCalledAllele* recs, int64_t n, int64_t i)
{
    const int32_t position = recs[i].position;
    int64_t e = i + 1;
    while (e < n && recs[e].position == position) e++;
    return e;
}

}  // namespace venn
}  // namespace pisces
