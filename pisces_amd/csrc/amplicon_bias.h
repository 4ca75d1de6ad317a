// amplicon_bias.h — AmpliconBiasCalculator.CalculateAmpliconBias (src/lib/Pisces.Calculators/AmpliconBiasCalculator.cs:45-134) over the
// amplicons of ONE SNV, one source for the host and the device, as genotype_core.h is for the genotypers.  The amplicons arrive as two
// parallel arrays — entry i is one amplicon name of the locus' coverage list, support[i] what the allele's support list holds under that
// name (0 when it holds none: AmpliconCounts.GetCountsForAmplicon) — so the names themselves never cross: no decision depends on them
// or on their order.  The per-amplicon q-score and AmpliconWithCandidateArtifact feed only the reference's AmpliconBias.csv and are
// not computed.
//   amplicon_bias.cpp     the host form: pisces_hip_amplicon_bias
// Poisson.Cdf is Pisces' own (src/lib/Pisces.Calculators/stats/Poisson.cs): poisson_cdf of poisson_core.h, the one the call phase uses.
#pragma once
#include <math.h>
#include <stdint.h>

#include "poisson_core.h"

namespace pisces {
namespace amplicon {

constexpr int kMaxOverlappingAmplicons = 6;    // Constants.MaxNumOverlappingAmplicons (Pisces.Domain/Constants.cs:54-62)
constexpr int kMinNumObservations = 5;         // AmpliconBiasCalculator.Constants
constexpr double kFreePassObservationFreq = 0.1;

// pChanceItsReal of one amplicon (AmpliconBiasCalculator.cs:93-112): the chance that a variant of frequency max_freq shows `support` times
// or fewer in `coverage` reads, 1.0 where the reference does not ask (too few expected, seen as often as expected, seen in over 10 %).
PISCES_GHD inline double chance_its_real(double support, double coverage, double freq, double max_freq)
{
    const double expected = max_freq * coverage;
    if (expected < (double)kMinNumObservations) return 1.0;
    if (expected <= support || freq > kFreePassObservationFreq) return 1.0;
    const double p = poisson_cdf(support, expected);
    return p > 0.0 ? p : 0.0;   // Math.Max(0.0, ...): the continued fraction's "no convergence" is -1
}

PISCES_GHD inline double frequency(int32_t support, int32_t coverage) { return coverage > 0 ? (double)support / (double)coverage : 0.0; }

// 1: bias detected (FilterType.AmpliconBias), 0: not detected, -1: no result (AmpliconBiasResults stays null: no amplicon of the allele's
// support list holds a count, or the locus has fewer than two amplicons).  chance_out[n] (may be null) receives every amplicon's
// pChanceItsReal when there is a result.  Any n: the six slots of a position are the store's limit, not the calculator's.
PISCES_GHD inline int32_t bias(const int32_t* support, const int32_t* coverage, int32_t n, float threshold, double* chance_out)
{
    if (n < 2) return -1;
    bool any_support = false;
    double max_freq = 0.0;
    for (int32_t i = 0; i < n; i++) {
        any_support |= support[i] > 0;
        const double f = frequency(support[i], coverage[i]);
        if (f >= max_freq) max_freq = f;
    }
    if (!any_support) return -1;
    const double allowable = (double)threshold;   // float? acceptanceCriteria, compared as a double (:91,120)
    int32_t detected = 0;
    for (int32_t i = 0; i < n; i++) {
        const double p = chance_its_real((double)support[i], (double)coverage[i], frequency(support[i], coverage[i]), max_freq);
        if (p < allowable) detected = 1;
        if (chance_out) chance_out[i] = p;
    }
    return detected;
}

}  // namespace amplicon
}  // namespace pisces
