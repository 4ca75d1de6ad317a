// poisson_core.h — Pisces' own Poisson CDF (src/lib/Pisces.Calculators/stats/Poisson.cs: an in-repo regularized incomplete gamma), ONE
// source for the host and the device: the call phase's q-scores and strand-bias statistics (device_math.hip.h) and the amplicon-bias
// decision (amplicon_bias.h, whose host form is pisces_hip_amplicon_bias).  Arithmetic order follows the reference (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PISCES_GHD __host__ __device__
#define PISCES_GHD_FORCE __host__ __device__ inline __attribute__((always_inline))
#else
#define PISCES_GHD
#define PISCES_GHD_FORCE inline
#endif

namespace pisces {

// ------------------------------------------------------------------------------------------
// lib/Pisces.Calculators/stats/Poisson.cs — in-repo regularized incomplete gamma
// ------------------------------------------------------------------------------------------
PISCES_GHD_FORCE double lanczos_approximation(double p)  // Poisson.cs:106-120
{
    double x = p;
    double tmp = x + 5.5;
    tmp = tmp - (x + 0.5) * log(tmp);
    double ser = 1.000000000190015 + 76.18009172947146 / (p + 1.0);
    ser -= 86.50532032941678 / (p + 2.0);
    ser += 24.01409824083091 / (p + 3.0);
    ser -= 1.231739572450155 / (p + 4.0);
    ser += 0.001208650973866179 / (p + 5.0);
    ser -= 5.395239384953E-06 / (p + 6.0);
    return (log(2.506628274631001 * ser / x) - tmp);
}

PISCES_GHD_FORCE double stirling_approximation(double n)  // Poisson.cs:125-128
{
    return (0.5 * log(2.0 * 3.14159265358979323846) + (0.5 + n) * log(n) - n);
}

PISCES_GHD inline double gamma_continued_fraction(double a, double x, double g)  // Poisson.cs:49-74
{
    const double kFpmin = 1.0E-50, kEpsilon = 1.0E-20;
    double b = x + 1.0 - a;
    double c = 1.0 / kFpmin;
    double d = 1.0 / b;
    double h = d;
    int i;
    for (i = 1; i <= 300; i++) {
        double an = i * (a - i);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < kFpmin) d = kFpmin;
        c = b + an / c;
        if (fabs(c) < kFpmin) c = kFpmin;
        d = 1.0 / d;
        double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < kEpsilon) break;
    }
    if (i > 300) return -1.0;
    return exp(a * log(x) - x - g) * h;
}

PISCES_GHD inline double gamma_series(double a, double x, double g)  // Poisson.cs:76-101
{
    // Same operations in the same order as the reference loop; only the scheduling differs: the quotients
    // x / (a + i) do not depend on the running term, so four of them are formed together (independent FP64
    // division sequences overlap in the pipeline) and then consumed one by one with the reference's
    // convergence test after each.  a is an integer-valued double here, so a + i is exactly the
    // reference's repeatedly incremented `ap`.
    const double kEpsilon = 1.0E-20;
    double retval = -1.0;
    if (x == 0.0) return 0.0;
    if (x < 0.0) return retval;
    double sum = 1.0 / a;
    double del = sum;
    bool done = false;
    for (int i = 1; i <= 300 && !done; i += 4) {
        const double ap0 = a + (double)i;
        const double q0 = x / ap0, q1 = x / (ap0 + 1.0), q2 = x / (ap0 + 2.0), q3 = x / (ap0 + 3.0);
        del *= q0; sum += del;
        if (fabs(del) < fabs(sum) * kEpsilon) { done = true; break; }
        del *= q1; sum += del;
        if (fabs(del) < fabs(sum) * kEpsilon) { done = true; break; }
        del *= q2; sum += del;
        if (fabs(del) < fabs(sum) * kEpsilon) { done = true; break; }
        del *= q3; sum += del;
        if (fabs(del) < fabs(sum) * kEpsilon) { done = true; break; }
    }
    if (done) retval = sum * exp(a * log(x) - x - g);
    return retval;
}

PISCES_GHD inline double incomplete_gamma_function(double a, double x)  // Poisson.cs:34-44
{
    if ((x < 0) || (a <= 0)) return -1.0;
    double g = (a >= 700.0 ? stirling_approximation(a) : lanczos_approximation(a));
    if (x >= a + 1.0) return gamma_continued_fraction(a, x, g);
    if ((g = gamma_series(a, x, g)) < 0) return g;
    return 1.0 - g;
}

PISCES_GHD_FORCE double poisson_cdf(double num_occurrences, double expected)  // Poisson.cs:26-29
{
    return incomplete_gamma_function((double)(int)(num_occurrences + 1.0), expected);
}

}  // namespace pisces
