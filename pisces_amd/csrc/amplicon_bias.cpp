// amplicon_bias.cpp — the host form of amplicon_bias.h: pisces_hip_amplicon_bias, for a caller that keeps the per-amplicon counts itself.
// Pure host code, no device, no handle.
#include "amplicon_bias.h"

#include "../../include/pisces_hip.h"

extern "C" {

int32_t pisces_hip_amplicon_bias(const int32_t* support, const int32_t* coverage, int32_t n, float threshold, double* chance_out)
{
    if (n < 2 || !support || !coverage) return -1;
    return pisces::amplicon::bias(support, coverage, n, threshold, chance_out);
}

}  // extern "C"
