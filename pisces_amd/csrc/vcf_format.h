// vcf_format.h — what the device formatter (surface_vcf.inc.h) takes from the host formatter (vcf_format.cpp) instead of restating it.
#pragma once
#include "../../include/pisces_hip.h"

// The number of VF decimals of a writer configuration (VcfFormatter.UpdateFrequencyFormat: GetNumSigDigits of Single.ToString() of the
// frequency thresholds), as pisces_hip_format_vcf computes it.
int pisces_vcf_frequency_decimals(const PiscesVcfConfig* cfg);
