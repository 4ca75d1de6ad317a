// vcf_kernels.hip.h — VCF body lines on the device (pisces_hip_format_vcf_device): the text csrc/vcf_format.cpp writes for uncrushed,
// unpadded output, byte for byte, from the 64-byte rows where pisces_hip_compact_records leaves them.  DESIGN.md section 3.12.
//
// Three launches on one stream, no workgroup ever waits for another:
//   vcf_length_kernel   one lane a row: the row's line length (the formatter below run into a counting sink), the 256-row chunk's total,
//                       and the lowest row the host formatter would have refused
//   vcf_scan_kernel     one workgroup: exclusive scan of the chunk totals, the size word, the go / no-go of the write pass
//   vcf_write_kernel    one lane a row: the same formatter into the wave's LDS chunk, copied out 16 bytes a lane; a wave whose 64 lines
//                       do not fit its LDS chunk (long allele strings, a long chrom) writes its bytes straight to global memory
// One formatter (vcf_format_row<Sink>) serves both passes, so a length can only disagree with the bytes written if a sink does.
//
// Numbers: Single/Double.ToString("0.000") of .NET Core 2.0 as vcf_format.cpp's dotnet_fixed restates it — the exact binary value
// correctly rounded (ties to even, what glibc's %e does) to 7 / 15 significant decimal digits, then that digit string rounded half-up
// to the requested decimals, no sign on a zero — in integer arithmetic only (vcf_sig_digits: 128-bit, range analysis in DESIGN 3.12).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pisces_hip.h"

namespace vcfdev {

typedef unsigned __int128 u128;
typedef unsigned long long u64;

constexpr int kRowsPerChunk = 256;       // rows a workgroup (= one entry of the scan)
constexpr int kWaveLdsBytes = 12288;     // the LDS chunk of a wave's 64 lines (192 bytes a line on average; a plain row is ~86)
constexpr int kMaxChrom = 1024;          // chrom travels in the kernel arguments
constexpr int kMaxDecimals = 7;          // VF decimals the 128-bit arithmetic holds for a Double
constexpr u64 kNoError = ~0ull;

struct VcfArgs {
    const PiscesCalledAllele* recs;
    int64_t n;
    const int32_t* d_count;
    const int32_t* cand_index;
    const PiscesCandidate* cands;
    const uint8_t* alleles;
    const PiscesGenotypePosteriors* gp;
    char* text;
    int64_t capacity;
    int64_t* line_offsets;
    int64_t* text_bytes;
    uint32_t* row_len;        // [n] scratch: bytes of every line
    int64_t* chunk_off;       // [chunks] scratch: the chunk totals, then their exclusive scan
    u64* ctrl;                // [0] lowest refused row << 8 | -code (kNoError: none), [1] 1 = the write pass runs
    int32_t variant_quality_filter, rmxn_max_repeat_length, rmxn_min_repetitions, noise_level;
    int32_t output_sb_nl, output_nc, noise_level_from_records, freq_decimals;
    int32_t chrom_len, format_len, qname_len, rname_len;
    char format[32];          // GT:GQ:AD:DP:VF[:NL:SB][:NC]
    char qname[16];           // q<N>
    char rname[32];           // R<M>x<N>
    char chrom[kMaxChrom];
    int32_t iname_len;        // 0: IndelRepeatFilterThreshold null, the bit prints nothing
    char iname[12];           // R<threshold>
};

__device__ inline int64_t vcf_rows(const VcfArgs& A)
{
    int64_t rows = A.n;
    if (A.d_count) {
        const int64_t c = (int64_t)*A.d_count;
        rows = c < rows ? c : rows;
    }
    return rows < 0 ? 0 : rows;
}

// ---- sinks ------------------------------------------------------------------------------------------------------------------
struct CountSink {
    u64 n = 0;
    __device__ void put(char) { n++; }
    __device__ void skip(u64 k) { n += k; }
    static constexpr bool kCounts = true;
};
struct ByteSink {   // bytes to [p, end): a store past `end` is dropped, the cursor still moves
    char* p;
    char* end;
    __device__ void put(char c)
    {
        if (p < end) *p = c;
        p++;
    }
    static constexpr bool kCounts = false;
};

template <typename S>
__device__ inline void put_str(S& s, const char* str, int len)
{
    for (int i = 0; i < len; i++) s.put(str[i]);
}
template <typename S>
__device__ inline void put_lit(S& s, const char* lit)   // a literal: the loop ends at its terminator, which the compiler sees
{
    for (int i = 0; lit[i] != 0; i++) s.put(lit[i]);
}
template <typename S>
__device__ inline void put_u64(S& s, u64 v)
{
    char d[20];
    int k = 0;
    do {
        d[k++] = (char)('0' + (int)(v % 10ull));
        v /= 10ull;
    } while (v != 0 && k < 20);
    while (k > 0) s.put(d[--k]);
}
template <typename S>
__device__ inline void put_i64(S& s, long long v)
{
    if (v < 0) {
        s.put('-');
        put_u64(s, (u64)0 - (u64)v);
    } else {
        put_u64(s, (u64)v);
    }
}
// exactly `width` digits of v (v < 10^width), leading zeros kept
template <typename S>
__device__ inline void put_digits(S& s, u64 v, int width)
{
    char d[20];
    if (width > 20) width = 20;
    for (int k = 0; k < width; k++) {
        d[k] = (char)('0' + (int)(v % 10ull));
        v /= 10ull;
    }
    for (int k = width - 1; k >= 0; k--) s.put(d[k]);
}
template <typename S>
__device__ inline void put_zeros(S& s, int n)
{
    for (int i = 0; i < n; i++) s.put('0');
}

__device__ inline u64 pow10_u64(int k)   // k <= 19
{
    u64 r = 1;
    for (int i = 0; i < k && i < 19; i++) r *= 10ull;
    return r;
}
__device__ inline u128 pow10_u128(int k)   // k <= 38
{
    u128 r = 1;
    for (int i = 0; i < k && i < 38; i++) r *= 10u;
    return r;
}
__device__ inline int bit_length(u128 v)
{
    const u64 hi = (u64)(v >> 64), lo = (u64)v;
    if (hi) return 128 - __clzll((long long)hi);
    if (lo) return 64 - __clzll((long long)lo);
    return 0;
}
// q = a / b, r = a % b by shift and subtract (no 128-bit division routine exists for the device); b != 0
__device__ inline void divmod_u128(u128 a, u128 b, u128& q, u128& r)
{
    q = 0;
    r = 0;
    for (int i = bit_length(a) - 1; i >= 0; i--) {
        r = (r << 1) | ((a >> i) & 1u);
        if (r >= b) {
            r -= b;
            q |= (u128)1 << i;
        }
    }
}

// |value| (finite, > 0) correctly rounded, ties to even, to `sig` significant decimal digits: value ~ D * 10^q, 10^(sig-1) <= D < 10^sig.
// false: the magnitude is outside what 128 bits hold — below every magnitude the caller lets through, above only for a Double of
// 10^15 or more, which no column produces; the caller prints zeros for it.
__device__ inline bool vcf_sig_digits(double av, int sig, u64& D, int& q)
{
    const u64 bits = (u64)__double_as_longlong(av);
    int be = (int)((bits >> 52) & 0x7ff);
    u64 m = bits & ((1ull << 52) - 1);
    if (be == 0) be = 1;   // subnormal
    else m |= 1ull << 52;
    int e = be - 1075;     // av = m * 2^e
    const int tz = __ffsll((long long)m) - 1;
    m >>= tz;
    e += tz;               // m odd
    const u64 top = pow10_u64(sig);
    int exp10;
    if (e >= 0) {          // an integer
        if (bit_length((u128)m) + e > 128) return false;
        const u128 V = (u128)m << e;
        exp10 = 0;
        {
            u128 p = 10;
            while (exp10 < 38 && V >= p) {
                exp10++;
                if (exp10 < 38) p *= 10u;
            }
        }
        if (exp10 <= sig - 1) {
            D = (u64)V * pow10_u64(sig - 1 - exp10);
        } else {
            const int k = exp10 - (sig - 1);
            const u128 den = pow10_u128(k);
            u128 qq, rr;
            divmod_u128(V, den, qq, rr);
            D = (u64)qq;
            const u128 twice = rr << 1;   // rr < 10^k <= 10^32
            if (twice > den || (twice == den && (D & 1ull))) D++;
        }
    } else {
        const int s = -e;
        if (s > 126) return false;
        const u64 ip = s < 64 ? (m >> s) : 0ull;   // integer part
        if (ip > 0) {
            exp10 = 0;
            u64 p = 10;
            while (exp10 < 19 && ip >= p) {
                exp10++;
                if (exp10 < 19) p *= 10ull;
            }
        } else {   // the smallest j with m * 10^j >= 2^s
            int j = 1;
            u128 t = (u128)m * 10u;
            const u128 one = (u128)1 << s;
            while (t < one && j < 20) {
                t *= 10u;
                j++;
            }
            if (t < one) return false;
            exp10 = -j;
        }
        const int p = sig - 1 - exp10;
        if (p >= 0) {
            // m * 10^p: 53 + 73.1 bits at p = 22, the largest a Double reaches (sig 15, exp10 >= -8); a Single has 24 bits and p <= 15
            if (p > 38 || bit_length((u128)m) + (p * 3322 + 999) / 1000 + 1 > 128) return false;
            const u128 N = (u128)m * pow10_u128(p);
            const u128 Q = N >> s;
            const u128 rem = N & (((u128)1 << s) - 1u);
            const u128 half = (u128)1 << (s - 1);
            D = (u64)Q;
            if (rem > half || (rem == half && (D & 1ull))) D++;
        } else {   // more than `sig` integer digits and a fraction, which is never zero here (m odd, e < 0) and never a half of 10^k
            const int k = -p;
            if (k > 19) return false;
            const u64 den = pow10_u64(k);
            D = ip / den;
            const u64 r = ip % den;
            if (2ull * r >= den) D++;
        }
    }
    if (D >= top) {   // 9.9999995 -> 10.00000
        D = top / 10ull;
        exp10++;
    }
    q = exp10 - (sig - 1);
    return true;
}

// dotnet_fixed of vcf_format.cpp: `sig` significant digits of the exact value, then half-up on that digit string to `decimals`
template <typename S>
__device__ inline void put_fixed(S& s, double value, int sig, int decimals)
{
    if (value != value) {
        put_lit(s, "NaN");
        return;
    }
    const double av = value < 0 ? -value : value;
    if (av > 1.7976931348623157e308) {
        put_lit(s, value > 0 ? "Infinity" : "-Infinity");
        return;
    }
    const bool neg = value < 0;
    u64 D = 0;
    int q = 0;
    // Below 2 * 10^-(decimals+1) the digit behind the last printed one is at most 2 after the first rounding: zeros, whatever the rest
    // (a comparison, no scaling: the constant only has to lie between 10^-(decimals+1), below which 128 bits may not hold the product,
    // and 5 * 10^-(decimals+1), from which on a digit can round up)
    static const double kTiny[9] = {2e-1, 2e-2, 2e-3, 2e-4, 2e-5, 2e-6, 2e-7, 2e-8, 2e-9};
    const int dd = decimals < 0 ? 0 : (decimals > 8 ? 8 : decimals);
    bool zero = av == 0.0 || av < kTiny[dd];
    if (!zero) zero = !vcf_sig_digits(av, sig, D, q);
    if (!zero && q + decimals < 0) {   // digits are dropped: half-up on the first dropped one
        const int r = -(q + decimals);
        if (r > sig) {
            zero = true;
        } else {
            const u64 cut = pow10_u64(r - 1);
            const u64 lead = D / cut;             // the kept digits and the first dropped one
            D = lead / 10ull + ((lead % 10ull) >= 5ull ? 1ull : 0ull);
            q = -decimals;
            zero = D == 0;
        }
    }
    if (zero) {
        s.put('0');
        if (decimals > 0) {
            s.put('.');
            put_zeros(s, decimals);
        }
        return;
    }
    if (neg) s.put('-');
    if (q >= 0) {   // an integer: its digits, q zeros
        put_u64(s, D);
        put_zeros(s, q);
        if (decimals > 0) {
            s.put('.');
            put_zeros(s, decimals);
        }
    } else {        // -q <= decimals digits behind the point
        const u64 unit = pow10_u64(-q);
        put_u64(s, D / unit);
        if (decimals > 0) {
            s.put('.');
            put_digits(s, D % unit, -q);
            put_zeros(s, decimals + q);
        }
    }
}
template <typename S>
__device__ inline void put_single(S& s, float v, int decimals) { put_fixed(s, (double)v, 7, decimals); }
template <typename S>
__device__ inline void put_double(S& s, double v, int decimals) { put_fixed(s, v, 15, decimals); }

__device__ inline const char* genotype_string(int gt, int& len)   // VcfFormatter.MapGenotype
{
    switch (gt) {
    case PISCES_GT_HOM_ALT: len = 3; return "1/1";
    case PISCES_GT_HOM_REF: len = 3; return "0/0";
    case PISCES_GT_HET_ALT_REF: len = 3; return "0/1";
    case PISCES_GT_HET_ALT1_ALT2: len = 3; return "1/2";
    case PISCES_GT_REF_AND_NOCALL: len = 3; return "0/.";
    case PISCES_GT_ALT_AND_NOCALL: len = 3; return "1/.";
    case PISCES_GT_HEMI_ALT: len = 1; return "1";
    case PISCES_GT_HEMI_NOCALL: len = 1; return ".";
    case PISCES_GT_HEMI_REF: len = 1; return "0";
    case PISCES_GT_OTHERS: len = 3; return "2/2";
    default: len = 3; return "./.";
    }
}

// One body line of row i into `s`.  Returns 0, or the PISCES_E_* code vcf_format.cpp returns when it reaches this row (nothing the
// sink received counts then).
template <typename S>
__device__ inline int vcf_format_row(const VcfArgs& A, int64_t i, S& s)
{
    const PiscesCalledAllele r = A.recs[i];
    const int gt = PISCES_INFO_GENOTYPE(r.info);
    const bool is_ref = PISCES_INFO_CATEGORY(r.info) == PISCES_CAT_REFERENCE;
    const bool alt12 = gt == PISCES_GT_HET_ALT1_ALT2 || gt == PISCES_GT_ALT12_LIKE_NOCALL;
    const bool others = gt == PISCES_GT_OTHERS;
    const bool forced = (r.filter_bits >> PISCES_FILTER_FORCED_REPORT) & 1u;
    const int phase = PISCES_FILTERBITS_PHASE(r.filter_bits);
    // GetDepthCountInt
    int depth = is_ref ? r.reference_support : r.reference_support + r.allele_support;
    depth = depth > r.total_coverage ? depth : r.total_coverage;
    depth = depth > r.allele_support ? depth : r.allele_support;
    // alleles
    const uint8_t* ref_p = nullptr;
    const uint8_t* alt_p = nullptr;
    int32_t ref_n = 1, alt_n = 1;
    static const char kBase[8] = {'A', 'G', 'C', 'T', 'N', 'D', 'N', 'N'};
    const int32_t ci = A.cand_index ? A.cand_index[i] : -1;
    if (ci >= 0) {
        if (!A.cands || !A.alleles) return PISCES_E_INVALID_ARG;
        const PiscesCandidate c = A.cands[ci];
        ref_n = c.ref_len < 0 ? 0 : c.ref_len;
        alt_n = c.alt_len < 0 ? 0 : c.alt_len;
        ref_p = A.alleles + c.allele_offset;
        alt_p = ref_p + ref_n;
    }
    // filters: each refusal of the host's loop, in its order
    static const int kOrder[11] = {PISCES_FILTER_LOW_DEPTH, PISCES_FILTER_LOW_VARIANT_QSCORE, PISCES_FILTER_NO_CALL, PISCES_FILTER_STRAND_BIAS,
                                   PISCES_FILTER_AMPLICON_BIAS, PISCES_FILTER_INDEL_REPEAT_LENGTH, PISCES_FILTER_RMXN, PISCES_FILTER_LOW_VARIANT_FREQUENCY, PISCES_FILTER_FORCED_REPORT,
                                   PISCES_FILTER_MULTI_ALLELIC_SITE, PISCES_FILTER_LOW_GENOTYPE_QUALITY};
    for (int k = 0; k < 11; k++) {
        if (!(r.filter_bits & (1u << kOrder[k]))) continue;
        if (kOrder[k] == PISCES_FILTER_LOW_VARIANT_QSCORE && A.variant_quality_filter < 0) return PISCES_E_INVALID_ARG;
        if (kOrder[k] == PISCES_FILTER_RMXN && (A.rmxn_max_repeat_length < 0 || A.rmxn_min_repetitions < 0)) return PISCES_E_INVALID_ARG;
    }

    put_str(s, A.chrom, A.chrom_len);
    s.put('\t');
    put_i64(s, r.position);
    put_lit(s, "\t.\t");
    if (ref_p) {
        if constexpr (S::kCounts) s.skip((u64)ref_n);
        else
            for (int32_t k = 0; k < ref_n; k++) s.put((char)ref_p[k]);
    } else {
        s.put(kBase[PISCES_INFO_REF(r.info)]);
    }
    s.put('\t');
    const bool ref_like_gt = gt == PISCES_GT_HOM_REF || gt == PISCES_GT_REF_LIKE_NOCALL || gt == PISCES_GT_REF_AND_NOCALL ||
                             gt == PISCES_GT_HEMI_NOCALL || gt == PISCES_GT_HEMI_REF;
    if (ref_like_gt && !forced) {
        s.put('.');
    } else {
        const bool decorated = alt12 || others;
        const bool alt_first = phase == 1 || others;
        if (decorated && !alt_first) put_lit(s, "<M>,");
        if (alt_p) {
            if constexpr (S::kCounts) s.skip((u64)alt_n);
            else
                for (int32_t k = 0; k < alt_n; k++) s.put((char)alt_p[k]);
        } else {
            s.put(kBase[PISCES_INFO_ALT(r.info)]);
        }
        if (decorated && alt_first) put_lit(s, ",<M>");
    }
    s.put('\t');
    put_i64(s, r.variant_qscore);
    s.put('\t');
    {
        bool any = false;
        for (int k = 0; k < 11; k++) {
            if (!(r.filter_bits & (1u << kOrder[k]))) continue;
            if (kOrder[k] == PISCES_FILTER_INDEL_REPEAT_LENGTH && A.iname_len <= 0) continue;   // threshold null: no name, as the host's loop
            if (any) s.put(';');
            any = true;
            switch (kOrder[k]) {
            case PISCES_FILTER_LOW_DEPTH: put_lit(s, "LowDP"); break;
            case PISCES_FILTER_LOW_VARIANT_QSCORE: put_str(s, A.qname, A.qname_len); break;
            case PISCES_FILTER_NO_CALL: put_lit(s, "NC"); break;
            case PISCES_FILTER_STRAND_BIAS: put_lit(s, "SB"); break;
            case PISCES_FILTER_AMPLICON_BIAS: put_lit(s, "AB"); break;
            case PISCES_FILTER_INDEL_REPEAT_LENGTH: put_str(s, A.iname, A.iname_len); break;
            case PISCES_FILTER_RMXN: put_str(s, A.rname, A.rname_len); break;
            case PISCES_FILTER_LOW_VARIANT_FREQUENCY: put_lit(s, "LowVariantFreq"); break;
            case PISCES_FILTER_FORCED_REPORT: put_lit(s, "ForcedReport"); break;
            case PISCES_FILTER_MULTI_ALLELIC_SITE: put_lit(s, "MultiAllelicSite"); break;
            default: put_lit(s, "LowGQ"); break;
            }
        }
        if (!any) put_lit(s, "PASS");
    }
    put_lit(s, "\tDP=");
    put_i64(s, depth);
    s.put('\t');
    put_str(s, A.format, A.format_len);
    const bool with_gp = A.gp && A.gp[i].n > 0;
    if (with_gp) put_lit(s, ":GP");
    s.put('\t');
    // sample
    {
        int gl = 0;
        const char* g = genotype_string(gt, gl);
        put_str(s, g, gl);
    }
    s.put(':');
    put_i64(s, r.genotype_qscore);
    s.put(':');
    // CalledAllele.Frequency
    float freq = r.total_coverage == 0 ? 0.0f : (float)r.allele_support / (float)r.total_coverage;
    freq = freq > 1.0f ? 1.0f : freq;
    const int fd = A.freq_decimals;
    if (is_ref) {
        put_i64(s, r.allele_support);
        s.put(':');
        put_i64(s, depth);
        s.put(':');
        put_single(s, r.total_coverage == 0 ? 0.0f : 1.0f - freq, fd);
    } else if (alt12 || others) {
        const int other = depth - r.allele_support - r.reference_support;
        put_i64(s, r.reference_support);
        s.put(',');
        put_i64(s, (phase == 1 || others) ? r.allele_support : other);
        s.put(',');
        put_i64(s, (phase == 1 || others) ? other : r.allele_support);
        s.put(':');
        put_i64(s, depth);
        s.put(':');
        if (others) put_single(s, freq, fd);
        else put_double(s, 0.0 + (double)r.allele_support / (double)depth, fd);
    } else {
        put_i64(s, r.reference_support);
        s.put(',');
        put_i64(s, r.allele_support);
        s.put(':');
        put_i64(s, depth);
        s.put(':');
        put_single(s, freq, fd);
    }
    if (A.output_sb_nl) {
        const long long nl = A.noise_level_from_records ? (r.noise_level == INT16_MIN ? (long long)INT32_MIN : (long long)r.noise_level)
                                                        : (r.allele_support > 0 ? (long long)A.noise_level : 0ll);
        double gatk = r.allele_support > 0 ? 10.0 * log10(r.strand_bias_score) : 0.0;
        gatk = (-100.0 < gatk) ? gatk : -100.0;   // std::max(-100.0, gatk): a NaN comes out -100
        gatk = (0.0 < gatk) ? 0.0 : gatk;         // std::min(.., 0.0)
        s.put(':');
        put_i64(s, nl);
        s.put(':');
        put_double(s, gatk, 4);
    }
    if (A.output_nc) {
        const float all = (float)(r.total_coverage + r.num_no_calls);
        const float nc = all == 0.0f ? 0.0f : (float)r.num_no_calls / all;
        s.put(':');
        put_single(s, nc, 4);
    }
    if (with_gp) {
        const PiscesGenotypePosteriors g = A.gp[i];
        s.put(':');
        for (int k = 0; k < g.n && k < 6; k++) {
            if (k) s.put(',');
            put_single(s, g.gp[k], 2);
        }
    }
    s.put('\n');
    return 0;
}

// ---- the three launches --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowsPerChunk) void vcf_length_kernel(const VcfArgs A)
{
    const int64_t rows = vcf_rows(A);
    const int64_t i = (int64_t)blockIdx.x * kRowsPerChunk + threadIdx.x;
    u64 len = 0;
    if (i < rows) {
        CountSink s;
        const int rc = vcf_format_row(A, i, s);
        if (rc != 0) atomicMin(&A.ctrl[0], ((u64)i << 8) | (u64)(-rc));
        else len = s.n;
        if (len > 0xffffffffull) {   // a line of 4 GiB: candidate lengths that are no lengths
            atomicMin(&A.ctrl[0], ((u64)i << 8) | (u64)(-PISCES_E_INVALID_ARG));
            len = 0;
        }
    }
    if (i < A.n) A.row_len[i] = (uint32_t)len;
    __shared__ u64 wave_sum[kRowsPerChunk / 64];
    u64 v = len;
    for (int d = 32; d >= 1; d >>= 1) v += (u64)__shfl_down((long long)v, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (int w = 0; w < kRowsPerChunk / 64; w++) t += wave_sum[w];
        A.chunk_off[blockIdx.x] = (int64_t)t;
    }
}

__global__ __launch_bounds__(1024) void vcf_scan_kernel(const VcfArgs A, int64_t chunks)
{
    __shared__ int64_t part[1024];
    __shared__ int64_t carry_s;
    const int t = (int)threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < chunks; base += 1024) {
        const int64_t k = base + t;
        const int64_t mine = k < chunks ? A.chunk_off[k] : 0;
        part[t] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t add = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const int64_t carry = carry_s;
        if (k < chunks) A.chunk_off[k] = carry + part[t] - mine;
        __syncthreads();
        if (t == 1023) carry_s = carry + part[1023];
        __syncthreads();
    }
    if (t == 0) {
        const int64_t total = carry_s;
        const u64 err = A.ctrl[0];
        int64_t result = total;
        if (err != kNoError) result = -(int64_t)(err & 0xffull);
        const bool go = err == kNoError && total <= A.capacity;
        A.ctrl[1] = go ? 1ull : 0ull;
        *A.text_bytes = result;
        if (go && A.line_offsets) A.line_offsets[vcf_rows(A)] = total;
    }
}

__global__ __launch_bounds__(kRowsPerChunk) void vcf_write_kernel(const VcfArgs A)
{
    if (A.ctrl[1] == 0) return;   // an error or a short buffer: not a byte (uniform: no barrier is skipped by a part of the workgroup)
    __shared__ __attribute__((aligned(16))) char lds[kRowsPerChunk / 64][kWaveLdsBytes + 16];
    __shared__ u64 wave_sum[kRowsPerChunk / 64];
    const int64_t rows = vcf_rows(A);
    const int64_t i = (int64_t)blockIdx.x * kRowsPerChunk + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const bool live = i < rows;
    const u64 len = live ? (u64)A.row_len[i] : 0ull;
    u64 incl = len;   // inclusive prefix sum inside the wave
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = (u64)__shfl_up((long long)incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    u64 before = 0;
    for (int w = 0; w < wave; w++) before += wave_sum[w];
    const u64 wave_total = wave_sum[wave];
    const int64_t wave_start = A.chunk_off[blockIdx.x] + (int64_t)before;   // byte offset of the wave's first line
    const int64_t row_off = wave_start + (int64_t)(incl - len);
    if (live && A.line_offsets) A.line_offsets[i] = row_off;
    const bool staged = wave_total <= (u64)kWaveLdsBytes;                   // wave-uniform
    // the chunk sits in LDS at the global address's own offset inside 16 bytes: aligned LDS reads feed aligned global stores
    const int shift = (int)(((uintptr_t)A.text + (uintptr_t)wave_start) & 15u);
    char* stage = &lds[wave][0];
    if (live) {
        if (staged) {
            char* p = stage + shift + (int)(incl - len);
            ByteSink s{p, p + len};
            (void)vcf_format_row(A, i, s);
        } else {
            const int64_t end = row_off + (int64_t)len < A.capacity ? row_off + (int64_t)len : A.capacity;
            ByteSink s{A.text + row_off, A.text + (end > row_off ? end : row_off)};
            (void)vcf_format_row(A, i, s);
        }
    }
    __syncthreads();
    if (!staged || wave_total == 0) return;
    const int total = (int)wave_total;
    int head = (16 - shift) & 15;
    head = head < total ? head : total;
    const int body = (total - head) >> 4;
    const int tail = total - head - (body << 4);
    char* dst = A.text + wave_start;
    if (lane < head && wave_start + lane < A.capacity) dst[lane] = stage[shift + lane];
    for (int j = lane; j < body; j += 64) {
        const int o = head + (j << 4);
        if (wave_start + o + 16 <= A.capacity) *(uint4*)(dst + o) = *(const uint4*)(stage + shift + o);
    }
    const int o = head + (body << 4);
    if (lane < tail && wave_start + o + lane < A.capacity) dst[o + lane] = stage[shift + o + lane];
}

}  // namespace vcfdev
