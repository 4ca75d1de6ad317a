// nbhd_kernels.hip.h — Scylla's neighbourhoods from rows that lie in device memory (pisces_hip_nbhd_build_device): the decisions of nbhd.h
// a lane a row, the tables in the order the host entry gives.  Ten launches, no host wait:
//   nbhd_class_kernel       a lane a row: nbhd::row_bits (forced, eligible, passing, no allele bytes), the lowest row that descends and the
//                           lowest without allele bytes by atomicMin, the eligible rows of every wave by __ballot
//   nbhd_scan_rows_kernel   one workgroup over the WAVES' counts: the eligible rows in front of every wave, their total
//   nbhd_compact_kernel     a lane a row: eligible row e = its wave's prefix + the eligible lanes below; row, position and allele lengths of e
//   nbhd_link_kernel        a lane an eligible row: nbhd::link_bits from the rows on both sides (member, head, tail); a wave's heads and
//                           passing members by __ballot, its members' allele bytes by a butterfly sum
//   nbhd_scan_links_kernel  one workgroup over the waves' three sums
//   nbhd_index_kernel       a lane an eligible row: passing members and allele bytes in front of it (so a neighbourhood's counts are two
//                           differences, no atomics), the raw neighbourhood of a member = heads up to and including it - 1; the head writes
//                           the neighbourhood's first row, the tail its end; pos + max(ref_len, alt_len) into the neighbourhood's look-ahead
//                           by atomicMax (an integer maximum: the same whichever wave runs first)
//   nbhd_scan_nbhds_kernel  one workgroup over the raw neighbourhoods: nbhd::dropped, then kept neighbourhoods, sites, allele bytes and
//                           reference bytes in front of each; n_out and the go word (no error, every count within its capacity)
//   nbhd_sites_kernel       a lane a row for row_class; a lane an eligible row for its site: nbhd::sorted_slot inside its position group
//                           (a walk over the rows of ONE position of one neighbourhood: a handful), the bytes, site_row and site_original
//   nbhd_info_kernel        a lane a raw neighbourhood: [begin, end), nbhd::make_info (vead::bounds over the sorted sites)
//   nbhd_reference_kernel   a lane a reference byte, its neighbourhood by a search over the reference prefixes (one lane copying the 100 KB
//                           of one long neighbourhood took 10 ms: tools/nbhd_profile.py.  Measured, then replaced.)
// Offsets and order come from prefix sums over the input order only.  Only vector stores and plain C++; no fence inside a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nbhd.h"

namespace pisces {
namespace nbhddev {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;
enum Ctrl { kDescending = 0, kNoAlleles = 1, kEligible = 2, kRaw = 3, kGo = 4, kRefBytes = 5, kCtrlWords = 8 };
constexpr unsigned long long kNone = ~0ull;

struct Args {
    PiscesVennRows rows;
    PiscesNbhdCriteria criteria;
    PiscesNbhdOut out;
    const uint8_t* reference;      // the handle's, position 1 at [0]; null without one
    int64_t reference_len;
    int32_t n_waves;               // waves of a launch over the rows
    // scratch, sized by rows.n
    uint8_t* row_bits;             // [n] nbhd::RowBits
    int32_t* wave_eligible;        // [n_waves]
    int64_t* wave_eligible_prefix; // [n_waves]
    int32_t* e_row;                // [n] the row of eligible row e
    int32_t* e_pos;                // [n]
    int32_t* e_ref_len;            // [n]
    int32_t* e_alt_len;            // [n]
    uint8_t* e_link;               // [n] nbhd::LinkBits
    int64_t* wave_sum;             // [3 * n_waves] heads, passing members, members' allele bytes of a wave; scanned in place
    int64_t* e_bytes;              // [n + 1] members' allele bytes in front of e
    int32_t* e_passing;            // [n + 1] passing members in front of e
    int32_t* e_nbhd;               // [n] a member's raw neighbourhood
    int32_t* nb_first;             // [n / 2 + 1] eligible rows [first, end) of a raw neighbourhood
    int32_t* nb_end;
    int32_t* nb_look;              // [n / 2 + 1] max of position + max(ref_len, alt_len)
    int64_t* nb_prefix;            // [4 * (n / 2 + 1)] kept neighbourhoods, sites, allele bytes, reference bytes in front
    uint8_t* nb_keep;              // [n / 2 + 1]
    unsigned long long* ctrl;      // [kCtrlWords]
};

__device__ __forceinline__ int64_t row_count(const Args& K)
{
    if (!K.rows.count) return K.rows.n;
    const int64_t c = *K.rows.count;
    return c < 0 ? 0 : (c < K.rows.n ? c : K.rows.n);
}
__device__ __forceinline__ nbhd::View view_of(const Args& K)
{
    nbhd::View v;
    v.recs = K.rows.recs;
    v.cand_index = K.rows.cand_index;
    v.cands = K.rows.cands;
    v.alleles = K.rows.alleles;
    return v;
}
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// exclusive prefix sums of COLS columns over m items by ONE workgroup of kScanBlock lanes; total[] in every lane afterwards
template <int COLS, typename Load, typename Store>
__device__ __forceinline__ void scan_block(int64_t m, int64_t* total, Load load, Store store)
{
    __shared__ int64_t wave_sum[COLS][kScanBlock / 64];
    __shared__ int64_t carry[COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < COLS) carry[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t base = 0; base < m; base += kScanBlock) {
        const int64_t i = base + threadIdx.x;
        int64_t v[COLS], inc[COLS], b[COLS];
        for (int c = 0; c < COLS; c++) v[c] = 0;
        if (i < m) load(i, v);
        for (int c = 0; c < COLS; c++) inc[c] = v[c];
        for (int d = 1; d < 64; d <<= 1)
            for (int c = 0; c < COLS; c++) {
                const int64_t o = __shfl_up(inc[c], d);
                if (lane >= d) inc[c] += o;
            }
        if (lane == 63)
            for (int c = 0; c < COLS; c++) wave_sum[c][wave] = inc[c];
        __syncthreads();
        for (int c = 0; c < COLS; c++) {
            b[c] = carry[c];
            for (int w = 0; w < wave; w++) b[c] += wave_sum[c][w];
        }
        if (i < m) {
            int64_t ex[COLS];
            for (int c = 0; c < COLS; c++) ex[c] = b[c] + inc[c] - v[c];
            store(i, ex);
        }
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1)
            for (int c = 0; c < COLS; c++) carry[c] = b[c] + inc[c];
        __syncthreads();
    }
    for (int c = 0; c < COLS; c++) total[c] = carry[c];
}

__global__ __launch_bounds__(kBlock) void nbhd_class_kernel(Args K)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n = row_count(K);
    uint8_t bits = 0;
    if (r < n) {
        bits = nbhd::row_bits(view_of(K), K.criteria, r);
        K.row_bits[r] = bits;
        if (r > 0 && K.rows.recs[r].position < K.rows.recs[r - 1].position) atomicMin(K.ctrl + kDescending, (unsigned long long)r);
        if (bits & nbhd::kNoAlleles) atomicMin(K.ctrl + kNoAlleles, (unsigned long long)r);
    }
    const unsigned long long m = __ballot((bits & nbhd::kEligible) != 0);
    if ((threadIdx.x & 63) == 0) K.wave_eligible[(blockIdx.x * (unsigned)kBlock + threadIdx.x) >> 6] = __popcll(m);
}

__global__ __launch_bounds__(kScanBlock) void nbhd_scan_rows_kernel(Args K)
{
    int64_t total[1];
    scan_block<1>(K.n_waves, total, [&](int64_t i, int64_t* v) { v[0] = K.wave_eligible[i]; }, [&](int64_t i, const int64_t* ex) { K.wave_eligible_prefix[i] = ex[0]; });
    if (threadIdx.x == 0) K.ctrl[kEligible] = (unsigned long long)total[0];
}

__global__ __launch_bounds__(kBlock) void nbhd_compact_kernel(Args K)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n = row_count(K);
    const uint8_t bits = r < n ? K.row_bits[r] : (uint8_t)0;
    const bool is_eligible = (bits & nbhd::kEligible) != 0;
    const unsigned long long m = __ballot(is_eligible);
    if (!is_eligible) return;
    const int64_t e = K.wave_eligible_prefix[r >> 6] + __popcll(m & lanes_below(threadIdx.x & 63));
    int32_t ref_len, alt_len;
    nbhd::allele_lengths(view_of(K), r, &ref_len, &alt_len);
    K.e_row[e] = (int32_t)r;
    K.e_pos[e] = K.rows.recs[r].position;
    K.e_ref_len[e] = ref_len;
    K.e_alt_len[e] = alt_len;
    K.e_link[e] = (bits & nbhd::kPassing) ? nbhd::kIsPassing : 0;
}

// the three values a member adds to the sums in front of the rows behind it
struct LinkSums { bool head, passing; int64_t bytes; };
__device__ __forceinline__ LinkSums link_sums(const Args& K, int64_t e, int64_t n_eligible, uint8_t bits)
{
    LinkSums s = {false, false, 0};
    if (e < n_eligible && (bits & nbhd::kMember)) {
        s.head = (bits & nbhd::kHead) != 0;
        s.passing = (bits & nbhd::kIsPassing) != 0;
        s.bytes = (int64_t)K.e_ref_len[e] + K.e_alt_len[e];
    }
    return s;
}

__global__ __launch_bounds__(kBlock) void nbhd_link_kernel(Args K)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n_eligible = (int64_t)K.ctrl[kEligible];
    uint8_t bits = 0;
    if (e < n_eligible) {
        bits = (uint8_t)(nbhd::link_bits(view_of(K), K.e_row, n_eligible, e, K.criteria.phasing_distance) | (K.e_link[e] & nbhd::kIsPassing));
        K.e_link[e] = bits;
    }
    const LinkSums s = link_sums(K, e, n_eligible, bits);
    const unsigned long long heads = __ballot(s.head), passing = __ballot(s.passing);
    int64_t bytes = s.bytes;
    for (int d = 32; d > 0; d >>= 1) bytes += __shfl_xor(bytes, d);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = e >> 6;
        K.wave_sum[3 * w] = __popcll(heads);
        K.wave_sum[3 * w + 1] = __popcll(passing);
        K.wave_sum[3 * w + 2] = bytes;
    }
}

__global__ __launch_bounds__(kScanBlock) void nbhd_scan_links_kernel(Args K)
{
    int64_t total[3];
    scan_block<3>(K.n_waves, total, [&](int64_t i, int64_t* v) { for (int c = 0; c < 3; c++) v[c] = K.wave_sum[3 * i + c]; },
                  [&](int64_t i, const int64_t* ex) { for (int c = 0; c < 3; c++) K.wave_sum[3 * i + c] = ex[c]; });
    if (threadIdx.x == 0) K.ctrl[kRaw] = (unsigned long long)total[0];
}

__global__ __launch_bounds__(kBlock) void nbhd_index_kernel(Args K)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n_eligible = (int64_t)K.ctrl[kEligible];
    const int lane = threadIdx.x & 63;
    const uint8_t bits = e < n_eligible ? K.e_link[e] : (uint8_t)0;
    const LinkSums s = link_sums(K, e, n_eligible, bits);
    const unsigned long long heads = __ballot(s.head), passing = __ballot(s.passing);
    int64_t inc = s.bytes;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (e >= n_eligible) return;
    const int64_t w = e >> 6;
    const int64_t bytes_front = K.wave_sum[3 * w + 2] + inc - s.bytes;
    const int64_t passing_front = K.wave_sum[3 * w + 1] + __popcll(passing & lanes_below(lane));
    K.e_bytes[e] = bytes_front;
    K.e_passing[e] = (int32_t)passing_front;
    if (e == n_eligible - 1) {
        K.e_bytes[n_eligible] = bytes_front + s.bytes;
        K.e_passing[n_eligible] = (int32_t)(passing_front + (s.passing ? 1 : 0));
    }
    if (!(bits & nbhd::kMember)) return;
    const int32_t nb = (int32_t)(K.wave_sum[3 * w] + __popcll(heads & lanes_below(lane)) + (s.head ? 1 : 0) - 1);
    K.e_nbhd[e] = nb;
    if (bits & nbhd::kHead) K.nb_first[nb] = (int32_t)e;
    if (bits & nbhd::kTail) K.nb_end[nb] = (int32_t)e + 1;
    const int64_t longest = K.e_ref_len[e] > K.e_alt_len[e] ? K.e_ref_len[e] : K.e_alt_len[e];
    const int64_t look = (int64_t)K.e_pos[e] + longest;
    atomicMax(K.nb_look + nb, (int32_t)(look > 0x7FFFFFFFll ? 0x7FFFFFFFll : look));
}

__global__ __launch_bounds__(kScanBlock) void nbhd_scan_nbhds_kernel(Args K)
{
    const int64_t n_raw = (int64_t)K.ctrl[kRaw];
    int64_t total[4];
    scan_block<4>(n_raw, total,
                  [&](int64_t nb, int64_t* v) {
                      const int32_t first = K.nb_first[nb], end = K.nb_end[nb];
                      const int64_t n_sites = end - first, n_passing = K.e_passing[end] - K.e_passing[first];
                      const bool keep = !nbhd::dropped(n_passing, n_sites - n_passing, K.criteria.min_passing_variants_in_nbhd);
                      K.nb_keep[nb] = keep ? 1 : 0;
                      if (!keep) return;
                      const int32_t first_pos = K.e_pos[first], look = K.nb_look[nb];
                      v[0] = 1;
                      v[1] = n_sites;
                      v[2] = K.e_bytes[end] - K.e_bytes[first];
                      v[3] = look > first_pos ? (int64_t)look - first_pos : 0;
                  },
                  [&](int64_t nb, const int64_t* ex) { for (int c = 0; c < 4; c++) K.nb_prefix[4 * nb + c] = ex[c]; });
    if (threadIdx.x != 0) return;
    const unsigned long long descending = K.ctrl[kDescending], no_alleles = K.ctrl[kNoAlleles];
    int64_t o[6] = {total[0], total[1], total[2], total[3], n_raw, (int64_t)K.ctrl[kEligible]};
    bool go = total[0] <= K.out.nbhd_capacity && total[1] <= K.out.site_capacity && total[2] <= K.out.allele_capacity && total[3] <= K.out.ref_capacity;
    if (descending != kNone || no_alleles != kNone || total[2] > 0x7FFFFFFFll || total[3] > 0x7FFFFFFFll) {
        go = false;
        for (int c = 0; c < 6; c++) o[c] = 0;
        o[0] = (descending != kNone || no_alleles != kNone) ? PISCES_E_INVALID_ARG : PISCES_E_UNSUPPORTED;
        if (descending != kNone) o[2] = (int64_t)descending;
        else if (no_alleles != kNone) { o[1] = 1; o[2] = (int64_t)no_alleles; }
    }
    for (int c = 0; c < 6; c++) K.out.n_out[c] = o[c];
    K.ctrl[kGo] = go ? 1 : 0;
    K.ctrl[kRefBytes] = (unsigned long long)total[3];
}

__global__ __launch_bounds__(kBlock) void nbhd_sites_kernel(Args K)
{
    if (!K.ctrl[kGo]) return;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (K.out.row_class && t < row_count(K)) {
        const uint8_t bits = K.row_bits[t];
        if (!(bits & nbhd::kEligible)) K.out.row_class[t] = (bits & nbhd::kForced) ? PISCES_NBHD_ROW_FORCED : PISCES_NBHD_ROW_INELIGIBLE;
    }
    const int64_t e = t;
    if (e >= (int64_t)K.ctrl[kEligible]) return;
    const int32_t row = K.e_row[e];
    if (!(K.e_link[e] & nbhd::kMember)) {
        if (K.out.row_class) K.out.row_class[row] = PISCES_NBHD_ROW_LONE;
        return;
    }
    const int32_t nb = K.e_nbhd[e];
    const bool keep = K.nb_keep[nb] != 0;
    if (K.out.row_class) K.out.row_class[row] = keep ? PISCES_NBHD_ROW_KEPT : PISCES_NBHD_ROW_DROPPED;
    if (!keep) return;
    const int64_t first = K.nb_first[nb], end = K.nb_end[nb];
    int64_t group, bytes_in_front;
    const int64_t slot = nbhd::sorted_slot(K.e_pos, K.e_ref_len, K.e_alt_len, first, end, e, &group, &bytes_in_front);
    const int64_t site_base = K.nb_prefix[4 * (int64_t)nb + 1], byte_base = K.nb_prefix[4 * (int64_t)nb + 2];
    const int64_t s = site_base + (slot - first);
    const int64_t offset = byte_base + (K.e_bytes[group] - K.e_bytes[first]) + bytes_in_front;
    PiscesVeadSite site;
    site.position = K.e_pos[e];
    site.ref_len = K.e_ref_len[e];
    site.alt_len = K.e_alt_len[e];
    site.allele_offset = (int32_t)offset;
    K.out.sites[s] = site;
    nbhd::copy_alleles(view_of(K), row, K.out.alleles + offset);
    K.out.site_row[s] = row;
    K.out.site_original[site_base + (e - first)] = row;
}

__global__ __launch_bounds__(kBlock) void nbhd_info_kernel(Args K)
{
    if (!K.ctrl[kGo]) return;
    const int64_t nb = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (nb >= (int64_t)K.ctrl[kRaw] || !K.nb_keep[nb]) return;
    const int32_t first = K.nb_first[nb], end = K.nb_end[nb];
    const int64_t k = K.nb_prefix[4 * nb], site_begin = K.nb_prefix[4 * nb + 1], ref_offset = K.nb_prefix[4 * nb + 3];
    const int32_t n_sites = end - first, n_passing = K.e_passing[end] - K.e_passing[first];
    PiscesVeadNeighborhood range;
    range.site_begin = (int32_t)site_begin;
    range.site_end = (int32_t)site_begin + n_sites;
    K.out.neighbourhoods[k] = range;
    const PiscesNbhdInfo info = nbhd::make_info(K.out.sites, range.site_begin, range.site_end, (int32_t)nb, n_passing, n_sites - n_passing, ref_offset);
    K.out.info[k] = info;
}

// a lane a reference byte (grid-stride: the launch is sized by the capacity): its neighbourhood is the last raw one whose reference prefix
// is at or below it, which is a kept one: a dropped neighbourhood shares its prefix with the one behind it
__global__ __launch_bounds__(kBlock) void nbhd_reference_kernel(Args K)
{
    if (!K.ctrl[kGo]) return;
    const int64_t n_bytes = (int64_t)K.ctrl[kRefBytes], n_raw = (int64_t)K.ctrl[kRaw];
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n_bytes; j += (int64_t)gridDim.x * kBlock) {
        int64_t a = 0, z = n_raw;
        while (z - a > 1) {
            const int64_t m = a + (z - a) / 2;
            if (K.nb_prefix[4 * m + 3] <= j) a = m; else z = m;
        }
        const int32_t first_pos = K.e_pos[K.nb_first[a]], look = K.nb_look[a];
        vead::Bounds b;
        b.first = first_pos;
        b.last_with_look_ahead = look > first_pos ? look : first_pos;
        b.soft_clip_end_before = b.soft_clip_pos_after = 0;
        K.out.ref_bytes[j] = nbhd::reference_byte(K.reference, K.reference_len, b, j - K.nb_prefix[4 * a + 3]);
    }
}

}  // namespace nbhddev
}  // namespace pisces
