// vead_kernels.hip.h — Scylla's read pass on reads that lie in device memory (pisces_hip_vead_groups_device): the states of vead.h per
// (neighbourhood, read), grouped per neighbourhood, in the order the host entry gives.
//   vead_spans_kernel     one lane a read: EndPosition, the two soft-clip flags, the sortedness check (first violation by atomicMin), and the
//                         batch's longest reach max(EndPosition - Position, 0) (one atomicMax a wave)
//   vead_ranges_kernel    one lane a neighbourhood: [lo, hi) by two binary searches over the POSITIONS, which ascend.  lo: the first read
//                         with Position >= SoftClipEndBeforeNbhd - longest reach: every read the skip test keeps (EndPosition >=
//                         FirstPositionOfInterest >= SoftClipEndBeforeNbhd) and every read the clip test counts (Position or EndPosition >=
//                         SoftClipEndBeforeNbhd) lies at or behind it; the reads in front that do neither cost a lane each.  hi: the first
//                         read with Position > LastPositionOfInterestWithLookAhead.  The read AT hi is the one the reference stops at; it
//                         is still clip-tested there (VeadGroupSource.cs:56-66 come before the break), so the pairs of a neighbourhood
//                         are the reads [lo, min(hi + 1, n)).
//                         (A running maximum of EndPosition, searched instead, bounds lo no better once one long read lies in front — it
//                         holds every later lo back just the same — and its scan by one workgroup took 440-520 us for 400 000 reads,
//                         a third of the call: tools/vead_profile.py.  Measured, then removed.)
//   -- the host reads the ranges and the verdict, lays the (neighbourhood, read) pairs out neighbourhood-major and sizes the scratch --
//   vead_states_kernel    one wave per (neighbourhood, 64 consecutive pairs), one lane a read: the filter, then vead.h's site_state per
//                         site packed 2 bits a site.  The wave's clipped / used counts by __ballot and one atomicAdd each.
//   vead_group_kernel     one lane a pair that is a vead: an open-addressing table per neighbourhood (twice its pairs, a power of two,
//                         so it never fills) whose slots hold a PAIR INDEX: claimed by atomicCAS, lowered by atomicMin by every pair whose
//                         full key equals the occupant's.  An occupant only ever gives way to a pair with the same key, so a slot's key
//                         never changes; the keys were complete when the kernel before ended, so no fence is needed to read them.
//   vead_mark_kernel      one lane a slot: the slot's count to its lowest pair.  Which slot a key landed in depends on who came first;
//                         (key -> lowest pair, count) does not.
//   vead_count_kernel     one wave per 64 pairs: how many of them represent a group (__ballot)
//   vead_scan_kernel      one workgroup over the WAVES' counts (a 64th of the pairs): groups and state bytes in front of every wave.
//                         Pairs are neighbourhood-major and read-minor, so the pair order of the representatives IS the contract's
//                         group order.  (Scanned pair by pair this kernel took 380-540 us for 200 000 pairs.)
//   vead_emit_kernel      one wave per 64 pairs: a representative's group index is its wave's prefix plus the representatives in the
//                         lanes below it; it writes its group and unpacks its states.  Then one lane a neighbourhood: its info.
// Only vector stores and plain C++; no fence inside a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vead.h"

namespace pisces {
namespace veaddev {

constexpr int32_t kNoPair = 0x7F7F7F7F;   // an empty slot (a byte pattern: the table is cleared by a memset)
constexpr int kScanBlock = 1024;

struct Plan {            // one neighbourhood, made by the host from the ranges
    int32_t lo, n_pairs; // the reads [lo, lo + n_pairs)
    int32_t hi;          // reads at or behind hi are only clip-tested
    int32_t words;       // 64-bit words of a key
    int64_t pair_base, key_base, table_base;
    uint32_t table_mask; // slots - 1 (0 with no pairs: no slot is touched)
    int32_t work_base;   // the neighbourhood's first entry of `work`
};

struct Args {
    // the reads
    const int32_t* position;
    const int32_t* cigar_offset;
    const uint8_t* cigar_op;
    const uint32_t* cigar_len;
    const int32_t* seq_offset;
    const uint8_t* bases;
    const uint8_t* quals;
    int32_t n_reads;
    int32_t min_q, min_sites;
    // the neighbourhoods (uploaded)
    const PiscesVeadSite* sites;
    const uint8_t* alleles;
    const PiscesVeadNeighborhood* nbhd;
    const vead::Bounds* bounds;
    const Plan* plan;
    const int2* work;    // (neighbourhood, first pair of the wave inside it)
    int32_t n_nbhd;
    int32_t n_work;
    int64_t n_pairs, n_slots;
    // scratch
    int32_t* end;            // [n_reads] EndPosition
    uint8_t* clip;           // [n_reads] bit0 starts with S, bit1 ends with S
    int32_t* range;          // [2 * n_nbhd] lo, hi
    unsigned long long* ctrl;// [0] lowest read whose position descends (all ones: none); [1] the longest reach of a read
    unsigned long long* keys;
    uint8_t* is_vead;        // [n_pairs]
    int32_t* table;          // [n_slots] lowest pair of the slot's key
    int32_t* slot_count;     // [n_slots]
    int32_t* pair_count;     // [n_pairs] a representative's group count, 0 otherwise
    int32_t* work_groups;    // [n_work] representatives among a wave's pairs
    int64_t* prefix;         // [2 * (n_work + 1)] groups, state bytes in front of a wave's pairs; the totals at n_work
    int32_t* counts;         // [2 * n_nbhd] clipped, used
    PiscesVeadOut out;
};

__global__ __launch_bounds__(256) void vead_spans_kernel(Args K)
{
    const int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    int32_t reach = 0;
    if (r < K.n_reads) {
        const int32_t c0 = K.cigar_offset[r], n = K.cigar_offset[r + 1] - c0;
        const int32_t pos = K.position[r];
        int64_t end = vead::end_position(pos, K.cigar_op + c0, K.cigar_len + c0, n);
        if (end > 0x7FFFFFFFll) end = 0x7FFFFFFFll;
        K.end[r] = (int32_t)end;
        K.clip[r] = (uint8_t)((n > 0 && K.cigar_op[c0] == 'S' ? 1 : 0) | (n > 0 && K.cigar_op[c0 + n - 1] == 'S' ? 2 : 0));
        if (r > 0 && pos < K.position[r - 1]) atomicMin(K.ctrl, (unsigned long long)r);
        const int64_t d = end - pos;
        reach = d > 0 ? (int32_t)(d > 0x7FFFFFFFll ? 0x7FFFFFFFll : d) : 0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t o = __shfl_xor(reach, d);
        reach = o > reach ? o : reach;
    }
    // load and test before the atomic: reads of one library reach alike, the maximum stands after a few waves (every wave's atomic on the
    // one word took this kernel from 5 to 75 us for 400 000 reads)
    if ((threadIdx.x & 63) == 0 && (unsigned long long)reach > __hip_atomic_load(K.ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(K.ctrl + 1, (unsigned long long)reach);
}

__global__ __launch_bounds__(256) void vead_ranges_kernel(Args K)
{
    const int32_t n = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (n >= K.n_nbhd) return;
    const vead::Bounds b = K.bounds[n];
    const int64_t from = (int64_t)b.soft_clip_end_before - (int64_t)K.ctrl[1];
    int32_t a = 0, z = K.n_reads;      // first read with position >= soft_clip_end_before - longest reach
    while (a < z) { const int32_t m = a + (z - a) / 2; if ((int64_t)K.position[m] >= from) z = m; else a = m + 1; }
    K.range[2 * n] = a;
    a = 0; z = K.n_reads;              // first read with position > last_with_look_ahead
    while (a < z) { const int32_t m = a + (z - a) / 2; if (K.position[m] > b.last_with_look_ahead) z = m; else a = m + 1; }
    K.range[2 * n + 1] = a;
}

__global__ __launch_bounds__(64) void vead_states_kernel(Args K)
{
    const int2 w = K.work[blockIdx.x];
    const Plan P = K.plan[w.x];
    const vead::Bounds b = K.bounds[w.x];
    const PiscesVeadNeighborhood nb = K.nbhd[w.x];
    const int32_t n_sites = nb.site_end - nb.site_begin;
    const int32_t k = w.y + (int32_t)threadIdx.x;   // the pair inside the neighbourhood
    bool is_clipped = false, used = false;
    if (k < P.n_pairs) {
        const int32_t r = P.lo + k;
        const int64_t pair = P.pair_base + k;
        const int32_t pos = K.position[r], end = K.end[r];
        const uint8_t cl = K.clip[r];
        used = vead::scan_read(pos, end, cl & 1, cl & 2, b, &is_clipped) == vead::kUse;   // (kPast: the read at hi, by sortedness)
        uint8_t vead_flag = 0;
        if (used) {
            vead::ReadView rv;
            const int32_t c0 = K.cigar_offset[r], s0 = K.seq_offset[r];
            rv.position = pos;
            rv.op = K.cigar_op + c0;
            rv.len = K.cigar_len + c0;
            rv.n_cigar = K.cigar_offset[r + 1] - c0;
            rv.bases = K.bases + s0;
            rv.quals = K.quals + s0;
            rv.n_bases = K.seq_offset[r + 1] - s0;
            const int64_t last = vead::last_position(rv);
            unsigned long long* const key = K.keys + P.key_base + (int64_t)k * P.words;
            int32_t found = 0;
            for (int32_t w0 = 0; w0 < P.words; w0++) {
                unsigned long long word = 0;
                const int32_t s_end = n_sites - w0 * 32 < 32 ? n_sites - w0 * 32 : 32;
                for (int32_t s = 0; s < s_end; s++) {
                    bool in_range;
                    const uint8_t st = vead::site_state(rv, K.min_q, last, K.sites[nb.site_begin + w0 * 32 + s], K.alleles, &in_range);
                    found += in_range ? 1 : 0;
                    word |= (unsigned long long)st << (2 * s);
                }
                key[w0] = word;
            }
            vead_flag = found >= K.min_sites ? 1 : 0;
        }
        K.is_vead[pair] = vead_flag;
    }
    const unsigned long long mc = __ballot(is_clipped), mu = __ballot(used);
    if (threadIdx.x == 0) {
        if (mc) atomicAdd(K.counts + 2 * w.x, __popcll(mc));
        if (mu) atomicAdd(K.counts + 2 * w.x + 1, __popcll(mu));
    }
}

__device__ __forceinline__ bool same_key(const unsigned long long* a, const unsigned long long* b, int32_t words)
{
    for (int32_t i = 0; i < words; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(64) void vead_group_kernel(Args K)
{
    const int2 w = K.work[blockIdx.x];
    const Plan P = K.plan[w.x];
    const int32_t k = w.y + (int32_t)threadIdx.x;
    if (k >= P.n_pairs || !K.is_vead[P.pair_base + k]) return;
    const unsigned long long* const keys = K.keys + P.key_base;
    const unsigned long long* const key = keys + (int64_t)k * P.words;
    unsigned long long hash = 0x9E3779B97F4A7C15ull;   // the hash decides where to look, never what is equal
    for (int32_t i = 0; i < P.words; i++) { hash ^= key[i]; hash *= 0xFF51AFD7ED558CCDull; hash ^= hash >> 32; }
    int32_t* const table = K.table + P.table_base;
    const int32_t me = (int32_t)(P.pair_base + k);   // slots hold pair indices of the whole call (below 2^31: the host has checked)
    uint32_t i = (uint32_t)hash & P.table_mask;
    for (uint32_t probes = 0; probes <= P.table_mask; probes++, i = (i + 1) & P.table_mask) {
        int32_t cur = __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kNoPair) {
            cur = atomicCAS(table + i, kNoPair, me);
            if (cur == kNoPair) cur = me;
        }
        if (cur != me && !same_key(key, keys + (cur - P.pair_base) * P.words, P.words)) continue;
        if (cur > me) atomicMin(table + i, me);
        atomicAdd(K.slot_count + P.table_base + i, 1);
        return;
    }
}

__global__ __launch_bounds__(256) void vead_mark_kernel(Args K)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n_slots) return;
    const int32_t rep = K.table[i];
    if (rep != kNoPair) K.pair_count[rep] = K.slot_count[i];
}

__global__ __launch_bounds__(64) void vead_count_kernel(Args K)
{
    const int2 w = K.work[blockIdx.x];
    const Plan P = K.plan[w.x];
    const int32_t k = w.y + (int32_t)threadIdx.x;
    const bool rep = k < P.n_pairs && K.pair_count[P.pair_base + k] > 0;
    const unsigned long long m = __ballot(rep);
    if (threadIdx.x == 0) K.work_groups[blockIdx.x] = __popcll(m);
}

// prefix[2 * w], prefix[2 * w + 1]: groups and state bytes in front of the pairs of wave w; entry n_work holds the totals
__global__ __launch_bounds__(kScanBlock) void vead_scan_kernel(Args K)
{
    __shared__ int64_t wave_sum[2][kScanBlock / 64];
    __shared__ int64_t carry[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2) carry[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t base = 0; base < K.n_work; base += kScanBlock) {
        const int64_t w = base + threadIdx.x;
        int64_t g = 0, s = 0;
        if (w < K.n_work) {
            const PiscesVeadNeighborhood nb = K.nbhd[K.work[w].x];
            g = K.work_groups[w];
            s = g * (nb.site_end - nb.site_begin);
        }
        int64_t ig = g, is = s;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t og = __shfl_up(ig, d), os = __shfl_up(is, d);
            if (lane >= d) { ig += og; is += os; }
        }
        if (lane == 63) { wave_sum[0][wave] = ig; wave_sum[1][wave] = is; }
        __syncthreads();
        int64_t bg = carry[0], bs = carry[1];
        for (int v = 0; v < wave; v++) { bg += wave_sum[0][v]; bs += wave_sum[1][v]; }
        if (w < K.n_work) { K.prefix[2 * w] = bg + ig - g; K.prefix[2 * w + 1] = bs + is - s; }
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) { carry[0] = bg + ig; carry[1] = bs + is; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        K.prefix[2 * (int64_t)K.n_work] = carry[0];
        K.prefix[2 * (int64_t)K.n_work + 1] = carry[1];
        K.out.n_out[0] = carry[0];
        K.out.n_out[1] = carry[1];
        K.out.n_out[2] = 0;
    }
}

__global__ __launch_bounds__(64) void vead_emit_kernel(Args K)
{
    const int2 w = K.work[blockIdx.x];
    const Plan P = K.plan[w.x];
    const int32_t k = w.y + (int32_t)threadIdx.x;
    const int64_t pair = P.pair_base + k;
    const bool rep = k < P.n_pairs && K.pair_count[pair] > 0;
    const unsigned long long m = __ballot(rep);
    const int64_t total_g = K.prefix[2 * (int64_t)K.n_work], total_s = K.prefix[2 * (int64_t)K.n_work + 1];
    if (!rep || total_g > K.out.group_capacity || total_s > K.out.state_capacity) return;   // short capacities: only the counts
    const int32_t n_sites = K.nbhd[w.x].site_end - K.nbhd[w.x].site_begin;
    const int32_t below = __popcll(m & ((1ull << threadIdx.x) - 1ull));
    PiscesVeadGroup g;
    g.neighborhood = w.x;
    g.first_read = P.lo + k;
    g.n_veads = K.pair_count[pair];
    g.pad = 0;
    g.state_offset = K.prefix[2 * (int64_t)blockIdx.x + 1] + (int64_t)below * n_sites;
    K.out.groups[K.prefix[2 * (int64_t)blockIdx.x] + below] = g;
    const unsigned long long* const key = K.keys + P.key_base + (int64_t)k * P.words;
    uint8_t* const st = K.out.states + g.state_offset;
    for (int32_t s = 0; s < n_sites; s++) st[s] = (uint8_t)((key[s >> 5] >> (2 * (s & 31))) & 3u);
}

// one lane a neighbourhood: sized by the input, always written
__global__ __launch_bounds__(256) void vead_info_kernel(Args K)
{
    const int32_t t = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (t >= K.n_nbhd) return;
    const Plan P = K.plan[t];
    const vead::Bounds b = K.bounds[t];
    const int32_t work_end = P.work_base + (P.n_pairs + 63) / 64;
    PiscesVeadNeighborhoodInfo o;
    o.first = b.first;
    o.last_with_look_ahead = b.last_with_look_ahead;
    o.soft_clip_end_before = b.soft_clip_end_before;
    o.soft_clip_pos_after = b.soft_clip_pos_after;
    o.group_begin = (int32_t)K.prefix[2 * (int64_t)P.work_base];
    o.n_groups = (int32_t)(K.prefix[2 * (int64_t)work_end] - K.prefix[2 * (int64_t)P.work_base]);
    o.n_clipped_reads = K.counts[2 * t];
    o.n_reads_used = K.counts[2 * t + 1];
    K.out.info[t] = o;
}

}  // namespace veaddev
}  // namespace pisces
