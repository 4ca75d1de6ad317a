// vqr_kernels.hip.h — VariantQualityRecalibration on device-resident rows (pisces_hip_vqr_count_device, pisces_hip_vqr_apply_device):
// the two per-row passes of src/exe/VariantQualityRecalibration between pisces_hip_compact_records / a flush and the VCF writer.  The
// decisions are vqr.h, the source the host entries use; the q-score is poisson_qscore_core of device_math.hip.h, the function the call
// phase evaluates.  Neither kernel is launched by a handle that does not call the two entries.
#pragma once
#include "device_math.hip.h"
#include "vqr.h"

namespace pisces {
namespace vqrdev {

constexpr int kBlock = 256;                               // rows a workgroup
constexpr int kStage = kBlock + 2 * vqr::kMaxExtent;      // its rows and the halo on both sides
constexpr int kBins = vqr::kCategories + 1;               // the 16 categories and NumPossibleVariants: the layout of PiscesVqrCounts

// the rows a call may read: min(n, *d_count), nothing at or beyond it (beyond the count a buffer holds garbage)
__device__ __forceinline__ int64_t rows_there(int64_t n, const int32_t* d_count)
{
    if (!d_count) return n;
    const int64_t c = *d_count;
    return c < 0 ? 0 : (c < n ? c : n);
}

// SignatureSorter.StrainVcf (SignatureSorter.cs:50-82) over rows [lo, hi): one lane per row.  A lane needs its row's position, coverage and
// the dword at byte 60 (filter_bits | info << 16), 12 of the 64 bytes.  The window of EdgeIssueCountData is the `extent` rows before and
// after, in row order: a workgroup stages (position, coverage) of its 256 rows and of `extent` halo rows on either side in LDS (3 KiB),
// once, and every lane's window — up to 128 neighbours — is read from there instead of 128 times from global.  Totals: LDS integer adds
// inside the workgroup, then one agent-scope 64-bit integer add per non-zero bin per workgroup; integer sums, so the totals do not depend
// on the launch geometry or on arrival order.  No float atomics, no fence, no workgroup waits for another.
__global__ __launch_bounds__(kBlock) void vqr_count_kernel(const PiscesCalledAllele* __restrict__ recs, int64_t n, const int32_t* __restrict__ d_count,
                                                           int64_t lo, int64_t hi, int32_t extent /* < 0: no edge counts */,
                                                           unsigned long long* __restrict__ counts /* [2][kBins] */, uint8_t* __restrict__ suspect)
{
    __shared__ int32_t s_pos[kStage], s_cov[kStage];
    __shared__ uint32_t s_bins[2 * kBins];
    const int64_t m = rows_there(n, d_count);
    const int64_t end = hi < m ? hi : m;
    const int64_t first = lo + (int64_t)blockIdx.x * kBlock;   // this workgroup's row 0
    const int tid = (int)threadIdx.x;
    const bool edges = extent >= 0;
    const int e = edges ? extent : 0;
    if (tid < 2 * kBins) s_bins[tid] = 0;
    // stage rows [first - e, first + kBlock + e) that exist
    for (int j = tid; j < kBlock + 2 * e; j += kBlock) {
        const int64_t g = first - e + j;
        if (g >= 0 && g < m) {
            const int32_t* w = reinterpret_cast<const int32_t*>(recs + g);
            s_pos[j] = w[0];
            s_cov[j] = w[1];
        }
    }
    __syncthreads();
    const int64_t i = first + tid;
    if (i < end) {   // (i >= lo by construction)
        const uint32_t w60 = reinterpret_cast<const uint32_t*>(recs + i)[15];
        const int32_t cat = vqr::count_category(w60);
        atomicAdd(&s_bins[vqr::kCategories], 1u);                       // CountData.Add: every row is a possible variant (:65)
        if (cat != vqr::kReference) atomicAdd(&s_bins[cat], 1u);       // :67-69
        if (edges) {
            const int me = tid + e;
            const bool edge = vqr::at_edge(i, s_pos[me], s_cov[me], e, [&](int64_t g, int32_t* p, int32_t* c) {
                if (g < 0 || g >= m) return false;
                const int j = (int)(g - (first - e));   // within [0, kBlock + 2e): |g - i| <= e
                *p = s_pos[j];
                *c = s_cov[j];
                return true;
            });
            const bool is_suspect = edge && cat != vqr::kReference;     // EdgeIssueCountData.Add (:38-53)
            if (edge) atomicAdd(&s_bins[kBins + vqr::kCategories], 1u);
            if (is_suspect) atomicAdd(&s_bins[kBins + cat], 1u);
            suspect[i] = is_suspect ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid < 2 * kBins && s_bins[tid] != 0) atomicAdd(&counts[tid], (unsigned long long)s_bins[tid]);
}

// VcfUpdater over QualityRecalibration.UpdateAllele: one lane per row, the four fields rewritten in place.  The tables travel in the kernel
// arguments.  Only a lane whose category is in a table reads more than its dword at byte 60, and only such a lane evaluates the Poisson
// score.  "Some row at my position is a suspect" (AmpliconEdgeVariantsList[chromosome].Contains(position)) is a scan left and right over
// the suspect bytes while the position stays equal, inside [0, rows): rows of one position are neighbours.
__global__ __launch_bounds__(kBlock) void vqr_apply_kernel(PiscesCalledAllele* recs /* lanes read their neighbours' positions */, int64_t n, const int32_t* __restrict__ d_count,
                                                           const uint8_t* __restrict__ suspect, const vqr::ApplyTables T,
                                                           unsigned long long* __restrict__ n_changed)
{
    __shared__ uint32_t s_changed;
    const int64_t m = rows_there(n, d_count);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
    bool changed = false;
    if (i < m) {
        const uint32_t w60 = reinterpret_cast<const uint32_t*>(recs + i)[15];
        const int32_t cat = vqr::update_category(w60);
        if (vqr::in_a_table(T, cat)) {
            PiscesCalledAllele* row = recs + i;
            const int32_t position = row->position;
            bool at_suspect = false;
            if (vqr::in_edge_table(T, cat) && suspect) {
                at_suspect = suspect[i] != 0;
                for (int64_t j = i - 1; !at_suspect && j >= 0 && recs[j].position == position; j--) at_suspect = suspect[j] != 0;
                for (int64_t j = i + 1; !at_suspect && j < m && recs[j].position == position; j++) at_suspect = suspect[j] != 0;
            }
            vqr::RowQ r;
            r.variant_qscore = row->variant_qscore;
            r.genotype_qscore = row->genotype_qscore;
            r.noise_level = row->noise_level;
            r.filter_bits = w60 & 0xffffu;
            r.changed = false;
            const double ln10 = T.ln10;
            vqr::update_row(r, T, cat, at_suspect, row->total_coverage, row->allele_support,
                            [ln10](int32_t call_count, int32_t depth, double err, int32_t cap) {
                                const QParams q = {cap, ln10};
                                return poisson_qscore_core(call_count, depth, err, q);
                            });
            if (r.changed) {
                row->variant_qscore = r.variant_qscore;
                row->genotype_qscore = (int16_t)r.genotype_qscore;
                row->noise_level = vqr::noise_level_field_of(r.noise_level);
                row->filter_bits = (uint16_t)r.filter_bits;
                changed = true;
            }
        }
    }
    if (n_changed) {
        const unsigned long long ballot = __ballot(changed);
        if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&s_changed, (uint32_t)__popcll(ballot));
        __syncthreads();
        if (threadIdx.x == 0 && s_changed) atomicAdd(n_changed, (unsigned long long)s_changed);
    }
}

}  // namespace vqrdev
}  // namespace pisces
