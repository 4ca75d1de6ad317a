// venn_kernels.hip.h — VennVcf's consensus of two probe pools on device-resident rows (pisces_hip_venn_consensus_device): the stage between
// two pools' flushes (or pisces_hip_compact_records) and pisces_hip_vqr_* / the VCF writer.  The decisions are venn.h, the source the host
// entries use; the q-score is poisson_qscore_core and the pool bias the Extended strand-bias statistics of device_math.hip.h, the functions
// the call phase evaluates.  No kernel here is launched by a handle that does not call the entry.
//
// The rows of both pools are one index space: A's rows, then B's, 256 to a workgroup (a workgroup holds rows of one pool).  A lane is a row.
// A row is a group HEAD when its predecessor has another position; a head finds the other pool's rows of its position by binary search.  A
// position present in both pools belongs to pool A's head, a B head with a match in A does nothing.
//   venn_count_kernel   a working head runs venn::walk_group with a Sink that stores nothing and keeps three numbers: rows, candidates and
//                       allele bytes the position emits.  The workgroup leaves the exclusive prefix of the three inside its 256 rows (every
//                       other lane contributes 0) and its three totals.  Every lane also compares its position with its predecessor's:
//                       the lowest row that steps back is the call's error word (integer atomicMin, the same value whatever the order).
//   venn_scan_kernel    one workgroup: exclusive scan of the workgroup totals of A and of B, the six grand totals, the three counts the
//                       caller reads, and `go` — no error and every capacity large enough.
//   venn_emit_kernel    the count kernel's walk with the stores on.  A's head i writes at scanA[i] + scanB[lower_bound_B(position)], a B-only
//                       head j at scanB[j] + scanA[lower_bound_A(position)]: position order, identical from run to run, no atomics in it.
// Kernel boundaries order the three; no fence, no host wait.  Groups are one row in a genome VCF and a handful at a multi-allelic site.
#pragma once
#include "device_math.hip.h"
#include "venn.h"

namespace pisces {

// The two scores venn::combine asks for, one source for host and device
struct VennMath {
    double ln10;   // Math.Log(10.0), evaluated on the host
    // VariantQualityCalculator.AssignPoissonQScore (VariantQualityCalculator.cs:54-65); QtoP(int.MinValue) is +infinity: MathNet's
    // Poisson(+inf).CumulativeDistribution is 0, p = 1, Q = 0 (vqr.h says the same)
    __host__ __device__ int32_t qscore(int32_t call_count, int32_t coverage, int32_t noise_level, int32_t max_qscore) const
    {
        if (call_count <= 0 || coverage <= 0) return 0;
        if (noise_level == venn::kIntMin) return 0;
        const double err = pow(10.0, -1 * (double)noise_level / 10.0);   // MathOperations.QtoP
        const QParams q = {max_qscore, ln10};
        return poisson_qscore_core(call_count, coverage, err, q);
    }
    // StrandBiasCalculator.CalculateStrandBiasResults (StrandBiasCalculator.cs:21-72) with StrandBiasModel.Extended over coverage
    // {DepthA, DepthB, 0} and support {AltA, AltB, 0}: the three statistics and their combination are strand_bias's own
    __host__ __device__ void pool_bias(int32_t depth_a, int32_t depth_b, int32_t alt_a, int32_t alt_b, int32_t noise_level, double min_frequency,
                                       double threshold, double* score, double* gatk, bool* acceptable) const
    {
        DeviceParams P = {};
        P.sb_model = PISCES_SB_EXTENDED;
        P.err_sb = pow(10.0, (double)((float)(int32_t)(0u - (uint32_t)noise_level) / 10.0f));   // Math.Pow(10, -1 * qNoise / 10f), the product unchecked
        P.min_freq = (float)min_frequency;
        P.sb_threshold = threshold;
        const int32_t cov[3] = {depth_a, depth_b, 0}, sup[3] = {alt_a, alt_b, 0};
        const SbStats overall = sb_stats_of<false>(0, cov, sup, P);
        const SbStats fwd = sb_stats_of<false>(1, cov, sup, P);
        const SbStats rev = sb_stats_of<false>(2, cov, sup, P);
        const SbResult r = sb_combine(overall, fwd, rev, P);
        *score = r.bias_score;
        *gatk = r.cov_both ? 10 * log10(r.bias_score) : -INFINITY;   // MathOperations.PtoGATKBiasScale; :62-66
        *acceptable = r.acceptable != 0;
    }
};

namespace venndev {

constexpr int kBlock = 256;   // rows a workgroup

__device__ __forceinline__ int64_t rows_there(int64_t n, const int32_t* d_count)
{
    if (!d_count) return n;
    const int64_t c = *d_count;
    return c < 0 ? 0 : (c < n ? c : n);
}

struct Args {
    PiscesVennRows a, b;
    PiscesVennOut out;
    PiscesVennOptions opts;
    VennMath math;
    int64_t chunks_a, chunks_b;
    uint32_t* prefix;            // [(a.n + b.n)][3]: a row's exclusive prefix inside its workgroup
    int64_t* chunk;              // [(chunks_a + chunks_b)][3]: workgroup totals, then their exclusive scan inside the pool
    unsigned long long* ctrl;    // [0] lowest (pool << 40 | row) that steps back, all ones = none; [1] go; [2..4] A's totals; [5..7] B's
};

__device__ __forceinline__ venn::Pool pool_of(const PiscesVennRows& r)
{
    venn::Pool p;
    p.recs = r.recs;
    p.n = rows_there(r.n, r.count);
    p.cand_index = r.cand_index;
    p.cands = r.cands;
    p.alleles = r.alleles;
    return p;
}

// This lane's row: which pool, which row, and — for a head that works — the rows of its position in both pools
struct Lane {
    bool in_b, works;
    int64_t row;
    int64_t a0, a1, b0, b1;
};
__device__ __forceinline__ Lane lane_of(const Args& K, const venn::Pool& A, const venn::Pool& B)
{
    Lane L;
    L.in_b = (int64_t)blockIdx.x >= K.chunks_a;
    L.row = ((int64_t)blockIdx.x - (L.in_b ? K.chunks_a : 0)) * kBlock + threadIdx.x;
    L.works = false;
    L.a0 = L.a1 = L.b0 = L.b1 = 0;
    const venn::Pool& mine = L.in_b ? B : A;
    const venn::Pool& other = L.in_b ? A : B;
    if (L.row >= mine.n) return L;
    const int32_t position = mine.recs[L.row].position;
    if (L.row > 0 && mine.recs[L.row - 1].position == position) return L;   // not a head
    const int64_t lb = venn::lower_bound(other.recs, other.n, position);
    const bool matched = lb < other.n && other.recs[lb].position == position;
    if (L.in_b && matched) return L;                                        // the position is pool A's head's
    const int64_t e = venn::group_end(mine.recs, mine.n, L.row);
    const int64_t oe = matched ? venn::group_end(other.recs, other.n, lb) : lb;
    if (L.in_b) { L.a0 = lb; L.a1 = oe; L.b0 = L.row; L.b1 = e; }
    else { L.a0 = L.row; L.a1 = e; L.b0 = lb; L.b1 = oe; }
    L.works = true;
    return L;
}

struct CountSink {
    __device__ void row(int64_t, const PiscesCalledAllele&, const PiscesConsensusInfo&) {}
    __device__ void cand(int64_t, int64_t, int64_t, const PiscesCandidate&, const uint8_t*) {}
    __device__ void no_cand(int64_t) {}
    __device__ void venn(int, int64_t, uint8_t) {}
};

__global__ __launch_bounds__(kBlock) void venn_count_kernel(const Args K)
{
    __shared__ uint32_t s_scan[3][kBlock];
    const venn::Pool A = pool_of(K.a), B = pool_of(K.b);
    const Lane L = lane_of(K, A, B);
    const venn::Pool& mine = L.in_b ? B : A;
    const int tid = (int)threadIdx.x;
    if (L.row > 0 && L.row < mine.n && mine.recs[L.row].position < mine.recs[L.row - 1].position)
        atomicMin(&K.ctrl[0], ((unsigned long long)(L.in_b ? 1 : 0) << 40) | (unsigned long long)L.row);
    venn::GroupCounts n = {0, 0, 0};
    if (L.works) {
        CountSink sink;
        n = venn::walk_group(A, L.a0, L.a1, B, L.b0, L.b1, K.opts, K.math, sink);
    }
    // exclusive prefix inside the workgroup (Hillis-Steele over 256 lanes, three sequences at once); a group's counts fit 32 bits, a
    // workgroup's total is kept in 64
    uint32_t v[3] = {(uint32_t)n.rows, (uint32_t)n.cands, (uint32_t)n.bytes};
    for (int k = 0; k < 3; k++) s_scan[k][tid] = v[k];
    __syncthreads();
    uint32_t inc[3] = {v[0], v[1], v[2]};
    for (int d = 1; d < kBlock; d <<= 1) {
        uint32_t add[3] = {0, 0, 0};
        if (tid >= d)
            for (int k = 0; k < 3; k++) add[k] = s_scan[k][tid - d];
        __syncthreads();
        for (int k = 0; k < 3; k++) { inc[k] += add[k]; s_scan[k][tid] = inc[k]; }
        __syncthreads();
    }
    const int64_t slot = (L.in_b ? K.a.n : 0) + L.row;   // (rows beyond a pool's count keep a slot: the scratch is sized by n)
    if (L.row < (L.in_b ? K.b.n : K.a.n))
        for (int k = 0; k < 3; k++) K.prefix[slot * 3 + k] = inc[k] - v[k];
    if (tid == kBlock - 1)
        for (int k = 0; k < 3; k++) K.chunk[(int64_t)blockIdx.x * 3 + k] = (int64_t)inc[k];
}

// One workgroup of 1024: lane t owns a contiguous slice of a pool's workgroup totals, the slices' sums are scanned in LDS.
__global__ __launch_bounds__(1024) void venn_scan_kernel(const Args K)
{
    __shared__ long long s_part[1024];
    __shared__ long long s_total[6];
    const int tid = (int)threadIdx.x;
    for (int seq = 0; seq < 6; seq++) {
        const int64_t first = seq < 3 ? 0 : K.chunks_a, count = seq < 3 ? K.chunks_a : K.chunks_b;
        const int k = seq % 3;
        const int64_t per = (count + 1023) / 1024;
        const int64_t lo = (int64_t)tid * per < count ? (int64_t)tid * per : count, hi = lo + per < count ? lo + per : count;
        long long sum = 0;
        for (int64_t c = lo; c < hi; c++) sum += K.chunk[(first + c) * 3 + k];
        s_part[tid] = sum;
        __syncthreads();
        long long inc = sum;
        for (int d = 1; d < 1024; d <<= 1) {
            const long long add = tid >= d ? s_part[tid - d] : 0;
            __syncthreads();
            inc += add;
            s_part[tid] = inc;
            __syncthreads();
        }
        long long run = inc - sum;
        for (int64_t c = lo; c < hi; c++) {
            const long long t = K.chunk[(first + c) * 3 + k];
            K.chunk[(first + c) * 3 + k] = run;
            run += t;
        }
        if (tid == 1023) s_total[seq] = inc;
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long bad = K.ctrl[0];
        const long long rows = s_total[0] + s_total[3], cands = s_total[1] + s_total[4], bytes = s_total[2] + s_total[5];
        for (int seq = 0; seq < 6; seq++) K.ctrl[2 + seq] = (unsigned long long)s_total[seq];
        if (bad != ~0ull) {   // "Vcf needs to be ordered"
            K.out.n_out[0] = PISCES_E_INVALID_ARG;
            K.out.n_out[1] = (int64_t)(bad >> 40);
            K.out.n_out[2] = (int64_t)(bad & ((1ull << 40) - 1));
            K.ctrl[1] = 0;
        } else {
            K.out.n_out[0] = rows;
            K.out.n_out[1] = cands;
            K.out.n_out[2] = bytes;
            K.ctrl[1] = (rows <= K.out.row_capacity && cands <= K.out.cand_capacity && bytes <= K.out.allele_capacity) ? 1 : 0;
        }
    }
}

struct EmitSink {
    const PiscesVennOut& out;
    int64_t row_base, cand_base, byte_base;
    __device__ void row(int64_t slot, const PiscesCalledAllele& r, const PiscesConsensusInfo& info)
    {
        venn::store_row(out.recs + row_base + slot, r);
        if (out.info) {
            venn::Quad q[2];   // 32 bytes: two 16-byte stores
            memcpy(q, &info, sizeof(info));
            venn::Quad* d = reinterpret_cast<venn::Quad*>(out.info + row_base + slot);
            d[0] = q[0];
            d[1] = q[1];
        }
    }
    __device__ void cand(int64_t slot, int64_t cslot, int64_t byte_off, const PiscesCandidate& c, const uint8_t* bytes)
    {
        out.cand_index[row_base + slot] = (int32_t)(cand_base + cslot);
        PiscesCandidate o = c;
        o.allele_offset = byte_base + byte_off;
        out.cands[cand_base + cslot] = o;
        const int64_t len = (int64_t)c.ref_len + (int64_t)c.alt_len;
        for (int64_t k = 0; k < len; k++) out.alleles[byte_base + byte_off + k] = bytes[k];
    }
    __device__ void no_cand(int64_t slot) { out.cand_index[row_base + slot] = -1; }
    __device__ void venn(int pool, int64_t i, uint8_t cls)
    {
        uint8_t* v = pool ? out.venn_b : out.venn_a;
        if (v) v[i] = cls;
    }
};

// the exclusive scan of a pool's three counts at row `i` of it (i == its rows: the pool's totals)
__device__ __forceinline__ void scan_at(const Args& K, bool in_b, int64_t i, int64_t pool_rows, int64_t at[3])
{
    if (i >= pool_rows) {
        for (int k = 0; k < 3; k++) at[k] = (int64_t)K.ctrl[2 + (in_b ? 3 : 0) + k];
        return;
    }
    const int64_t chunk = (in_b ? K.chunks_a : 0) + i / kBlock, slot = (in_b ? K.a.n : 0) + i;
    for (int k = 0; k < 3; k++) at[k] = K.chunk[chunk * 3 + k] + (int64_t)K.prefix[slot * 3 + k];
}

__global__ __launch_bounds__(kBlock) void venn_emit_kernel(const Args K)
{
    if (K.ctrl[1] == 0) return;   // an unsorted pool or a capacity too small: nothing is written
    const venn::Pool A = pool_of(K.a), B = pool_of(K.b);
    const Lane L = lane_of(K, A, B);
    if (!L.works) return;
    int64_t mine[3], other[3];
    scan_at(K, L.in_b, L.row, L.in_b ? B.n : A.n, mine);
    scan_at(K, !L.in_b, L.in_b ? L.a0 : L.b0, L.in_b ? A.n : B.n, other);
    EmitSink sink = {K.out, mine[0] + other[0], mine[1] + other[1], mine[2] + other[2]};
    venn::walk_group(A, L.a0, L.a1, B, L.b0, L.b1, K.opts, K.math, sink);
}

}  // namespace venndev
}  // namespace pisces
