// amplicon_kernels.hip.h — the amplicon-bias filter on the read store (AmpliconBiasFilterThreshold, -abfilter, FILTER AB).
// IAlleleSource.GetCoverageByAmplicon is one more histogram over the reads the store holds: the quality-passing A / C / G / T bases of a
// locus split by the amplicon id of their read (RegionStateManager.cs:179-189: AddAmpliconCount for every base whose allele type, after
// quality < minBQ -> N, is not N; a read without a tag, id -1, counts nothing, RegionState.cs:269-307); an SNV's SupportByAmplicon is the
// same histogram split by allele (with MNV calling off the SNVs fall out of the counts).  A tracking handle keeps an id
// per read and per fragment next to a segment's descriptors (amplicon_scatter_ids_kernel); amplicon_tiles_kernel walks a tile's
// fragments as the flush kernel finds them (position order, floors, row codes; reads whose fragments do not fit their fields through
// read_walk.h) and then decides, per SNV record slot of the tile, with the source the host entry uses (amplicon_bias.h).
#pragma once
#include "amplicon_bias.h"
#include "store_kernels.hip.h"

namespace pisces {

constexpr int kAmpSlots = amplicon::kMaxOverlappingAmplicons;
constexpr int kAmpLocusWords = kAmpSlots + 4 * kAmpSlots;   // per locus: 6 slot ids, then [AlleleType A G C T][6] counters
constexpr int32_t kAmpNoOverflow = 0x7FFFFFFF;              // the overflow word's preset: atomicMin leaves the lowest position that overflowed

// the ids of a tracking handle's segments, in StoreView's order (kept out of SegmentView: the flush kernels' arguments stay as they are)
struct AmpliconView {
    const int32_t* read_ids[kMaxSegments];
    const int32_t* frag_ids[kMaxSegments];
};

// One lane per read of a batch that has just joined a segment: its id to the read's slot and to the slots of its CIGAR operations
// (fragment f of a read is its operation f).  ids == nullptr: a batch without tags (-1).  cigar_offset is the batch's own (checked by the add).
__global__ __launch_bounds__(256) void amplicon_scatter_ids_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cigar_offset, int32_t n_reads,
                                                                   int32_t n_ops, int32_t* __restrict__ read_ids, int32_t* __restrict__ frag_ids)
{
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r >= n_reads) return;
    const int32_t id = ids ? ids[r] : -1;
    read_ids[r] = id;
    const int32_t c0 = max(cigar_offset[r], 0), c1 = min(cigar_offset[r + 1], n_ops);
    for (int32_t c = c0; c < c1; c++) frag_ids[c] = id;
}

// flag[0] = 1 when an id of a device batch is below -1
__global__ __launch_bounds__(256) void amplicon_check_ids_kernel(const int32_t* __restrict__ ids, int32_t n, int32_t* __restrict__ flag)
{
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r < n && ids[r] < -1) flag[0] = 1;
}

// One workgroup (one wave) per tile.  records != nullptr: the flush's pass — tiles without a supported SNV slot leave at once, the others
// count and OR 1 << PISCES_FILTER_AMPLICON_BIAS into the filter_bits of the SNV slots the decision fails.  table_out != nullptr
// (pisces_hip_get_amplicon_counts): the tile's table [64 loci][kAmpLocusWords] is copied out.  overflow[0]: the lowest position at which a
// seventh id turned up (atomicMin; the host presets kAmpNoOverflow).
__global__ __launch_bounds__(64) void amplicon_tiles_kernel(StoreView S, AmpliconView A, const PiscesTile* __restrict__ tiles, RegularTiles R, int32_t n_tiles,
                                                            int32_t min_bq, PiscesCalledAllele* __restrict__ records, const PiscesTileResult* __restrict__ tr,
                                                            float threshold, int32_t* __restrict__ overflow, int32_t* __restrict__ table_out)
{
    __shared__ int32_t s_tab[kTile * kAmpLocusWords];
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (t >= n_tiles) return;
    const PiscesTile tile = tiles ? tiles[t] : regular_tile(R, t);
    const int tile_start = tile.start_position, n_loci = min(max(tile.n_loci, 0), kTile);
    uint32_t my_snvs = 0;   // bit k: slot 4 * lane + k holds a supported SNV
    int32_t rec0 = 0;
    if (records) {
        const PiscesTileResult res = tr[t];
        rec0 = res.record_begin;
        if (lane < n_loci)
            for (int k = 0; k < 4; k++) {
                const int slot = 4 * lane + k;
                if (!((res.valid[slot >> 5] >> (slot & 31)) & 1u)) continue;
                const PiscesCalledAllele& rec = records[rec0 + slot];
                if (PISCES_INFO_CATEGORY(rec.info) == PISCES_CAT_SNV && rec.allele_support > 0) my_snvs |= 1u << k;
            }
        if (__ballot(my_snvs != 0u) == 0ull) return;   // (wave-uniform: nothing of this tile can get the filter)
    }
    for (int i = lane; i < kTile * kAmpLocusWords; i += 64) s_tab[i] = (i % kAmpLocusWords) < kAmpSlots ? -1 : 0;
    __syncthreads();
    const long long tile_last = (long long)tile_start + n_loci - 1;
    auto count = [&](int position, uint32_t allele, int32_t id) {
        int32_t* const row = s_tab + (position - tile_start) * kAmpLocusWords;
        int s = 0;
        for (; s < kAmpSlots; s++) {
            const int32_t old = atomicCAS(row + s, -1, id);
            if (old == -1 || old == id) break;
        }
        if (s == kAmpSlots) { atomicMin(overflow, position); return; }
        atomicAdd(row + kAmpSlots + (int)allele * kAmpSlots + s, 1);
    };
    for (int sg = 0; sg < S.n_segments; sg++) {
        const SegmentView& G = S.seg[sg];
        const int32_t* const frag_ids = A.frag_ids[sg];
        const int32_t* const read_ids = A.read_ids[sg];
        if (G.n_frags <= 0 || !frag_ids || !read_ids) continue;
        const bool sorted = G.state[kStateUnsorted] == 0;
        const int x_lo = (int)max((long long)tile_start - G.state[kStateReach] + 1, -0x7FFFFFFFll);
        const int x_hi = tile_last >= 0x7FFFFFFFll ? 0x7FFFFFFF : (int)tile_last + 1;
        int lo = 0, hi = G.n_frags;
        if (sorted) wave_lower_bound2(G.frag, G.n_frags, x_lo, x_hi, lane, &lo, &hi);
        // ---- the aligned fragments of the range, one lane a fragment: the bases on the tile at or above the floor, by their row codes
        // (the codes' low-quality bit is made with the threshold clamped to 127: above it the qualities themselves decide, as in the generic walk)
        for (int f = lo + lane; f < hi; f += 64) {
            const ReadDesc d = G.frag[f];
            if (d.meta & kFragDeletion) continue;
            const int len = (int)(d.meta & kDescLenMask);
            const int32_t id = frag_ids[f];
            if (len == 0 || id < 0) continue;
            const long long first = (long long)d.pos0 + frag_delta(d.aoff);
            const long long floor_pos = f < G.n_floored_frags ? G.floor : 0;
            const long long p_lo = max(max(first, floor_pos), max((long long)tile_start, 1ll)), p_hi = min(first + len - 1, tile_last);
            const uint8_t* const codes = G.codes + (d.aoff & kFragAoffMask);
            const uint8_t* const quals = G.quals + (d.aoff & kFragAoffMask);
            for (long long p = p_lo; p <= p_hi; p++) {
                const uint32_t code = codes[p - first];
                const uint32_t allele = (code >> 2) & 7u;
                if ((code & 0x20u) || allele >= (uint32_t)PISCES_ALLELE_N) continue;
                if (min_bq > 127 && (int)quals[p - first] < min_bq) continue;
                count((int)p, allele, id);
            }
        }
        // ---- reads whose fragments did not fit their fields: base by base (read_walk.h), as walk_segment_complex takes them
        if (G.state[kStateFrags] & 1) {
            int rlo = 0, rhi = G.n_reads;
            if (sorted) wave_lower_bound2(G.desc, G.n_reads, x_lo, x_hi, lane, &rlo, &rhi);
            for (int r = rlo; r < rhi; r++) {   // (wave-uniform: the lanes share a read's bases)
                const ReadDesc d = G.desc[r];
                const int32_t id = read_ids[r];
                if (!(d.meta & kDescGeneric) || id < 0) continue;
                const ReadExt e = G.ext[r];
                const ReadShape shape = read_shape(d.pos0, e.n_bases, e.n_cigar, G.cigar_op + e.cig_off, G.cigar_len + e.cig_off);
                if (d.pos0 > tile_last || (long long)d.pos0 + shape.ref_span - 1 < tile_start) continue;
                long long aoff = d.aoff;
                if (!(d.meta & kDescComplex)) {   // (a read of one aligned run keeps the index of its first ALIGNED base: back to its first base)
                    int lead = 0;
                    for (int c = 0; c < e.n_cigar; c++) {
                        const uint8_t op = G.cigar_op[e.cig_off + c];
                        if (op == 'S') lead += (int)G.cigar_len[e.cig_off + c];
                        else if (op != 'H' && op != 'P') break;
                    }
                    aoff -= lead;
                }
                const int floor_pos = r < G.n_floored ? G.floor : 0;
                const long long p_lo = max((long long)tile_start, (long long)max(floor_pos, 1));
                const uint8_t* const quals = G.quals + aoff;
                const uint8_t* const bases = G.bases + aoff;
                for (int i = lane; i < shape.n; i += 64) {
                    const BaseWalk bw = walk_base(shape, i, quals, min_bq);
                    if (bw.position == -1 || !bw.n_base || bw.position < p_lo || bw.position > tile_last) continue;
                    const uint32_t allele = walk_allele_type(bases[i]);
                    if ((int)quals[i] >= min_bq && allele < (uint32_t)PISCES_ALLELE_N) count(bw.position, allele, id);
                }
            }
        }
    }
    __syncthreads();
    if (table_out)
        for (int i = lane; i < kTile * kAmpLocusWords; i += 64) table_out[(long long)t * kTile * kAmpLocusWords + i] = s_tab[i];
    if (!records || my_snvs == 0u) return;
    // ---- the decision, lane = locus: the locus' amplicons are its claimed slots (claimed from slot 0 on), coverage = the four alleles added up
    const int32_t* const row = s_tab + lane * kAmpLocusWords;
    int32_t cov[kAmpSlots], sup[kAmpSlots];
    int n = 0;
    while (n < kAmpSlots && row[n] != -1) n++;
    for (int s = 0; s < kAmpSlots; s++) {
        cov[s] = 0;
        for (int a = 0; a < 4; a++) cov[s] += row[kAmpSlots + a * kAmpSlots + s];
    }
    for (int k = 0; k < 4; k++) {
        if (!((my_snvs >> k) & 1u)) continue;
        PiscesCalledAllele& rec = records[rec0 + 4 * lane + k];
        const uint32_t alt = PISCES_INFO_ALT(rec.info);
        if (alt >= (uint32_t)PISCES_ALLELE_N) continue;
        for (int s = 0; s < kAmpSlots; s++) sup[s] = row[kAmpSlots + (int)alt * kAmpSlots + s];
        if (amplicon::bias(sup, cov, n, threshold, nullptr) == 1) rec.filter_bits = (uint16_t)(rec.filter_bits | (1u << PISCES_FILTER_AMPLICON_BIAS));
    }
}

}  // namespace pisces
