/*
 * pisces_hip.h — C ABI of libpisceship.so: the MI355X (gfx950) pileup-and-likelihood
 * engine that sits behind Pisces' ICandidateVariantFinder / IStateManager / IAlleleCaller.
 *
 * Conventions (mirror the only P/Invoke precedent in the reference,
 * src/lib/Common.IO/FileCompression.cs:10-35): cdecl, every function returns int32
 * (0 = ok, <0 = error, see PISCES_E_*), plain pointers + sizes, caller-owned buffers that
 * are only read/written for the duration of the call, opaque handle owning all device
 * memory.  No function throws or aborts; pisces_hip_last_error() returns the message the
 * C# shim turns into an exception (caught per job at
 * src/lib/Pisces.Processing/Logic/BaseGenomeProcessor.cs:121-128).
 *
 * Each entry point cites the reference interface member it replaces.
 */
#ifndef PISCES_HIP_H
#define PISCES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PISCES_HIP_ABI_VERSION 9

/* ---- error codes -------------------------------------------------------- */
#define PISCES_OK                 0
#define PISCES_E_INVALID_ARG     -1  /* reference: ArgumentException (RegionStateManager.cs:363-364, RegionState.cs:315-316) */
#define PISCES_E_BUFFER_TOO_SMALL -2 /* caller grows the output buffer and repeats the call */
#define PISCES_E_DEVICE          -3  /* HIP runtime error, message in last_error */
#define PISCES_E_UNMAPPED_BASE   -4  /* reference: RegionStateManager.cs:109-113 */
#define PISCES_E_UNSUPPORTED     -5
#define PISCES_E_STATE           -6  /* call protocol violated */
#define PISCES_E_INTERNAL        -7  /* an exception inside the library (e.g. out of host memory): caught at the boundary, message in last_error */

/* ---- enums: numeric values are the reference's ------------------------- */
/* src/lib/Pisces.Domain/Types/AlleleType.cs:3-11 */
enum { PISCES_ALLELE_A = 0, PISCES_ALLELE_G = 1, PISCES_ALLELE_C = 2, PISCES_ALLELE_T = 3,
       PISCES_ALLELE_N = 4, PISCES_ALLELE_DEL = 5, PISCES_NUM_ALLELE_TYPES = 6 };
/* src/lib/Pisces.Domain/Types/DirectionType.cs:3-8 */
enum { PISCES_DIR_FORWARD = 0, PISCES_DIR_REVERSE = 1, PISCES_DIR_STITCHED = 2, PISCES_NUM_DIRECTIONS = 3 };
/* src/lib/Pisces.Domain/Types/CallType.cs:3-12 */
enum { PISCES_CAT_SNV = 0, PISCES_CAT_INSERTION = 1, PISCES_CAT_DELETION = 2, PISCES_CAT_MNV = 3,
       PISCES_CAT_REFERENCE = 4 };
/* src/lib/Pisces.Domain/Types/Genotype.cs:3-18 */
enum { PISCES_GT_HET_ALT1_ALT2 = 0, PISCES_GT_ALT12_LIKE_NOCALL = 1, PISCES_GT_HET_ALT_REF = 2,
       PISCES_GT_HOM_ALT = 3, PISCES_GT_HOM_REF = 4, PISCES_GT_REF_LIKE_NOCALL = 5,
       PISCES_GT_ALT_LIKE_NOCALL = 6, PISCES_GT_REF_AND_NOCALL = 7, PISCES_GT_ALT_AND_NOCALL = 8,
       PISCES_GT_HEMI_REF = 9, PISCES_GT_HEMI_ALT = 10, PISCES_GT_HEMI_NOCALL = 11 /* PloidyModel.Haploid */,
       PISCES_GT_OTHERS = 12 /* a forced allele next to other variants, DiploidLocusProcessor.cs:36-38 */ };
/* src/lib/Pisces.Domain/Types/FilterType.cs:3-19 — bit i of filter_bits = enum value i */
enum { PISCES_FILTER_STRAND_BIAS = 0, PISCES_FILTER_POOL_BIAS = 1, PISCES_FILTER_AMPLICON_BIAS = 2,
       PISCES_FILTER_LOW_VARIANT_QSCORE = 3, PISCES_FILTER_LOW_DEPTH = 4,
       PISCES_FILTER_LOW_VARIANT_FREQUENCY = 5, PISCES_FILTER_LOW_GENOTYPE_QUALITY = 6,
       PISCES_FILTER_INDEL_REPEAT_LENGTH = 7, PISCES_FILTER_MULTI_ALLELIC_SITE = 8,
       PISCES_FILTER_RMXN = 9, PISCES_FILTER_FORCED_REPORT = 10, PISCES_FILTER_OFF_TARGET = 11,
       PISCES_FILTER_NO_CALL = 12 };
/* src/lib/Pisces.Domain/Types (StrandBiasModel): Poisson, Extended, Diploid */
enum { PISCES_SB_POISSON = 0, PISCES_SB_EXTENDED = 1, PISCES_SB_DIPLOID = 2 };
enum { PISCES_NOISE_FLAT = 0, PISCES_NOISE_WINDOW = 1 };
enum { PISCES_PLOIDY_SOMATIC = 0, PISCES_PLOIDY_DIPLOID = 1, PISCES_PLOIDY_HAPLOID = 2,
       PISCES_PLOIDY_DIPLOID_ADAPTIVE = 3 };   /* PloidyModel.Somatic / DiploidByThresholding / Haploid / DiploidByAdaptiveGT
                                                  (Pisces.Domain/Types/ModelTypes.cs:13) */

/* Anchor bins: NumAnchorIndexes = 2*trackedAnchorSize+1 (RegionStateManager.cs:30-31), default 5 -> 11 */
#define PISCES_ANCHOR_SIZE   5
#define PISCES_NUM_ANCHORS   11
#define PISCES_COUNTS_PER_LOCUS (PISCES_NUM_ALLELE_TYPES * PISCES_NUM_DIRECTIONS * PISCES_NUM_ANCHORS) /* 198 */
#define PISCES_FOLDED_PER_LOCUS (PISCES_NUM_ALLELE_TYPES * PISCES_NUM_DIRECTIONS)                      /* 18  */

/* ---- packed observation tuple (4 bytes) ---------------------
 * Laid out so that the hot kernel's LDS counter address is a mask of the tuple: bits 2..12 are the byte
 * offset of the (allele, direction, column) counter in a [32 rows][64 columns] int32 histogram.
 * bit  0..1   zero
 * bit  2..7   column = PISCES_TUPLE_COLUMN(locus-in-tile, direction): a bank-spreading bijection of the locus
 *             (0..63).  A dwordx4 load hands each lane four consecutive loci of a read, so one LDS instruction sees the
 *             loci c + 4q of a few reads: the column puts q in the low four bank bits and the direction parity in
 *             the fifth, so a forward and a reverse read of the same loci never meet on a bank.
 * bit  8..9   direction 0..2
 * bit 10..12  raw allele code 0..5 (before the min-base-quality test)
 * bit 13..16  anchor bin 0..10  (GetAnchorType, RegionStateManager.cs:83-116)
 * bit 17..23  zero
 * bit 24..31  base quality (deletion tuples carry 255: their quality gate,
 *             CheckDeletionQuality, was applied when the read was expanded)
 * The kernel applies "qual < minBQ -> N" (RegionStateManager.cs:179-181).
 * A tile has at most 64 loci and the column has six bits, so no tuple can address memory outside its tile's histogram.
 * Tuples that count for nothing, in every kernel that takes tuples (tests/test_tuple_geometry_gpu.py): a locus at or beyond
 * the tile's n_loci (a tile may have fewer than 64 loci; the column of such a locus is a counter nobody reads), allele codes
 * 6, 7 and direction 3 (rows nobody reads), an anchor code of 11..15 (there is no such bin: it adds 0), and the pad word.
 * Bits 0..1 and 17..23 must be zero as stated: the hot kernel tells a valid anchor by a carry out of bit 16. */
#define PISCES_TUPLE_MAX_TILE   64
#define PISCES_TUPLE_COLUMN(locus, dir) \
    (((((uint32_t)(locus) >> 2) & 15u) | (((uint32_t)(locus) & 3u) << 4)) ^ (((uint32_t)(dir) & 1u) << 4))
#define PISCES_TUPLE_PACK(locus, anchor, dir, allele, qual) \
    ((PISCES_TUPLE_COLUMN(locus, dir) << 2) | ((uint32_t)(dir) << 8) | ((uint32_t)(allele) << 10) | \
     ((uint32_t)(anchor) << 13) | ((uint32_t)(qual) << 24))
#define PISCES_TUPLE_DIR(t)    (((t) >> 8) & 0x3u)
#define PISCES_TUPLE_ALLELE(t) (((t) >> 10) & 0x7u)
#define PISCES_TUPLE_ANCHOR(t) (((t) >> 13) & 0xFu)
#define PISCES_TUPLE_QUAL(t)   ((t) >> 24)
#define PISCES_TUPLE_COL(t)    (((t) >> 2) & 63u)
/* inverse of PISCES_TUPLE_COLUMN */
#define PISCES_TUPLE_LOCUS_OF(col, dir) \
    ((((((uint32_t)(col)) ^ (((uint32_t)(dir) & 1u) << 4)) & 15u) << 2) | ((((uint32_t)(col)) ^ (((uint32_t)(dir) & 1u) << 4)) >> 4))
#define PISCES_TUPLE_LOCUS(t)  PISCES_TUPLE_LOCUS_OF(PISCES_TUPLE_COL(t), PISCES_TUPLE_DIR(t))
/* the tuple with another locus (same observation) */
#define PISCES_TUPLE_WITH_LOCUS(t, locus) (((t) & ~0xFCu) | (PISCES_TUPLE_COLUMN(locus, PISCES_TUPLE_DIR(t)) << 2))
/* A tuple with all bits set is padding and is ignored by every kernel. */
#define PISCES_TUPLE_PAD 0xFFFFFFFFu

/* ---- configuration: VariantCallerConfig (src/exe/Pisces/Logic/VariantCalling/AlleleCaller.cs:266-291)
 * + the state-manager/finder settings wired in Factory.cs:123-227.
 * Defaults (pisces_hip_default_config) are the reference's
 * (src/lib/Pisces.Domain/Options/VariantCallingParameters.cs:57-156). */
typedef struct PiscesHipConfig {
    int32_t abi_version;              /* PISCES_HIP_ABI_VERSION */
    int32_t min_base_call_quality;    /* BamFilterParameters.MinimumBaseCallQuality, 20 */
    int32_t noise_level;              /* NoiseLevelUsedForQScoring, = minBQ unless forced */
    int32_t max_variant_qscore;       /* 100 */
    int32_t min_variant_qscore;       /* 20 */
    int32_t variant_qscore_filter;    /* VariantQscoreFilterThreshold, 30; -1 = null */
    int32_t min_coverage;             /* MinCoverage, 10 */
    int32_t low_depth_filter;         /* LowDepthFilter, 10; -1 = null */
    int32_t min_genotype_qscore;      /* 0 */
    int32_t max_genotype_qscore;      /* 100 */
    int32_t low_gq_filter;            /* LowGTqFilter; -1 = null */
    int32_t strand_bias_model;        /* PISCES_SB_EXTENDED */
    int32_t filter_single_strand;     /* FilterSingleStrandVariants, 0 */
    int32_t include_reference_calls;  /* gVCF, 1 */
    int32_t emit_zero_coverage_refs;  /* 1 when an interval set is supplied (RegionState.cs:446) */
    int32_t expect_stitched_reads;    /* IAlleleSource.ExpectStitchedReads */
    int32_t tile_loci;                /* device tile, power of two <= 1024; 0 = default 64 */
    int32_t block_size;               /* GlobalConstants.RegionSize, 1000 */
    float   min_frequency;            /* MinFrequency, 0.01f */
    float   variant_freq_filter;      /* VariantFreqFilter (MinimumFrequencyFilter), 0.01f; <0 = null */
    float   genotype_min_freq_filter; /* SomaticGenotyper._minVariantFrequencyFilter, 0.01f */
    float   target_lod_frequency;     /* TargetLODFrequency, 0.01f */
    float   strand_bias_threshold;    /* StrandBiasFilterThreshold, 0.5f */
    float   no_call_filter_threshold; /* NoCallFilterThreshold, 0.6f; <0 = null */
    int32_t rmxn_max_repeat_length;   /* RMxNFilterMaxLengthRepeat, 5; <0 = filter off */
    int32_t rmxn_min_repetitions;     /* RMxNFilterMinRepetitions, 9 */
    float   rmxn_frequency_limit;     /* RMxNFilterFrequencyLimit, 0.35f */
    int32_t collapse;                 /* PiscesApplicationOptions.Collapse (VariantCollapser on insertion / deletion candidates; SNV twins are
                                         the device counts already); reference default true, see pisces_hip_default_config */
    float   collapse_freq_threshold;        /* CollapseFreqThreshold, 0f */
    float   collapse_freq_ratio_threshold;  /* CollapseFreqRatioThreshold, 0.5f */
    int32_t call_mnvs;                /* PiscesApplicationOptions.CallMNVs, 0: with it on, SNV / MNV candidates come from the read walk
                                         (CandidateVariantFinder.cs:90-232), no longer from the allele counts */
    int32_t max_mnv_length;           /* MaxSizeMNV, 3 */
    int32_t max_gap_between_mnv;      /* MaxGapBetweenMNV, 1 */
    int32_t noise_model;              /* VariantCallingParameters.NoiseModel: PISCES_NOISE_FLAT (default) or PISCES_NOISE_WINDOW, where the
                                         variant q-score of an allele uses (int)PtoQ(SumOfBaseQuality / TotalCoverage) as its noise level
                                         (AlleleCaller.cs:215-218, RegionStateManager.cs:191) */
    int32_t ploidy;                   /* PISCES_PLOIDY_SOMATIC (default), PISCES_PLOIDY_DIPLOID, PISCES_PLOIDY_HAPLOID or
                                         PISCES_PLOIDY_DIPLOID_ADAPTIVE (the mixture model, see PiscesAdaptiveParams): one genotype per locus from the
                                         variant frequencies, alleles beyond the ploidy pruned (DiploidThresholdingGenotyper.cs:54-141,
                                         HaploidGenotyper.cs:36-83, which takes MinorVF / MajorVF from the SNV parameters below).  Made on the
                                         device over the tile kernels' record slots (pisces_hip_call_tiles*, and a flush whose rows are
                                         the tile kernels' alone); by the host pass of the flush when rows of insertions / deletions / MNVs
                                         or forced alleles join them.  Both are csrc/genotype_core.h */
    float   diploid_snv_params[3];    /* DiploidSNVThresholdingParameters {MinorVF, MajorVF, SumVFforMultiAllelicSite}: 0.20, 0.70, 0.80 */
    float   diploid_indel_params[3];  /* DiploidINDELThresholdingParameters, same defaults */
} PiscesHipConfig;

/* ---- one called allele (64 bytes; what CalledAllele carries to the VCF writer,
 * src/lib/Pisces.Domain/Models/Alleles/CalledAllele.cs:7-140, VcfFormatter.cs:224) */
typedef struct PiscesCalledAllele {
    int32_t position;            /* ReferencePosition, 1-based */
    int32_t total_coverage;      /* TotalCoverage */
    int32_t allele_support;      /* AlleleSupport */
    int32_t reference_support;   /* ReferenceSupport */
    int32_t num_no_calls;        /* NumNoCalls */
    int32_t coverage_by_dir[3];  /* EstimatedCoverageByDirection */
    int32_t support_by_dir[3];   /* SupportByDirection */
    int32_t variant_qscore;      /* VariantQscore */
    double  strand_bias_score;   /* StrandBiasResults.BiasScore; GATKBiasScore = 10*log10 of it */
    int16_t genotype_qscore;     /* GenotypeQscore */
    int16_t noise_level;         /* NoiseLevelApplied: set where the q-score is computed (VariantQualityCalculator.cs:13), so 0 for an
                                    allele without support; the configured level with NoiseModel.Flat, (int)PtoQ(SumOfBaseQuality /
                                    TotalCoverage) with NoiseModel.Window (AlleleCaller.cs:215-218); -32768 stands for int.MinValue (the
                                    C# cast of a non-finite PtoQ) */
    uint16_t filter_bits;        /* bit i = FilterType i */
    uint16_t info;               /* see PISCES_INFO_* */
} PiscesCalledAllele;

/* info: genotype[0..3] | category[4..6] | ref allele code[7..9] | alt allele code[10..12] |
 *       BiasAcceptable[13] | VarPresentOnBothStrands[14] | CovPresentOnBothStrands[15]
 * ref/alt codes are AlleleType values (single-base alleles).  For host-supplied spanning
 * candidates the strings stay with the caller; alt code then holds PISCES_ALLELE_N. */
#define PISCES_INFO_GENOTYPE(i)  ((i) & 0xF)
#define PISCES_INFO_CATEGORY(i)  (((i) >> 4) & 0x7)
#define PISCES_INFO_REF(i)       (((i) >> 7) & 0x7)
#define PISCES_INFO_ALT(i)       (((i) >> 10) & 0x7)
#define PISCES_INFO_SB_OK(i)     (((i) >> 13) & 1)
#define PISCES_INFO_VAR_BOTH(i)  (((i) >> 14) & 1)
#define PISCES_INFO_COV_BOTH(i)  (((i) >> 15) & 1)
/* filter_bits 14..15: CalledAllele.PhaseSetIndex of a diploid call (0 reference, 1 / 2 the variant alleles in frequency order) */
#define PISCES_FILTERBITS_PHASE(f) (((f) >> 14) & 3)
#define PISCES_INFO_PACK(gt, cat, ref, alt, sbok, varboth, covboth) \
    ((uint16_t)((gt) | ((cat) << 4) | ((ref) << 7) | ((alt) << 10) | ((sbok) << 13) | \
                ((varboth) << 14) | ((covboth) << 15)))

/* ---- PloidyModel.DiploidByAdaptiveGT (src/lib/Pisces.Genotyping/Adaptive/DiploidAdaptiveGenotyper.cs:45-176, AdaptiveGenotyperCalculator.cs:18-82,
 * MixtureModel.cs:281-346, 378-406, 449-518): the genotype of a locus is the most probable component of a three-component binomial mixture
 * (hom-ref, het, hom-alt) at the dominant variant's depth, the genotype q-score and the phred-scaled genotype posteriors (the VCF GP column)
 * come from the same mixture at effective depths {25, 25, 10}; a 1/2 locus gets six posteriors from a multinomial.  The means and priors are
 * AdaptiveGenotypingParameters (src/lib/Pisces.Domain/Options/VariantCallingParameters.cs:28-55); fitting them (the stand-alone
 * recalibration tool's EM) is not part of the library.  In this mode the reference leaves VariantCallerConfig.MinFrequency at 0
 * (exe/Pisces/Logic/Factory.cs:128-147: the adaptive genotyper never sets MinVarFrequency) and uses SomaticLocusProcessor: a host sets
 * cfg.min_frequency = 0 itself, and forced alleles get no DiploidLocusProcessor treatment. */
typedef struct PiscesAdaptiveParams {
    double  snv_model[3];                   /* SnvModel {0.037, 0.439, 0.976}: SNV, MNV and Reference alleles */
    double  indel_model[3];                 /* IndelModel {0.037, 0.443, 0.905}: insertions and deletions */
    double  snv_prior[3];                   /* SnvPrior {0.755, 0.154, 0.0919} */
    double  indel_prior[3];                 /* IndelPrior {0.962, 0.0266, 0.0114} */
    float   sum_vf_for_multi_allelic_site;  /* SumVFforMultiAllelicSite, 0.80f */
    int32_t max_genotype_posteriors;        /* MaxGenotypePosteriors, 3000: the three posteriors of an allele without coverage */
} PiscesAdaptiveParams;
/* CalledAllele.GenotypePosteriors of one row (32 bytes): n = 3 {hom-ref, het, hom-alt}, 6 at a 1/2 locus (MixtureModel.cs:449-518), 0 = null
 * (a row no adaptive genotyper touched: every row of another ploidy, a forced-report row).  A row and its posteriors share one index
 * wherever rows leave the library. */
typedef struct PiscesGenotypePosteriors {
    float   gp[6];
    int32_t n;
    int32_t reserved;
} PiscesGenotypePosteriors;

/* ---- tile descriptor: a run of <= tile_loci consecutive reference positions ------------
 * The unit of device work and of interval sharding.  Tiles of one call must
 * not overlap; tuples [tuple_begin, tuple_end) of the tuple buffer belong to this tile. */
typedef struct PiscesTile {
    int32_t start_position;   /* 1-based position of locus 0 */
    int32_t n_loci;           /* 1..tile_loci */
    int64_t tuple_begin;
    int64_t tuple_end;
} PiscesTile;

/* per-tile output directory entry written by the device (48 bytes).
 * The record of (locus l of the tile, allele of alphabetical rank k in A,C,G,T) lives in slot
 * record_begin + 4*l + k of the record buffer; bit (4*l + k) of valid[] says whether that slot holds a called
 * allele.  Walking the valid slots in ascending order yields the tile's alleles sorted by (position, ref, alt);
 * a Reference allele sits at the rank of its base and is not marked valid when a variant is called at its locus. */
typedef struct PiscesTileResult {
    int32_t record_begin;     /* 256 * tile index */
    int32_t n_records;        /* number of valid slots */
    int32_t n_candidate_loci; /* positions with >= 1 called allele */
    int32_t n_called;         /* alleles for which IsCallable was true (IAlleleCaller.TotalNumCalled) */
    uint32_t valid[8];        /* 256 slot-validity bits */
} PiscesTileResult;

/* ---- a batch of reads, structure-of-arrays (what the C# shim pins per call) ------------
 * replaces the Read object walked by FindCandidates/AddAlleleCounts
 * (src/lib/Pisces.Domain/Models/Read.cs:74-96, 535-562). Reads must already have passed
 * AlignmentSource.ShouldSkipRead (src/exe/Pisces/Logic/Alignment/AlignmentsSource.cs:84-92). */
typedef struct PiscesReadBatch {
    int32_t        n_reads;
    const int32_t* position;      /* [n_reads] Read.Position (1-based) */
    const uint8_t* flags;         /* [n_reads] bit0 = reverse strand */
    const int32_t* cigar_offset;  /* [n_reads+1] into cigar_op / cigar_len */
    const uint8_t* cigar_op;      /* 'M','I','D','S','N','=','X','H','P' */
    const uint32_t* cigar_len;
    const int32_t* seq_offset;    /* [n_reads+1] into bases / quals / directions */
    const uint8_t* bases;         /* upper-case ASCII */
    const uint8_t* quals;         /* phred */
    const uint8_t* directions;    /* optional per-base DirectionType (stitched reads, XD tag); NULL = from flags */
    const uint8_t* deletion_directions; /* optional, 2 bytes per CIGAR op (indexed like cigar_op): for a 'D' op the DirectionType of
                                     * its first and of its last deleted base in Read.CigarDirections.Expand() (the XD tag covers
                                     * deleted bases too) - what GetDeletionDirectionForStitchedRead reads,
                                     * CandidateVariantFinder.cs:417-420, 468-487; 255 = this read tracks no directions inside
                                     * deletions (CigarDirections == null, :422-428); ignored for other ops.  NULL = 255 throughout */
} PiscesReadBatch;
#define PISCES_DIR_UNTRACKED 255

/* ---- a candidate allele crossing the boundary (CandidateAllele.cs:8-49) ---- */
typedef struct PiscesCandidate {
    int32_t position;
    int32_t category;             /* PISCES_CAT_* */
    int32_t ref_len, alt_len;
    int32_t support_by_dir[3];
    int32_t well_anchored_by_dir[3];
    uint8_t open_left, open_right;
    uint8_t pad[2];
    int64_t allele_offset;        /* ref bytes then alt bytes at this offset of the allele byte pool */
} PiscesCandidate;

typedef struct PiscesHip PiscesHip;

/* ---- lifecycle ----------------------------------------------------------- */
/* fills *cfg with the reference defaults */
int32_t pisces_hip_default_config(PiscesHipConfig* cfg);
/* Factory.CreateStateManager / CreateVariantCaller / CreateVariantFinder (Factory.cs:123,128,209):
 * one handle per (BAM, chromosome) job; owns one HIP stream; no global mutable state. */
int32_t pisces_hip_create(const PiscesHipConfig* cfg, int32_t device, PiscesHip** out);
/* The number of HIP devices this process sees (what `device` above ranges over), or PISCES_E_DEVICE.  With -threadbychr the reference
 * runs its (BAM, chromosome) jobs on a thread pool (src/lib/Pisces.Processing/Logic/BaseGenomeProcessor.cs:40-90, JobManager.cs:70-73):
 * a host gives job j the device j % count, handles on different devices share nothing. */
int32_t pisces_hip_device_count(void);
int32_t pisces_hip_destroy(PiscesHip* h);
/* Device and pinned host memory of destroyed handles is kept for the handles that follow (a job per chromosome, or per interval range,
 * makes and destroys one each: BaseGenomeProcessor.cs:40-90): up to PISCES_HIP_ALLOC_CACHE_MB of device memory per device (default
 * 8192; 0 = keep nothing) and a quarter of that pinned.  This gives it all back; returns the bytes released. */
int64_t pisces_hip_trim_memory(void);
const char* pisces_hip_last_error(const PiscesHip* h);   /* h may be NULL: message of the last failed create */
int32_t pisces_hip_abi_version(void);

/* ChrReference.Sequence (upper-cased whole chromosome, src/lib/Pisces.IO/Genome.cs:84-96).
 * bases[i] is position i+1. Copied to the device. */
int32_t pisces_hip_set_reference(PiscesHip* h, const uint8_t* upper_bases, int64_t length);

/* ChrIntervalSet after SortAndCollapse (src/lib/Pisces.Domain/Models/IntervalSet.cs:38-74): sorted,
 * disjoint, inclusive [start, end].  With intervals, calls are made only inside them
 * (AlleleCaller.ShouldReport, AlleleCaller.cs:260-263; RegionState.GetAllCandidates clips the
 * reference candidates, RegionState.cs:406-408); set emit_zero_coverage_refs = 1 alongside. n = 0 clears. */
int32_t pisces_hip_set_intervals(PiscesHip* h, const int32_t* starts, const int32_t* ends, int32_t n);

/* Interval sharding: the positions [lo, hi] this handle OWNS.  A shard is fed the reads that overlap its range plus
 * a halo, so that counts and spanning alleles at its edges are complete; candidates the halo reads bring that lie outside the range
 * belong to the neighbouring shard: they are neither reported nor counted in IAlleleCaller.TotalNumCalled here, so that the shards'
 * totals add up to the unsharded job's (the reference has no such notion: one job per chromosome, BaseGenomeProcessor.cs:40-90).
 * Default: everything.  Give the shard's own intervals to pisces_hip_set_intervals as well. */
int32_t pisces_hip_set_owned_range(PiscesHip* h, int32_t lo, int32_t hi);

/* ---- streaming surface: IStateManager -------------------------------------- */
/* ICandidateVariantFinder.FindCandidates + IStateManager.AddCandidates + AddAlleleCounts
 * (SmallVariantCaller.cs:88-98) for a batch of reads.  The batch crosses PCIe once, packed (2 bytes per base), and the
 * read walk of AddAlleleCounts (RegionStateManager.cs:118-220) runs on the device into an observation log in HBM; the
 * host only reads the CIGARs: argument checks, the blocks a read touches, and the insertion / deletion candidates
 * (needs set_reference first; without a reference only the AddAlleleCounts half runs).  The whole batch is checked
 * before any of it is committed. */
int32_t pisces_hip_add_reads(PiscesHip* h, const PiscesReadBatch* batch);
/* The arrays of a batch of n_reads reads (n_cigar_ops CIGAR operations, n_bases bases in all) inside the handle's pinned staging
 * buffer: `views` receives pointers the caller may WRITE through (the const of PiscesReadBatch's members is for add_reads).  A host
 * that marshals its reads anyway (the C# shim packs Read objects into arrays) fills them -- cigar_offset[n_reads] and
 * seq_offset[n_reads] included -- and hands `views` to pisces_hip_add_reads, which then sends the batch as it lies instead of
 * copying it into that buffer first (the copy is the larger part of pisces_hip_add_reads for a large batch).  The views are valid
 * until the next call on the handle that is not pisces_hip_add_reads(views). */
int32_t pisces_hip_stage_reads(PiscesHip* h, int32_t n_reads, int64_t n_cigar_ops, int64_t n_bases, int32_t with_directions,
                               int32_t with_deletion_directions, PiscesReadBatch* views);
/* pisces_hip_add_reads for a batch that lies in DEVICE memory of the handle's device already: every pointer of `device_batch` is a device
 * pointer (the struct itself is host memory), n_cigar_ops = cigar_offset[n_reads] and n_bases = seq_offset[n_reads] (which the host
 * cannot read).  What an upstream stage on the device hands over — a decoder, an aligner, the bench's generator — and the form in which
 * the reads -> records rate of the device is measured (inputs resident in HBM when the timed region starts).  The arrays must
 * be complete when the call is made (synchronise the stream that made them) and are copied: the caller may reuse them when the call
 * returns — overwrite them from any stream, or free them.  (The call waits for the launch's copying workgroups to have read the last byte
 * of every array, not for the rest of the stream.)  The checks pisces_hip_add_reads makes in a host pass over the CIGARs
 * (Read.ValidateCigar, Read.cs:603-605; position > 0, RegionStateManager.cs:363-364; the blocks a read touches, :361-383) run on the
 * device, in the same launch that copies the arrays (add_fused_kernel); same refusals, same messages, the state unchanged when a read is
 * refused. */
int32_t pisces_hip_add_device_reads(PiscesHip* h, const PiscesReadBatch* device_batch, int64_t n_cigar_ops, int64_t n_bases);
/* Pre-expanded observations for the block grid: positions[i] is the 1-based locus of tuples[i]
 * (the tuple's locus field is ignored). */
int32_t pisces_hip_add_observations(PiscesHip* h, const int32_t* positions, const uint32_t* tuples, int64_t n);
/* IStateManager.GetCandidatesToProcess(upTo) + IAlleleCaller.Call + DoneProcessing
 * (SmallVariantCaller.cs:157-189).  up_to_position < 0 = final flush (Call(null)).
 * Writes called alleles sorted by (position, ref, alt) into out[0..capacity); *n_out = number
 * produced.  Returns PISCES_E_BUFFER_TOO_SMALL (and *n_out = required) without consuming the
 * batch when capacity is insufficient: grow and repeat.  The batch is made at that point (what AlleleCaller.Call hands back to the state
 * — MNV leftovers, candidates that did not collapse — has been handed back) and waits for the repeated call: until then every entry that
 * would change the state (add_reads, add_observations, add_candidates, add_decoded_reads, add_gapped_mnv_ref, a flush with another
 * up_to_position) returns PISCES_E_STATE. */
int32_t pisces_hip_flush(PiscesHip* h, int32_t up_to_position, PiscesCalledAllele* out,
                         int64_t capacity, int64_t* n_out);
/* The same call, also returning the allele strings of the called insertions / deletions:
 * cand_index_out[i] (capacity entries, may be NULL) is -1 for Reference / SNV rows (their alleles are the
 * info base codes) or the index into cand_out of row i's candidate; alleles_out receives ref then alt bytes of each
 * candidate at cand_out[j].allele_offset. PISCES_E_BUFFER_TOO_SMALL if any buffer is short (counts reported). */
int32_t pisces_hip_flush_ex(PiscesHip* h, int32_t up_to_position, PiscesCalledAllele* out, int64_t capacity, int64_t* n_out,
                            int32_t* cand_index_out, PiscesCandidate* cand_out, int64_t cand_capacity, int64_t* n_cand,
                            uint8_t* alleles_out, int64_t allele_capacity, int64_t* allele_bytes);
/* The flush as a pair, for a host that wants the device to work on block k while it prepares block k + 1:
 * pisces_hip_flush_begin(upTo) does what pisces_hip_flush does up to the point where it would wait for the device and commits
 * DoneProcessing (the flushed blocks are gone, the observation log is the compacted one); pisces_hip_flush_end waits for what is
 * still in flight and returns the same alleles pisces_hip_flush would have returned (PISCES_E_BUFFER_TOO_SMALL with *n_out = the
 * count needed: repeat flush_end with a larger buffer, nothing is lost).  Between the two the caller may stage and add the next
 * reads (pisces_hip_stage_reads, pisces_hip_add_reads, pisces_hip_add_observations, pisces_hip_bam_decode +
 * pisces_hip_add_decoded_reads) and read counts; pisces_hip_flush[_ex] and another pisces_hip_flush_begin return PISCES_E_STATE
 * until flush_end has been called.  A batch that needs the host between its device passes (insertion / deletion / MNV candidates,
 * forced alleles, the diploid / haploid genotypers, NoiseModel.Window, gapped-MNV reference counts) is flushed synchronously inside
 * flush_begin; flush_end returns it all the same (pisces_hip_flush_end_ex: with the candidates' allele strings). */
int32_t pisces_hip_flush_begin(PiscesHip* h, int32_t up_to_position);
int32_t pisces_hip_flush_end(PiscesHip* h, PiscesCalledAllele* out, int64_t capacity, int64_t* n_out);
/* pisces_hip_flush_end with pisces_hip_flush_ex's candidate outputs (same meaning, same PISCES_E_BUFFER_TOO_SMALL protocol: all three
 * counts are reported, repeat with larger buffers).  A flush that needed no host-side candidates returns cand_index -1 everywhere. */
int32_t pisces_hip_flush_end_ex(PiscesHip* h, PiscesCalledAllele* out, int64_t capacity, int64_t* n_out, int32_t* cand_index_out,
                                PiscesCandidate* cand_out, int64_t cand_capacity, int64_t* n_cand, uint8_t* alleles_out,
                                int64_t allele_capacity, int64_t* allele_bytes);
/* The flushes without the copy into the caller's array, for a host that reads the rows where they lie (a managed host marshals them into
 * its own objects anyway; 2.8 M rows are 179 MB): *rows points at *n_rows called alleles in memory of the handle — for a batch the device
 * called alone, the pinned host buffer the last kernel wrote them to — valid until the next pisces_hip_flush* / pisces_hip_flush_begin on the
 * handle.  cand_index / cands / alleles (any may be NULL) as pisces_hip_flush_ex returns them; *cand_index is NULL when no row has a
 * candidate (every row is a Reference or SNV row).  No PISCES_E_BUFFER_TOO_SMALL: nothing is copied. */
int32_t pisces_hip_flush_view(PiscesHip* h, int32_t up_to_position, const PiscesCalledAllele** rows, int64_t* n_rows, const int32_t** cand_index,
                              const PiscesCandidate** cands, int64_t* n_cand, const uint8_t** alleles, int64_t* allele_bytes);
int32_t pisces_hip_flush_end_view(PiscesHip* h, const PiscesCalledAllele** rows, int64_t* n_rows, const int32_t** cand_index,
                                  const PiscesCandidate** cands, int64_t* n_cand, const uint8_t** alleles, int64_t* allele_bytes);
/* PloidyModel.DiploidByAdaptiveGT: the mixture's parameters.  A handle created with PISCES_PLOIDY_DIPLOID_ADAPTIVE starts with
 * pisces_hip_adaptive_default_params (the reference's defaults).  PISCES_E_INVALID_ARG for means or priors outside (0, 1) or means that do
 * not ascend, PISCES_E_STATE on a handle of another ploidy.  Any time before the flush / launch that should see them. */
int32_t pisces_hip_adaptive_default_params(PiscesAdaptiveParams* params);
int32_t pisces_hip_set_adaptive_params(PiscesHip* h, const PiscesAdaptiveParams* params);
/* CalledAllele.GenotypePosteriors of the rows the most recent pisces_hip_flush / _flush_ex / _flush_view / _flush_end* handed out: same
 * order, same count (*n_out; PISCES_E_BUFFER_TOO_SMALL with *n_out = the count needed when capacity is short, nothing is lost).  Rows of
 * a handle of another ploidy, and forced-report rows, have n = 0.  pisces_hip_posteriors_view: where they lie in memory of the handle, valid
 * as long as the rows of pisces_hip_flush_view / pisces_hip_flush_end_view are (until the next flush on the handle; same thread as the
 * flush).  In a flush the adaptive genotyper is the host pass over the merged rows. */
int32_t pisces_hip_get_posteriors(PiscesHip* h, PiscesGenotypePosteriors* out, int64_t capacity, int64_t* n_out);
int32_t pisces_hip_posteriors_view(PiscesHip* h, const PiscesGenotypePosteriors** rows, int64_t* n_rows);
/* IAlleleSource.GetAlleleCount for a run of positions: out[n][6][3][11] int32
 * (RegionState.cs:57); blocks never touched read as zero (RegionStateManager.cs:222-226). */
int32_t pisces_hip_get_counts(PiscesHip* h, int32_t start_position, int32_t n, int32_t* out);
/* IAlleleSource.GetSumOfAlleleBaseQualities (src/lib/Pisces.Domain/Interfaces/IAlleleSource.cs:16; RegionState.cs:61,233-239): the
 * base-quality sums double[n][6][3][11] of [start_position, start_position + n), same layout and rules as pisces_hip_get_counts (the
 * caller applies the anchor window, AlleleCountHelper.GetAnchorAdjustedTotalQuality).  Served by any handle, not only NoiseModel.Window.
 * The device accumulates in fixed point: each cell is the true sum rounded once, identical from run to run. */
int32_t pisces_hip_get_base_quality_sums(PiscesHip* h, int32_t start_position, int32_t n, double* out);
/* IAlleleSource.GetGappedMnvRefCount (IAlleleSource.cs:19; RegionStateManager.cs:256-261): what pisces_hip_add_gapped_mnv_ref (or a flush,
 * for the gaps of its callable MNVs) registered for the position and no flush has retired with the position's block since; 0 for every
 * other position > 0, however far out (no block: no count, as for the allele counts).  position <= 0: PISCES_E_INVALID_ARG, *count
 * untouched (GetBlock's "Position must be greater than 0.", :363-364).  The handle is the manager, its blocks are made on demand: the
 * single RegionState's "outside the region" (RegionState.cs:86-92, 375-381) has no counterpart here. */
int32_t pisces_hip_get_gapped_mnv_ref(PiscesHip* h, int32_t position, int32_t* count);
/* IAlleleSource.AddGappedMnvRefCount (RegionStateManager.cs:74-81): counts[i] is added to what positions[i] holds (0 changes nothing, a
 * position not named keeps its count); every position > 0 is accepted and makes its block.  A position <= 0 anywhere in the call:
 * PISCES_E_INVALID_ARG and nothing of the call is added. */
int32_t pisces_hip_add_gapped_mnv_ref(PiscesHip* h, const int32_t* positions, const int32_t* counts, int32_t n);
/* host-side candidates (insertion / deletion) found so far with position <= up_to (< 0 = all)
 * (IStateManager.GetCandidatesToProcess for the host collapser). alleles = byte pool; out may be NULL to count. */
int32_t pisces_hip_get_candidates(PiscesHip* h, int32_t up_to_position, PiscesCandidate* out,
                                  int64_t capacity, int64_t* n_out, uint8_t* alleles,
                                  int64_t allele_capacity, int64_t* allele_bytes);
/* IStateManager.AddCandidates (src/lib/Pisces.Domain/Interfaces/IStateManager.cs; RegionStateManager.cs:83-116) for candidates the caller
 * brings itself: merged with the candidates the library finds in the reads by RegionState.AddCandidate's rules (RegionState.cs:94-174).
 * cands[i].allele_offset / ref_len / alt_len index `alleles` (ref bytes then alt bytes), as pisces_hip_get_candidates writes them. */
int32_t pisces_hip_add_candidates(PiscesHip* h, const PiscesCandidate* cands, int64_t n, const uint8_t* alleles, int64_t allele_bytes);
/* Forced genotyping (-forcedalleles; Factory.GetForcedAlleles :56-96 + SelectForcedAllele :270-286, src/exe/Pisces/Logic/Factory.cs): the
 * alleles of this chromosome that are reported whatever the reads say.  Only position and the allele strings are read (the category
 * is SmallVariantCaller.GetAlleleCategory's, SmallVariantCaller.cs:141-150); alleles equal to the reference, with an ALT outside
 * A/C/G/T or outside the intervals of pisces_hip_set_intervals are dropped as the reference drops them.  From then on every flush first
 * adds the forced alleles up to upTo as candidates without support (AddForcedAlleleAsCandidate :118-132), reports a forced allele that
 * is not callable with PISCES_FILTER_FORCED_REPORT, genotype 0/1 and genotype q-score 0 (AlleleCaller.cs:98-131, 143-170), keeps the
 * Reference row beside it, and when include_reference_calls is off makes Reference rows at the forced positions
 * (RegionState.GetAllCandidates :393-450).  With the diploid model DiploidLocusProcessor's rules apply (PISCES_GT_OTHERS).  Call it
 * after pisces_hip_set_intervals and before the first flush. */
int32_t pisces_hip_set_forced_alleles(PiscesHip* h, const PiscesCandidate* alleles_of, int64_t n, const uint8_t* alleles, int64_t allele_bytes);
/* IAlleleCaller.TotalNumCalled with an interval set and MNV calling off: AlleleCaller.Call counts in IsCallable, BEFORE ShouldReport
 * (AlleleCaller.cs:109-131), so the reference's total includes the callable SNVs of loci OUTSIDE the intervals, which it does not report.
 * By default the library evaluates the intervals' loci only (the total then counts the callable alleles inside them; every reported row
 * is the reference's either way).  on != 0: every flush also runs its kernel over the off-interval loci of the flushed blocks, drops the
 * records and adds their callable alleles — the reference's number, at the price of a second launch per flush.  With MNV calling on (or collapser
 * thresholds that keep an open-ended SNV and its twin apart) the SNVs are candidates and the candidate path counts the callable ones outside the intervals itself (the switch changes
 * nothing).  The counting launch is the read store's flush kernel: a flush of a configuration that kernel does not serve (NoiseModel.Window,
 * the Diploid strand-bias model, a gapped-MNV reference count in the flushed blocks, the observation-log read path, minimum base quality
 * above 127) fails with PISCES_E_UNSUPPORTED while the switch is on instead of reporting the smaller total. */
int32_t pisces_hip_set_exact_total_called(PiscesHip* h, int32_t on);
/* The chromosome's known (prior) variants: what Factory.cs:204 hands VariantCollapser (the priors file's insertions and MNVs, Factory.cs:378-395).
 * With the collapser on, a candidate that equals one (position, reference allele, alternate allele, type) is anchored on both sides and
 * preferred among the potential matches of an open-ended candidate (VariantCollapser.cs:16-24, 178-190, 216-218).  Same arguments as
 * pisces_hip_set_forced_alleles (position, ref_len, alt_len, allele_offset of every entry; the rest is ignored); n = 0 clears.  Any time
 * before the flush that should see them. */
int32_t pisces_hip_set_known_variants(PiscesHip* h, const PiscesCandidate* variants, int64_t n, const uint8_t* alleles, int64_t allele_bytes);
/* PiscesApplicationOptions.ExcludeMNVsFromCollapsing (Options/PiscesApplicationOptions.cs:62; Factory.cs:204 hands it to VariantCollapser):
 * on != 0: MNV candidates are left out of the collapser's targets (VariantCollapser.cs:33) — an open-ended MNV is not collapsed, and no
 * open-ended SNV / MNV collapses INTO an MNV.  Off by default, as the option.  Any time before the flush that should see it. */
int32_t pisces_hip_set_exclude_mnvs_from_collapsing(PiscesHip* h, int32_t on);
/* totals lines: {allelesCalled (IAlleleCaller.TotalNumCalled), variantsCollapsed, readsProcessed, readsSkipped}
 * (SmallVariantCaller.cs:114-115; readsSkipped = AlignmentSource's count of the reads ShouldSkipRead dropped, AlignmentsSource.cs:63,84-92:
 * the reads pisces_hip_bam_decode dropped from the batches that pisces_hip_add_decoded_reads added; reads a host hands over through
 * pisces_hip_add_reads have passed that filter already).  This is the vector pisces_hip_reduce_summary adds up over the interval shards. */
int32_t pisces_hip_stats(PiscesHip* h, int64_t out[4]);

/* Where the host's time went inside the streaming surface since the handle was made (or since the last call with reset != 0), seconds:
 * {pisces_hip_add_reads / pisces_hip_add_decoded_reads, pisces_hip_flush / _flush_ex / _flush_begin / _flush_end in all, of that waiting
 * for the device (stream / event synchronisation), number of flushes that made a batch}.  (flush - waiting) / flushes is the serial host
 * work per flush: block bookkeeping, candidate merge, VariantCollapser, MnvReallocator, the diploid genotyper, record assembly
 * (what runs on one core of the host next to the device; IAlleleCaller.Call's host half, AlleleCaller.cs:60-141). */
int32_t pisces_hip_host_time(PiscesHip* h, double out[4], int32_t reset);
/* Bytes that crossed PCIe for this handle since the last reset: {host -> device: read batches as handed to pisces_hip_add_reads, or the
 * compressed file bytes and block table of pisces_hip_bam_decode; device -> host: called-allele records; device -> host: the candidate
 * records of the device finder (64 B per read event + long ALT alleles); device -> host: allele counts for the collapser / reallocator}. */
int32_t pisces_hip_transfer_bytes(PiscesHip* h, int64_t out[4], int32_t reset);

/* ---- multi-GPU: the per-chromosome summary across interval shards --------------------------------------------------
 * Loci shard by genomic interval, one process (or one handle) per GPU, no data-path exchange; the only collective is the sum of
 * the int64[4] totals above over the shards (the reference concatenates per-chromosome jobs and prints their totals,
 * src/lib/Pisces.Processing/Logic/BaseGenomeProcessor.cs:40-90, SmallVariantCaller.cs:114-115).  RCCL over xGMI, bound at run time
 * (librccl is loaded when comm_init is first called, so a single-GPU host needs no RCCL):
 *   rank 0:      pisces_hip_comm_unique_id(id)            -> hands the 128 bytes to the other processes (file, pipe, MPI, ...)
 *   every rank:  pisces_hip_comm_init(h, id, rank, world) -> ncclCommInitRank on the handle's device
 *   every rank:  pisces_hip_reduce_summary(h, totals)     -> one ncclAllReduce(sum) of int64[4] on the handle's stream, in place
 * Without a communicator (never initialised, or world == 1) reduce_summary leaves `inout` as it is.  Handles of ONE process on
 * several GPUs can simply add their pisces_hip_stats on the host. */
#define PISCES_COMM_ID_BYTES 128
int32_t pisces_hip_comm_unique_id(uint8_t* id_out, int32_t capacity);
int32_t pisces_hip_comm_init(PiscesHip* h, const uint8_t* id, int32_t rank, int32_t world);
int32_t pisces_hip_reduce_summary(PiscesHip* h, int64_t inout[4]);
int32_t pisces_hip_comm_destroy(PiscesHip* h);
/* Which librccl the library binds, and how it found it — in this order, the first that applies deciding: (1) the file PISCES_HIP_RCCL_PATH
 * names (an error naming it if it cannot be bound); (2) a librccl.so the process has mapped already (a PyTorch host brings its own under
 * torch/lib: binding THAT copy keeps one RCCL per process); (3) librccl.so.1 / librccl.so on the loader's path, then /opt/rocm/lib.
 * Writes "<source>: <path>" (source = PISCES_HIP_RCCL_PATH | mapped | default) and returns its length, or PISCES_E_DEVICE. */
int32_t pisces_hip_comm_library(char* out, int32_t capacity);
/* ncclCommCount of the handle's communicator (1 without one). */
int32_t pisces_hip_comm_ranks(PiscesHip* h, int32_t* ranks);

/* ---- device-resident surface (bench / multi-GPU shards) --------------------
 * All d_* pointers are device pointers on the handle's device; stream is a hipStream_t
 * (NULL = the handle's own stream).  One launch: per tile, observation tuples -> LDS
 * allele-count histogram -> coverage, Poisson q-score, strand bias, somatic genotype and
 * filters for the reference allele and every SNV candidate -> 64-byte records.
 * d_ref_bases[i] is the reference base of position ref_start_position+i.
 * d_records needs record_capacity >= 256 * n_tiles slots (PiscesTileResult explains the slot layout: no
 * allocation atomics, placement independent of scheduling); d_tile_results[n_tiles] is the directory.
 * Asynchronous; launches of one handle must be stream-ordered with respect to each other. */
/* The tile size (<= 64 loci) at which a launch over n_loci contiguous loci loads every CU of the handle's device equally: a launch
 * that is resident at once ends with the CU that holds the most tiles (100 000 loci: 56, i.e. 1786 tiles = 7 per CU, instead of 1563
 * tiles of 64 = 6 or 7 per CU).  64 for launches of many rounds.  A hint for whoever buckets tuples by tile. */
int32_t pisces_hip_balanced_tile_loci(PiscesHip* h, int64_t n_loci);
int32_t pisces_hip_call_tiles(PiscesHip* h, const uint32_t* d_tuples, const PiscesTile* d_tiles,
                              int32_t n_tiles, const uint8_t* d_ref_bases, int32_t ref_start_position,
                              int64_t ref_length, PiscesCalledAllele* d_records, int32_t record_capacity,
                              PiscesTileResult* d_tile_results, void* stream);
/* Several independent batches at once: the launches are spread over the handle's own HIP streams ("lanes"), so that the call phase
 * that ends one launch runs under the streaming phase of the next (at BASELINE config 2 a step takes ~37 us this way instead of ~52 us
 * one after the other).  Every batch in flight needs its own d_records / d_tile_results.  Ordering is on the host: the call first
 * waits for `stream` (NULL = nothing to wait for: the inputs are ready), returns once everything is enqueued, and the outputs are
 * complete after pisces_hip_synchronize (a lane that has waited on another stream's event runs its later kernels ~5 us slower on
 * this runtime, so no event fork / join).  The process should run with GPU_MAX_HW_QUEUES >= 8 so that each lane owns a hardware
 * queue. */
typedef struct PiscesTileBatch {
    const uint32_t*     d_tuples;
    const PiscesTile*   d_tiles;
    int32_t             n_tiles;
    int32_t             ref_start_position;
    const uint8_t*      d_ref_bases;
    int64_t             ref_length;
    PiscesCalledAllele* d_records;
    PiscesTileResult*   d_tile_results;
    int32_t             record_capacity;
    int32_t             pad;
} PiscesTileBatch;
int32_t pisces_hip_call_tiles_batched(PiscesHip* h, const PiscesTileBatch* batches, int32_t n_batches, void* stream);

/* The same launches as ONE HIP graph: pisces_hip_call_tiles_graph_build captures the n_batches launches (in order, on one stream: what
 * pisces_hip_call_tiles n_batches times does) into a graph the handle keeps and returns its id; pisces_hip_call_tiles_graph_launch replays
 * it on `stream` (NULL = the handle's) with one submission — the launches then follow each other at the device's own pace instead of the
 * host's (a launch call per step leaves ~10 us between 38 us kernels at BASELINE config 2).  With pisces_hip_set_timing(n) in force when
 * the graph is built, every n-th launch is bracketed by event records inside the graph, read back by pisces_hip_kernel_time after a
 * replay.  The buffers named by `batches` must stay where they are while the graph is in use; graphs go with the handle. */
int32_t pisces_hip_call_tiles_graph_build(PiscesHip* h, const PiscesTileBatch* batches, int32_t n_batches, int32_t* graph_id);
int32_t pisces_hip_call_tiles_graph_launch(PiscesHip* h, int32_t graph_id, void* stream);

/* Ordered compaction of a call_tiles result: d_out[0 .. *d_count) receives every called allele of the launch
 * sorted by (position, ref, alt) (tiles must be in ascending position order); d_offsets[n_tiles] (int32 scratch)
 * receives each tile's first index in d_out. Asynchronous. */
int32_t pisces_hip_compact_records(PiscesHip* h, const PiscesCalledAllele* d_records,
                                   const PiscesTileResult* d_tile_results, int32_t n_tiles, int32_t* d_offsets,
                                   PiscesCalledAllele* d_out, int32_t out_capacity, int32_t* d_count, void* stream);
/* PloidyModel.DiploidByAdaptiveGT on the device-resident surface: names the device buffer, slot-parallel to d_records (entry i = the
 * posteriors of record slot i; capacity >= 256 * n_tiles entries, else pisces_hip_call_tiles returns PISCES_E_BUFFER_TOO_SMALL), that every
 * later pisces_hip_call_tiles of this handle fills behind its tile kernel; capacity 0 = none (genotypes and q-scores only).
 * PISCES_E_STATE on a handle of another ploidy.  pisces_hip_call_tiles_batched and pisces_hip_call_tiles_graph_build refuse an adaptive
 * handle with PISCES_E_UNSUPPORTED (one posteriors buffer a handle). */
int32_t pisces_hip_set_posteriors_buffer(PiscesHip* h, PiscesGenotypePosteriors* d_posteriors, int64_t capacity);
/* The posteriors in the order of pisces_hip_compact_records' output: d_out[i] belongs to its d_out[i].  d_offsets is what
 * pisces_hip_compact_records left there for the same d_tile_results (call it first, on the same stream).  Asynchronous. */
int32_t pisces_hip_compact_posteriors(PiscesHip* h, const PiscesGenotypePosteriors* d_posteriors, const PiscesTileResult* d_tile_results,
                                      int32_t n_tiles, const int32_t* d_offsets, PiscesGenotypePosteriors* d_out, int32_t out_capacity,
                                      void* stream);
/* VCF body lines of device-resident rows, written on the device: the bytes pisces_hip_format_vcf_ex writes for the same rows (one line
 * a row; see "VCF body lines" below for the columns and PiscesVcfConfig).  Asynchronous on `stream` and ordered behind whatever made
 * the rows: pisces_hip_call_tiles -> pisces_hip_compact_records -> this, with no host wait in between.  Every d_* pointer is
 * device-accessible (d_text may be pinned host memory).
 *   d_count        optional: the word pisces_hip_compact_records leaves; min(n, *d_count) rows are formatted (NULL: n)
 *   d_cand_index, d_cands, d_alleles
 *                  optional: what pisces_hip_flush_ex returns, in device memory; a row without an index >= 0 takes its alleles from
 *                  the base codes of `info`
 *   d_gp           optional: d_gp[i] belongs to row i, a row with n > 0 gets the :GP column
 *   d_line_offsets optional, rows + 1 entries: the byte offset of every line, then the total (written when the text is)
 *   *d_text_bytes  the bytes of text.  Above text_capacity: no byte of d_text was written, repeat with a larger buffer.  Negative:
 *                  the PISCES_E_* code pisces_hip_format_vcf_ex returns for these rows (a LowVariantQscore bit with
 *                  variant_quality_filter < 0, an RMxN bit without its two numbers, a cand_index >= 0 without candidates: the lowest
 *                  such row decides, PISCES_E_INVALID_ARG), and no text either.
 * Calls of one handle share the handle's scratch (4 bytes a row): like every launch of this surface they must be stream-ordered with
 * respect to each other — one stream, or serialised by the caller.  A call that has to grow the scratch waits first: for its stream, or
 * for the whole device once the handle has seen a stream that is not its own.
 * Refused at the call: null h / cfg / chrom / d_text_bytes or a negative size (PISCES_E_INVALID_ARG); cfg->crush (crushed lines merge
 * the rows of a position) and RegionMapper's padding stay with the host formatter, as do a chrom above 1024 bytes and thresholds that
 * ask for more than 7 VF decimals (PISCES_E_UNSUPPORTED, each with a message). */
struct PiscesVcfConfig;   /* defined with the VCF entries below */
int32_t pisces_hip_format_vcf_device(PiscesHip* h, const struct PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* d_recs,
                                     int64_t n, const int32_t* d_count, const int32_t* d_cand_index, const PiscesCandidate* d_cands,
                                     const uint8_t* d_alleles, const PiscesGenotypePosteriors* d_gp, char* d_text,
                                     int64_t text_capacity, int64_t* d_line_offsets, int64_t* d_text_bytes, void* stream);
/* tuples -> anchor-resolved counts added into d_counts[n_tiles*tile_loci][6][3][11]
 * (the IAlleleSource view for host-side collapsing / spanning coverage). Asynchronous. */
int32_t pisces_hip_accumulate_tiles(PiscesHip* h, const uint32_t* d_tuples, const PiscesTile* d_tiles,
                                    int32_t n_tiles, int32_t* d_counts, void* stream);
/* Device-side running totals bumped by every call_tiles launch of this handle:
 * {records written, candidate loci, IsCallable==true alleles (IAlleleCaller.TotalNumCalled), tiles}.
 * Synchronizes the handle's stream; reset != 0 zeroes them afterwards.  This is the per-chromosome
 * summary a multi-GPU job all-reduces (SmallVariantCaller.cs:114-115 totals line). */
int32_t pisces_hip_device_totals(PiscesHip* h, int64_t out[4], int32_t reset);
/* Kernel timing with HIP events bound to the kernel's own dispatch on the launch stream (start and stop events of
 * hipExtLaunchKernel).  Off by default.
 * enable = n > 0 starts a fresh measurement window in which every n-th call_tiles / accumulate_tiles launch is timed
 * (up to 4096 timed launches are kept); enable = 0 ends it. */
int32_t pisces_hip_set_timing(PiscesHip* h, int32_t enable);
/* A span on the launch stream: pisces_hip_mark(h, 0, stream) before the first of a run of launches, pisces_hip_mark(h, 1, stream) behind the
 * last (HIP events on `stream`, NULL = the handle's own stream: the stream the launches go to); pisces_hip_marked_ms waits for the
 * second mark and returns the time between the two.  Two event records for any number of launches: what bench.py brackets its timed
 * region with (events of every dispatch, pisces_hip_set_timing, put 5-10 us between launches). */
int32_t pisces_hip_mark(PiscesHip* h, int32_t which, void* stream);
int32_t pisces_hip_marked_ms(PiscesHip* h, float* ms);
/* Sum of the timed kernel durations (ms) and number of timed launches since set_timing(n). Waits for them. */
int32_t pisces_hip_kernel_time(PiscesHip* h, double* total_ms, int64_t* launches);
/* The device time of the streaming surface's chain reads -> records (bench.py's roofline_chain).  enable != 0: every
 * pisces_hip_add_device_reads records an event on the handle's stream before the first thing it enqueues and one behind the last, every
 * flush one in front of its first kernel and one behind the kernel that leaves the compacted records in HBM (the transfer to the host
 * follows that event).  pisces_hip_chain_time waits for the last add's and the last flush's events: out_ms[0] = the add's span
 * (IStateManager.AddAlleleCounts + ICandidateVariantFinder.FindCandidates of the batch, RegionStateManager.cs:118-220,
 * CandidateVariantFinder.cs:36-83), out_ms[1] = the flush's (GetCandidatesToProcess + IAlleleCaller.Call); PISCES_E_STATE when either has
 * not happened since timing was switched on. */
int32_t pisces_hip_set_chain_timing(PiscesHip* h, int32_t enable);
int32_t pisces_hip_chain_time(PiscesHip* h, double out_ms[2]);
/* Streaming-read bandwidth of the handle's device, GB/s: best of `reps` timed passes of a kernel that only reads `nbytes`
 * with the hot kernel's load pattern.  Reported beside the spec peak in bench.py; allocates and frees nbytes. */
int32_t pisces_hip_probe_read_bandwidth(PiscesHip* h, int64_t nbytes, int32_t reps, double* gb_per_s);
/* waits for the handle's stream */
int32_t pisces_hip_synchronize(PiscesHip* h);
/* The handle's own stream (a hipStream_t), i.e. what a NULL `stream` argument of the calls above stands for.  It is created
 * hipStreamNonBlocking: it does NOT order against HIP's null stream.  A host whose runtime fills or allocates-and-zeroes device
 * buffers on the null stream (PyTorch's default stream is the null stream) must therefore either enqueue that work on this stream
 * (torch.cuda.ExternalStream over the value returned here) or wait for it before handing the buffers to the library; passing its
 * own null-stream handle (0) as `stream` selects THIS stream, not the null stream, and orders nothing. */
int32_t pisces_hip_get_stream(PiscesHip* h, void** stream);
/* duration of the most recent timed launch of the current window, in milliseconds (PISCES_E_STATE when timing is off) */
int32_t pisces_hip_last_kernel_ms(PiscesHip* h, float* ms);

/* ---- host-side helpers (pure CPU, no device needed) -------------------------- */
/* Expands reads to (position, tuple) observations exactly as AddAlleleCounts walks a read
 * (RegionStateManager.cs:118-220).  Returns the number written or PISCES_E_BUFFER_TOO_SMALL. */
int64_t pisces_hip_expand_reads(const PiscesReadBatch* batch, int32_t min_base_call_quality,
                                int32_t* positions, uint32_t* tuples, int64_t capacity);

/* ICandidateVariantFinder.FindCandidates restricted to insertions and deletions
 * (CandidateVariantFinder.cs:234-292, Create :334-345, Annotate :496-553), one entry per read event, unmerged,
 * in read order. ref[i] is position i+1. Returns the count or PISCES_E_BUFFER_TOO_SMALL. */
int64_t pisces_hip_find_indel_candidates(const PiscesReadBatch* batch, const uint8_t* ref, int64_t ref_len,
                                         int32_t min_base_call_quality, PiscesCandidate* out, int64_t capacity,
                                         uint8_t* alleles, int64_t allele_capacity, int64_t* allele_bytes);
/* The whole of CandidateVariantFinder.FindCandidates (CandidateVariantFinder.cs:36-387,496-553): with snvs_and_mnvs the M operations are
 * walked too (ExtractSnvsFromOperation :90-232; call_mnvs / max_mnv_length / max_gap_between_mnv are ShouldBuildUpMNV's :170-181).
 * Same outputs as above.  Host form of the walk (no handle, no device); pisces_hip_add_reads runs the device form below. */
int64_t pisces_hip_find_candidates(const PiscesReadBatch* batch, const uint8_t* ref, int64_t ref_len, int32_t min_base_call_quality,
                                   int32_t snvs_and_mnvs, int32_t call_mnvs, int32_t max_mnv_length, int32_t max_gap_between_mnv,
                                   PiscesCandidate* out, int64_t capacity, uint8_t* alleles, int64_t allele_capacity, int64_t* allele_bytes);
/* The same walk on the handle's device (find_count_kernel / find_emit_kernel: one lane per read), against the reference given to
 * pisces_hip_set_reference and with the handle's minimum base quality: the candidate discovery pisces_hip_add_reads enqueues for
 * every batch, here with its records returned per read event, unmerged, in read order — what the parity tests compare with
 * the reference's own finder cases.  Same outputs and return values as pisces_hip_find_candidates. */
int64_t pisces_hip_find_candidates_device(PiscesHip* h, const PiscesReadBatch* batch, int32_t snvs_and_mnvs, int32_t call_mnvs,
                                          int32_t max_mnv_length, int32_t max_gap_between_mnv, PiscesCandidate* out, int64_t capacity,
                                          uint8_t* alleles, int64_t allele_capacity, int64_t* allele_bytes);

/* ---- the host half of IAlleleCaller.Call as functions of their own (pure CPU) ------------------------------------------------------
 * What pisces_hip_flush runs on the host between its device passes, callable on alleles the caller brings — the reference's own unit
 * tests drive MnvReallocator and the genotypers this way (MNVReallocatorTests.cs, GenotypeCalculatorTest.cs), and so do this repository's
 * (tests/test_product_goldens.py: the reference's known answers through the PRODUCT's code, not through the oracle's restatement).
 *
 * MnvReallocator.ReallocateFailedMnvs(failedMnvs, callableAlleles, blockMaxPos) (src/exe/Pisces/Logic/VariantCalling/MnvReallocator.cs:12-98):
 * the support of MNVs that are not callable goes to the callable alleles inside them (longest first, then most support), what is left
 * becomes smaller MNVs / SNVs, and — with block_max_position >= 0 — what lies past the block goes to `outside`.  An allele's
 * AlleleSupport is the sum of support_by_dir (the product keeps no second number).  Candidates in, candidates out (same pool layout as
 * pisces_hip_get_candidates); returns PISCES_E_BUFFER_TOO_SMALL with the three counts set when an output is short. */
int32_t pisces_hip_reallocate_failed_mnvs(const PiscesCandidate* failed, int64_t n_failed, const PiscesCandidate* callable, int64_t n_callable,
                                          const uint8_t* alleles, int64_t allele_bytes, int32_t block_max_position,
                                          PiscesCandidate* callable_out, int64_t callable_capacity, int64_t* n_callable_out,
                                          PiscesCandidate* outside_out, int64_t outside_capacity, int64_t* n_outside_out,
                                          uint8_t* alleles_out, int64_t allele_capacity, int64_t* allele_bytes_out);
/* The per-locus genotypers of the germline modes over the alleles of ONE locus (Reference row gone when a variant is there, rows in
 * (ref, alt) order — what pisces_hip_flush hands them): DiploidThresholdingGenotyper.SetGenotypes
 * (src/lib/Pisces.Genotyping/Thresholding/DiploidThresholdingGenotyper.cs:54-141) with cfg->ploidy == PISCES_PLOIDY_DIPLOID,
 * HaploidGenotyper.SetGenotypes (Haploid/HaploidGenotyper.cs:36-83) with PISCES_PLOIDY_HAPLOID; thresholds, minimum depth (min_coverage)
 * and the q-score range come from cfg.  Fills the result fields of every allele; returns the locus' genotype (PISCES_GT_*) or < 0. */
typedef struct PiscesGenotypeAllele {
    int32_t category;                 /* PISCES_CAT_* */
    int32_t ref_len, alt_len;
    int32_t support, coverage, reference_support;
    int64_t allele_offset;            /* ref bytes then alt bytes in the allele pool */
    int32_t genotype, genotype_qscore, phase_set_index;   /* results */
    uint8_t multi_allelic, prune, pad[2];                 /* results: FilterType.MultiAllelicSite; the genotyper drops the allele */
} PiscesGenotypeAllele;
int32_t pisces_hip_set_genotypes(const PiscesHipConfig* cfg, PiscesGenotypeAllele* alleles_of_one_locus, int32_t n, const uint8_t* alleles,
                                 int64_t allele_bytes);
/* DiploidAdaptiveGenotyper.SetGenotypes (Adaptive/DiploidAdaptiveGenotyper.cs:45-176) over the alleles of ONE locus, n >= 1, in the caller's
 * order (the 1/2 multinomial takes the first two as given, a Reference row included): minimum depth and q-score range from cfg, the mixture
 * from params; posteriors_out[n] (may be NULL) receives every allele's posteriors, the pruned ones' too.  Returns the locus' genotype or < 0. */
int32_t pisces_hip_set_genotypes_adaptive(const PiscesHipConfig* cfg, const PiscesAdaptiveParams* params, PiscesGenotypeAllele* alleles_of_one_locus,
                                          int32_t n, const uint8_t* alleles, int64_t allele_bytes, PiscesGenotypePosteriors* posteriors_out);
/* AdaptiveGenotyperCalculator.GetGenotypeAndQScore (AdaptiveGenotyperCalculator.cs:32-36) for one allele with coverage: the mixture component
 * (0 hom-ref, 1 het, 2 hom-alt), the q-score before the handle's [min, max] clamp (0..100) and three phred-scaled posteriors; `category`
 * (PISCES_CAT_*) selects the SNV or the indel pair, is_reference the reference allele's depth (coverage - support). */
int32_t pisces_hip_adaptive_genotype_qscore(const PiscesAdaptiveParams* params, int32_t category, int32_t is_reference, int32_t allele_support,
                                            int32_t total_coverage, int32_t* category_out, int32_t* qscore_out, float* gp_out);
/* DiploidGenotypeQualityCalculator.Compute (Thresholding/DiploidGenotypeQualityCalculator.cs:17-103) for one allele */
int32_t pisces_hip_diploid_genotype_qscore(int32_t genotype, int32_t total_coverage, int32_t allele_support, int32_t min_qscore, int32_t max_qscore);
/* AmpliconBiasCalculator.CalculateAmpliconBias (src/lib/Pisces.Calculators/AmpliconBiasCalculator.cs:45-134; -abfilter, FILTER AB) for ONE
 * SNV, host only, no handle: entry i of the two arrays is one amplicon of the locus' CoverageByAmplicon, support[i] what the allele's
 * SupportByAmplicon holds under the same name (0 when it holds none, AmpliconCounts.GetCountsForAmplicon); counts >= 0, any order (no
 * decision depends on it).  With freq_i = support_i / coverage_i (0 without coverage) and expected_i = max(freq) * coverage_i, an
 * amplicon's chance is 1 when expected_i < 5, expected_i <= support_i or freq_i > 0.1, else max(0, Poisson.Cdf(support_i, expected_i))
 * (Pisces' own stats/Poisson.cs).  Returns 1 when any chance < (double)threshold (the row gets PISCES_FILTER_AMPLICON_BIAS), 0 when none is,
 * and -1 for no result (AmpliconBiasResults stays null, nothing to filter on): n < 2, or no entry of `support` above zero — aligned by
 * name, a support list without counts and an empty one are the same arrays; the reference fails neither.  -1 as well for a NULL array: this
 * entry returns no PISCES_E_* code.  chance_out[n] (may be NULL) receives the chances when the result is 0 or 1.  The per-amplicon
 * q-score and AmpliconWithCandidateArtifact (the AmpliconBias.csv columns) are not computed.  csrc/amplicon_bias.h, written for host and
 * device alike. */
int32_t pisces_hip_amplicon_bias(const int32_t* support, const int32_t* coverage, int32_t n, float threshold, double* chance_out);

/* ---- the amplicon-bias filter on the streaming surface (VariantCallingParameters.AmpliconBiasFilterThreshold, -abfilter, FILTER AB) ----
 * Factory.ShouldTrackAmpliconCounts: threshold >= 0 makes the handle track per-amplicon counts and end every flush (pisces_hip_flush, _ex,
 * _view, _begin / _end*) with the filter: for every called SNV row with support, CoverageByAmplicon of its position and the row's
 * SupportByAmplicon go through the decision of pisces_hip_amplicon_bias, and a detected bias ORs 1 << PISCES_FILTER_AMPLICON_BIAS into the row's
 * filter_bits (AlleleProcessor.ApplyFilters, AlleleProcessor.cs:45-63) — nothing else of the row changes, rows of other categories never get
 * it (AmpliconBiasCalculator.cs:27).  threshold < 0 = null: off, the default; a handle that is off launches nothing for it.  Must come before
 * the first read is added (PISCES_E_STATE afterwards).  A read's amplicon (Read.GetAmpliconNameIfExists: the BAM XN tag, Read.cs:483-486)
 * crosses as an int32 id, -1 = no tag: an id the host chooses (pisces_hip_add_reads_amplicons), or an id of the handle's name dictionary,
 * which pisces_hip_bam_decode fills from the XN tags on the device (below).  PISCES_E_UNSUPPORTED, each with a message, for what cannot go together with
 * tracking: call_mnvs, collapse thresholds that take SNV candidates from the read walk (collapse_freq_threshold > 0 or
 * collapse_freq_ratio_threshold >= 1), forced alleles (set before: the setter refuses; pisces_hip_set_forced_alleles refuses afterwards),
 * PISCES_HIP_READ_PATH=log; and on a tracking handle pisces_hip_add_observations (tuples have no read identity) and
 * pisces_hip_add_decoded_reads when the decoded batch carries no ids (nothing decoded, or decoded before tracking was switched on).  The tuple surface (pisces_hip_call_tiles*) never had tags and is untouched.
 * A flush that meets a position with more than six amplicons (Constants.MaxNumOverlappingAmplicons, Constants.cs:54-62: the reference
 * indexes slot -1 and throws IndexOutOfRangeException) returns PISCES_E_INVALID_ARG naming the lowest such position; the blocks stay held.
 * A flush counts only in the 64-locus tiles that hold a called SNV row with support (the others cannot get the filter and are skipped), so
 * it meets such a position only there; pisces_hip_get_amplicon_counts counts every tile of its range and always reports it.
 * min_base_call_quality above 127 is served: the store's per-base codes hold the quality test only up to 127, above it the counting reads
 * the qualities themselves, so the counts by amplicon drop the bases the caller's own counts drop.
 * A tracking flush waits for its kernels before it returns (pisces_hip_flush_begin included). */
int32_t pisces_hip_set_amplicon_bias_filter(PiscesHip* h, float threshold);
/* pisces_hip_add_reads / pisces_hip_add_device_reads with one id per read (amplicon_id[n_reads]; the device form's is a device pointer,
 * copied like the batch).  pisces_hip_stage_reads' views are accepted by the host form.  On a handle without the filter the ids are ignored
 * and nothing is stored: exactly the plain add.  On a tracking handle the plain adds still work, their reads carry -1 (they count in no
 * slot).  An id below -1: PISCES_E_INVALID_ARG, the state unchanged. */
int32_t pisces_hip_add_reads_amplicons(PiscesHip* h, const PiscesReadBatch* batch, const int32_t* amplicon_id);
int32_t pisces_hip_add_device_reads_amplicons(PiscesHip* h, const PiscesReadBatch* device_batch, int64_t n_cigar_ops, int64_t n_bases,
                                              const int32_t* device_amplicon_id);
/* IAlleleSource.GetCoverageByAmplicon for [start_position, start_position + n) plus the support split, same rules as pisces_hip_get_counts
 * (positions of held blocks; others read as empty): ids[n][6] the amplicon ids of a position, coverage[n][6] their counts of A/C/G/T bases
 * at or above the minimum base quality (deleted positions, N and low-quality bases and reads without a tag count nowhere,
 * RegionStateManager.cs:179-189), support[n][4][6] the same split by base in the order A C G T (an SNV's SupportByAmplicon is the row of
 * its alternate base).  Slots are in ASCENDING ID order with -1 / 0 in the unused ones: the reference's first-arrival order is not
 * reproduced, and no decision depends on it.  PISCES_E_STATE on a handle that does not track; more than six ids at a position of the range:
 * PISCES_E_INVALID_ARG as in a flush. */
int32_t pisces_hip_get_amplicon_counts(PiscesHip* h, int32_t start_position, int32_t n, int32_t* ids, int32_t* coverage, int32_t* support);

/* ---- VCF body lines (pure CPU) ---------------------------------------
 * What the writer needs of VcfWriterConfig (src/lib/Pisces.IO/VcfFileWriter.cs:264-330). */
typedef struct PiscesVcfConfig {
    int32_t variant_quality_filter;             /* VariantQualityFilterThreshold (names the q<N> filter); -1 = null */
    int32_t rmxn_max_repeat_length;             /* RMxNFilterMaxLengthRepeat, names R<M>x<N>; -1 = null */
    int32_t rmxn_min_repetitions;               /* RMxNFilterMinRepetitions */
    int32_t noise_level;                        /* EstimatedBaseCallQuality = NoiseLevelUsedForQScoring (the NL field) */
    int32_t output_strand_bias_and_noise_level; /* ShouldOutputStrandBiasAndNoiseLevel */
    int32_t output_no_call_fraction;            /* ShouldOutputNoCallFraction (-reportnocalls) */
    float   min_frequency_threshold;            /* MinFrequencyThreshold: sets the number of VF decimals */
    float   frequency_filter_threshold;         /* FrequencyFilterThreshold; < 0 = null */
    int32_t crush;                              /* !AllowMultipleVcfLinesPerLoci (-crushvcf): co-located alleles share one line */
    int32_t noise_level_from_records;           /* 1: the NL column is the record's noise_level (CalledAllele.NoiseLevelApplied: records made by
                                                   this library, exact with NoiseModel.Window too); 0: noise_level above for every allele
                                                   with support (records assembled elsewhere) */
    int32_t indel_repeat_filter;                /* IndelRepeatFilterThreshold (VcfFileWriter.cs:303), names the R<n> filter of PISCES_FILTER_INDEL_REPEAT_LENGTH;
                                                   <= 0 = null: a row's bit then prints nothing (the reference's MapFilter throws, VcfFormatter.cs:163-166) */
} PiscesVcfConfig;
int32_t pisces_hip_vcf_default_config(PiscesVcfConfig* cfg);
/* One VCF body line per record, or with cfg->crush one per position (VcfFileWriter.WriteListOfColocatedAlleles, VcfFileWriter.cs:206-262
 * with VcfFormatter.cs:52-495): CHROM POS . REF ALT QUAL FILTER DP=<n> GT:GQ:AD:DP:VF[:NL:SB][:NC] <sample>.  cand_index / cands /
 * alleles are what pisces_hip_flush_ex returned (may be NULL when no row is an insertion / deletion / MNV).  Returns the number of
 * bytes of text; when that exceeds `capacity` nothing is written and the call is repeated with a larger buffer; < 0 = error. */
int64_t pisces_hip_format_vcf(const PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* recs, int64_t n,
                              const int32_t* cand_index, const PiscesCandidate* cands, const uint8_t* alleles, char* out,
                              int64_t capacity);
/* The same with RegionMapper's padding (src/lib/Pisces.IO/RegionMapper.cs:31-84, VcfFileWriter.PadIfNeeded / WriteRemaining :124-172):
 * positions of the interval set that no allele covers get a no-call row (./., LowDP, DP=0, NL = cfg->noise_level) before the next
 * written position, and with `finish` up to the end of the last interval.  `state` carries the writer's and the mapper's cursors from
 * one call to the next (zero-initialise, then {0, 0, -1}: see PiscesVcfPadState); it is only advanced when the text fitted. */
typedef struct PiscesVcfPadState {
    int32_t last_variant_position_written;   /* VcfFileWriter._lastVariantPositionWritten, starts at 0 */
    int32_t last_padded_position;            /* RegionMapper._lastPaddedPosition, starts at 0 */
    int32_t last_cleared_interval_index;     /* RegionMapper._lastClearedIntervalIndex, starts at -1 */
} PiscesVcfPadState;
int64_t pisces_hip_format_vcf_padded(const PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* recs, int64_t n,
                                     const int32_t* cand_index, const PiscesCandidate* cands, const uint8_t* alleles,
                                     const uint8_t* ref_bases, int64_t ref_len, const int32_t* interval_starts,
                                     const int32_t* interval_ends, int32_t n_intervals, PiscesVcfPadState* state, int32_t finish,
                                     char* out, int64_t capacity);
/* The padding of such a call without its text, for a caller that sizes buffers or splits a chromosome's rows into calls: the no-call
 * rows and the lines (rows written, one per position with `crush`, plus the no-call rows) pisces_hip_format_vcf_padded would write for
 * `recs` from *state_in, and the state it would leave (each output may be NULL).  Closed form over the interval table — a binary search
 * and a prefix sum per written line, no walk over the positions of a gap — so it asks for what the closed form
 * needs: intervals positive, sorted and disjoint (PISCES_E_INVALID_ARG otherwise), rows at positions >= 1 that do not descend, the
 * first not below state_in->last_variant_position_written, and a state that zero-initialisation or the formatter produced: no negative
 * word, no index below -1, no last_padded_position ahead of last_variant_position_written while intervals are uncleared
 * (PISCES_E_UNSUPPORTED otherwise: the formatter itself still takes such input).  A finished state, (0, L, n - 1), pads nothing more. */
int32_t pisces_hip_vcf_pad_plan(const PiscesCalledAllele* recs, int64_t n, int32_t crush, const int32_t* interval_starts,
                                const int32_t* interval_ends, int32_t n_intervals, const PiscesVcfPadState* state_in, int32_t finish,
                                int64_t* pad_rows, int64_t* lines, PiscesVcfPadState* state_out);
/* The two entries above with CalledAllele.GenotypePosteriors: gp[i] belongs to recs[i] (NULL: exactly the bytes of the entries above).
 * A line whose first allele has gp.n > 0 gets ":GP" behind its FORMAT keys and the values, each "0.00", comma-joined, behind its sample
 * (VcfFormatter.cs:263-269; ShouldReportGp is on with DiploidByAdaptiveGT); RegionMapper's no-call rows have none. */
int64_t pisces_hip_format_vcf_ex(const PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* recs, int64_t n,
                                 const int32_t* cand_index, const PiscesCandidate* cands, const uint8_t* alleles, char* out,
                                 int64_t capacity, const PiscesGenotypePosteriors* gp);
int64_t pisces_hip_format_vcf_padded_ex(const PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* recs, int64_t n,
                                        const int32_t* cand_index, const PiscesCandidate* cands, const uint8_t* alleles,
                                        const uint8_t* ref_bases, int64_t ref_len, const int32_t* interval_starts,
                                        const int32_t* interval_ends, int32_t n_intervals, PiscesVcfPadState* state, int32_t finish,
                                        char* out, int64_t capacity, const PiscesGenotypePosteriors* gp);

/* ---- BGZF inflate on the device (the stage upstream of the read batch) ------------------------------------
 * A BAM file is a chain of BGZF blocks, gzip members of <= 64 KiB whose 'BC' extra subfield holds the block size; each is an
 * independent DEFLATE stream.  Replaces BamReader.ReadBlock's per-block call into the native zlib binding
 * (src/lib/Alignment.IO/BamReader.cs:603-645 -> SafeNativeMethods.UncompressBlock, src/lib/Common.IO/FileCompression.cs:14-16):
 * the host walks the block headers (pisces_hip_bgzf_scan), the device inflates every block of the table at once, one wave per block. */
typedef struct PiscesBgzfBlock {
    int64_t  in_offset;    /* first byte of the DEFLATE payload in the file bytes */
    int64_t  out_offset;   /* where the block's bytes go in the inflated stream (running sum of ISIZE) */
    int32_t  in_length;    /* payload bytes (block size - header - 8 trailer bytes) */
    int32_t  out_length;   /* ISIZE */
    uint32_t crc32;        /* CRC-32 of the inflated bytes, from the trailer */
    int32_t  reserved;
} PiscesBgzfBlock;
/* Host: the block table of file[0, n_bytes).  Returns the number of blocks (the empty end-of-file block included); fills at most
 * `capacity` of them; *inflated_bytes = sum of ISIZE.  PISCES_E_INVALID_ARG: not a BGZF block chain (bad magic, no BC subfield, a
 * block running past the end - what BamReader.ReadBlock throws InvalidDataException for). */
int64_t pisces_hip_bgzf_scan(const uint8_t* file, int64_t n_bytes, PiscesBgzfBlock* blocks, int64_t capacity, int64_t* inflated_bytes);
/* Device: inflates blocks[0, n_blocks) of the file bytes into out (host memory, out_capacity >= the blocks' last out_offset +
 * out_length).  check_crc: the trailer CRC-32s are verified on the host afterwards.  PISCES_E_INVALID_ARG with the index of the first
 * bad block in the message when a stream is corrupt (UncompressBlock < 0 -> ReadBlock returns -1).  kernel_ms (optional): the inflate
 * kernel's own duration. */
int32_t pisces_hip_bgzf_inflate(PiscesHip* h, const uint8_t* file, int64_t n_bytes, const PiscesBgzfBlock* blocks, int64_t n_blocks,
                                uint8_t* out, int64_t out_capacity, int32_t check_crc, float* kernel_ms);

/* ---- BAM records cut on the device (the rest of row f4): the compressed file is the only thing that crosses PCIe --------------------
 * pisces_hip_bam_decode: the BGZF blocks of `file` are inflated into HBM (as above, without the copy back), the BAM record chain is cut
 * there (no serial pass: every byte offset of the first 4 KiB of a 32 KiB chunk is tried as a record start and its chain followed
 * to where it leaves the chunk), AlignmentSource.ShouldSkipRead (src/exe/Pisces/Logic/Alignment/AlignmentsSource.cs:84-92: unmapped, secondary,
 * optionally improper pairs and duplicates, MAPQ below the minimum, no CIGAR) drops what the reference drops, and the alignments of
 * reference sequence `ref_id` are decoded into the PiscesReadBatch arrays in device memory, in file order — what BamReader.GetNextAlignment
 * (src/lib/Alignment.IO/BamReader.cs:137) + Read's constructor do per record on the host.  counts = {reads kept, reads of the chromosome
 * skipped, CIGAR operations, bases}.  Records longer than 32 KiB (long reads) are reported as a broken chain.
 * Where the record chain enters each chunk is first taken, for all chunks at once, from the one exit that the live chains of the chunk
 * before share, and every link checked; a file where that fails somewhere (records of several KiB, ...) gets the serial hop chunk to
 * chunk instead.  pisces_hip_bam_chain_mode says which it was for the last decode (0 = all at once, 1 = serial hop): diagnostics
 * (the environment variable PISCES_HIP_BAM_SERIAL_CHAIN=1 forces the serial hop).
 * pisces_hip_bam_fetch: the decoded batch to host arrays sized from `counts` (any pointer may be NULL) — for inspection and tests.
 * pisces_hip_add_decoded_reads: pisces_hip_add_reads for the decoded batch without anything of it leaving the device: what
 * pisces_hip_add_reads takes from a host pass over the CIGARs (log slots, candidate-record slots, the blocks every read touches, the
 * reads it refuses: position <= 0, a CIGAR longer than the read, a read past 2^31 - 1 or far past the end of its reference sequence)
 * the decode has made where the reads are (the blocks as a bit map that came back with `counts`); the call enqueues the read walk and
 * the candidate discovery and returns without waiting.  On a handle that tracks amplicon counts the batch must carry amplicon ids (below:
 * decoded after pisces_hip_set_amplicon_bias_filter), PISCES_E_UNSUPPORTED otherwise; the ids join the read store with the reads. */
int32_t pisces_hip_bam_decode(PiscesHip* h, const uint8_t* file, int64_t n_bytes, const PiscesBgzfBlock* blocks, int64_t n_blocks, int32_t ref_id,
                              int32_t min_map_quality, int32_t skip_duplicates, int32_t only_proper_pairs, int64_t counts[4]);
int32_t pisces_hip_bam_fetch(PiscesHip* h, int32_t* position, uint8_t* flags, int32_t* cigar_offset, uint8_t* cigar_op, uint32_t* cigar_len,
                             int32_t* seq_offset, uint8_t* bases, uint8_t* quals);
int32_t pisces_hip_add_decoded_reads(PiscesHip* h);
int32_t pisces_hip_bam_chain_mode(PiscesHip* h);
/* Stitched reads (the Stitcher's XD tag, one DirectionType per base of the expanded CIGAR; Read.CigarDirections / SequencedBaseDirectionMap,
 * src/lib/Pisces.Domain/Models/Read.cs:340-400, 664-682): when a record of the decoded chromosome carries the tag, the decode makes
 * PiscesReadBatch.directions (per base; reads without the tag: their strand's direction) and .deletion_directions (two per CIGAR
 * operation) for the batch, and pisces_hip_add_decoded_reads counts and discovers candidates with them.  This entry copies them to the
 * host (either pointer may be NULL): returns 1 when the batch has them, 0 when no read of it was stitched, < 0 on error.  A malformed tag
 * (CigarDirection's "Unexpected format in direction string") makes pisces_hip_add_decoded_reads refuse the batch. */
int32_t pisces_hip_bam_fetch_directions(PiscesHip* h, uint8_t* directions, uint8_t* deletion_directions);
/* Amplicon names (Read.GetAmpliconNameIfExists: the XN tag, Read.cs:483-486; TagUtils.GetStringTag, BamCommon.cs:1182-1216).  On a handle
 * that tracks amplicon counts (pisces_hip_set_amplicon_bias_filter) pisces_hip_bam_decode also reads the XN tag of every kept record where
 * the records are: the FIRST field with the key XN decides; its type byte is upper-cased; Z / H give the bytes up to the NUL, A / C (so
 * also a / c) a one-byte name; no such field = no amplicon (-1: the read counts under none); an empty string is a name like any other;
 * names are equal when their bytes are.  An XN field of another type (GetStringTag throws InvalidDataException) lets the decode succeed
 * and makes pisces_hip_add_decoded_reads refuse the batch with PISCES_E_INVALID_ARG, naming the lowest such read.  Deviation: B arrays in
 * front of the tag are skipped as the SAM specification says; the reference's walk throws on them.
 * The distinct names of the batch are interned on the device; only they come to the host, where the handle keeps a dictionary name <-> id:
 * a name the handle knows keeps its id, new names get the next ids (from 0) in the order of the first kept read that carries each, decodes
 * in call order — the same files in the same order give the same ids on every run.  A decode that is never added still leaves its names in
 * the dictionary (harmless: ids only number names).  A handle that does not track reads no tag, launches nothing for it and has no ids.
 * pisces_hip_bam_fetch_amplicons: the decoded batch's ids (amplicon_id[reads kept]) to the host; returns 1 when the batch has ids, 0 when
 * it has none, PISCES_E_STATE without a batch or once it has moved into the store (the rules of pisces_hip_bam_fetch_directions).
 * pisces_hip_amplicon_name_count / pisces_hip_get_amplicon_name: the dictionary; the name's length is returned and its bytes (no
 * terminator) written only when capacity holds them all; PISCES_E_INVALID_ARG for an id the dictionary does not have.
 * pisces_hip_intern_amplicon_name: the id of name[0, length) in the same dictionary, a new one when it is new — for a host that parses
 * some reads itself and feeds pisces_hip_add_reads_amplicons beside the decode; PISCES_E_STATE on a handle that does not track.
 * Ids a caller invents and ids of the dictionary must not be mixed on one handle: both count from small numbers, and an invented id that
 * equals a dictionary id is the same amplicon to every count. */
int32_t pisces_hip_bam_fetch_amplicons(PiscesHip* h, int32_t* amplicon_id);
int32_t pisces_hip_amplicon_name_count(PiscesHip* h);
int32_t pisces_hip_get_amplicon_name(PiscesHip* h, int32_t id, char* out, int32_t capacity);
int32_t pisces_hip_intern_amplicon_name(PiscesHip* h, const char* name, int32_t length);

/* ---- CoverageMethod.Exact (PiscesApplicationOptions.CoverageMethod, -coveragemethod exact) on the streaming surface ----
 * pisces_hip_exact_span_direction: ExactCoverageCalculator's decision for ONE read's coverage summary and ONE span, host only, no handle
 * (ExactCoverageCalculator.cs:62-96 with GetIndexBoundaries and GetDirection).  cs / ce: the summary's clip-adjusted start and end; the
 * CIGAR as operation characters and lengths; the directions as runs (DirectionInfo: dir_run_type[i] a PISCES_DIR_* value).  preceding /
 * trailing: the allele's span (deletion at p of length L: p, p + L + 1; MNV: p - 1, p + L; insertion: p, p + 1); is_insertion is taken
 * and, as in the reference, never read.  Returns the direction the read counts in (0 / 1 / 2), -1 when it does not span the allele, -2
 * where the reference throws InvalidDataException (a read of several direction runs with no base at or before `preceding` and none at
 * or behind `trailing`), -3 for arguments the reference would index out of bounds with (several runs longer than the CIGAR's read
 * span, a direction above 2, null arrays); runs that fall short leave the rest of the read Forward, as a new direction map does.  The summary is taken as given: it need not be one a read can leave behind.
 * csrc/exact_span.h, written for host and device: exact_span_kernel compiles the same source. */
int32_t pisces_hip_exact_span_direction(int32_t cs, int32_t ce, const uint8_t* cigar_op, const uint32_t* cigar_len, int32_t n_cigar,
                                        const uint8_t* dir_run_type, const uint32_t* dir_run_len, int32_t n_runs, int32_t preceding,
                                        int32_t trailing, int32_t is_insertion);
/* pisces_hip_set_coverage_method: PISCES_COVERAGE_EXACT makes the handle an EXACT one.  Every read that joins the read store then leaves
 * a summary next to its descriptor (clip-adjusted ends, first / last operation an insertion, one direction or several), touches the block
 * of its clip-adjusted END as well (RegionStateManager.AddAlleleCounts stores the summary through GetBlock, :212-219: a trailing soft clip
 * that reaches into the next block makes that block exist, and it is flushed like any other), and the coverage of every insertion,
 * deletion and MNV row of a flush is the number of reads that span the allele, by direction, counted on the device (exact_span_kernel):
 * EstimatedCoverageByDirection holds the three counts as they are (no stitched redistribution: coverage_by_dir[2] is filled),
 * TotalCoverage their sum, ReferenceSupport max(0, TotalCoverage - AlleleSupport); q-score, strand bias, genotype, filters and the
 * collapser's frequencies follow.  SNV and Reference rows are what an Approximate handle gives.  A read is seen by a span while the
 * block of its clip-adjusted end is held and that end lies at or below trailing + 2 * (length of the first read the handle was given)
 * (GetSpanningReadSummaries, :234-254).  A flush that meets the reference's InvalidDataException (-2 above) returns PISCES_E_INVALID_ARG
 * naming the allele's position; the blocks stay held.  Before the first read is added (PISCES_E_STATE afterwards); an unknown value:
 * PISCES_E_INVALID_ARG.  PISCES_E_UNSUPPORTED, each with a message, for what Exact cannot go together with — here when the handle has it
 * already, at the other entry when it comes later: NoiseModel.Window (the Exact calculator's own base-quality sum is not carried),
 * forced alleles, pisces_hip_set_owned_range (a shard's halo is cut by aligned span, not by clip-adjusted span), PISCES_HIP_READ_PATH=log
 * and pisces_hip_add_observations (observation tuples have no reads), and the tile surface pisces_hip_call_tiles* (tuples have no reads).
 * An exact handle waits for the device where an Approximate one does not: every add of reads ends with one small transfer and a wait (the
 * word that says whether a read's clip-adjusted end made a block), so adds do not return ahead of their kernels; and a flush whose batch
 * holds an insertion, deletion or MNV candidate (never one pisces_hip_flush_begin leaves to the device alone) waits once more per
 * candidate pass — once ahead of the collapse, once ahead of each call_spanning_kernel pass — for the counts and their error word.
 * pisces_hip_get_spanning_read_counts waits for its launch.  What it costs on one mix: DESIGN section 7.
 * pisces_hip_get_spanning_read_counts: what a host needs of IAlleleSource.GetSpanningReadSummaries — out[3] = the reads that span
 * [preceding, trailing] by direction, from the reads the store holds now.  PISCES_E_STATE on a handle that is not exact. */
enum { PISCES_COVERAGE_APPROXIMATE = 0, PISCES_COVERAGE_EXACT = 1 };
int32_t pisces_hip_set_coverage_method(PiscesHip* h, int32_t method);
int32_t pisces_hip_get_spanning_read_counts(PiscesHip* h, int32_t preceding, int32_t trailing, int32_t is_insertion, int32_t* out);

/* ---- the indel repeat-length filter (VariantCallingParameters.IndelRepeatFilter, -RepeatFilter_ToBeRetired, FILTER R<n>) ----
 * pisces_hip_indel_repeat_length: AlleleProcessor.ComputeIndelRepeatLength (src/exe/Pisces/Logic/VariantCalling/AlleleProcessor.cs:80-213) for ONE
 * allele, host only, no handle.  ref_bases[i] is position i + 1 of the chromosome (upper-cased as it is read, :100-103); the alleles as
 * PiscesCandidate carries them, anchor base first.  The variant bases (an insertion's ALT[1:], a deletion's REF[1:]) are reduced to their
 * shortest generating unit and counted in the stretch of the reference from 50 bases upstream of position - 1 to 49 behind it, with the
 * reference's quirks: 1 when the stretch ends within unit + 1 bases of the scan's start (an allele anchored on the last or second-to-last
 * base), at most 48 single-base repeats to the right.  0 for SNV, MNV and Reference alleles and for an empty reference.  Any position the
 * reference accepts is accepted, 0 and L + 1 included; where its Substring throws (position < -49 or position > L + 1, insertion, deletion
 * or SNV) PISCES_E_INVALID_ARG, as for a null array or an insertion / deletion without its anchor base.  csrc/indel_repeat.h, written for
 * host and device: indel_repeat_kernel compiles the same source. */
int32_t pisces_hip_indel_repeat_length(int32_t category, int32_t position, const uint8_t* ref_allele, int32_t ref_len, const uint8_t* alt_allele,
                                       int32_t alt_len, const uint8_t* ref_bases, int64_t ref_length);
/* pisces_hip_set_indel_repeat_filter: threshold > 0 makes every flush (pisces_hip_flush, _ex, _view, _begin / _end*) OR
 * 1 << PISCES_FILTER_INDEL_REPEAT_LENGTH into the filter_bits of every insertion and deletion row with threshold <= repeat length
 * (AlleleProcessor.ApplyFilters, AlleleProcessor.cs:52-57) — forced-report rows included, nothing else of a row changes, rows of other
 * categories cannot get it (their length is 0).  One small launch behind the candidate kernel, on the device, before the rows leave it.
 * 0 = off, the default: a handle that is off launches nothing for it.  A negative value: PISCES_E_INVALID_ARG, the state unchanged.
 * Any time; it holds from the next flush that makes a batch (a batch waiting for a larger buffer keeps its rows).  The tuple surface
 * (pisces_hip_call_tiles*) has no insertions or deletions and is untouched.  Give PiscesVcfConfig.indel_repeat_filter the same value. */
int32_t pisces_hip_set_indel_repeat_filter(PiscesHip* h, int32_t threshold);

/* ---- VariantQualityRecalibration (VQR, src/exe/VariantQualityRecalibration/) over called-allele rows ----
 * The stage a Pisces user runs behind the caller on FFPE and amplicon samples, on the rows where they lie instead of on the VCF read back
 * from disk: count the 12 SNV mutation categories over all rows (SignatureSorter.StrainVcf, SignatureSorter.cs:39-90), turn the
 * over-represented ones into noise levels (QualityRecalibration.GetRecalibrationTables, QualityRecalibration.cs:58-129), re-score those SNVs
 * with VariantQualityCalculator.AssignPoissonQScore (UpdateAllele, :131-155) — and, with do_amplicon_position_checks, the same for the
 * rows next to an amplicon edge (EdgeIssueCountData.cs).  Three calls, between pisces_hip_compact_records (or a flush) and the VCF writer:
 *   pisces_hip_vqr_count_device   once per chromosome, adding into one pair of counters
 *   pisces_hip_vqr_tables         once, on the host, from the counters
 *   pisces_hip_vqr_apply_device   once per chromosome
 * A row is its record alone: total_coverage is the VCF's DP, allele_support AD[1], variant_qscore QUAL; rows are uncrushed, one allele
 * each.  A call sees the rows of ONE chromosome: the reference's "did we switch chromosome" edge (EdgeIssueCountData.cs:95) is the
 * buffer's end here.  Not part of the library: the .counts / .edgecounts / .edgevariants files, the VQR header lines and VQRVcfWriter's
 * re-sorting, crushed and multi-allelic diploid lines.  csrc/vqr.h, written for host and device; the kernels are csrc/vqr_kernels.hip.h. */
/* VQROptions (src/exe/VariantQualityRecalibration/VQROptions.cs) as far as the three passes read them */
typedef struct PiscesVqrOptions {
    int32_t do_basic_checks;               /* DoBasicChecks, 1 */
    int32_t do_amplicon_position_checks;   /* DoAmpliconPositionChecks, 0 */
    int32_t extent_of_edge_region;         /* ExtentofEdgeRegion, 4: rows looked at before and behind a row; 0..64 */
    int32_t loci_count;                    /* LociCount, -1; above 0 it replaces both NumPossibleVariants (SignatureSorter.cs:78-82) */
    int32_t base_q_noise;                  /* BamFilterParams.MinimumBaseCallQuality, 20: baselineQNoise */
    int32_t filter_qscore;                 /* VariantCallingParams.MinimumVariantQScoreFilter, 30: sets PISCES_FILTER_LOW_VARIANT_QSCORE */
    int32_t max_qscore;                    /* MaxQScore, 100 */
    int32_t reserved;
    double  z_factor;                      /* ZFactor, 2: threshold = mean + z * sigma */
    double  alignment_warning_threshold;   /* AlignmentWarningThreshold, 10: the host's own warning on general_edge_risk_increase */
} PiscesVqrOptions;
/* One CountData (CountData.cs): by_category[MutationCategory - 1] (MutationCategory.cs:12-30: AtoC AtoG AtoT CtoA CtoG CtoT GtoA GtoC GtoT
 * TtoA TtoC TtoG Insertion Deletion Reference Other; Reference stays 0) and NumPossibleVariants.  Every entry takes two: [0] over all
 * rows, [1] over the rows at an edge (EdgeIssueCountData). */
typedef struct PiscesVqrCounts {
    int64_t by_category[16];
    int64_t num_possible_variants;
} PiscesVqrCounts;
/* QualityRecalibrationData (QualityRecalibration.cs:14-21): phred-scaled rates by SNV category; bit c of a mask = the table holds
 * category c (Dictionary.ContainsKey).  edge_risk holds all 12 when has_edge_risk; -2147483648 = int.MinValue, the C# cast of a rate
 * that is NaN or infinite (no mutation at an edge: 0 / 0). */
typedef struct PiscesVqrTables {
    int32_t  basic[12], edge[12], edge_risk[12];
    uint32_t basic_mask, edge_mask;
    int32_t  has_edge_risk;
    int32_t  reserved;
    double   general_edge_risk_increase;   /* GeneralEdgeRiskIncrease (:281), may be NaN or infinite */
} PiscesVqrTables;
int32_t pisces_hip_vqr_default_options(PiscesVqrOptions* opts);
/* The counting pass over device-resident rows: rows [lo, hi) of d_recs[0, min(n, *d_count)) (d_count NULL: n) are counted into
 * d_counts[2] (device memory, ADDED to: zero it once, the calls of several chromosomes sum), by MutationCategoryUtil.GetMutationCategory
 * (MutationCategory.cs:41-81: the alleles alone, a ForcedReport row counts like any other; every row, Reference rows included, is a
 * possible variant).  With do_amplicon_position_checks a row at an edge also counts in d_counts[1], and d_suspect[i] (n bytes) becomes 1
 * for a row at an edge that is not Reference, 0 for every other counted row.  A row is at an edge (DidWeDetectAnEdge,
 * EdgeIssueCountData.cs:67-118) when it has coverage and, among the extent_of_edge_region rows before and behind it in ROW order, one is
 * missing, has less than half its coverage, or lies further away in position than in rows (rows of one position are legal).  The
 * neighbours are read from the whole buffer, not from [lo, hi) alone: a caller that streams a chromosome in pieces brings
 * extent_of_edge_region halo rows on either side of a piece.  Asynchronous on `stream` (NULL: the handle's own).  The totals are integer
 * sums: identical from run to run.  PISCES_E_INVALID_ARG, each with a message: null h / opts / d_counts (d_recs with n > 0),
 * extent_of_edge_region outside 0..64, lo / hi outside 0 <= lo <= hi <= n, do_amplicon_position_checks without d_suspect. */
int32_t pisces_hip_vqr_count_device(PiscesHip* h, const PiscesVqrOptions* opts, const PiscesCalledAllele* d_recs, int64_t n, const int32_t* d_count,
                                    int64_t lo, int64_t hi, PiscesVqrCounts* d_counts, uint8_t* d_suspect, void* stream);
/* The same over host rows recs[0, n), no handle and no device: counts[2] is added to.  The message of a refusal is
 * pisces_hip_last_error(NULL)'s, as for every entry without a handle. */
int32_t pisces_hip_vqr_count(const PiscesVqrOptions* opts, const PiscesCalledAllele* recs, int64_t n, int64_t lo, int64_t hi, PiscesVqrCounts* counts,
                             uint8_t* suspect);
/* GetPhredScaledCalibratedRates and GetPhredScaledCalibratedRatesForEdges (QualityRecalibration.cs:276-381) from counts[2]; host only.
 * basic with do_basic_checks, edge with do_amplicon_position_checks, edge_risk with both.  A category is in a table when its count is
 * strictly above mean + z_factor * sigma of the 12 sorted SNV counts without the two lowest and the two highest; its rate is
 * (int)PtoQ(count / NumPossibleVariants + QtoP(base_q_noise)).  The reference's quirks are kept: the first function removes Insertion /
 * Deletion / Other / Reference from the counts it is handed, so every total the edge-risk table reads is over the 12. */
int32_t pisces_hip_vqr_tables(const PiscesVqrOptions* opts, const PiscesVqrCounts* counts, PiscesVqrTables* tables);
/* The update pass over device-resident rows d_recs[0, min(n, *d_count)), in place (UpdateAllele, QualityRecalibration.cs:131-155): a row
 * whose category (MutationCounter.GetMutationCategory, MutationCounter.cs:133-172: a ForcedReport row has none) is in `basic` gets
 * AssignPoissonQScore(allele_support, total_coverage, rate, min(variant_qscore, max_qscore)); one whose category is in `edge` and at whose
 * position some row is a suspect (d_suspect, from the counting pass over the same rows) then gets the edge_risk rate with depth and support
 * subsampled to 1 / QtoP(rate).  An update writes variant_qscore, genotype_qscore (the same value) and noise_level (the rate), and sets
 * PISCES_FILTER_LOW_VARIANT_QSCORE when the new score is below filter_qscore; no bit is ever cleared, a row with variant_qscore < 1 is left
 * alone, and so is every byte of every other row.  *d_n_changed (optional, device memory, ADDED to): the rows rewritten.  The tables
 * travel in the kernel arguments; with no category in a table nothing is launched.  Asynchronous on `stream`.  PISCES_E_INVALID_ARG:
 * null h / opts / tables, an edge table with do_amplicon_position_checks but without d_suspect or without has_edge_risk. */
int32_t pisces_hip_vqr_apply_device(PiscesHip* h, const PiscesVqrOptions* opts, const PiscesVqrTables* tables, PiscesCalledAllele* d_recs, int64_t n,
                                    const int32_t* d_count, const uint8_t* d_suspect, int64_t* d_n_changed, void* stream);

/* ---- VennVcf (src/exe/VennVcf/): the consensus of two probe pools ------------------------------------------------------------------------
 * The two pools' rows of ONE chromosome, each sorted by position, become one consensus call set with the probe-pool-bias filter
 * (PISCES_FILTER_POOL_BIAS, the VCF's PB): rows of a position are paired (SelectPairs), a pair is one of four cases (GetComparisonCase) and
 * becomes one row (ConsensusBuilder.CombineVariants); several HomozygousRef calls of a position merge into the first.  The reference's
 * quirks are kept (csrc/venn.h).  The output has the shape of a flush, so pisces_hip_format_vcf*, pisces_hip_vqr_* and
 * every other entry over rows take it unchanged.  Where the reference defines nothing a consensus row holds the sums (coverage_by_dir,
 * support_by_dir, num_no_calls) or the ORs (filter_bits, the three bias bits) of its components; strand_bias_score is the larger one, copied.
 * Not part of the library: reading VCFs, file names, header lines, chromosome order across calls, the PB / VF0..DP1 columns, crushed lines. */
typedef struct PiscesVennOptions {
    float   min_frequency;          /* VariantCallingParams.MinimumFrequency, 0.01f */
    float   min_frequency_filter;   /* VariantCallingParams.MinimumFrequencyFilter, 0.01f (unset, the reference raises it to MinimumFrequency) */
    float   pool_bias_threshold;    /* SampleAggregationParameters.ProbePoolBiasThreshold, 0.5f */
    int32_t min_coverage;           /* VariantCallingParams.MinimumCoverage, 10 */
    int32_t max_variant_qscore;     /* VariantCallingParams.MaximumVariantQScore, 100 */
    int32_t combine_qscore_method;  /* HowToCombineQScore: 0 = CombinePoolsAndReCalculate, 1 = TakeMin */
    int32_t reserved[2];
} PiscesVennOptions;
/* What AggregateAllele adds to CalledAllele, one per consensus row (32 bytes); row_a / row_b feed the debug columns VF0/VF1/AD0/AD1/DP0/DP1 */
typedef struct PiscesConsensusInfo {
    int32_t row_a, row_b;           /* the pair's rows in pool A and pool B, -1 = absent; the FIRST pair's for a merged reference */
    int32_t comparison_case;        /* VariantComparisonCase: 0 AgreedOnReference, 1 AgreedOnAlternate, 2 OneReferenceOneAlternate, 3 CanNotCombine */
    int32_t alt_changed_to_ref;     /* PushThroughRamificationsOfGTChange cut the alleles down to "ref ." */
    double  pool_bias_score;        /* PoolBiasResults.BiasScore, at most 1; 0 after a reference merge (the reference makes a new BiasResults) */
    double  pool_bias_gatk;         /* PoolBiasResults.GATKBiasScore in [-100, 0]: the PB column; the maximum over a merged reference */
} PiscesConsensusInfo;
/* One pool's rows as a flush gives them out; every pointer in host memory for pisces_hip_venn_consensus, device-accessible for
 * pisces_hip_venn_consensus_device (recs 16-byte aligned there). */
typedef struct PiscesVennRows {
    const PiscesCalledAllele* recs;
    int64_t n;
    const int32_t* count;           /* optional: min(n, *count) rows are there (pisces_hip_compact_records' word) */
    const int32_t* cand_index;      /* optional; with it, cands and alleles */
    const PiscesCandidate* cands;
    const uint8_t* alleles;
} PiscesVennRows;
typedef struct PiscesVennOut {
    PiscesCalledAllele* recs;       /* row_capacity rows */
    int32_t* cand_index;            /* row_capacity entries, -1 = the alleles are the base codes of info */
    PiscesCandidate* cands;         /* cand_capacity */
    uint8_t* alleles;               /* allele_capacity bytes; a candidate's allele_offset points into them */
    PiscesConsensusInfo* info;      /* optional, row_capacity */
    uint8_t* venn_a;                /* optional, one byte per row of pool A: 0 in no set, 1 "and" (AgreedOnAlternate), 2 "not" (the non-reference */
    uint8_t* venn_b;                /*   member of a OneReferenceOneAlternate or CanNotCombine pair): the four files of WriteVarsToVennFiles */
    int64_t* n_out;                 /* [3]: rows, candidates, allele bytes of the consensus.  On the device n_out doubles as the d_count word of the
                                       entries that follow (they read its low 32 bits, little-endian; an error word reads as no rows) */
    int64_t row_capacity, cand_capacity, allele_capacity;
} PiscesVennOut;
int32_t pisces_hip_venn_default_options(PiscesVennOptions* opts);
/* The consensus of device-resident rows.  Asynchronous on `stream` (NULL: the handle's own) and ordered behind whatever made the rows, no
 * host wait inside.  out->n_out (device-accessible) receives the three counts.  When one of them is above its capacity nothing else is
 * written: repeat with larger buffers (the protocol of pisces_hip_format_vcf_device's d_text_bytes).  A pool that is not sorted by position
 * (the reference's "Vcf needs to be ordered") leaves n_out = {PISCES_E_INVALID_ARG, the pool (0 / 1), its lowest offending row} and writes
 * nothing else.  Every call overwrites: nothing is added to what the buffers held.  The output is in position order, a position's rows in
 * the reference's pair order, identical from run to run (no atomics take part in the ordering).  Calls of one handle share the handle's
 * scratch (24 bytes an input row) and must be stream-ordered with respect to each other, as pisces_hip_format_vcf_device's; a call that
 * has to grow the scratch waits first.  PISCES_E_INVALID_ARG, each with a message: null h / opts / a / b / out / out->n_out, null recs
 * with n > 0, null output arrays with a capacity > 0, negative sizes or capacities, a cand_index without cands or alleles, thresholds
 * outside [0, 1], an unknown combine_qscore_method, rows that are not 16-byte aligned. */
int32_t pisces_hip_venn_consensus_device(PiscesHip* h, const PiscesVennOptions* opts, const PiscesVennRows* a, const PiscesVennRows* b,
                                         const PiscesVennOut* out, void* stream);
/* The same over host arrays: no handle and no device, the function the device runs.  PISCES_E_BUFFER_TOO_SMALL with the three counts in
 * n_out and nothing else written when a capacity is too small; PISCES_E_INVALID_ARG for an unsorted pool, n_out as above. */
int32_t pisces_hip_venn_consensus(const PiscesVennOptions* opts, const PiscesVennRows* a, const PiscesVennRows* b, const PiscesVennOut* out);
/* One pair (CombineVariants), host only: a or b may be NULL, `comparison_case` < 0 asks GetComparisonCase.  The alleles are the base codes of
 * info.  vq_ab (optional, [2]): VariantA / VariantB .VariantQscore as the call leaves them (PushThroughRamificationsOfGTChange rewrites them). */
int32_t pisces_hip_venn_combine(const PiscesVennOptions* opts, const PiscesCalledAllele* a, const PiscesCalledAllele* b, int32_t comparison_case,
                                PiscesCalledAllele* row_out, PiscesConsensusInfo* info_out, int32_t* vq_ab);

/* ---- Scylla's read pass (src/lib/VariantPhasing): vead groups per neighbourhood from resident reads ----------------------------------
 * For every neighbourhood of nearby variant sites Scylla asks each read, site by site, whether it carries the variant, the reference,
 * something else or nothing usable (a "vead", VeadFinder.FindVariantResults) and collapses identical answers into counted groups
 * (VeadGroupSource.GetVeadGroups).  csrc/vead.h restates the decision for host and device; the reference's quirks are kept (N, =, X, H
 * and P operations advance nothing in the walk; a "gone past" result is overwritten by the tail below the loop).
 * A site's state is one byte.  A site whose own alleles are one equal base (A>A) prints the same for REF and ALT in the reference's group
 * key (Vead.ToVariantSequence): it is given as PISCES_VEAD_REF, so equal keys are equal state vectors. */
#define PISCES_VEAD_NONE  0   /* N>N: out of range, insufficient data, unknown */
#define PISCES_VEAD_REF   1   /* ref[0]>ref[0] */
#define PISCES_VEAD_ALT   2   /* ref>alt */
#define PISCES_VEAD_OTHER 3   /* X>X */
#define PISCES_VEAD_MAX_SITES 256   /* sites of one neighbourhood (the reference has no cap; neighbourhoods chain at PhasingDistance 50) */
typedef struct PiscesVeadSite { int32_t position, ref_len, alt_len; int32_t allele_offset; } PiscesVeadSite; /* ref bytes then alt bytes in `alleles` */
typedef struct PiscesVeadNeighborhood { int32_t site_begin, site_end; } PiscesVeadNeighborhood;           /* [begin, end) into sites */
typedef struct PiscesVeadOptions { int32_t min_base_call_quality /* 20 */, min_number_variants_in_read /* 1 */; } PiscesVeadOptions;
typedef struct PiscesVeadGroup { int32_t neighborhood, first_read, n_veads; int32_t pad; int64_t state_offset; } PiscesVeadGroup;
typedef struct PiscesVeadNeighborhoodInfo { int32_t first, last_with_look_ahead, soft_clip_end_before, soft_clip_pos_after;
                                            int32_t n_groups, n_clipped_reads, n_reads_used, group_begin; } PiscesVeadNeighborhoodInfo;
/* Where the groups go.  Host memory for pisces_hip_vead_groups, device-accessible for pisces_hip_vead_groups_device.  info[n_neighbourhoods]
 * is sized by the input and always written; n_out[3] = {groups, state bytes, 0}.  When a count is above its capacity only n_out and info
 * are written: repeat with larger arrays. */
typedef struct PiscesVeadOut {
    PiscesVeadGroup* groups;
    uint8_t* states;                     /* one byte a site of the group's neighbourhood at groups[g].state_offset */
    PiscesVeadNeighborhoodInfo* info;
    int64_t* n_out;
    int64_t group_capacity, state_capacity;
} PiscesVeadOut;
int32_t pisces_hip_vead_default_options(PiscesVeadOptions* opts);
/* ONE read against one site list, host only, no handle: states[n_sites] and *n_in_range (numSitesFoundInRead; the read is a vead when it
 * reaches min_number_variants_in_read).  position is Read.Position (1-based).  Returns PISCES_OK or PISCES_E_INVALID_ARG. */
int32_t pisces_hip_vead_site_states(const PiscesVeadOptions* opts, int32_t position, const uint8_t* cigar_op, const uint32_t* cigar_len, int32_t n_cigar,
                                    const uint8_t* bases, const uint8_t* quals, int32_t n_bases, const PiscesVeadSite* sites, int32_t n_sites,
                                    const uint8_t* alleles, int64_t n_allele_bytes, uint8_t* states, int32_t* n_in_range);
/* VcfNeighborhood.SetRangeOfInterest for a site list in the caller's order (nothing is sorted), host only: the four bounds of *info. */
int32_t pisces_hip_vead_neighborhood_info(const PiscesVeadSite* sites, int32_t n_sites, PiscesVeadNeighborhoodInfo* info);
/* The groups of every neighbourhood over a HOST batch: the statement of the output contract and the function the device runs.
 * Neighbourhoods come in input order; within one the groups come in the order of their first read (the reference's Dictionary enumerates
 * in insertion order); first_read is the batch index of the representative vead (the host makes VeadGroup.Name from it), n_veads the
 * group's count.  Per neighbourhood the scan is VeadGroupSource's: every read up to and including the first with position >
 * last_with_look_ahead is tested for IsClippedWithinNeighborhood (n_clipped_reads, counted BEFORE the skip test), a read with EndPosition <
 * first is skipped, the others are used (n_reads_used) and are veads when enough sites are in range.  The MAPQ, duplicate and proper-pair
 * tests belong to whoever made the batch.  Refused, each with a message: positions that descend (PISCES_E_INVALID_ARG naming the first
 * offending read, n_out = {PISCES_E_INVALID_ARG, 0, that read}: sortedness is what makes "stop at the first read past" a per-read test),
 * more than PISCES_VEAD_MAX_SITES sites in a neighbourhood (PISCES_E_UNSUPPORTED), an empty neighbourhood or one outside the site list, a
 * site with ref_len or alt_len below 1 or allele bytes outside `alleles`, null arrays, negative sizes (PISCES_E_INVALID_ARG);
 * PISCES_E_BUFFER_TOO_SMALL with the counts in n_out when a capacity is short.  Bit-reproducible from run to run. */
int32_t pisces_hip_vead_groups(const PiscesVeadOptions* opts, const PiscesReadBatch* batch, const PiscesVeadSite* sites, int32_t n_sites,
                               const uint8_t* alleles, int64_t n_allele_bytes, const PiscesVeadNeighborhood* neighbourhoods, int32_t n_neighbourhoods,
                               const PiscesVeadOut* out);
/* The same over reads in device memory: device_batch as for pisces_hip_add_device_reads (n_cigar_ops, n_bases: its array sizes), or NULL
 * for the handle's decoded batch (pisces_hip_bam_decode) before it has moved into the store.  sites, alleles and neighbourhoods are small
 * host arrays; the library uploads them.  Every array of `out` is caller-owned device-accessible memory.  The call waits ONCE, for the
 * read range of every neighbourhood and the sortedness verdict (8 bytes a neighbourhood come back): that sizes the scratch and lets
 * descending positions be refused with a status and a message as above.  Everything behind that is enqueued on `stream` (NULL: the
 * handle's own) and the call returns without waiting for it; a count above its capacity leaves only n_out and info written.  The
 * output is the host entry's, byte for byte, whichever wave runs first.  The handle's reads, store and decoded batch are left alone.
 * Deviation: the reference hands Scylla every BAM record (BamFileAlignmentExtractor.GetNextAlignment); the decode drops unmapped,
 * secondary and CIGAR-less records (AlignmentSource.ShouldSkipRead).  A host that wants those phased passes its own batch. */
int32_t pisces_hip_vead_groups_device(PiscesHip* h, const PiscesVeadOptions* opts, const PiscesReadBatch* device_batch, int64_t n_cigar_ops, int64_t n_bases,
                                      const PiscesVeadSite* sites, int32_t n_sites, const uint8_t* alleles, int64_t n_allele_bytes,
                                      const PiscesVeadNeighborhood* neighbourhoods, int32_t n_neighbourhoods, const PiscesVeadOut* out, void* stream);

/* ---- Scylla's neighbourhoods (src/lib/VariantPhasing): the tables the read pass takes, from called rows ---------------------------------
 * NeighborhoodBuilder, VariantSite, VcfNeighborhood and the front of CallableNeighborhood over the rows of ONE chromosome as a flush gives
 * them out (PiscesVennRows; a row's alleles are its candidate's bytes when cand_index[r] >= 0, otherwise the single bases of
 * PISCES_INFO_REF / PISCES_INFO_ALT).  csrc/nbhd.h restates the decision for host and device and quotes the C#:
 *   - a row with PISCES_FILTER_FORCED_REPORT is skipped before anything else;
 *   - a row is eligible unless it is a Reference row, of a category above PISCES_CAT_REFERENCE, one of the four no-calls of
 *     CalledAllele.IsNocall (ALT12_LIKE_NOCALL, ALT_LIKE_NOCALL, HEMI_NOCALL, REF_LIKE_NOCALL; REF_AND_NOCALL and ALT_AND_NOCALL are not),
 *     HOM_ALT with het_variants_only, or carries a filter (bits 0..13 of filter_bits; 14..15 are the phase set) with passing_variants_only;
 *   - an eligible row is proximal when position - (position of the last ELIGIBLE row) < phasing_distance, strictly;
 *   - the neighbourhoods are the maximal runs of two or more consecutive eligible rows each proximal to the one before; a distance below 1
 *     gives none;
 *   - a neighbourhood with passing < min_passing_variants_in_nbhd && non_passing > 0 is dropped and still takes a raw_index;
 *   - the sites of a neighbourhood are sorted by position + (ref_len != alt_len), STABLY (within one position the equal-length alleles go
 *     in front of the indels); the reference writes OriginalAlleleFromVcf back in the pre-sort order, so site s holds the alleles of row
 *     site_row[s] and the original allele of row site_original[s];
 *   - the bounds are pisces_hip_vead_neighborhood_info of the sorted sites, plus last_in_vcf.
 * Deviations: .NET's List.Sort is unspecified among equal keys above 16 elements, the stable order is given at every
 * size; the reference's split of one crushed multi-allelic VCF line at a full batch is not reproduced (rows are uncrushed). */
typedef struct PiscesNbhdCriteria {
    int32_t phasing_distance;              /* PhasableVariantCriteria.PhasingDistance, 50 */
    int32_t passing_variants_only;         /* PassingVariantsOnly, 1 */
    int32_t het_variants_only;             /* HetVariantsOnly, 0 */
    int32_t min_passing_variants_in_nbhd;  /* MinPassingVariantsInNbhd, 0 */
    int32_t reserved[4];
} PiscesNbhdCriteria;
/* one kept neighbourhood (48 bytes) */
typedef struct PiscesNbhdInfo {
    int32_t raw_index;                     /* its number among all neighbourhoods, dropped ones included (NbhdNum of one unbounded batch) */
    int32_t n_passing, n_non_passing;      /* VcfNeighborhood.PassingVariants / NonPassingVariants */
    int32_t first, last_in_vcf, last_with_look_ahead, soft_clip_end_before, soft_clip_pos_after;
    int32_t ref_len;                       /* last_with_look_ahead - first bytes of NbhdReferenceSequenceSubstring ... */
    int32_t reserved;
    int64_t ref_offset;                    /* ... at this offset of ref_bytes */
} PiscesNbhdInfo;
#define PISCES_NBHD_ROW_FORCED     0   /* forced-report row, skipped */
#define PISCES_NBHD_ROW_INELIGIBLE 1
#define PISCES_NBHD_ROW_LONE       2   /* eligible, in no neighbourhood */
#define PISCES_NBHD_ROW_DROPPED    3   /* in a dropped neighbourhood */
#define PISCES_NBHD_ROW_KEPT       4   /* in a kept neighbourhood: a row phasing may replace */
/* Where the tables go: host memory for pisces_hip_nbhd_build, device-accessible memory (pinned host memory included) for
 * pisces_hip_nbhd_build_device.  sites / alleles / neighbourhoods are exactly what pisces_hip_vead_groups[_device] takes: the kept
 * neighbourhoods in input order as [begin, end) into sites, each site's ref bytes then alt bytes starting where the previous site's end.
 * n_out[6] = {kept neighbourhoods, sites, allele bytes, reference bytes, raw neighbourhoods, eligible rows}.  When one of the first four is
 * above its capacity only n_out is written: repeat with larger arrays.  Rows that descend by position leave n_out = {PISCES_E_INVALID_ARG,
 * 0, lowest offending row, 0, 0, 0}; otherwise an insertion, deletion or MNV row without a candidate to take bytes from leaves
 * {PISCES_E_INVALID_ARG, 1, lowest such row, 0, 0, 0}; more than 2^31 - 1 allele or reference bytes {PISCES_E_UNSUPPORTED, 0, ...}.
 * Nothing else is written then.  There is no cap on the sites of a neighbourhood (PISCES_VEAD_MAX_SITES is the read pass's, which
 * refuses it). */
typedef struct PiscesNbhdOut {
    PiscesVeadSite* sites;                 /* site_capacity */
    uint8_t* alleles;                      /* allele_capacity bytes */
    int32_t* site_row;                     /* site_capacity: the row whose alleles site s holds */
    int32_t* site_original;                /* site_capacity: the row of the s-th site before sorting (OriginalAlleleFromVcf) */
    PiscesVeadNeighborhood* neighbourhoods;/* nbhd_capacity */
    PiscesNbhdInfo* info;                  /* nbhd_capacity */
    uint8_t* ref_bytes;                    /* ref_capacity */
    uint8_t* row_class;                    /* optional, one PISCES_NBHD_ROW_* a row of the input (rows->n of them; min(n, *count) are written) */
    int64_t* n_out;                        /* [6] */
    int64_t nbhd_capacity, site_capacity, allele_capacity, ref_capacity;
} PiscesNbhdOut;
int32_t pisces_hip_nbhd_default_criteria(PiscesNbhdCriteria* criteria);
/* Over host arrays, no handle and no device: the statement of the contract and the function the device runs.  reference (optional):
 * reference[i] is position i + 1; a neighbourhood's reference bytes are copied from first - 1 when the reference reaches
 * last_with_look_ahead - 1, otherwise they are that many 'R' (CallableNeighborhood.cs:102-107).  PISCES_E_BUFFER_TOO_SMALL with the counts
 * in n_out and nothing else written when a capacity is short; PISCES_E_INVALID_ARG / PISCES_E_UNSUPPORTED with n_out as above and a
 * message; PISCES_E_INVALID_ARG for null criteria / rows / out / n_out, a negative row count or capacity, null recs with rows, a
 * cand_index without cands and alleles, a null array with a capacity above 0, a negative reference length. */
int32_t pisces_hip_nbhd_build(const PiscesNbhdCriteria* criteria, const PiscesVennRows* rows, const uint8_t* reference, int64_t reference_length,
                              const PiscesNbhdOut* out);
/* The same over device-resident rows, byte for byte, whichever wave runs first.  Asynchronous on `stream` (NULL: the handle's own),
 * ordered behind whatever made the rows, no host wait inside: errors of the DATA (descending rows, a missing candidate, short capacities)
 * arrive in n_out as above and the call still returns PISCES_OK.  Every call overwrites.  The reference bytes come from
 * pisces_hip_set_reference's when it was called.  The scratch (about 50 bytes a row) is the handle's and only grows; calls of one handle
 * must be stream-ordered with respect to each other, and a call that has to grow the scratch waits first. */
int32_t pisces_hip_nbhd_build_device(PiscesHip* h, const PiscesNbhdCriteria* criteria, const PiscesVennRows* rows, const PiscesNbhdOut* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PISCES_HIP_H */
