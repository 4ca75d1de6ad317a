"""Scylla's neighbourhood builder as a plain-Python statement, transcribed from the C# (src/lib/VariantPhasing) with its lists, its
_lastVariantSite, its batches and its hanging neighbourhoods:
    NeighborhoodBuilder        Logic/NeighborhoodBuilder.cs        GetBatchOfCallableNeighborhoods, ConvertToCallableNeighborhoods,
                                                                   IsEligibleVariant, IsProximal, FitVariantsInNeighborhood,
                                                                   MakeAHangingNeighborhood, AddNewNeighborhoodToBatch
    VariantSite                Models/VariantSite.cs               TrueFirstBaseOfDiff, CompareTo, IsPassing
    VcfNeighborhood            Models/VcfNeighborhood.cs           AddVariantSite, LastPositionIsNotMatch,
                                                                   OrderVariantSitesByFirstTrueStartPosition, SetRangeOfInterest
    CallableNeighborhood       Models/CallableNeighborhood.cs      the constructor's front: order, range, NbhdReferenceSequenceSubstring
    phase_loop                 Logic/VariantPhaser.cs:44-57        the loop over batches
It is NOT written from csrc/nbhd.h: there are no prefix sums and no runs here, only the reference's objects.  The alleles arrive one per
GetNextVariants call (rows are uncrushed).  Two things are this file's own and are said where they stand: List.Sort is taken as a stable
sort, and a row's Filters are bits 0..13 of filter_bits (bits 14..15 are the phase-set index, which is no FilterType).

COUNTS tallies the branches the tests want taken."""
import collections

from pisces_amd import _abi

COUNTS = collections.Counter()

NOCALLS = (_abi.GT_ALT12_LIKE_NOCALL, _abi.GT_ALT_LIKE_NOCALL, _abi.GT_HEMI_NOCALL, _abi.GT_REF_LIKE_NOCALL)   # CalledAllele.IsNocall
UNSUPPORTED = 5   # AlleleCategory.Unsupported: whatever lies above Reference


class CalledAllele:
    """what the builder reads of a CalledAllele; `row` is the row it came from"""

    def __init__(self, row, position, ref, alt, category, genotype, filter_bits, chromosome="chr"):
        self.row, self.chromosome, self.position, self.ref, self.alt = row, chromosome, position, ref, alt
        self.category, self.genotype = category, genotype
        self.filters = [i for i in range(14) if (filter_bits >> i) & 1]   # FilterType values; the phase-set bits are not among them


class Criteria:
    """PhasableVariantCriteria (Options/PhasingOptions.cs)"""

    def __init__(self, phasing_distance=50, passing_variants_only=True, het_variants_only=False, min_passing_variants_in_nbhd=0, chr_to_process=()):
        self.phasing_distance, self.passing_variants_only, self.het_variants_only = phasing_distance, passing_variants_only, het_variants_only
        self.min_passing_variants_in_nbhd, self.chr_to_process = min_passing_variants_in_nbhd, list(chr_to_process)


class VariantSite:
    def __init__(self, allele=None):
        self.ref, self.alt, self.reference_name, self.position, self.original, self.is_passing = None, None, None, 0, None, False
        self.row = None   # (a trace for the tests: the row these alleles came from, which the sort carries along)
        if allele is not None:
            self.row = allele.row
            self.reference_name, self.position, self.ref, self.alt = allele.chromosome, allele.position, allele.ref, allele.alt
            self.original = allele
            self.is_passing = len(allele.filters) == 0   # IsAcceptablePhasingCandidate

    def is_insertion_or_deletion(self):
        return len(self.ref) != len(self.alt)

    @property
    def true_first_base_of_diff(self):
        return self.position + 1 if self.is_insertion_or_deletion() else self.position

    def deep_copy(self):
        c = VariantSite()
        c.ref, c.alt, c.reference_name, c.position, c.original, c.is_passing = self.ref, self.alt, self.reference_name, self.position, self.original, self.is_passing
        c.row = self.row
        return c

    def variant_type(self):
        return "D" if len(self.ref) > len(self.alt) else "I" if len(self.ref) < len(self.alt) else "M"


class VcfNeighborhood:
    def __init__(self, nbhd_num, ref_name, vs1, vs2):
        self.sites, self.reference_name, self.passing, self.non_passing = [], ref_name, 0, 0
        self.add_variant_site(vs1)
        self.add_variant_site(vs2)
        self.nbhd_num = nbhd_num
        self.id = f"NbhdNum{nbhd_num}_{ref_name}_{self.sites[0].position}"

    def add_variant_site(self, site):
        self.sites.append(site.deep_copy())
        if site.is_passing:
            self.passing += 1
        else:
            self.non_passing += 1

    def last_position_is_not_match(self, site):
        return self.sites[-1].position != site.position

    def order_variant_sites_by_first_true_start_position(self):
        indexes = [s.original for s in self.sites]
        before = [id(s) for s in self.sites]
        self.sites.sort(key=lambda s: s.true_first_base_of_diff)   # List.Sort by CompareTo, taken as STABLE (this file's own: see the module text)
        if [id(s) for s in self.sites] != before:
            COUNTS["reorder"] += 1
        for i, s in enumerate(self.sites):
            s.original = indexes[i]

    def set_range_of_interest(self):
        self.last_with_look_ahead = self.sites[0].position
        self.last_in_vcf = self.sites[-1].position
        for s in self.sites:
            look_ahead = s.position + max(len(s.alt), len(s.ref))
            if look_ahead > self.last_with_look_ahead:
                self.last_with_look_ahead = look_ahead
        self.first = self.sites[0].position
        first_site, last_site = self.sites[0], self.sites[-1]
        if first_site.variant_type() in ("D", "I"):
            self.soft_clip_end_before = first_site.position
        else:
            self.soft_clip_end_before = first_site.position - 1
        self.soft_clip_pos_after = last_site.position + len(last_site.ref)


class CallableNeighborhood:
    def __init__(self, vcf_neighborhood, chr_reference=None):
        self.vcf = vcf_neighborhood
        vcf_neighborhood.order_variant_sites_by_first_true_start_position()
        vcf_neighborhood.set_range_of_interest()
        length = vcf_neighborhood.last_with_look_ahead - vcf_neighborhood.first
        if chr_reference is None or vcf_neighborhood.first - 1 + length > len(chr_reference):
            # (past the end Substring throws ArgumentOutOfRangeException; the library answers as it does without a genome)
            self.reference_substring = "R" * length
        else:
            self.reference_substring = chr_reference[vcf_neighborhood.first - 1: vcf_neighborhood.first - 1 + length]
        n = len(vcf_neighborhood.sites)
        if n > 16:
            COUNTS["nbhd_above_16"] += 1
        if n > 256:
            COUNTS["nbhd_above_256"] += 1


class NeighborhoodBuilder:
    def __init__(self, criteria, alleles, batch_size, chr_reference=None):
        """alleles: the CalledAlleles in file order; GetNextVariants gives one of them a call"""
        self.criteria, self.max_in_batch, self.chr_reference = criteria, batch_size, chr_reference
        self.source = iter(alleles)
        self.next_batch, self.unfinished = [], []
        self.last_site = VariantSite()   # ReferenceName null: proximal to nothing
        self.trace_eligible, self.trace_raw = [], []   # (for the tests: the eligible rows, every neighbourhood made)

    def get_next_variants(self):
        for allele in self.source:
            return True, [allele]
        return False, []

    def get_batch_of_callable_neighborhoods(self, num_so_far):
        self.next_batch = list(self.unfinished)
        self.unfinished = []
        keep_adding = True
        while keep_adding:
            keep_adding, unpacked = self.get_next_variants()
            if not keep_adding:
                break
            for allele in unpacked:
                if _abi.FILTER_FORCED_REPORT in allele.filters:
                    COUNTS["forced_skip"] += 1
                    continue
                site = VariantSite(allele)
                if not self.is_eligible_variant(allele):
                    continue
                self.trace_eligible.append(allele.row)
                if self.is_proximal(site, self.last_site, self.criteria.phasing_distance):
                    keep_adding = self.fit_variants_in_neighborhood(self.last_site, site, num_so_far)
                elif self.last_site.reference_name is not None:
                    COUNTS["break_by_distance"] += 1
                self.last_site = site
        raw = len(self.next_batch)
        return self.convert_to_callable_neighborhoods(self.next_batch), raw

    def convert_to_callable_neighborhoods(self, neighborhoods):
        out = []
        for nbhd in neighborhoods:
            if nbhd.passing < self.criteria.min_passing_variants_in_nbhd and nbhd.non_passing > 0:
                COUNTS["drop_by_minimum"] += 1
                continue
            out.append(CallableNeighborhood(nbhd, self.chr_reference))
        return out

    def is_eligible_variant(self, allele):
        c = self.criteria
        if c.chr_to_process and allele.chromosome not in c.chr_to_process:
            return False
        if allele.category == _abi.CAT_REFERENCE or allele.genotype in NOCALLS:
            COUNTS["ineligible_reference" if allele.category == _abi.CAT_REFERENCE else "ineligible_nocall"] += 1
            return False
        if allele.category >= UNSUPPORTED:
            COUNTS["ineligible_unsupported"] += 1
            return False
        if c.het_variants_only:
            if allele.genotype == _abi.GT_HOM_ALT:
                COUNTS["ineligible_hom_alt"] += 1
                return False
        if not c.passing_variants_only:
            return True
        if len(allele.filters) != 0:
            COUNTS["ineligible_filtered"] += 1
        return len(allele.filters) == 0

    @staticmethod
    def is_proximal(site, other, phasing_distance):
        return site.reference_name == other.reference_name and abs(site.position - other.position) < phasing_distance

    def fit_variants_in_neighborhood(self, last_site, site, num_so_far):
        ok_to_add = len(self.next_batch) < self.max_in_batch
        if len(self.next_batch) == 0:
            self.add_new_neighborhood_to_batch(last_site, site, num_so_far)
            return ok_to_add
        last_neighborhood = self.next_batch[-1]
        if last_neighborhood.last_position_is_not_match(last_site):
            if ok_to_add:
                self.add_new_neighborhood_to_batch(last_site, site, num_so_far)
                return True
            self.make_a_hanging_neighborhood(last_site, site, num_so_far)
            return False
        COUNTS["append"] += 1
        last_neighborhood.add_variant_site(site)
        return True

    def make_a_hanging_neighborhood(self, last_site, site, num_so_far):
        COUNTS["chain_start"] += 1
        self.unfinished.append(VcfNeighborhood(num_so_far + self.max_in_batch, site.reference_name, last_site, site))
        self.trace_raw.append(self.unfinished[-1])

    def add_new_neighborhood_to_batch(self, last_site, site, num_so_far):
        COUNTS["chain_start"] += 1
        self.next_batch.append(VcfNeighborhood(num_so_far + len(self.next_batch), site.reference_name, last_site, site))
        self.trace_raw.append(self.next_batch[-1])


UNBOUNDED = 1 << 60


def phase_loop(alleles, criteria, batch_size=UNBOUNDED, chr_reference=None):
    """VariantPhaser.Execute's loop (VariantPhaser.cs:44-57): batches until one comes back with no raw neighbourhood.
    Returns (every callable neighbourhood in the order given out, the raw neighbourhoods counted)."""
    builder = NeighborhoodBuilder(criteria, alleles, batch_size, chr_reference)
    callable_nbhds, raw_total, num_so_far = [], 0, 0
    while True:
        batch, raw = builder.get_batch_of_callable_neighborhoods(num_so_far)
        if raw == 0:
            break
        num_so_far += len(batch)
        raw_total += raw
        callable_nbhds += batch
    return callable_nbhds, raw_total, builder
