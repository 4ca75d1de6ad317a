"""Shared by tests/test_nbhd_cpu.py and tests/test_nbhd_gpu.py: rows made from VCF lines (the tests' own construction, not AlleleReader),
the statement's neighbourhoods (tests/nbhd_ref.py) laid out like the library's tables so that whole arrays are compared, the named cases
and the seeded row lists."""
import os
import random

import numpy as np

from pisces_amd import _abi

from tests import nbhd_ref as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
VCF_DIR = os.path.join(GOLDEN, "nbhd_vcf")
FIXTURES = ["NbhdBuilderTest0", "NbhdBuilderTest1", "NbhdBuilderTest2", "NbhdBuilderTest3", "NbhdBuilderTest4", "NbhdBuilderTest5", "NbhdBuilderForcedGT",
            "VeryMutated", "chr21_11085587_S1"]
TABLES = ("sites", "alleles", "site_row", "site_original", "neighbourhoods", "info", "ref_bytes", "row_class")

CODE = {"A": 0, "G": 1, "C": 2, "T": 3}
GT_OF_STRING = {"0/1": _abi.GT_HET_ALT_REF, "1/1": _abi.GT_HOM_ALT, "0/0": _abi.GT_HOM_REF, "1/2": _abi.GT_HET_ALT1_ALT2, "0/.": _abi.GT_REF_AND_NOCALL,
                "1/.": _abi.GT_ALT_AND_NOCALL, "0": _abi.GT_HEMI_REF, "1": _abi.GT_HEMI_ALT, ".": _abi.GT_HEMI_NOCALL}
FILTER_OF_STRING = {"SB": _abi.FILTER_STRAND_BIAS, "LowDP": _abi.FILTER_LOW_DEPTH, "LowVariantFreq": _abi.FILTER_LOW_VARIANT_FREQUENCY,
                    "LowGQ": _abi.FILTER_LOW_GENOTYPE_QUALITY, "MultiAllelicSite": _abi.FILTER_MULTI_ALLELIC_SITE, "ForcedReport": _abi.FILTER_FORCED_REPORT}


def category_of(r, a):
    if a == ".":
        return _abi.CAT_REFERENCE
    if len(r) == len(a):
        return _abi.CAT_SNV if len(r) == 1 else _abi.CAT_MNV
    return _abi.CAT_INSERTION if len(r) < len(a) else _abi.CAT_DELETION


def make_rows(rows):
    """[(position, ref, alt, genotype code, filter_bits[, category])] as (CALLED_ALLELE_DTYPE rows, the (ref, alt) pairs format_vcf takes)"""
    recs = np.zeros(len(rows), dtype=_abi.CALLED_ALLELE_DTYPE)
    pairs = []
    for i, row in enumerate(rows):
        position, r, a, gt, bits = row[:5]
        category = row[5] if len(row) > 5 else category_of(r, a)
        single = len(r) == 1 and len(a) == 1
        ref_code = CODE.get(r[0], 4)
        alt_code = ref_code if a == "." else (CODE.get(a, 4) if single else 4)
        recs[i]["position"] = position
        recs[i]["total_coverage"] = 100
        recs[i]["filter_bits"] = bits
        recs[i]["info"] = gt | (category << 4) | (ref_code << 7) | (alt_code << 10)
        pairs.append((r, a))
    return recs, pairs


def rows_of_vcf(name):
    """The tests' reading of a VCF fixture: one row an alternate allele; the GT string to a genotype code ("./." is the alt-like or the
    ref-like no-call by ALT), any FILTER other than PASS to a filter bit (ForcedReport to its own), ALT == "." to category Reference;
    <M>-style alternates of crushed forced-report lines are dropped."""
    rows = []
    with open(os.path.join(VCF_DIR, name + ".genome.vcf"), encoding="utf-8-sig") as f:   # (some begin with a byte-order mark)
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            c = line.rstrip("\n").split("\t")
            position, r, filters, gt_text = int(c[1]), c[3], c[6], c[9].split(":")[0]
            bits = 0
            if filters not in ("PASS", "."):
                for word in filters.split(";"):
                    bits |= 1 << FILTER_OF_STRING.get(word, _abi.FILTER_LOW_VARIANT_QSCORE)
            for a in c[4].split(","):
                if a.startswith("<"):
                    continue
                gt = GT_OF_STRING.get(gt_text)
                if gt is None:
                    gt = (_abi.GT_REF_LIKE_NOCALL if a == "." else _abi.GT_ALT_LIKE_NOCALL) if gt_text == "./." else _abi.GT_OTHERS
                rows.append((position, r, a, gt, bits))
    return rows


def ascending(rows):
    """(the rows in front of the first one that descends, that row's index or None): NbhdBuilderTest3 ends on a row out of order, which the
    reference takes (Math.Abs in IsProximal) and the library refuses"""
    for i in range(1, len(rows)):
        if rows[i][0] < rows[i - 1][0]:
            return rows[:i], i
    return rows, None


def alleles_of(recs, pairs):
    """the statement's CalledAlleles of rows"""
    return [ref.CalledAllele(i, int(rec["position"]), r, a, (int(rec["info"]) >> 4) & 7, int(rec["info"]) & 15, int(rec["filter_bits"]))
            for i, (rec, (r, a)) in enumerate(zip(recs, pairs))]


def criteria_pair(distance=50, passing_only=True, het_only=False, min_passing=0):
    """the same criteria for the statement and for the library"""
    from pisces_amd import engine
    return (ref.Criteria(distance, passing_only, het_only, min_passing),
            engine.nbhd_criteria(phasing_distance=distance, passing_variants_only=passing_only, het_variants_only=het_only, min_passing_variants_in_nbhd=min_passing))


def statement(recs, pairs, criteria, reference=None, batch_size=ref.UNBOUNDED):
    """tests/nbhd_ref.py over the rows, as the tables the library gives (a dict like engine.nbhd_build's)"""
    if isinstance(reference, (bytes, np.ndarray)):
        reference = bytes(reference).decode()
    kept, raw_total, builder = ref.phase_loop(alleles_of(recs, pairs), criteria, batch_size, reference)
    sites, pool, site_row, site_original, nbhds, info, ref_bytes = [], bytearray(), [], [], [], [], bytearray()
    row_class = np.full(len(recs), _abi.NBHD_ROW_INELIGIBLE, dtype=np.uint8)
    row_class[[i for i, rec in enumerate(recs) if (int(rec["filter_bits"]) >> _abi.FILTER_FORCED_REPORT) & 1]] = _abi.NBHD_ROW_FORCED
    row_class[builder.trace_eligible] = _abi.NBHD_ROW_LONE
    for nb in builder.trace_raw:
        row_class[[s.row for s in nb.sites]] = _abi.NBHD_ROW_DROPPED
    for c in kept:
        nb = c.vcf
        row_class[[s.row for s in nb.sites]] = _abi.NBHD_ROW_KEPT
        begin = len(sites)
        for s in nb.sites:
            sites.append((s.position, len(s.ref), len(s.alt), len(pool)))
            pool += s.ref.encode() + s.alt.encode()
            site_row.append(s.row)
            site_original.append(s.original.row)
        nbhds.append((begin, len(sites)))
        info.append((nb.nbhd_num, nb.passing, nb.non_passing, nb.first, nb.last_in_vcf, nb.last_with_look_ahead, nb.soft_clip_end_before, nb.soft_clip_pos_after,
                     len(c.reference_substring), 0, len(ref_bytes)))
        ref_bytes += c.reference_substring.encode()
    arr = lambda rows, dt: np.array(rows, dtype=dt) if rows else np.zeros(0, dt)
    return {"sites": arr(sites, _abi.VEAD_SITE_DTYPE), "alleles": np.frombuffer(bytes(pool), dtype=np.uint8), "site_row": arr(site_row, np.int32),
            "site_original": arr(site_original, np.int32), "neighbourhoods": arr(nbhds, _abi.VEAD_NEIGHBORHOOD_DTYPE), "info": arr(info, _abi.NBHD_INFO_DTYPE),
            "ref_bytes": np.frombuffer(bytes(ref_bytes), dtype=np.uint8), "row_class": row_class,
            "n_out": (len(nbhds), len(sites), len(pool), len(ref_bytes), raw_total, len(builder.trace_eligible))}


def assert_same(got, want, what=""):
    """whole arrays, and the six counts"""
    assert tuple(got["n_out"]) == tuple(want["n_out"]), (what, got["n_out"], want["n_out"])
    for k in TABLES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g[:12], w[:12])


def members(tables):
    """[[(position, ref, alt) of a neighbourhood's sites]]"""
    out = []
    for b, e in tables["neighbourhoods"]:
        nb = []
        for s in tables["sites"][b:e]:
            o = int(s["allele_offset"])
            nb.append((int(s["position"]), bytes(tables["alleles"][o:o + s["ref_len"]]).decode(), bytes(tables["alleles"][o + s["ref_len"]:o + s["ref_len"] + s["alt_len"]]).decode()))
        out.append(nb)
    return out


# ---- named cases: (rows, criteria keywords) ---------------------------------------------------------------------------------------------
HET, HOM, REFGT = _abi.GT_HET_ALT_REF, _abi.GT_HOM_ALT, _abi.GT_HOM_REF
LOWQ = 1 << _abi.FILTER_LOW_VARIANT_QSCORE
NAMED = {
    # VcfNeighborhood.cs:62-68: "chr7 140453137 C CGTA / chr7 140453137 C T ... the insertion should come after the C>T.  So, we reorder."
    "the_comments_insertion_before_snv": ([(140453136, "A", ".", REFGT, 0), (140453137, "C", "CGTA", HET, 0), (140453137, "C", "T", HET, 0),
                                           (140453140, "G", "A", HET, 0)], {}),
    "an_insertion_then_an_snv_one_base_on": ([(100, "C", "CGTA", HET, 0), (101, "C", "T", HET, 0)], {}),
    "ref_and_nocall_is_eligible": ([(100, "A", "C", _abi.GT_REF_AND_NOCALL, 0), (101, "A", "C", _abi.GT_ALT_AND_NOCALL, 0), (102, "A", "C", _abi.GT_ALT_LIKE_NOCALL, 0)], {}),
    "phase_bits_do_not_fail_a_row": ([(100, "A", "C", HET, 1 << 14), (101, "A", "G", HET, 2 << 14), (102, "A", "T", HET, 3 << 14)], {"min_passing": 3}),
    # the row in between is a Reference row half the distance along: it neither breaks the chain of 100 and 108 nor makes one of 200 and 210
    "an_ineligible_row_between": ([(100, "A", "C", HET, 0), (104, "A", ".", REFGT, 0), (108, "A", "C", HET, 0),
                                   (200, "A", "C", HET, 0), (205, "A", ".", REFGT, 0), (210, "A", "C", HET, 0)], {"distance": 10}),
    "a_far_eligible_row_breaks_the_chain": ([(100, "A", "C", HET, 0), (104, "A", "C", HET, 0), (130, "A", "C", HET, 0), (134, "A", "C", HET, 0),
                                             (200, "A", "C", HET, 0), (204, "A", "G", HET, 0)], {"distance": 10}),
    "distance_exactly_the_phasing_distance": ([(100, "A", "C", HET, 0), (110, "A", "C", HET, 0), (119, "A", "C", HET, 0)], {"distance": 10}),
    "all_passing_below_the_minimum": ([(100, "A", "C", HET, 0), (101, "A", "C", HET, 0), (200, "A", "C", HET, 0), (201, "A", "C", HET, LOWQ),
                                       (300, "A", "C", HET, 0), (301, "A", "G", HET, 0)], {"passing_only": False, "min_passing": 3}),
    "distance_zero": ([(100, "A", "C", HET, 0), (100, "A", "G", HET, 0), (101, "A", "C", HET, 0)], {"distance": 0}),
    "distance_negative": ([(100, "A", "C", HET, 0), (100, "A", "G", HET, 0), (101, "A", "C", HET, 0)], {"distance": -5}),
    "co_located_rows_chain": ([(100, "A", "C", HET, 0), (100, "A", "G", HET, 0)], {"distance": 1}),
    "het_only_drops_hom_alt": ([(100, "A", "C", HET, 0), (101, "A", "C", HOM, 0), (102, "A", "C", HET, 0)], {"het_only": True, "distance": 2}),
    "a_forced_row_is_no_last_site": ([(100, "A", "C", HET, 0), (105, "A", "G", HET, 1 << _abi.FILTER_FORCED_REPORT), (109, "A", "C", HET, 0)], {"distance": 5, "passing_only": False}),
    "an_unsupported_category": ([(100, "A", "C", HET, 0), (101, "A", "C", HET, 0, 5), (102, "A", "C", HET, 0, 7), (103, "A", "C", HET, 0)], {}),
    "mixed_group_of_five": ([(100, "AC", "A", HET, 0), (100, "A", "C", HET, 0), (100, "A", "AGG", HET, LOWQ), (100, "AC", "GT", HET, 0), (100, "A", "G", HET, 0),
                             (101, "C", "CT", HET, 0), (101, "C", "G", HET, 0)], {"passing_only": False}),
}


def named(name):
    rows, kw = NAMED[name]
    recs, pairs = make_rows(rows)
    return recs, pairs, kw


# ---- seeded rows ------------------------------------------------------------------------------------------------------------------------
def random_alleles(rng, category):
    letters = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    anchor = rng.choice("ACGT")
    if category == _abi.CAT_REFERENCE:
        return anchor, "."
    if category == _abi.CAT_INSERTION:
        return anchor, anchor + letters(rng.randint(1, 5))
    if category == _abi.CAT_DELETION:
        return anchor + letters(rng.randint(1, 5)), anchor
    if category == _abi.CAT_MNV:
        k = rng.randint(2, 4)
        return letters(k), letters(k)
    return anchor, rng.choice([b for b in "ACGT" if b != anchor])


def seeded_rows(seed, n=None, distance=50, dense=None):
    """One list of rows at ascending positions with gaps around `distance`, co-located groups of up to five, all five categories and the
    unsupported ones, every genotype code, filter bits (ForcedReport and the phase bits among them).  dense: mostly eligible rows in
    small gaps, for the long neighbourhoods."""
    rng = random.Random(seed)
    dense = (seed % 4 == 0) if dense is None else dense
    if n is None:
        n = rng.randint(370, 400) if dense else rng.randint(0, 400)
    rows, position = [], rng.randint(1, 1000)
    while len(rows) < n:
        d = max(distance, 1)
        gap = rng.choice((1, 2, d // 2, d - 1, d - 1, d, d, d + 1, 3 * d)) if not dense else rng.choice((1, 1, 1, 2))
        position += max(gap, 1) if rng.random() < 0.9 else 0
        for _ in range(rng.choice((1, 1, 1, 1, 2, 3, 5))):
            if len(rows) == n:
                break
            quiet = dense and rng.random() < 0.97
            category = rng.choice((0, 0, 0, 1, 2, 3)) if quiet else rng.choice((0, 0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 7))
            gt = rng.choice((HET,) * 19 + (HOM,)) if quiet else (rng.choice((HET, HET, HET, HOM, HOM)) if rng.random() < 0.7 else rng.randrange(13))
            bits = 0
            if not quiet:
                if rng.random() < 0.3:
                    bits |= 1 << rng.randrange(14)
                if rng.random() < 0.05:
                    bits |= 1 << rng.randrange(14)
                if rng.random() < 0.2:
                    bits |= rng.randrange(1, 4) << 14
            elif rng.random() < 0.03:
                bits |= LOWQ
            r, a = random_alleles(rng, min(category, 4) if category >= 5 else category)
            if category >= 5:
                r, a = r[:1], (a[:1] if a != "." else r[:1])
            rows.append((position, r, a, gt, bits, category))
    return rows


def seeded_criteria(seed):
    rng = random.Random(seed * 7919 + 1)
    return {"distance": rng.choice((1, 2, 5, 10, 50, 50)), "passing_only": rng.random() < 0.5, "het_only": rng.random() < 0.5,
            "min_passing": rng.choice((0, 0, 1, 2, 3, 5))}
