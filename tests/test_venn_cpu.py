"""VennVcf's consensus of two probe pools without a GPU: the plain-Python statement (tests/venn_ref.py) against the reference's own known answers
(tests/golden/venn_cases.json, README_venn.md), and the library's host entries (pisces_hip_venn_consensus, pisces_hip_venn_combine) against
the statement on the goldens and on seeded pools that take every branch."""
import numpy as np
import pytest

from pisces_amd import _abi, engine
from pisces_amd._native import PiscesHipError
from tests import venn_cases as V
from tests import venn_ref as R

G = V.GOLDEN
PAIRS_WITH_FILES = [name for name, p in G["pairs"].items() if p["expected"]]
E_INVALID_ARG, E_BUFFER_TOO_SMALL = -1, -2


def by_chromosome(pair):
    """[(chromosome, pool A's rows, pool B's rows)]: a call sees one chromosome"""
    p = G["pairs"][pair]
    rows_a, rows_b = V.rows_of_file(p["a"]), V.rows_of_file(p["b"])
    return [(c, [r for r in rows_a if r["chrom"] == c], [r for r in rows_b if r["chrom"] == c]) for c in V.chromosomes(rows_a, rows_b)]


def host_consensus(rows_a, rows_b, o, **kw):
    recs_a, alleles_a = V.records_of(rows_a)
    recs_b, alleles_b = V.records_of(rows_b)
    return engine.venn_consensus(recs_a, recs_b, V.options_struct(o), alleles_a, alleles_b, **kw)


def frequency(c):   # CalledAllele.Frequency
    return 0.0 if c["total_coverage"] == 0 else min(float(np.float32(c["allele_support"]) / np.float32(c["total_coverage"])), 1.0)


def filter_names(bits):
    names = {0: "StrandBias", 1: "PoolBias", 3: "LowVariantQscore", 4: "LowDepth", 5: "LowVariantFrequency"}
    return [names[b] for b in sorted(names) if (bits >> b) & 1]


def check_facts(c, facts, where):
    for k, want in facts.items():
        if k == "frequency":
            assert round(frequency(c), want[1]) == round(want[0], want[1]), (where, k, frequency(c), want)   # xUnit Assert.Equal(a, b, precision) rounds both
        elif k == "filters":
            assert filter_names(c["filters"]) == want, (where, k, c["filters"], want)
        elif k == "pos":
            assert c["position"] == want, (where, k, c, want)
        elif k == "sb_gatk":
            assert 10 * np.log10(c["sb"]) == want, (where, k, c["sb"], want)
        elif k == "pb_gatk":
            assert c["pb_gatk"] == want, (where, k, c, want)
        else:
            assert c[k] == want, (where, k, c[k], want)


def read_back(c, rows_a, rows_b):
    """a consensus row as AlleleReader reads it back from the file VennVcfWriter wrote: the tests that assert on CombinedVariants see the
    writer's DP (its own recomputation) and its ALT"""
    f = V.line_fields(c, rows_a, rows_b)
    return dict(c, total_coverage=f["dp"], alt=f["alt"])


def both_ways(rows_a, rows_b, o):
    """(statement's consensus, Venn classes) after checking that the host entry says the same"""
    cons, venn_a, venn_b = R.consensus(rows_a, rows_b, o)
    res = host_consensus(rows_a, rows_b, o)
    V.assert_same_consensus(V.dicts_of(res), cons)
    assert list(res["venn_a"]) == venn_a and list(res["venn_b"]) == venn_b
    return cons, venn_a, venn_b


# ---- the reference's expected files -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS_WITH_FILES)
def test_expected_consensus_files_are_reproduced(pair):
    """every body line of the expected consensus, by the statement and by the host entry: QUAL, FILTER, DP, GT, GQ, AD, NL, PB, and VF0..DP1's
    AD / DP where the file was written in debug mode"""
    p = G["pairs"][pair]
    o = V.options_of(p["options"])
    expected = G["files"][p["expected"]]
    n = 0
    for chrom, rows_a, rows_b in by_chromosome(pair):
        cons, _, _ = both_ways(rows_a, rows_b, o)
        lines = [ln for ln in expected if ln["chrom"] == chrom]
        assert len(cons) == len(lines), (pair, chrom)
        for c, line in zip(V.written_order(cons), lines):
            V.assert_line(c, rows_a, rows_b, line, p.get("debug"), (pair, chrom, line["line"]))
            n += 1
    assert n == len(expected) and n > 30


def venn_sets(pair, o):
    sets = {"a_and_b": [], "a_not_b": [], "b_and_a": [], "b_not_a": []}
    for chrom, rows_a, rows_b in by_chromosome(pair):
        _, venn_a, venn_b = both_ways(rows_a, rows_b, o)
        for rows, classes, names in ((rows_a, venn_a, ("a_and_b", "a_not_b")), (rows_b, venn_b, ("b_and_a", "b_not_a"))):
            for r, k in zip(rows, classes):
                if k:
                    sets[names[k - 1]].append([chrom, r["position"], r["ref"], r["alt"]])
    return sets


def test_the_four_venn_files_of_grch37():
    p = G["pairs"]["GRCH37"]
    got = venn_sets("GRCH37", V.options_of(p["options"]))
    for key, name in p["venn"].items():
        want = [[ln["chrom"], ln["pos"], ln["ref"], ln["alt"]] for ln in G["files"][name]]
        assert sorted(got[key]) == sorted(want), key
    assert len(got["b_not_a"]) == 9 and len(got["a_not_b"]) == 1 and not got["a_and_b"]


def test_small_pair_probe_pool_bias_facts():
    """VennVcf_CombineTwoPoolVariants_ProbePoolBias_Tests: a reference called in one pool alone is PB, not PASS; the 1 % variant of one
    pool does not come out at 6 %; and the four Venn lists"""
    facts = G["assertions"]["small"]
    o = V.options_of(G["pairs"]["small"]["options"])
    (_, rows_a, rows_b), = by_chromosome("small")
    cons, _, _ = both_ways(rows_a, rows_b, o)
    written = V.written_order(cons)
    for index, want in facts["consensus"].items():
        check_facts(read_back(written[int(index)], rows_a, rows_b), want, ("small", index))
    got = venn_sets("small", o)
    for key, want in facts["venn"].items():
        assert [g[1:] for g in got[key]] == want, key


def test_rules_a_to_d():
    """VennVcf_CombineTwoPoolVariants_RulesAthroughD_Tests: PoolAVariants[i] with PoolBVariants[i] through CombineVariants"""
    o = V.options_of(G["pairs"]["09H"]["options"])
    (_, rows_a, rows_b), = by_chromosome("09H")
    for rule in G["assertions"]["09H"]:
        a, b = dict(rows_a[rule["index"]]), dict(rows_b[rule["index"]])
        check_facts(a, rule["a"], ("09H a", rule["index"]))
        check_facts(b, rule["b"], ("09H b", rule["index"]))
        case = R.comparison_case(a, b)
        assert case == rule["case"]
        rec_a, rec_b = V.record_of(a)[0], V.record_of(b)[0]
        c = R.combine_variants(a, b, case, o)
        check_facts(c, rule["consensus"], ("09H", rule["index"]))
        row, info, _ = engine.venn_combine(rec_a, rec_b, V.options_struct(o))
        assert R.CASES[info.comparison_case] == rule["case"]
        assert (int(row["variant_qscore"]), R.GENOTYPES[int(row["info"]) & 15], int(row["filter_bits"]), int(row["allele_support"]), int(row["total_coverage"])) == \
               (c["variant_qscore"], c["genotype"], c["filters"], c["allele_support"], c["total_coverage"])


def test_rules_e_and_f():
    """VennVcf_CombineTwoPoolVariants_RulesEandF_Tests: several REF calls of one position become one, several no-calls stay apart"""
    facts = G["assertions"]["RulesEandF"]
    o = V.options_of(G["pairs"]["RulesEandF"]["options"])
    (_, rows_a, rows_b), = by_chromosome("RulesEandF")
    for rows, key in ((rows_a, "a"), (rows_b, "b")):
        for index, want in facts[key].items():
            check_facts(rows[int(index)], want, (key, index))
    cons, _, _ = both_ways(rows_a, rows_b, o)
    written = V.written_order(cons)
    for index, want in facts["consensus"].items():
        check_facts(read_back(written[int(index)], rows_a, rows_b), want, ("consensus", index))


def test_merge_ref_calls_leaves_one_row():
    """VennVcf_CombineTwoPoolVariants_MergeRefCalls: co-located variants in one pool, a reference in the other -> ONE reference row"""
    want = G["assertions"]["C64"]["rows_at"]
    o = V.options_of(G["pairs"]["C64"]["options"])
    for chrom, rows_a, rows_b in by_chromosome("C64"):
        cons, _, _ = both_ways(rows_a, rows_b, o)
        if chrom == want["chrom"]:
            assert sum(1 for c in cons if c["position"] == want["pos"]) == want["count"]
            assert sorted(r["type"] for r in rows_a + rows_b if r["position"] == want["pos"]) == ["Mnv", "Reference"]


def test_empty_inputs_give_an_empty_consensus():
    assert by_chromosome("Empty") == []
    res = host_consensus([], [], R.default_options())
    assert res["n_out"] == (0, 0, 0) and len(res["records"]) == 0
    assert R.consensus([], [], R.default_options()) == ([], [], [])


# ---- the unit goldens ---------------------------------------------------------------------------------------------------------------
def unit_row(d):
    gatk = d.get("sb_gatk", 0.0)
    return {"position": d.get("position", 1), "ref": d["ref"], "alt": d["alt"], "type": d["category"], "genotype": d["genotype"], "total_coverage": d["total_coverage"],
            "allele_support": d["allele_support"], "reference_support": d["reference_support"], "variant_qscore": d.get("variant_qscore", 0),
            "genotype_qscore": d.get("genotype_qscore", 0), "noise_level": d.get("noise_level", 0), "filters": 0, "sb": 10.0 ** (gatk / 10.0)}


def library_combine(a, b, case, o):
    """pisces_hip_venn_combine on the rows of two statement dicts; the rewritten q-scores are written back as the reference does"""
    row, info, vq = engine.venn_combine(None if a is None else V.record_of(a)[0], None if b is None else V.record_of(b)[0], V.options_struct(o),
                                        R.CASES.index(case))
    src = a if (info.comparison_case in (0, 1) or (info.comparison_case == 2 and a["type"] != "Reference") or (info.comparison_case == 3 and b is None)) else b
    word = int(row["info"])
    is_ref = ((word >> 4) & 7) == _abi.CAT_REFERENCE
    c = {"genotype": R.GENOTYPES[word & 15], "ref": src["ref"][:1] if info.alt_changed_to_ref else src["ref"], "alt": "." if is_ref else src["alt"],
         "total_coverage": int(row["total_coverage"]), "allele_support": int(row["allele_support"]), "reference_support": int(row["reference_support"]),
         "variant_qscore": int(row["variant_qscore"]), "genotype_qscore": int(row["genotype_qscore"]), "noise_level": int(row["noise_level"]),
         "sb": float(row["strand_bias_score"]), "pb_gatk": info.pool_bias_gatk, "filters": int(row["filter_bits"])}
    return c, vq


@pytest.mark.parametrize("name", ["CombineHaploidCalls", "CombineHalfCallHalfNoCalls"])
def test_simple_combinations(name):
    """ConsensusBuilderTests.CheckSimpleCombinations: A+B, B+A, A+null, null+B, by the statement and by the library"""
    case_of = G["unit"][name]
    o = R.default_options()
    for chk in case_of["checks"]:
        for combine in ("statement", "library"):
            a, b = unit_row(case_of["alleles"][chk["a"]]), unit_row(case_of["alleles"][chk["b"]])
            expected_count = a["allele_support"] + b["allele_support"]
            if chk["case"] == "OneReferenceOneAlternate":
                expected_count = a["allele_support"] if a["type"] == "Snv" else b["allele_support"]
            run = (lambda x, y, k: R.combine_variants(x, y, k, o)) if combine == "statement" else (lambda x, y, k: library_combine(x, y, k, o)[0])
            for x, y in ((a, b), (b, a)):
                c = run(dict(x), dict(y), chk["case"])
                assert (c["genotype"], c["ref"], c["alt"], c["total_coverage"], c["allele_support"]) == \
                       (chk["genotype"], a["ref"], chk["alt"], a["total_coverage"] + b["total_coverage"], expected_count), (name, chk, combine)
            for x, y, v in ((dict(a), None, a), (None, dict(b), b)):
                c = run(x, y, "CanNotCombine")
                assert (c["genotype"], c["ref"], c["alt"], c["total_coverage"], c["allele_support"]) == \
                       (R.do_defensive_genotyping(dict(v)), v["ref"], v["alt"], v["total_coverage"], v["allele_support"]), (name, chk, combine)


def test_qscore_test_take_min_of_30_and_75_is_100():
    """VennVcf_CombineTwoPoolVariants_Qscore_Test (quirk: PushThroughRamificationsOfGTChange rewrites the COMPONENT q-scores with the
    reference model before TakeMin looks at them)"""
    u = G["unit"]["Qscore_Test"]
    o = V.options_of(u["options"])
    a, b = unit_row(u["a"]), unit_row(u["b"])
    c = R.combine_variants(dict(a), dict(b), R.comparison_case(a, b), o)
    check_facts(c, u["expected"], "statement")
    lib, vq = library_combine(a, b, "OneReferenceOneAlternate", o)
    check_facts(lib, u["expected"], "library")
    assert vq == (100, 100) and (a["variant_qscore"], b["variant_qscore"]) == (30, 75)


def test_qscore_different_noise_levels_through_six_calls():
    """VennVcf_CombineTwoPoolVariants_Qscore_DiffentNL_Test: averaged and minimal noise level, either member absent, both methods; the objects
    keep a call's rewritten q-score for the next call"""
    u = G["unit"]["Qscore_DiffentNL_Test"]
    for combine in ("statement", "library"):
        a, b = unit_row(u["a"]), unit_row(u["b"])
        for step in u["steps"]:
            o = V.options_of(dict(u["options"], combine_qscore_method=step["method"]))
            x, y = (a if "a" in step["members"] else None), (b if "b" in step["members"] else None)
            case = R.comparison_case(x, y)
            if combine == "statement":
                c = R.combine_variants(x, y, case, o)
            else:
                c, vq = library_combine(x, y, case, o)
                if x is not None:
                    x["variant_qscore"] = vq[0]
                if y is not None:
                    y["variant_qscore"] = vq[1]
                for v in (x, y):
                    if v is not None:
                        R.do_defensive_genotyping(v)
            check_facts(c, step["expected"], (combine, step))


# ---- seeded pools: the host entry is the statement, on every branch --------------------------------------------------------------------
WANTED_BRANCHES = {
    "case:AgreedOnReference", "case:AgreedOnAlternate", "case:OneReferenceOneAlternate", "case:CanNotCombine",
    "gt:nothing-present", "gt:below-min-frequency-both-pools-low", "gt:below-min-frequency-one-pool-high", "gt:below-filter-frequency", "gt:kept", "gt:low-depth",
    "gt:reference-kept", "alt-changed-to-ref", "method:pool", "method:take-min", "noise-levels-differ",
    "defensive:AltAndNoCall", "defensive:HemizygousAlt", "defensive:RefAndNoCall", "defensive:HemizygousRef", "defensive:HemizygousNoCall",
    "pairs:ref-a-with-3", "pairs:ref-b-with-3", "pairs:ref-a-with-2", "pairs:ref-b-with-2", "pairs:partial-agreement", "reference-merge", "multi-allelic",
    "allele:Insertion", "allele:Deletion", "allele:Mnv", "deletion-against-reference", "cannot-combine-reference-model", "pool-bias:biased", "pool-bias:acceptable"}


def test_seeded_pools_take_every_branch_and_the_host_entry_agrees():
    taken = set()
    for seed in range(6):
        rng = np.random.default_rng(9100 + seed)
        rows_a, rows_b = V.make_pools(rng, 150)
        o = R.default_options(min_frequency_filter=0.03, combine_qscore_method=seed % 2)
        cons, venn_a, venn_b = R.consensus(rows_a, rows_b, o, taken)
        res = host_consensus(rows_a, rows_b, o)
        V.assert_same_consensus(V.dicts_of(res), cons, seed)
        assert list(res["venn_a"]) == venn_a and list(res["venn_b"]) == venn_b
        assert [c["position"] for c in cons] == sorted(c["position"] for c in cons)
        # the candidate table is compact, in row order, and the bytes are the alleles
        used = [int(i) for i in res["cand_index"] if i >= 0]
        assert used == list(range(res["n_out"][1]))
        assert res["n_out"][2] == sum(len(r) + len(a) for (r, a), i in zip(res["alleles"], res["cand_index"]) if i >= 0)
        for c, i in zip(cons, res["cand_index"]):
            assert (i >= 0) == (len(c["ref"]) > 1 or len(c["alt"]) > 1)
    assert WANTED_BRANCHES <= taken, sorted(WANTED_BRANCHES - taken)


# ---- the named quirks ---------------------------------------------------------------------------------------------------------------
def _ref(position, depth, support, gt="HomozygousRef", q=100, nl=20, filters=0, sb=1e-10):
    return {"position": position, "ref": "A", "alt": ".", "type": "Reference", "genotype": gt, "total_coverage": depth, "allele_support": support,
            "reference_support": support, "variant_qscore": q, "genotype_qscore": q, "noise_level": nl, "filters": filters, "sb": sb}


def _alt(position, depth, support, alt="T", ref="A", gt="HeterozygousAltRef", q=100, nl=20, filters=0, sb=1e-10):
    return {"position": position, "ref": ref, "alt": alt, "type": R.set_type(ref, alt), "genotype": gt, "total_coverage": depth, "allele_support": support,
            "reference_support": depth - support, "variant_qscore": q, "genotype_qscore": q, "noise_level": nl, "filters": filters, "sb": sb}


def test_quirk_merged_reference_takes_the_min_of_variant_and_genotype_qscore():
    """VennVcf.cs:239: VariantQscore = min(VariantQscore, Consensus.GenotypeQscore); filters are merged, PB and SB take the maximum, the row
    names its first pair"""
    rows_a = [_ref(7, 5000, 30, filters=1 << 4)]   # (few reference reads: the second pair's pooled reference q-score is low)
    rows_b = [_alt(7, 5000, 10, "T", sb=0.25), _alt(7, 40, 0, "G", nl=12, filters=1 << 5), _alt(7, 5000, 2000, "C")]
    cons, _, _ = both_ways(rows_a, rows_b, R.default_options(min_frequency_filter=0.03))
    assert [(c["ref"], c["alt"], c["genotype"]) for c in cons] == [("A", ".", "HomozygousRef"), ("A", "C", "HeterozygousAltRef")]
    merged = cons[0]
    first = R.combine_variants(dict(rows_a[0]), dict(rows_b[0]), "OneReferenceOneAlternate", R.default_options(min_frequency_filter=0.03))
    second = R.combine_variants(dict(rows_a[0]), dict(rows_b[1]), "OneReferenceOneAlternate", R.default_options(min_frequency_filter=0.03))
    assert second["genotype"] == "HomozygousRef" and second["variant_qscore"] < first["variant_qscore"]
    assert merged["variant_qscore"] == merged["genotype_qscore"] == min(first["variant_qscore"], second["genotype_qscore"])
    assert merged["noise_level"] == min(first["noise_level"], second["noise_level"]) and merged["filters"] == (1 << 4) | (1 << 5)
    assert merged["sb"] == 0.25 and (merged["row_a"], merged["row_b"]) == (0, 0) and merged["total_coverage"] == first["total_coverage"] and merged["pb_score"] == 0.0


def test_quirk_reference_typed_consensus_reports_reference_support_as_allele_support():
    cons, _, _ = both_ways([_alt(3, 3067, 54, "G", q=30, nl=35)], [_ref(3, 3795, 3780, q=75, nl=35)], R.default_options(min_frequency_filter=0.03))
    (c,) = cons
    assert c["alt_changed_to_ref"] and c["type"] == "Reference" and (c["ref"], c["alt"]) == ("A", ".") and c["allele_support"] == c["reference_support"] == 3013 + 3780
    assert c["filters"] == 0 and c["pb_gatk"] == -100.0   # OneReferenceOneAlternate adds PoolBias — unless the alt changed to ref


def test_quirk_can_not_combine_without_alt_depth_uses_the_reference_model_and_is_pool_biased():
    o = R.default_options()
    cons, _, _ = both_ways([_ref(5, 1000, 990, q=3)], [], o)
    (c,) = cons
    assert c["case"] == "CanNotCombine" and c["variant_qscore"] == R.assign_poisson_qscore(990, 1000, 20, 100) == 100
    assert c["filters"] == 1 << R.FILTER_POOL_BIAS and (c["pb_score"], c["pb_gatk"]) == (1.0, 0.0)
    cons, _, _ = both_ways([], [_alt(5, 1000, 60, q=3)], o)   # with alt depth: the variant model, and PoolBias all the same
    assert cons[0]["variant_qscore"] == R.assign_poisson_qscore(60, 1000, 20, 100) and cons[0]["filters"] == 1 << R.FILTER_POOL_BIAS


def test_quirk_one_reference_one_alternate_is_always_pool_biased():
    cons, _, _ = both_ways([_ref(9, 1000, 700)], [_alt(9, 1000, 300)], R.default_options())
    (c,) = cons
    assert c["case"] == "OneReferenceOneAlternate" and not c["alt_changed_to_ref"] and c["filters"] == 1 << R.FILTER_POOL_BIAS and c["genotype"] == "HeterozygousAltRef"


def test_quirk_rewritten_component_qscores_stay_for_the_positions_later_pairs():
    """TakeMin at ref + {alt, alt'}: the first pair turns to a reference and rewrites the shared reference row's q-score (3 -> 100), which
    the second pair's minimum then reads"""
    o = R.default_options(min_frequency_filter=0.03, combine_qscore_method=R.TAKE_MIN)
    rows_a = [_ref(11, 5000, 4990, q=3)]
    rows_b = [_alt(11, 5000, 10, "T", q=50), _alt(11, 5000, 2000, "G", q=77)]
    cons, _, _ = both_ways(rows_a, rows_b, o)
    assert [c["variant_qscore"] for c in cons] == [100, 77]
    assert [c["variant_qscore"] for c in both_ways(rows_a, rows_b[1:], o)[0]] == [3]


def test_strand_bias_score_is_copied_bit_for_bit():
    sb_a, sb_b = float(np.nextafter(0.3, 1)), 0.3
    res = host_consensus([_alt(2, 900, 300, sb=sb_a)], [_alt(2, 900, 310, sb=sb_b)], R.default_options())
    assert res["records"]["strand_bias_score"][0].tobytes() == np.float64(sb_a).tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_each_with_a_message():
    rows, alleles = V.records_of([_alt(2, 900, 300)])
    good = lambda: dict(records_a=rows, records_b=rows)
    for field, value in (("min_frequency", -0.5), ("min_frequency_filter", 1.5), ("pool_bias_threshold", float("nan")), ("combine_qscore_method", 2)):
        with pytest.raises(PiscesHipError) as e:
            engine.venn_consensus(options=engine.venn_options(**{field: value}), **good())
        assert e.value.code == E_INVALID_ARG and field in e.value.message
    opts = engine.venn_options()
    n_out = np.zeros(3, dtype=np.int64)
    out = engine.venn_out(np.zeros(4, dtype=_abi.CALLED_ALLELE_DTYPE), np.zeros(4, dtype=np.int32), None, None, n_out, 4, 0, 0)
    pool = engine.venn_rows(rows, 1)
    lib = engine.lib
    import ctypes as C
    call = lambda o, a, b, out_: lib.pisces_hip_venn_consensus(None if o is None else C.byref(o), None if a is None else C.byref(a), None if b is None else C.byref(b),
                                                               None if out_ is None else C.byref(out_))
    assert call(opts, pool, pool, out) == 0 and n_out[0] == 1
    for args, word in (((None, pool, pool, out), "options"), ((opts, None, pool, out), "pool A"), ((opts, pool, None, out), "pool B"), ((opts, pool, pool, None), "out"),
                       ((opts, engine.venn_rows(rows, -1), pool, out), "negative"), ((opts, engine.venn_rows(None, 1), pool, out), "null recs"),
                       ((opts, engine.venn_rows(rows, 1, cand_index=np.zeros(1, dtype=np.int32)), pool, out), "cand_index"),
                       ((opts, pool, pool, engine.venn_out(None, None, None, None, n_out, 4, 0, 0)), "null output"),
                       ((opts, pool, pool, engine.venn_out(rows, np.zeros(4, dtype=np.int32), None, None, n_out, -1, 0, 0)), "negative capacity"),
                       ((opts, pool, pool, engine.venn_out(rows, np.zeros(4, dtype=np.int32), None, None, None, 4, 0, 0)), "n_out")):
        assert call(*args) == E_INVALID_ARG, word
        assert word in lib.pisces_hip_last_error(None).decode(), (word, lib.pisces_hip_last_error(None))
    with pytest.raises(PiscesHipError):
        engine.venn_combine(None, None)
    with pytest.raises(AttributeError):
        engine.venn_options(no_such_field=1)


def test_unsorted_pool_is_an_error_and_writes_nothing():
    rows_a = [_alt(5, 900, 300), _alt(4, 900, 300), _alt(3, 900, 300)]
    rows_b = [_alt(5, 900, 300)]
    with pytest.raises(ValueError):
        R.consensus(rows_a, rows_b)
    for a, b, pool in ((rows_a, rows_b, 0), (rows_b, rows_a, 1)):
        with pytest.raises(PiscesHipError) as e:
            host_consensus(a, b, R.default_options())
        assert e.value.code == E_INVALID_ARG and e.value.n_out == [E_INVALID_ARG, pool, 1] and "sorted" in e.value.message


def test_capacities_one_short_report_the_counts_and_write_nothing():
    rng = np.random.default_rng(77)
    rows_a, rows_b = V.make_pools(rng, 60)
    o = R.default_options(min_frequency_filter=0.03)
    full = host_consensus(rows_a, rows_b, o)
    n = full["n_out"]
    assert min(n) > 0
    exact = host_consensus(rows_a, rows_b, o, capacities=n)
    assert exact["records"].tobytes() == full["records"].tobytes() and exact["allele_bytes"].tobytes() == full["allele_bytes"].tobytes()
    for k in range(3):
        caps = list(n)
        caps[k] -= 1
        with pytest.raises(PiscesHipError) as e:
            host_consensus(rows_a, rows_b, o, capacities=tuple(caps))
        assert e.value.code == E_BUFFER_TOO_SMALL and tuple(e.value.n_out) == n
