"""pisces_hip_format_vcf_device without a GPU: the entry exists and refuses what it can refuse before it touches a device, and the seeded
generator the GPU tests format (tests/vcf_device_cases.py) holds what it promises — judged by Python's decimal and numpy, not by the
library."""
import ctypes as C
import math

import numpy as np

from pisces_amd import _abi, engine
from tests import vcf_device_cases as cases


def test_the_library_exports_the_device_formatter():
    from pisces_amd import _native
    assert "pisces_hip_format_vcf_device" in _native.EXPORTS
    assert hasattr(_native.lib, "pisces_hip_format_vcf_device")


def test_a_null_handle_is_refused_before_any_device_is_touched():
    cfg = _abi.PiscesVcfConfig()
    assert engine.lib.pisces_hip_vcf_default_config(C.byref(cfg)) == 0
    word = C.c_int64(12345)
    for crush in (0, 1):   # crush = 1 is PISCES_E_UNSUPPORTED on a handle (the GPU tests); without one the null handle decides
        cfg.crush = crush
        rc = engine.lib.pisces_hip_format_vcf_device(None, C.byref(cfg), b"chr1", None, 0, None, None, None, None, None, None, 0, None, C.addressof(word), None)
        assert rc == _abi.E_INVALID_ARG
    assert word.value == 12345


def test_every_genotype_category_and_filter_bit_occurs():
    rows, gps, stats = cases.cases()
    info, bits = rows["info"].astype(np.int64), rows["filter_bits"].astype(np.int64) & cases.ALL_FILTERS
    assert set((info & 15).tolist()) == set(range(cases.N_GENOTYPES))
    assert set(((info >> 4) & 7).tolist()) == set(range(cases.N_CATEGORIES))
    assert {(int(g), int(c)) for g, c in zip(info & 15, (info >> 4) & 7)} >= {(g, c) for g in range(13) for c in range(5)}
    present = set(bits.tolist())
    for b in range(cases.FILTER_BITS):
        assert (1 << b) in present, b
    assert cases.ALL_FILTERS in present and 0 in present
    assert set(((info >> 7) & 7).tolist()) <= set(range(6)) and set(((info >> 10) & 7).tolist()) <= set(range(6))   # codes the host's table has


def test_two_step_rounding_rows_are_there_and_nothing_was_discarded():
    rows, gps, stats = cases.cases()
    assert len(rows) >= 5000 and stats["discarded"] * 100 <= stats["drawn"]
    plain = ((rows["info"] & 15) == cases.GT_HET) & (((rows["info"] >> 4) & 7) == cases.CAT_SNV)
    for d in (3, 5):
        n = sum(cases.rounding_differs(int(r["allele_support"]), int(r["total_coverage"]), d) for r in rows[plain] if int(r["total_coverage"]) == 2 * 10 ** d)
        assert n >= stats["differing"][d] >= 200, (d, n, stats)   # (a row of the plain mix may land on such a coverage too)
    # the oracle itself on three values where the two schemes part
    f32 = lambda a, b: float(np.float32(a) / np.float32(b))
    assert str(cases.two_step(f32(502, 1600), 7, 4)) == "0.3138" and str(cases.one_step(f32(502, 1600), 4)) == "0.3137"
    assert str(cases.two_step(f32(816, 1591), 7, 5)) == "0.51289" and str(cases.one_step(f32(816, 1591), 5)) == "0.51288"
    tiny = float(np.float32(0.00049999997))
    assert str(cases.two_step(tiny, 7, 3)) == "0.001" and str(cases.one_step(tiny, 3)) == "0.000"


def test_the_named_edge_cases_are_there():
    rows, gps, stats = cases.cases()
    with_support = rows[rows["allele_support"] > 0]
    sb = with_support["strand_bias_score"]
    assert np.isnan(sb).any() and (sb == 0.0).any() and (sb < 0).any() and (sb > 1).any()
    for k in range(1, 11):
        assert (sb == 10.0 ** -k).any(), k
    assert (sb == math.nextafter(1.0, 0.0)).any() and (sb == math.nextafter(1.0, 2.0)).any()
    below = 10.0 * np.log10(sb[(sb > 0) & (sb < 1)])
    assert ((below < 0) & (below > -0.00005)).any()    # prints 0.0000, and must not print -0.0000
    assert (rows["total_coverage"] == 0).any() and (rows["allele_support"] > rows["total_coverage"]).any()
    assert (rows["noise_level"] == -32768).any()
    assert set(gps["n"].tolist()) >= {0, 3, 6}
    shown = gps[gps["n"] > 0]["gp"]
    assert (shown == 0.0).any() and (shown == 3000.0).any() and np.isnan(shown).any()
    alt12 = rows[(rows["info"] & 15) == cases.GT_ALT12]
    assert set((alt12["filter_bits"] >> 14).tolist()) >= {0, 1, 2}


def test_the_generator_is_seeded():
    a = cases.generate(n=300, need_differing=5)
    b = cases.generate(n=300, need_differing=5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_allele_cases_have_the_lengths_next_to_point_rows():
    rows, alleles = cases.allele_cases()
    lens = {max(len(r), len(a)) for r, a in alleles}
    assert {1, 2, 63, 64, 65, 300, 301} <= lens
    assert sum(1 for r, a in alleles if len(r) == 1 and len(a) == 1) > len(alleles) // 2
