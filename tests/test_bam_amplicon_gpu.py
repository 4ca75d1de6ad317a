"""The BAM XN tag decoded on the device for the amplicon-bias filter (bam_kernels.hip.h bam_find_tags, bam_amplicon_kernels.hip.h): the ids
pisces_hip_bam_decode gives a tracking handle's batch against the plain-Python statement of GetStringTag on the files read back by the
plain reader (tests/bam_amplicon_cases.py, whose promises tests/test_bam_amplicon_cpu.py asserts without a device), the handle's name
dictionary, and "file bytes in, AB-filtered rows out" against the host-fed path and tests/amplicon_ref.py."""
import functools

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import amplicon_cases as S
from tests import amplicon_ref as R
from tests import bam_amplicon_cases as K
from tests.test_amplicon_gpu import AB, assert_only_the_bit_differs, caller, expected_bits
from tests.test_bgzf import _expected_directions
from tests.test_read_store import env, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def tracking(ref=None):
    c = engine.HipVariantCaller(_abi.default_config(), device=0)
    if ref is not None:
        c.SetReference(ref)
    c.SetAmpliconBiasFilter(S.THRESHOLD)
    return c


@functools.lru_cache(maxsize=None)
def expected_of(case):
    """(file bytes, kept reads by the plain reader, their names by the statement, ids by first appearance, the dictionary)"""
    bam = {"shapes": K.shapes_case, "probe": lambda: K.probe_case()[1], "regrow": lambda: K.regrow_case()[1], "second": lambda: K.second_case()[1]}[case]()
    data = bam.file()
    keep, _ = K.read_back(data)
    names = [K.amplicon_name(r["tags"]) for r in keep]
    ids, table = K.first_appearance_ids(names)
    return data, keep, names, ids, table


def decode_and_check(c, data, names, known=()):
    """bam_decode on a tracking handle: the ids are first appearance over the kept reads, continuing `known`; every name round-trips"""
    want, table = K.first_appearance_ids(names, known)
    counts = c.bam_decode(data, 0)
    assert counts["reads"] == len(names)
    got = c.bam_fetch_amplicons()
    assert got is not None and got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    have = c.AmpliconNames()
    assert have == table
    assert [None if i < 0 else have[i] for i in got] == names
    return table


@pytest.mark.parametrize("serial", [False, True], ids=["guessed entries", "serial chain"])
def test_every_shape_of_the_tag(torch_cuda, serial):
    data, keep, names, ids, table = expected_of("shapes")
    with env(PISCES_HIP_BAM_SERIAL_CHAIN="1" if serial else None):
        with tracking() as c:
            decode_and_check(c, data, names)
            assert c.bam_decode(data, 0)["chain"] == ("hopped" if serial else "guessed")
            got = c.bam_fetch()
            dirs = c.bam_fetch_directions()
            have = set(c.AmpliconNames())
        with engine.HipVariantCaller(_abi.default_config(), device=0) as c:           # a handle that does not track: the same batch, no ids
            c.bam_decode(data, 0)
            plain, plain_dirs = c.bam_fetch(), c.bam_fetch_directions()
            assert c.bam_fetch_amplicons() is None and c.AmpliconNames() == []
    assert not any(n.startswith(b"skipped_") for n in have) and b"second_never_wins" not in have and b"fake" not in have and b"" in have
    for k in plain:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    want_dirs, want_dd = _expected_directions(keep)                                    # XD and XN on one record, in either order
    for d in (dirs, plain_dirs):
        assert d is not None
        np.testing.assert_array_equal(d[0], want_dirs)
        np.testing.assert_array_equal(d[1], want_dd)
    assert (want_dirs == _abi.DIR_STITCHED).any()


def test_probe_chains_compare_bytes(torch_cuda):
    """Names that differ in their last byte, names that are prefixes of one another: as many ids as names, whatever their hashes do"""
    data, keep, names, ids, table = expected_of("probe")
    with tracking() as c:
        decode_and_check(c, data, names)
        assert len(c.AmpliconNames()) == len(K.LAST_BYTE) + len(K.PREFIXES)


def test_regrow_second_decode_and_the_shared_dictionary(torch_cuda):
    """3 000 names do not fit half of the table's first 4 096 slots: ids 0..2999 in order all the same; a second file on the same handle
    keeps the known names' ids and numbers its new ones from 3 000; a name interned by the host is the decode's name too"""
    data, keep, names, ids, table = expected_of("regrow")
    assert ids.tolist() == list(range(K.N_REGROW)) * 2
    data2, keep2, names2, _, _ = expected_of("second")
    with tracking() as c:
        known = decode_and_check(c, data, names)
        known = decode_and_check(c, data2, names2, known)
        assert len(known) == K.N_REGROW + 10 and sorted(set(c.bam_fetch_amplicons().tolist()) - set(range(K.N_REGROW))) == list(range(K.N_REGROW, K.N_REGROW + 10))
        assert c.InternAmpliconName(names2[0]) == K.N_REGROW and c.InternAmpliconName(b"never seen") == K.N_REGROW + 10
    with tracking() as c:
        assert c.InternAmpliconName(b"ampA") == 0 and c.InternAmpliconName("ampA") == 0 and c.InternAmpliconName(b"") == 1
        shared = [b"ampB", b"ampA", None, b"", b"ampA"]
        decode_and_check(c, K.named_file(shared).file(), shared, [b"ampA", b""])
        assert c.bam_fetch_amplicons().tolist() == [2, 0, -1, 1, 0]


# ---------------------------------------------------------------- end to end

@functools.lru_cache(maxsize=None)
def scenario(which):
    if which == "filter":
        ref, reads, ids = S.filter_scenario()
        threshold = S.THRESHOLD
    else:
        sc = S.planted_scenario(*S.PLANTED_SEEDS[0])
        ref, reads, ids, threshold = sc["ref"], sc["reads"], sc["ids"], sc["threshold"]
    names = [K.name_of_id(i) for i in ids]
    coverage, support = R.amplicon_counts(reads, names)
    return ref, reads, ids, threshold, names, coverage, support, K.scenario_file(ref, reads, ids).file()


def by_name(c, n):
    """{position: {name: (coverage, [support A C G T])}} of GetCoverageByAmplicon over 1..n"""
    ids, cov, sup = c.GetCoverageByAmplicon(1, n)
    table = c.AmpliconNames()
    return {p + 1: {table[i]: (int(cov[p, k]), [int(x) for x in sup[p, :, k]]) for k, i in enumerate(ids[p]) if i >= 0} for p in range(n) if (ids[p] >= 0).any()}


@pytest.mark.parametrize("which", ["filter", "planted"])
def test_file_bytes_in_filtered_rows_out(torch_cuda, which):
    ref, reads, ids, threshold, names, coverage, support, data = scenario(which)
    want_counts = {p: {n: (c, [support.get(p, {}).get(b, {}).get(n, 0) for b in "ACGT"]) for n, c in by.items()} for p, by in coverage.items()}
    rows = {}
    for view in (False, True):
        with caller(ref, threshold) as c:                                             # the bytes, decoded and added on the device
            assert c.bam_decode(data, 0)["reads"] == len(reads)
            c.AddDecodedReads()
            assert c.Stats()["reads"] == len(reads)
            assert by_name(c, len(ref)) == want_counts
            rows["decoded", view] = c.CallView().copy() if view else c.Call()
        with caller(ref, threshold) as c:                                             # the same reads parsed by the host
            c.AddAlleleCounts(reads, amplicon_ids=ids)
            rows["host", view] = c.CallView().copy() if view else c.Call()
        assert rows["decoded", view].tobytes() == rows["host", view].tobytes() and len(rows["host", view])
    assert rows["decoded", False].tobytes() == rows["decoded", True].tobytes()
    with caller(ref) as c:                                                            # without the filter: the rows as they always were
        c.bam_decode(data, 0)
        c.AddDecodedReads()
        plain = c.Call()
    with caller(ref) as c:
        c.AddAlleleCounts(reads)
        assert plain.tobytes() == c.Call().tobytes()
    filtered = rows["decoded", False]
    assert_only_the_bit_differs(filtered, plain, expected_bits(filtered, ref, coverage, support, threshold))
    assert ((filtered["filter_bits"] & AB) != 0).any()


def test_appended_decodes_carry_their_ids_into_the_open_segment(torch_cuda):
    """Small decoded batches join the open segment behind the ids it holds: the filter scenario in three files, added one after another"""
    ref, reads, ids, threshold, names, coverage, support, data = scenario("filter")
    want = {p: {n: c for n, c in by.items()} for p, by in coverage.items()}
    cuts = [0, 150, 400, len(reads)]
    with env(PISCES_HIP_STORE_DIRECT_BYTES=1 << 40, PISCES_HIP_STORE_SEAL_BYTES=1 << 40):
        with caller(ref, threshold) as c:
            for a, b in zip(cuts, cuts[1:]):
                c.bam_decode(K.scenario_file(ref, reads[a:b], ids[a:b]).file(), 0)
                c.AddDecodedReads()
            assert {p: {n: v[0] for n, v in by.items()} for p, by in by_name(c, len(ref)).items()} == want
            rows = c.Call()
    with caller(ref, threshold) as c:
        c.AddAlleleCounts(reads, amplicon_ids=ids)
        assert rows.tobytes() == c.Call().tobytes()


# ---------------------------------------------------------------- refusals

def refused(code, f, *words):
    with pytest.raises(engine.PiscesHipError) as e:
        f()
    assert e.value.code == code and all(w in e.value.message for w in words), e.value


def test_refusals(torch_cuda):
    bad, clean = K.bad_type_case().file(), K.named_file([b"a", None, b"b", b"a"]).file()
    with tracking() as c:
        assert c.bam_decode(bad, 0)["reads"] == 12                                    # the decode succeeds
        refused(_abi.E_INVALID_ARG, c.AddDecodedReads, "read 5 ", "XN")               # the lowest read is named: 5, not 9
        assert c.Stats()["reads"] == 0
        refused(_abi.E_INVALID_ARG, c.AddDecodedReads, "read 5 ")                     # and the batch stays refused
        c.bam_decode(clean, 0)
        c.AddDecodedReads()                                                            # the handle takes a clean batch
        assert c.Stats()["reads"] == 4
        refused(_abi.E_STATE, c.AddDecodedReads)                                       # (added already)
        n = len(c.AmpliconNames())
        for i in (-1, n):
            assert engine.lib.pisces_hip_get_amplicon_name(c.handle, i, None, 0) == _abi.E_INVALID_ARG
        buf = (engine.C.c_char * 4)(b"#", b"#", b"#", b"#")                            # a name that does not fit: its length, nothing written
        assert engine.lib.pisces_hip_get_amplicon_name(c.handle, 0, buf, 2) == 3 and buf.raw == b"####" and c.AmpliconNames()[0] == b"ok0"
    with engine.HipVariantCaller(_abi.default_config(), device=0) as c:               # decoded before tracking was switched on: no ids
        c.bam_decode(clean, 0)
        assert c.bam_fetch_amplicons() is None
        refused(_abi.E_STATE, lambda: c.InternAmpliconName(b"a"))
        c.SetAmpliconBiasFilter(S.THRESHOLD)
        refused(_abi.E_UNSUPPORTED, c.AddDecodedReads)
        assert c.Stats()["reads"] == 0
        c.bam_decode(clean, 0)                                                         # decoded again, now with ids
        assert c.bam_fetch_amplicons().tolist() == [0, -1, 1, 0]
        c.AddDecodedReads()
        assert c.Stats()["reads"] == 4
    with tracking() as c:
        refused(_abi.E_UNSUPPORTED, c.AddDecodedReads)                                 # nothing decoded: the refusal comes before "no batch"
        assert engine.lib.pisces_hip_bam_fetch_amplicons(c.handle, None) == _abi.E_STATE


def test_ten_fresh_handles_give_the_same_ids_and_names(torch_cuda):
    """Which read represents a name and which slot it lands in differ from run to run; ids and names may not"""
    data, keep, names, ids, table = expected_of("shapes")
    seen = set()
    for _ in range(10):
        with tracking() as c:
            c.bam_decode(data, 0)
            seen.add((c.bam_fetch_amplicons().tobytes(), tuple(c.AmpliconNames())))
    assert seen == {(ids.tobytes(), tuple(table))}
