"""Scylla's neighbourhoods on the GPU (pisces_hip_nbhd_build_device): device output == host entry (pisces_hip_nbhd_build) == the
plain-Python statement (tests/nbhd_ref.py), compared as whole arrays.  tests/test_nbhd_cpu.py pins the host entry and the statement to the
reference's own facts.  The shapes are those at which the kernels can go wrong; each says why it is here."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from pisces_amd import _abi
from pisces_amd._native import PiscesHipError
from tests import nbhd_cases as N
from tests import vead_cases as V

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
ITEM = {"sites": 16, "alleles": 1, "site_row": 4, "site_original": 4, "neighbourhoods": 8, "info": 48, "ref_bytes": 1}
CAPACITY_OF = {"neighbourhoods": 0, "info": 0, "sites": 1, "site_row": 1, "site_original": 1, "alleles": 2, "ref_bytes": 3}
DTYPE = {"sites": _abi.VEAD_SITE_DTYPE, "alleles": np.uint8, "site_row": np.int32, "site_original": np.int32, "neighbourhoods": _abi.VEAD_NEIGHBORHOOD_DTYPE,
         "info": _abi.NBHD_INFO_DTYPE, "ref_bytes": np.uint8}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def caller(torch_cuda):
    from pisces_amd import engine
    with engine.HipVariantCaller(_abi.default_config()) as c:
        yield c


class DeviceRows:
    """rows (and their candidate table, when `pairs` is given) uploaded; .rows is the PiscesVennRows over them"""

    def __init__(self, torch, c, recs, pairs, count=None, tail=None):
        from pisces_amd import engine
        dev = torch.device("cuda", c.device)
        up = lambda a: torch.from_numpy(np.frombuffer(bytes(a) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.n_valid = len(recs) if count is None else count
        body = recs.tobytes() + (tail if tail is not None else b"")
        self.n = len(body) // 64
        self.keep = [up(body)]
        table = [None, None, None]
        if pairs is not None:
            idx, cands, pool = engine.candidate_table(recs, pairs)
            idx_bytes = idx.tobytes() + (b"\x7f" * 4 * (self.n - len(recs)))   # garbage indices behind the count
            self.keep += [up(idx_bytes), up(bytes(cands)), up(pool.tobytes())]
            table = self.keep[1:4]
        self.count = None
        if count is not None:
            self.count = torch.tensor([count], dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.rows = engine.venn_rows(self.keep[0], self.n, self.count, *table)


def run_device(torch, c, drows, caps, criteria=None, row_class=True, calls=1):
    """`calls` calls into sentinel-filled device buffers: (n_out, raw buffers)"""
    from pisces_amd import engine
    dev = torch.device("cuda", c.device)
    with torch.cuda.stream(c.torch_stream()):
        full = lambda nbytes: torch.full((max(nbytes, 1) + 16,), SENTINEL, dtype=torch.uint8, device=dev)
        t = {k: full(caps[CAPACITY_OF[k]] * ITEM[k]) for k in ITEM}
        t["row_class"], t["n_out"] = full(drows.n), full(48)
    out = engine.nbhd_out(t["sites"], t["alleles"], t["site_row"], t["site_original"], t["neighbourhoods"], t["info"], t["ref_bytes"], t["n_out"], *caps,
                          row_class=t["row_class"] if row_class else None)
    for _ in range(calls):
        c.nbhd_build_device(drows.rows, out, criteria)
    c.synchronize()
    raw = {k: v.cpu().numpy() for k, v in t.items()}
    raw["n_out"] = raw["n_out"][:48].view(np.int64).copy()
    return raw


def untouched(raw, keys):
    return all((raw[k] == SENTINEL).all() for k in keys)


def device_tables(torch, c, drows, criteria=None):
    """the protocol a host follows: counts first (short capacities write only n_out), then the sizes they ask for; nothing is written
    past them"""
    first = run_device(torch, c, drows, (0, 0, 0, 0), criteria)
    counts = tuple(int(v) for v in first["n_out"])
    assert counts[0] >= 0, counts
    raw = first
    if any(counts[:4]):
        assert untouched(first, list(ITEM) + ["row_class"]), "short capacities: only the counts come back"
        raw = run_device(torch, c, drows, counts[:4], criteria)
        assert tuple(int(v) for v in raw["n_out"]) == counts
    got = {"n_out": counts}
    for k in ITEM:
        used = counts[CAPACITY_OF[k]] * ITEM[k]
        assert (raw[k][used:] == SENTINEL).all(), k
        got[k] = raw[k][:used].view(DTYPE[k]).copy()
    assert (raw["row_class"][drows.n_valid:] == SENTINEL).all()
    got["row_class"] = raw["row_class"][:drows.n_valid].copy()
    return got


def three_way(torch, c, recs, pairs, kw, reference=None, table=True):
    """statement == host entry == device, whole arrays"""
    from pisces_amd import engine
    statement_criteria, criteria = N.criteria_pair(**kw)
    want = N.statement(recs, pairs, statement_criteria, reference)
    host = engine.nbhd_build(recs, pairs if table else None, criteria, reference)
    N.assert_same(host, want, "host entry")
    got = device_tables(torch, c, DeviceRows(torch, c, recs, pairs if table else None), criteria)
    N.assert_same(got, want, "device")
    return got


@pytest.mark.parametrize("fixture", N.FIXTURES)
def test_fixtures(torch_cuda, caller, fixture):
    recs, pairs = N.make_rows(N.ascending(N.rows_of_vcf(fixture))[0])
    for kw in ({}, {"distance": 2}, {"distance": 10}, {"distance": 5, "passing_only": False, "min_passing": 3}):
        three_way(torch_cuda, caller, recs, pairs, kw)


@pytest.mark.parametrize("name", sorted(N.NAMED))
def test_named_cases(torch_cuda, caller, name):
    recs, pairs, kw = N.named(name)
    three_way(torch_cuda, caller, recs, pairs, kw)


def edge_rows(n_eligible):
    """n_eligible passing rows one base apart with a Reference row behind every fifth (so eligible indices and row indices part), ONE chain
    but for a far gap at a third: neighbourhoods lie across every wave (64) and workgroup (256) edge of both indices.  At the eligible
    indices 63|64, 255|256 and 1023|1024 an insertion and an SNV share a position: a reorder group split by the edge."""
    rows, position = [], 1000
    for e in range(n_eligible):
        position += 1
        if e == n_eligible // 3 and e > 0:
            position += 100
        kind = "snv"
        for edge in (64, 256, 1024):
            if e == edge - 1 and n_eligible > edge:
                kind = "ins"
            if e == edge and n_eligible > edge:
                position -= 1
        rows.append((position, "A", "ACG", N.HET, 0) if kind == "ins" else (position, "A", "C", N.HET, 0))
        if e % 5 == 4:
            rows.append((position, "A", ".", N.REFGT, 0))
    return rows


@pytest.mark.parametrize("n_eligible", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_eligible_rows_at_the_wave_and_workgroup_edges(torch_cuda, caller, n_eligible):
    recs, pairs = N.make_rows(edge_rows(n_eligible))
    got = three_way(torch_cuda, caller, recs, pairs, {})
    assert got["n_out"][5] == n_eligible
    if n_eligible > 64:
        assert (got["site_row"] != got["site_original"]).sum() == 2 * sum(1 for edge in (64, 256, 1024) if n_eligible > edge)


def test_one_neighbourhood_of_300_sites(torch_cuda, caller):
    recs, pairs = N.make_rows(N.seeded_rows(4, n=300, distance=50, dense=True))
    got = three_way(torch_cuda, caller, recs, pairs, {"passing_only": False})
    assert got["n_out"][0] == 1 and got["n_out"][1] > 256


def test_2000_two_site_neighbourhoods(torch_cuda, caller):
    rows = []
    for k in range(2000):
        rows += [(1000 + 100 * k, "A", "C", N.HET, 0), (1000 + 100 * k + 3, "AT", "A", N.HET, N.LOWQ if k % 3 == 0 else 0)]
    recs, pairs = N.make_rows(rows)
    got = three_way(torch_cuda, caller, recs, pairs, {"passing_only": False, "min_passing": 2})
    assert got["n_out"][4] == 2000 and got["n_out"][0] == 2000 - 667


def test_all_rows_ineligible_and_all_rows_forced(torch_cuda, caller):
    recs, pairs = N.make_rows([(1000 + i, "A", ".", N.REFGT, 0) for i in range(300)])
    got = three_way(torch_cuda, caller, recs, pairs, {})
    assert got["n_out"] == (0, 0, 0, 0, 0, 0) and (got["row_class"] == _abi.NBHD_ROW_INELIGIBLE).all()
    recs, pairs = N.make_rows([(1000 + i, "A", "C", N.HET, 1 << _abi.FILTER_FORCED_REPORT) for i in range(300)])
    got = three_way(torch_cuda, caller, recs, pairs, {"passing_only": False})
    assert got["n_out"] == (0, 0, 0, 0, 0, 0) and (got["row_class"] == _abi.NBHD_ROW_FORCED).all()


def test_a_count_word_below_n_with_garbage_behind_it(torch_cuda, caller):
    recs, pairs = N.make_rows(N.seeded_rows(9, n=200, distance=10))
    kw = {"distance": 10, "passing_only": False}
    want = N.statement(recs, pairs, N.criteria_pair(**kw)[0])
    garbage = random.Random(9).randbytes(64 * 70)
    got = device_tables(torch_cuda, caller, DeviceRows(torch_cuda, caller, recs, pairs, count=len(recs), tail=garbage), N.criteria_pair(**kw)[1])
    N.assert_same(got, want, "count")


def test_candidate_tables_present_absent_and_absent_with_an_indel_row(torch_cuda, caller):
    snvs = [(100 + 2 * i, "A", "C", N.HET, 0) for i in range(70)]
    recs, pairs = N.make_rows(snvs)
    present = three_way(torch_cuda, caller, recs, pairs, {}, table=True)     # a table with no candidate in it
    absent = three_way(torch_cuda, caller, recs, pairs, {}, table=False)     # no table: the bases of info
    N.assert_same(absent, present)
    recs, pairs = N.make_rows(snvs[:66] + [(300, "AC", "A", N.HET, 0), (301, "A", "AT", N.HET, 0)])
    raw = run_device(torch_cuda, caller, DeviceRows(torch_cuda, caller, recs, None), (10, 100, 400, 400))
    assert tuple(int(v) for v in raw["n_out"]) == (_abi.E_INVALID_ARG, 1, 66, 0, 0, 0)
    assert untouched(raw, list(ITEM) + ["row_class"])


def test_each_capacity_one_short_and_a_second_call_that_overwrites(torch_cuda, caller):
    recs, pairs = N.make_rows(N.seeded_rows(21, n=300, distance=10))
    criteria = N.criteria_pair(distance=10, passing_only=False)[1]
    drows = DeviceRows(torch_cuda, caller, recs, pairs)
    full = device_tables(torch_cuda, caller, drows, criteria)
    counts = full["n_out"]
    assert all(v > 1 for v in counts[:4])
    for short in range(4):
        caps = tuple(v - (1 if i == short else 0) for i, v in enumerate(counts[:4]))
        raw = run_device(torch_cuda, caller, drows, caps, criteria)
        assert tuple(int(v) for v in raw["n_out"]) == counts
        assert untouched(raw, list(ITEM) + ["row_class"]), short
    # two calls on the stream into the same buffers, other rows first: the second's tables stand, byte for byte
    other_recs, other_pairs = N.make_rows(N.seeded_rows(22, n=300, distance=10))
    from pisces_amd import engine
    dev = torch_cuda.device("cuda", caller.device)
    other = DeviceRows(torch_cuda, caller, other_recs, other_pairs)
    other_counts = device_tables(torch_cuda, caller, other, criteria)["n_out"]
    caps = tuple(max(a, b) for a, b in zip(counts[:4], other_counts[:4]))
    once = run_device(torch_cuda, caller, drows, caps, criteria)
    with torch_cuda.cuda.stream(caller.torch_stream()):
        t = {k: torch_cuda.full((max(caps[CAPACITY_OF[k]] * ITEM[k], 1) + 16,), SENTINEL, dtype=torch_cuda.uint8, device=dev) for k in ITEM}
        t["row_class"], t["n_out"] = torch_cuda.full((drows.n + 16,), SENTINEL, dtype=torch_cuda.uint8, device=dev), torch_cuda.full((64,), SENTINEL, dtype=torch_cuda.uint8, device=dev)
    out = engine.nbhd_out(t["sites"], t["alleles"], t["site_row"], t["site_original"], t["neighbourhoods"], t["info"], t["ref_bytes"], t["n_out"], *caps, row_class=t["row_class"])
    caller.nbhd_build_device(other.rows, out, criteria)
    caller.nbhd_build_device(drows.rows, out, criteria)
    caller.synchronize()
    assert tuple(int(v) for v in t["n_out"].cpu().numpy()[:48].view(np.int64)) == counts
    for k in ITEM:
        used = counts[CAPACITY_OF[k]] * ITEM[k]
        assert t[k].cpu().numpy()[:used].tobytes() == once[k][:used].tobytes(), k
    assert t["row_class"].cpu().numpy()[:len(recs)].tobytes() == once["row_class"][:len(recs)].tobytes()


def test_a_descending_row_is_named(torch_cuda, caller):
    rows = [(1000 + i, "A", "C", N.HET, 0) for i in range(700)]
    for bad in (600, 130):   # the lower one wins, whichever wave sees its own first
        rows[bad] = (rows[bad - 1][0] - 1,) + rows[bad][1:]
    recs, pairs = N.make_rows(rows)
    raw = run_device(torch_cuda, caller, DeviceRows(torch_cuda, caller, recs, pairs), (400, 800, 1600, 1600))
    assert tuple(int(v) for v in raw["n_out"]) == (_abi.E_INVALID_ARG, 0, 130, 0, 0, 0)
    assert untouched(raw, list(ITEM) + ["row_class"])


def test_twenty_repeats_are_bit_identical(torch_cuda, caller):
    recs, pairs = N.make_rows(N.seeded_rows(33, n=400, distance=5) + [(p + 100000, r, a, g, b, k) for p, r, a, g, b, k in N.seeded_rows(36, n=400, distance=5)])
    criteria = N.criteria_pair(distance=5, passing_only=False, min_passing=2)[1]
    drows = DeviceRows(torch_cuda, caller, recs, pairs)
    counts = device_tables(torch_cuda, caller, drows, criteria)["n_out"]
    first = run_device(torch_cuda, caller, drows, counts[:4], criteria)
    for _ in range(19):
        again = run_device(torch_cuda, caller, drows, counts[:4], criteria)
        assert all(again[k].tobytes() == first[k].tobytes() for k in first)


def test_host_side_refusals(torch_cuda, caller):
    from pisces_amd import engine
    recs, pairs = N.make_rows([(100, "A", "C", N.HET, 0), (101, "A", "C", N.HET, 0)])
    drows = DeviceRows(torch_cuda, caller, recs, pairs)
    ok = lambda **kw: engine.nbhd_out(*([drows.keep[0]] * 7), drows.keep[0], 1, 1, 1, 1, **kw)
    cases = []
    out = ok(); out.n_out = None; cases.append((drows.rows, out, "null n_out"))
    out = ok(); out.site_capacity = -1; cases.append((drows.rows, out, "negative capacity"))
    out = ok(); out.site_row = None; cases.append((drows.rows, out, "a capacity above 0 with a null output array"))
    rows = engine.venn_rows(None, 2); cases.append((rows, ok(), "rows and a null recs"))
    rows = engine.venn_rows(drows.keep[0], -1); cases.append((rows, ok(), "negative row count"))
    rows = engine.venn_rows(drows.keep[0], 2, None, drows.keep[1], None, None); cases.append((rows, ok(), "a cand_index without its candidates"))
    for rows, out, text in cases:
        with pytest.raises(PiscesHipError) as e:
            caller.nbhd_build_device(rows, out)
        assert e.value.code == _abi.E_INVALID_ARG and text in e.value.message, text
    from pisces_amd._native import lib
    assert lib.pisces_hip_nbhd_build_device(caller._h, None, C.byref(drows.rows), C.byref(ok()), None) == _abi.E_INVALID_ARG
    assert b"null criteria" in lib.pisces_hip_last_error(caller._h)


def test_reference_substring_with_and_without_a_reference(torch_cuda):
    from pisces_amd import engine
    recs, pairs, kw = N.named("a_far_eligible_row_breaks_the_chain")
    reference = ("ACGT" * 60)[:203].encode()   # reaches the neighbourhoods at 100 and 130, not the look-ahead of the one at 200
    with engine.HipVariantCaller(_abi.default_config()) as c:
        bare = three_way(torch_cuda, c, recs, pairs, kw)
        assert bytes(bare["ref_bytes"]) == b"R" * 15
        c.SetReference(reference)
        statement_criteria, criteria = N.criteria_pair(**kw)
        want = N.statement(recs, pairs, statement_criteria, reference)
        N.assert_same(engine.nbhd_build(recs, pairs, criteria, reference), want, "host entry")
        got = device_tables(torch_cuda, c, DeviceRows(torch_cuda, c, recs, pairs), criteria)
        N.assert_same(got, want, "device")
        assert bytes(got["ref_bytes"]) == reference[99:104] + reference[129:134] + b"RRRRR"


def test_chr21_rows_and_reads_to_phasing_evidence(torch_cuda):
    """BAM bytes and called rows in, phasing evidence out, without a table made on the host: the reference's Scylla BAM decoded on the
    device, the rows of its VCF, phase_evidence_device == vead_groups_device over the tests' own chain of the same rows"""
    from pisces_amd import engine
    from tests.test_vead_gpu import device_groups
    z = np.load(os.path.join(V.GOLDEN, "bam_scylla_chr21.npz"))
    site_rows = [(int(p), str(r), str(a)) for p, r, a in zip(z["vcf_position"], z["vcf_ref"], z["vcf_alt"])]
    recs, pairs = N.make_rows(N.rows_of_vcf("chr21_11085587_S1"))
    with engine.HipVariantCaller(_abi.default_config()) as c:
        c.bam_decode(z["bam"], int(z["ref_id"]), min_map_quality=0, skip_duplicates=False)
        want = device_groups(torch_cuda, c, None, site_rows, V.chain(site_rows, 50))
        got = c.phase_evidence_device(DeviceRows(torch_cuda, c, recs, pairs).rows)
        V.assert_same(got, (want["groups"], want["states"], want["info"]), "phase_evidence_device")
        assert N.members(got["nbhd"]) == [site_rows] and len(got["groups"]) > 50
        # the read pass's refusals pass through unchanged
        long_recs, long_pairs = N.make_rows([(11085600 + i, "A", "C", N.HET, 0) for i in range(_abi.VEAD_MAX_SITES + 1)])
        with pytest.raises(PiscesHipError) as e:
            c.phase_evidence_device(DeviceRows(torch_cuda, c, long_recs, long_pairs).rows)
        assert e.value.code == _abi.E_UNSUPPORTED and "PISCES_VEAD_MAX_SITES" in e.value.message
