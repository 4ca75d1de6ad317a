"""VariantQualityRecalibration on the GPU (pisces_hip_vqr_count_device, pisces_hip_vqr_apply_device): every comparison is against the
plain-Python statement (tests/vqr_ref.py), which tests/test_vqr_cpu.py pins to the reference's own known answers.  The shapes are those
at which the two kernels can go wrong: rows around a wave (64) and a workgroup (256) boundary, windows and equal-position runs that
straddle them, a count word below n with garbage behind it, sub-ranges with halo rows, accumulation."""
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi
from tests import vqr_cases, vqr_ref as R

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vqr_cases.json")))
SENTINEL = 0xA5


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


def upload(torch, c, arr):
    with torch.cuda.stream(c.torch_stream()):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", c.device))


def lib_options(o):
    from pisces_amd import engine
    return engine.vqr_options(**o)


def zero_counts(torch, c):
    with torch.cuda.stream(c.torch_stream()):
        return torch.zeros(2 * 17, dtype=torch.int64, device=torch.device("cuda", c.device))


def pair_of(d_counts):
    v = d_counts.cpu().numpy()
    return [([int(x) for x in v[k * 17:k * 17 + 16]], int(v[k * 17 + 16])) for k in range(2)]


def device_count(torch, c, recs, o, lo=0, hi=None, count=None, d_counts=None, n=None):
    """one pisces_hip_vqr_count_device over uploaded rows: (counts pair, the whole suspect buffer with its sentinel where nothing was written)"""
    n = len(recs) if n is None else n
    d_recs = upload(torch, c, recs)
    d_counts = d_counts if d_counts is not None else zero_counts(torch, c)
    with torch.cuda.stream(c.torch_stream()):
        d_sus = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device=d_recs.device)
        d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device=d_recs.device)
    c.synchronize()
    c.vqr_count_device(d_recs, n, d_counts, lib_options(o), d_count=d_count, lo=lo, hi=hi, d_suspect=d_sus)
    c.synchronize()
    return pair_of(d_counts), d_sus.cpu().numpy()


def device_apply(torch, c, recs, suspect, o, T, count=None, n=None):
    """one pisces_hip_vqr_apply_device: (the rows afterwards, rows rewritten)"""
    n = len(recs) if n is None else n
    d_recs = upload(torch, c, recs)
    d_sus = None if suspect is None else upload(torch, c, np.asarray(suspect, dtype=np.uint8))
    with torch.cuda.stream(c.torch_stream()):
        d_changed = torch.zeros(1, dtype=torch.int64, device=d_recs.device)
        d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device=d_recs.device)
    c.synchronize()
    c.vqr_apply_device(d_recs, n, R.struct_of_tables(T), lib_options(o), d_count=d_count, d_suspect=d_sus, d_n_changed=d_changed)
    c.synchronize()
    return d_recs.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE).copy(), int(d_changed.cpu()[0])


def by_chromosome(vcf):
    out = []
    for v in G["vcfs"][vcf]:
        if not out or out[-1][0] != v["chrom"]:
            out.append((v["chrom"], []))
        out[-1][1].append(R.row_of_vcf(v))
    return out


# ---- the reference's known answers through the device --------------------------------------------------------------------------------
def test_golden_dirty_vcf_through_the_device(torch_cuda, caller):
    """TestWithArtifacts.vcf + Dirty.counts -> ExpectedDirty.vcf.recal (RecalTests.RecalibrateDirtyVcf): host tables, device update"""
    from pisces_amd import engine
    o = R.options(**G["options"]["RecalibrateDirtyVcf"])
    c = G["counts"]["Dirty.counts"]
    tables = engine.vqr_tables(engine.vqr_counts_array([(c["by_category"], c["num_possible_variants"]), ([0] * 16, 0)]), lib_options(o))
    rows = [R.row_of_vcf(v) for v in G["vcfs"]["TestWithArtifacts.vcf"]]
    recs = R.records_of_rows(rows)
    got, changed = device_apply(torch_cuda, caller, recs, None, o, R.tables_of_struct(tables))
    exp = R.fields_of_rows([R.row_of_vcf(v) for v in G["vcfs"]["ExpectedDirty.vcf.recal"]])
    assert [(int(r["variant_qscore"]), int(r["genotype_qscore"]), int(r["noise_level"]), int(r["filter_bits"])) for r in got] == exp
    untouched = [i for i in range(len(rows)) if R.fields_of_rows([rows[i]])[0] == exp[i]]
    assert changed == 3 and len(untouched) == 7
    assert all(got[i].tobytes() == recs[i].tobytes() for i in untouched)
    assert R.write_back(recs, [R.row_of_vcf(v) for v in G["vcfs"]["ExpectedDirty.vcf.recal"]]).tobytes() == got.tobytes()


def test_golden_edge_example_through_the_device(torch_cuda, caller):
    """TestEdgeExample.vcf end to end with -extentofedgeregion 2 -> ExpectedEdgeExample.vcf.recal (EdgeIssueRecalTests): a chromosome a call,
    one pair of counters, the library's tables, rates of int.MinValue among them"""
    from pisces_amd import engine
    o = R.options(**G["options"]["RecalibrateDirtyVcfs"])
    d_counts = zero_counts(torch_cuda, caller)
    per = []
    for _, rows in by_chromosome("TestEdgeExample.vcf"):
        recs = R.records_of_rows(rows)
        _, sus = device_count(torch_cuda, caller, recs, o, d_counts=d_counts)
        per.append((recs, sus))
    tables = engine.vqr_tables(engine.vqr_counts_array(pair_of(d_counts)), lib_options(o))
    T = R.tables_of_struct(tables)
    assert R.INT_MIN in T["edge_risk"].values()
    got = []
    for recs, sus in per:
        after, _ = device_apply(torch_cuda, caller, recs, sus, o, T)
        got += [(int(r["variant_qscore"]), int(r["genotype_qscore"]), int(r["noise_level"]), int(r["filter_bits"])) for r in after]
        same = [i for i in range(len(recs)) if after[i]["variant_qscore"] == recs[i]["variant_qscore"] and after[i]["noise_level"] == recs[i]["noise_level"]]
        assert all(after[i].tobytes() == recs[i].tobytes() for i in same)
    exp = R.fields_of_rows([R.row_of_vcf(v) for v in G["vcfs"]["ExpectedEdgeExample.vcf.recal"]])
    assert len(got) == 24 and got == exp


# ---- counts and suspect bytes == statement -------------------------------------------------------------------------------------------
def check_count(torch, c, rows, extent, lo=0, hi=None):
    hi = len(rows) if hi is None else hi
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=extent)
    basic, edge, s = R.strain(rows, extent, True, lo, hi)
    pair, sus = device_count(torch, c, R.records_of_rows(rows), o, lo, hi)
    assert pair == R.counts_pair(basic, edge), (len(rows), extent, lo, hi)
    assert list(sus[lo:hi]) == s[lo:hi], (len(rows), extent, lo, hi)
    assert (sus[:lo] == SENTINEL).all() and (sus[hi:] == SENTINEL).all()   # only the counted rows get a byte
    return s


def test_counts_at_the_sizes_around_a_wave_and_a_workgroup(torch_cuda, caller):
    rng = np.random.default_rng(31)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025):
        for extent in (2, 4):
            check_count(torch_cuda, caller, vqr_cases.make_rows(rng, n), extent)
    check_count(torch_cuda, caller, vqr_cases.make_rows(rng, 700), 64)
    check_count(torch_cuda, caller, vqr_cases.make_rows(rng, 300), 0)
    check_count(torch_cuda, caller, vqr_cases.make_rows(rng, 300), 1)


def flat_rows(n, ref="C", alt="T", coverage=100):
    return [{"position": 1000 + i, "total_coverage": coverage, "allele_support": 10, "variant_qscore": 100, "genotype_qscore": 100, "noise_level": 20,
             "filter_bits": 0, "type": "Snv", "ref": ref, "alt": alt} for i in range(n)]


def test_windows_that_straddle_a_wave_and_a_workgroup_boundary(torch_cuda, caller):
    """a coverage drop at row 64 and one at row 256: the rows two before and behind each are at an edge, through the wave and the workgroup"""
    rows = flat_rows(600)
    rows[64]["total_coverage"] = 10
    rows[256]["total_coverage"] = 10
    s = check_count(torch_cuda, caller, rows, 2)
    inner = [i for i in range(2, 598) if s[i]]
    assert inner == [62, 63, 65, 66, 254, 255, 257, 258]
    # and a jump in position between rows 63 | 64 and 255 | 256
    rows = flat_rows(600)
    for i in range(64, 600):
        rows[i]["position"] += 7
    for i in range(256, 600):
        rows[i]["position"] += 7
    s = check_count(torch_cuda, caller, rows, 4)
    assert [i for i in range(4, 596) if s[i]] == list(range(60, 68)) + list(range(252, 260))


def test_equal_position_run_across_the_wave_boundary_in_the_update(torch_cuda, caller):
    """five rows of one position over rows 62..66 (and 254..258), one suspect among them: every one of the five takes the edge update, the
    neighbours at other positions do not — the scan for a suspect at the position crosses the wave and the workgroup"""
    rows = flat_rows(600, coverage=400)
    for lo in (62, 254):
        for i in range(lo, lo + 5):
            rows[i]["position"] = rows[lo]["position"]
        for i in range(lo + 5, 600):
            rows[i]["position"] -= 4
    suspect = [0] * 600
    suspect[66] = 1
    suspect[254] = 1
    o = R.options(do_amplicon_position_checks=1)
    T = {"basic": {}, "edge": {"CtoT": 9}, "edge_risk": {k: 15 for k in R.SNV_CATEGORIES}}
    got, changed = device_apply(torch_cuda, caller, R.records_of_rows(rows), suspect, o, T)
    exp = [dict(r) for r in rows]
    R.apply(o, T, exp, suspect)
    assert got.tobytes() == R.write_back(R.records_of_rows(rows), exp).tobytes()
    assert changed == 10 and [i for i in range(600) if got[i]["noise_level"] == 15] == list(range(62, 67)) + list(range(254, 259))


def test_count_word_below_n_with_garbage_behind_it(torch_cuda, caller):
    """*d_count = 320 under n = 4097: rows beyond the count are 0xFF bytes and are neither read nor written, by either kernel"""
    rng = np.random.default_rng(8)
    rows = vqr_cases.make_rows(rng, 320, snv_share=0.8)
    recs = np.zeros(4097, dtype=_abi.CALLED_ALLELE_DTYPE)
    recs.view(np.uint8)[:] = 0xFF
    recs[:320] = R.records_of_rows(rows)
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=4)
    basic, edge, s = R.strain(rows, 4, True)
    pair, sus = device_count(torch_cuda, caller, recs, o, count=320)
    assert pair == R.counts_pair(basic, edge) and list(sus[:320]) == s and (sus[320:] == SENTINEL).all()
    T = {"basic": {"CtoT": 12, "AtoG": 7}, "edge": {k: 9 for k in R.SNV_CATEGORIES}, "edge_risk": {k: 14 for k in R.SNV_CATEGORIES}}
    full_sus = np.full(4097, 1, dtype=np.uint8)
    full_sus[:320] = s
    got, changed = device_apply(torch_cuda, caller, recs, full_sus, o, T, count=320)
    exp = [dict(r) for r in rows]
    R.apply(o, T, exp, s)
    assert got[:320].tobytes() == R.write_back(recs[:320], exp).tobytes()
    assert (got[320:].view(np.uint8) == 0xFF).all()
    assert changed == sum(1 for r in exp if r.get("rewritten")) and changed > 50
    # a negative count word is no rows
    pair, sus = device_count(torch_cuda, caller, recs, o, count=-5)
    assert pair == R.counts_pair(R.new_counts(), R.new_counts()) and (sus == SENTINEL).all()


def test_two_calls_accumulate_and_sub_ranges_with_halo_rows_equal_one_call(torch_cuda, caller):
    rng = np.random.default_rng(12)
    extent = 4
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=extent)
    a, b = vqr_cases.make_rows(rng, 300), vqr_cases.make_rows(rng, 517)
    d_counts = zero_counts(torch_cuda, caller)
    device_count(torch_cuda, caller, R.records_of_rows(a), o, d_counts=d_counts)
    pair, _ = device_count(torch_cuda, caller, R.records_of_rows(b), o, d_counts=d_counts)
    basic, edge = R.new_counts(), R.new_counts()
    R.strain(a, extent, True, basic=basic, edge=edge)
    R.strain(b, extent, True, basic=basic, edge=edge)
    assert pair == R.counts_pair(basic, edge)
    # one chromosome in two pieces over the whole buffer
    whole_pair, whole_sus = device_count(torch_cuda, caller, R.records_of_rows(b), o)
    d_counts = zero_counts(torch_cuda, caller)
    _, s1 = device_count(torch_cuda, caller, R.records_of_rows(b), o, 0, 250, d_counts=d_counts)
    pair, s2 = device_count(torch_cuda, caller, R.records_of_rows(b), o, 250, 517, d_counts=d_counts)
    assert pair == whole_pair and list(s1[:250]) + list(s2[250:]) == list(whole_sus)
    # and streamed: each piece with `extent` halo rows of the other
    d_counts = zero_counts(torch_cuda, caller)
    _, s1 = device_count(torch_cuda, caller, R.records_of_rows(b[:250 + extent]), o, 0, 250, d_counts=d_counts)
    pair, s2 = device_count(torch_cuda, caller, R.records_of_rows(b[250 - extent:]), o, extent, 517 - 250 + extent, d_counts=d_counts)
    assert pair == whole_pair and list(s1[:250]) + list(s2[extent:]) == list(whole_sus)


def test_twenty_repeats_are_bit_identical(torch_cuda, caller):
    rng = np.random.default_rng(3)
    rows = vqr_cases.make_rows(rng, 3000)
    recs = R.records_of_rows(rows)
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=4)
    first = device_count(torch_cuda, caller, recs, o)
    for _ in range(19):
        again = device_count(torch_cuda, caller, recs, o)
        assert again[0] == first[0] and again[1].tobytes() == first[1].tobytes()


# ---- the update == statement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_qscore", [66, 120])
@pytest.mark.parametrize("filter_qscore", [-1, 0, 30])
def test_apply_matches_statement_on_seeded_rows(torch_cuda, caller, max_qscore, filter_qscore):
    """4 000 rows, most of them SNVs, a third or more in a table: supports 0..2000, depths 0..5000, VariantQscore 0 and 1 among the scores,
    rows that have the bit already, rates of int.MinValue in the edge-risk table"""
    rng = np.random.default_rng(1000 * max_qscore + filter_qscore + 7)
    rows = vqr_cases.make_rows(rng, 4000, snv_share=0.85, qscores=[0, 1, 2, 30, 66, 100, 130, 666], depths=[0, 1, 10, 100, 5000])
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=2, max_qscore=max_qscore, filter_qscore=filter_qscore)
    _, _, suspect = R.strain(rows, 2, True)
    T = {"basic": {"CtoT": 12, "GtoA": 20, "AtoC": 3, "TtoG": -4}, "edge": {"CtoT": 9, "CtoA": 9, "TtoC": 9, "GtoT": 9, "AtoG": 0},
         "edge_risk": {k: v for k, v in zip(R.SNV_CATEGORIES, [11, R.INT_MIN, 18, 13, R.INT_MIN, 6, 25, 0, R.INT_MIN, 40, 4, -3])}}
    recs = R.records_of_rows(rows)
    got, changed = device_apply(torch_cuda, caller, recs, suspect, o, T)
    exp = [dict(r) for r in rows]
    R.INT_MIN_REACHED_POISSON[0] = 0
    R.apply(o, T, exp, suspect)
    want = R.write_back(recs, exp)
    diff = [i for i in range(len(rows)) if got[i].tobytes() != want[i].tobytes()]
    assert not diff, (len(diff), [(rows[i], R.fields_of_rows([exp[i]]), got[i]) for i in diff[:3]])
    assert R.INT_MIN_REACHED_POISSON[0] == 0
    assert 3 * sum(1 for r in rows if R.update_category(r) in set(T["basic"]) | set(T["edge"])) >= len(rows)   # a third are SNVs in a table
    touched = sum(1 for a, b in zip(rows, exp) if R.fields_of_rows([a]) != R.fields_of_rows([b]))
    assert touched > 800 and changed == sum(1 for r in exp if r.get("rewritten")) >= touched
    assert any(r["noise_level"] == R.INT_MIN for r in exp)


def test_tables_with_no_category_launch_nothing_and_change_nothing(torch_cuda, caller):
    rows = flat_rows(300)
    recs = R.records_of_rows(rows)
    got, changed = device_apply(torch_cuda, caller, recs, None, R.options(), {"basic": {}, "edge": {}, "edge_risk": None})
    assert got.tobytes() == recs.tobytes() and changed == 0


def test_device_refusals(torch_cuda, caller):
    import ctypes as C
    from pisces_amd import engine
    lib = engine.lib
    d = zero_counts(torch_cuda, caller)
    recs = upload(torch_cuda, caller, R.records_of_rows(flat_rows(10)))
    o = engine.vqr_options(do_amplicon_position_checks=1)
    t = R.struct_of_tables({"basic": {}, "edge": {"CtoT": 9}, "edge_risk": {k: 9 for k in R.SNV_CATEGORIES}})
    h = caller._h
    err = lambda: lib.pisces_hip_last_error(h).decode()
    assert lib.pisces_hip_vqr_count_device(h, None, recs.data_ptr(), 10, None, 0, 10, d.data_ptr(), None, None) == _abi.E_INVALID_ARG and "null" in err()
    assert lib.pisces_hip_vqr_count_device(h, C.byref(o), recs.data_ptr(), 10, None, 0, 10, None, None, None) == _abi.E_INVALID_ARG and "null" in err()
    assert lib.pisces_hip_vqr_count_device(h, C.byref(o), recs.data_ptr(), 10, None, 0, 10, d.data_ptr(), None, None) == _abi.E_INVALID_ARG and "suspect" in err()
    assert lib.pisces_hip_vqr_count_device(h, C.byref(o), recs.data_ptr(), 10, None, 3, 11, d.data_ptr(), recs.data_ptr(), None) == _abi.E_INVALID_ARG and "rows [" in err()
    bad = engine.vqr_options(extent_of_edge_region=65)
    assert lib.pisces_hip_vqr_count_device(h, C.byref(bad), recs.data_ptr(), 10, None, 0, 10, d.data_ptr(), None, None) == _abi.E_INVALID_ARG and "extent_of_edge_region" in err()
    assert lib.pisces_hip_vqr_apply_device(h, C.byref(o), None, recs.data_ptr(), 10, None, None, None, None) == _abi.E_INVALID_ARG and "null" in err()
    assert lib.pisces_hip_vqr_apply_device(h, C.byref(o), C.byref(t), recs.data_ptr(), 10, None, None, None, None) == _abi.E_INVALID_ARG and "suspect" in err()
    t.has_edge_risk = 0
    assert lib.pisces_hip_vqr_apply_device(h, C.byref(o), C.byref(t), recs.data_ptr(), 10, None, recs.data_ptr(), None, None) == _abi.E_INVALID_ARG and "edge-risk" in err()
    caller.synchronize()
    assert pair_of(d) == R.counts_pair(R.new_counts(), R.new_counts())   # a refused call counts nothing


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def test_chain_from_tuples_through_vqr_to_text(torch_cuda):
    """2000 loci of synthetic reads with a C>T artefact planted (one C observation in sixteen reads T) -> call_tiles -> compact_records ->
    count / tables / apply -> format_vcf_device, against the host formatter over the statement applied to the rows copied back; and the
    text without the three VQR calls is the old text"""
    torch = torch_cuda
    from pisces_amd import engine, synth
    p = synth.make_pileup(n_loci=2000, depth=100, seed=5, device="cpu", snv_every=10 ** 6)
    t = p.tuples.to(torch.int64) & 0xFFFFFFFF
    g = torch.Generator()
    g.manual_seed(11)
    flip = (((t >> 10) & 7) == _abi.ALLELE_C) & (t != 0xFFFFFFFF) & (torch.rand(t.shape, generator=g) < 1.0 / 16)
    t = torch.where(flip, (t & ~(7 << 10)) | (_abi.ALLELE_T << 10), t)
    tuples = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).contiguous()
    o = R.options(do_amplicon_position_checks=1, extent_of_edge_region=4)
    vcf = dict(output_strand_bias_and_noise_level=1, noise_level_from_records=1)
    with engine.HipVariantCaller(_abi.default_config()) as c:
        ts, dev = c.torch_stream(), torch.device("cuda", c.device)
        cap = p.n_tiles * _abi.SLOTS_PER_TILE
        with torch.cuda.stream(ts):
            d_tup, d_tiles, d_ref = tuples.to(dev), p.tiles.to(dev), p.ref.to(dev)
            recs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
            tres = torch.zeros(p.n_tiles * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            out_d = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
            offs = torch.zeros(p.n_tiles, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            d_sus = torch.zeros(cap, dtype=torch.uint8, device=dev)
            d_counts = torch.zeros(34, dtype=torch.int64, device=dev)
        c.synchronize()
        c.call_tiles(d_tup.data_ptr(), d_tiles.data_ptr(), p.n_tiles, d_ref.data_ptr(), p.ref_start, p.ref_len, recs.data_ptr(), cap, tres.data_ptr(), ts)
        c.compact_records(recs.data_ptr(), tres.data_ptr(), p.n_tiles, offs.data_ptr(), out_d.data_ptr(), cap, count.data_ptr(), ts)
        old_text = c.format_vcf_device("chr7", out_d, cap, d_count=count, stream=ts, **vcf)          # a caller that skips VQR
        c.vqr_count_device(out_d, cap, d_counts, lib_options(o), d_count=count, d_suspect=d_sus, stream=ts)
        c.synchronize()
        n = int(count.cpu()[0])
        before = out_d.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy()
        tables = engine.vqr_tables(engine.vqr_counts_array(pair_of(d_counts)), lib_options(o))        # the one host step: 34 words back
        c.vqr_apply_device(out_d, cap, tables, lib_options(o), d_count=count, d_suspect=d_sus, stream=ts)
        new_text = c.format_vcf_device("chr7", out_d, cap, d_count=count, stream=ts, **vcf)
    assert old_text == engine.format_vcf("chr7", before, **vcf).encode()
    rows = R.rows_of_records(before)
    assert n >= 2000 and sum(1 for r in rows if R.count_category(r) == "CtoT") > 300   # (a variant's row stands in for its locus' Reference row)
    basic, edge, suspect = R.strain(rows, 4, True)
    assert pair_of(d_counts) == R.counts_pair(basic, edge)
    T = R.tables(o, basic, edge)
    assert "CtoT" in T["basic"] and R.tables_of_struct(tables)["basic"] == T["basic"]   # the planted artefact is what the counts single out
    R.apply(o, T, rows, suspect)
    want = engine.format_vcf("chr7", R.write_back(before, rows), **vcf).encode()
    assert new_text == want and new_text != old_text
