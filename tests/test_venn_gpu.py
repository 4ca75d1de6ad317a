"""VennVcf's consensus of two probe pools on the GPU (pisces_hip_venn_consensus_device): every comparison is against the host entry
(pisces_hip_venn_consensus), which tests/test_venn_cpu.py pins to the plain-Python statement and to the reference's own known answers.
Rows, cand_index, candidates, allele bytes, the info's integers and the Venn bytes are compared byte for byte; pool_bias_score /
pool_bias_gatk at the project's rtol for the strand-bias score (tests/test_gpu_parity.py: 1e-9).  The shapes are those at which the three
kernels can go wrong: group heads and multi-row groups around lane 63/64 and row 255/256 in A, in B and in both, positions only in one pool
before, between and behind the other's, an empty pool, a count word below n with garbage behind it, capacities one short and exact."""
import ctypes as C

import numpy as np
import pytest

from pisces_amd import _abi
from tests import venn_cases as V
from tests import venn_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
G = V.GOLDEN


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
        return torch.from_numpy(np.frombuffer(bytes(arr) if isinstance(arr, C.Array) else np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()).to(
            torch.device("cuda", c.device))


class Buffers:
    """device output buffers filled with a sentinel, and what a call left in them"""
    def __init__(self, torch, c, caps, n_a, n_b):
        self.caps = caps
        dev = torch.device("cuda", c.device)
        with torch.cuda.stream(c.torch_stream()):
            full = lambda nbytes: torch.full((max(nbytes, 1) + 16,), SENTINEL, dtype=torch.uint8, device=dev)
            self.recs, self.cand_index, self.cands, self.alleles = full(caps[0] * 64), full(caps[0] * 4), full(caps[1] * 56), full(caps[2])
            self.info, self.venn_a, self.venn_b, self.n_out = full(caps[0] * 32), full(n_a), full(n_b), full(24)

    def out(self):
        from pisces_amd import engine
        return engine.venn_out(self.recs, self.cand_index, self.cands, self.alleles, self.n_out, self.caps[0], self.caps[1], self.caps[2], info=self.info,
                               venn_a=self.venn_a, venn_b=self.venn_b)

    def raw(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("recs", "cand_index", "cands", "alleles", "info", "venn_a", "venn_b", "n_out")}


def device_pool(torch, c, recs, alleles, n=None, count=None, with_table=True):
    """(PiscesVennRows, keep-alive) of rows uploaded with their candidate table"""
    from pisces_amd import engine
    d_recs = upload(torch, c, recs) if len(recs) else None
    keep = [d_recs]
    table = [None, None, None]
    if with_table and alleles is not None:
        idx, cands, pool = engine.candidate_table(recs[:len(alleles)], alleles)
        if len(idx) < len(recs):
            idx = np.concatenate([idx, np.full(len(recs) - len(idx), 0x5A5A5A5A, dtype=np.int32)])   # garbage behind the count
        table = [upload(torch, c, idx) if len(idx) else None, upload(torch, c, cands), upload(torch, c, pool)]
        keep += table
    d_count = None
    if count is not None:
        with torch.cuda.stream(c.torch_stream()):
            d_count = torch.tensor([count], dtype=torch.int32, device=torch.device("cuda", c.device))
        keep.append(d_count)
    return engine.venn_rows(d_recs, len(recs) if n is None else n, d_count, *table), keep


def gather(raw, n_a, n_b):
    """what the device left, in the shape engine.venn_consensus returns"""
    n, nc, nb = (int(x) for x in raw["n_out"][:24].view(np.int64))
    fit = min(max(n, 0), len(raw["recs"]) // 64)   # (a call whose counts exceed the capacities wrote nothing: the views stay inside the buffers)
    recs = raw["recs"][:fit * 64].view(_abi.CALLED_ALLELE_DTYPE)
    cand_index = raw["cand_index"][:fit * 4].view(np.int32)
    cands = raw["cands"][:max(nc, 0) * 56]
    pool = raw["alleles"][:max(nb, 0)]
    info = raw["info"][:fit * 32].view(_abi.CONSENSUS_INFO_DTYPE)
    return {"records": recs, "cand_index": cand_index, "cands_bytes": cands, "allele_bytes": pool, "info": info, "venn_a": raw["venn_a"][:n_a], "venn_b": raw["venn_b"][:n_b],
            "n_out": (n, nc, nb)}


def assert_device_is_host(dev, host, where=""):
    assert dev["n_out"] == host["n_out"], (where, dev["n_out"], host["n_out"])
    n, nc, nb = host["n_out"]
    assert dev["records"].tobytes() == host["records"].tobytes(), (where, "rows", [i for i in range(n) if dev["records"][i].tobytes() != host["records"][i].tobytes()][:5])
    assert dev["cand_index"].tolist() == host["cand_index"].tolist(), where
    assert dev["cands_bytes"].tobytes() == bytes(host["cands"])[:nc * 56], where
    assert dev["allele_bytes"].tobytes() == host["allele_bytes"].tobytes(), where
    for k in ("row_a", "row_b", "comparison_case", "alt_changed_to_ref"):
        assert dev["info"][k].tolist() == host["info"][k].tolist(), (where, k)
    for k in ("pool_bias_score", "pool_bias_gatk"):
        np.testing.assert_allclose(dev["info"][k], host["info"][k], rtol=1e-9, atol=0, err_msg=str((where, k)))
    assert dev["venn_a"].tolist() == host["venn_a"].tolist() and dev["venn_b"].tolist() == host["venn_b"].tolist(), where


def untouched(raw, caps_used=(0, 0, 0)):
    """no byte behind what a call may write differs from the sentinel (caps_used = (0, 0, 0): no byte at all, n_out aside)"""
    n, nc, nb = caps_used
    return all((raw[k][start:] == SENTINEL).all() for k, start in (("recs", n * 64), ("cand_index", n * 4), ("cands", nc * 56), ("alleles", nb), ("info", n * 32)))


def run_device(torch, c, rows_a, rows_b, o, caps=None, with_table=(True, True), garbage=(0, 0)):
    """both entries over the same rows: (device result, host result, raw buffers).  garbage = rows of junk appended behind each pool and
    hidden by a count word."""
    from pisces_amd import engine
    recs_a, alleles_a = V.records_of(rows_a)
    recs_b, alleles_b = V.records_of(rows_b)
    host = engine.venn_consensus(recs_a, recs_b, V.options_struct(o), alleles_a if with_table[0] else None, alleles_b if with_table[1] else None)
    pools, keep = [], []
    for recs, alleles, table, junk in ((recs_a, alleles_a, with_table[0], garbage[0]), (recs_b, alleles_b, with_table[1], garbage[1])):
        count = None
        if junk:
            count = len(recs)
            recs = np.concatenate([recs, np.frombuffer(np.random.default_rng(junk).bytes(64 * junk), dtype=_abi.CALLED_ALLELE_DTYPE)])
        p, k = device_pool(torch, c, recs, alleles, count=count, with_table=table)
        pools.append(p)
        keep.append(k)
    caps = caps if caps is not None else host["n_out"]
    buf = Buffers(torch, c, caps, len(rows_a) + garbage[0], len(rows_b) + garbage[1])
    c.synchronize()
    c.venn_consensus_device(pools[0], pools[1], buf.out(), V.options_struct(o))
    c.synchronize()
    raw = buf.raw()
    return gather(raw, len(rows_a), len(rows_b)), host, raw


# ---- the reference's known answers through the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(G["pairs"]))
def test_every_golden_pair_through_the_device(torch_cuda, caller, pair):
    """a chromosome a call; the device's consensus is the host entry's, and where the reference has an expected file its lines hold for the
    device's rows: QUAL, FILTER, DP, GT, GQ, AD, NL, PB (|difference| <= 5e-5 + 1e-9), VF0..DP1's AD / DP"""
    p = G["pairs"][pair]
    o = V.options_of(p["options"])
    rows_a, rows_b = V.rows_of_file(p["a"]), V.rows_of_file(p["b"])
    expected = G["files"][p["expected"]] if p["expected"] else None
    lines_checked = 0
    for chrom in V.chromosomes(rows_a, rows_b) or [None]:
        a, b = [r for r in rows_a if r["chrom"] == chrom], [r for r in rows_b if r["chrom"] == chrom]
        dev, host, raw = run_device(torch_cuda, caller, a, b, o)
        assert_device_is_host(dev, host, (pair, chrom))
        assert untouched(raw, host["n_out"])
        if expected is not None:
            dev["alleles"] = host["alleles"]   # (the strings: candidates and bytes were compared above)
            lines = [ln for ln in expected if ln["chrom"] == chrom]
            cons = V.written_order(V.dicts_of(dev))
            assert len(cons) == len(lines)
            for cns, line in zip(cons, lines):
                V.assert_line(cns, a, b, line, p.get("debug"), (pair, chrom, line["line"]))
                lines_checked += 1
    assert expected is None or lines_checked == len(expected)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
def _single(position, k=0):
    return {"position": position, "ref": "A", "alt": ".", "type": "Reference", "genotype": "HomozygousRef", "total_coverage": 900 + k, "allele_support": 890,
            "reference_support": 890, "variant_qscore": 100, "genotype_qscore": 100, "noise_level": 20, "filters": 0, "sb": 1e-10}


def _group(position, alts, depth=4000, support=300):
    return [{"position": position, "ref": r, "alt": a, "type": R.set_type(r, a), "genotype": "HeterozygousAltRef", "total_coverage": depth, "allele_support": support + 7 * k,
             "reference_support": depth - support - 7 * k, "variant_qscore": 100, "genotype_qscore": 90, "noise_level": 20, "filters": 0, "sb": 1e-10}
            for k, (r, a) in enumerate(alts)]


@pytest.mark.parametrize("at_a,at_b", [(62, 0), (63, 3), (254, 1), (255, 0), (0, 63), (2, 255), (63, 63), (255, 255), (63, 255), (254, 62), (511, 767)])
def test_groups_that_straddle_a_wave_and_a_workgroup_boundary(torch_cuda, caller, at_a, at_b):
    """a three-row group whose head sits at row at_a of pool A and at_b of pool B (lane 62..63 and row 254..255: the group crosses a wave
    or a workgroup; its members agree in part), single rows before and behind it"""
    alts_a, alts_b = [("A", "T"), ("A", "ATG"), ("AC", "TT")], [("A", "ATG"), ("A", "G"), ("AC", "TT")]
    rows_a = [_single(10 + i) for i in range(at_a)] + _group(5000, alts_a) + [_single(6000 + i, i) for i in range(70)]
    rows_b = [_single(10 + 2 * i) for i in range(at_b)] + _group(5000, alts_b, 3000, 200) + [_single(6000 + 3 * i, i) for i in range(40)]
    dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, R.default_options(min_frequency_filter=0.03))
    assert_device_is_host(dev, host, (at_a, at_b))
    assert untouched(raw, host["n_out"]) and host["n_out"][1] == 2
    assert sorted(host["venn_a"][at_a:at_a + 3].tolist()) == [1, 1, 2]


def test_positions_in_one_pool_only_before_between_and_behind_the_others(torch_cuda, caller):
    rng = np.random.default_rng(4242)
    for flip in (False, True):
        rows_a = [_single(p) for p in range(100, 400)] + _group(450, [("A", "T"), ("A", "AT")]) + [_single(p) for p in range(1000, 1300)] + [_single(p) for p in range(5000, 5300)]
        rows_b = [_single(p, 3) for p in range(500, 900)] + [_single(p, 3) for p in range(1100, 1150)] + _group(1200, [("ACC", "A")]) + [_single(p, 3) for p in range(2000, 2600)]
        if flip:
            rows_a, rows_b = rows_b, rows_a
        dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, R.default_options())
        assert_device_is_host(dev, host, flip)
        assert dev["records"]["position"].tolist() == sorted(dev["records"]["position"].tolist())
    rows_a, rows_b = V.make_pools(rng, 700)
    for o in (R.default_options(min_frequency_filter=0.03), R.default_options(min_frequency_filter=0.03, combine_qscore_method=1)):
        dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, o)
        assert_device_is_host(dev, host, "seeded")
        assert untouched(raw, host["n_out"]) and len(rows_a) > 512 and len(rows_b) > 512


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_one_pool_empty(torch_cuda, caller, which):
    rows = [_single(p) for p in range(1, 300)] + _group(400, [("A", "T"), ("AC", "A")])
    rows_a, rows_b = ([] if which in ("a", "both") else rows), ([] if which in ("b", "both") else rows)
    dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, R.default_options())
    assert_device_is_host(dev, host, which)
    assert host["n_out"][0] == len(rows_a) + len(rows_b) and untouched(raw, host["n_out"])


def test_count_word_below_n_with_garbage_behind_it(torch_cuda, caller):
    rows_a, rows_b = V.make_pools(np.random.default_rng(31), 200)
    dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, R.default_options(min_frequency_filter=0.03), garbage=(77, 300))
    assert_device_is_host(dev, host)
    assert (raw["venn_a"][len(rows_a):len(rows_a) + 77] == SENTINEL).all() and (raw["venn_b"][len(rows_b):len(rows_b) + 300] == SENTINEL).all()


def test_capacities_one_short_report_the_counts_and_write_nothing(torch_cuda, caller):
    rows_a, rows_b = V.make_pools(np.random.default_rng(32), 300)
    o = R.default_options(min_frequency_filter=0.03)
    dev, host, raw = run_device(torch_cuda, caller, rows_a, rows_b, o)           # the exact capacities
    assert_device_is_host(dev, host)
    assert untouched(raw, host["n_out"]) and min(host["n_out"]) > 0
    for k in range(3):
        caps = list(host["n_out"])
        caps[k] -= 1
        dev, _, raw = run_device(torch_cuda, caller, rows_a, rows_b, o, caps=tuple(caps))
        assert dev["n_out"] == host["n_out"], k
        assert untouched(raw) and (raw["venn_a"] == SENTINEL).all() and (raw["venn_b"] == SENTINEL).all(), k


def test_candidate_tables_in_one_pool_only(torch_cuda, caller):
    """pool B comes without cand_index (single-base rows only): its alleles are the base codes of info, compared with A's candidate bytes"""
    snvs = [("A", "T"), ("A", "G")]
    rows_a = [_single(p) for p in range(1, 100)] + _group(200, [("A", "T"), ("A", "ATG")]) + _group(201, [("AC", "A")]) + _group(202, [("A", "G")])
    rows_b = [_single(p) for p in range(50, 150)] + _group(200, snvs) + [_single(201)] + _group(202, [("A", "G")])
    for flip in (False, True):
        a, b = (rows_b, rows_a) if flip else (rows_a, rows_b)
        dev, host, raw = run_device(torch_cuda, caller, a, b, R.default_options(), with_table=(not flip, flip))
        assert_device_is_host(dev, host, flip)
        assert host["n_out"][1] == 2 and 1 in host["venn_a"].tolist()


def test_unsorted_pool_is_an_error_word_and_nothing_is_written(torch_cuda, caller):
    rows = [_single(p) for p in range(1, 600)]
    bad = list(rows)
    bad[300], bad[301] = bad[301], bad[300]
    bad[500], bad[501] = bad[501], bad[500]
    for a, b, pool in ((bad, rows, 0), (rows, bad, 1)):
        recs_a, recs_b = V.records_of(a)[0], V.records_of(b)[0]
        pa, ka = device_pool(torch_cuda, caller, recs_a, None)
        pb, kb = device_pool(torch_cuda, caller, recs_b, None)
        buf = Buffers(torch_cuda, caller, (2000, 10, 10), len(a), len(b))
        caller.synchronize()
        caller.venn_consensus_device(pa, pb, buf.out(), V.options_struct(R.default_options()))
        caller.synchronize()
        raw = buf.raw()
        assert raw["n_out"][:24].view(np.int64).tolist() == [_abi.E_INVALID_ARG, pool, 301]   # the lowest offending row decides
        assert untouched(raw) and (raw["venn_a"] == SENTINEL).all() and (raw["venn_b"] == SENTINEL).all()


def test_a_second_call_on_the_stream_overwrites_the_first(torch_cuda, caller):
    """two calls, one stream, one set of buffers, no wait in between: nothing accumulates"""
    from pisces_amd import engine
    big_a, big_b = V.make_pools(np.random.default_rng(33), 400)
    small_a, small_b = V.make_pools(np.random.default_rng(34), 90)
    o = R.default_options(min_frequency_filter=0.03)
    pools, keep = [], []
    for rows in (big_a, big_b, small_a, small_b):
        recs, alleles = V.records_of(rows)
        p, k = device_pool(torch_cuda, caller, recs, alleles)
        pools.append(p)
        keep.append(k)
    host_big = engine.venn_consensus(*[x for rows in (big_a, big_b) for x in [V.records_of(rows)[0]]], V.options_struct(o), V.records_of(big_a)[1], V.records_of(big_b)[1])
    host = engine.venn_consensus(V.records_of(small_a)[0], V.records_of(small_b)[0], V.options_struct(o), V.records_of(small_a)[1], V.records_of(small_b)[1])
    buf = Buffers(torch_cuda, caller, host_big["n_out"], len(big_a), len(big_b))
    caller.synchronize()
    caller.venn_consensus_device(pools[0], pools[1], buf.out(), V.options_struct(o))
    caller.venn_consensus_device(pools[2], pools[3], buf.out(), V.options_struct(o))
    caller.synchronize()
    dev = gather(buf.raw(), len(small_a), len(small_b))
    assert_device_is_host(dev, host)
    assert host_big["n_out"][0] > host["n_out"][0]


def test_twenty_repeats_are_bit_identical(torch_cuda, caller):
    rows_a, rows_b = V.make_pools(np.random.default_rng(35), 500)
    o = R.default_options(min_frequency_filter=0.03)
    first = None
    recs_a, alleles_a = V.records_of(rows_a)
    recs_b, alleles_b = V.records_of(rows_b)
    pa, ka = device_pool(torch_cuda, caller, recs_a, alleles_a)
    pb, kb = device_pool(torch_cuda, caller, recs_b, alleles_b)
    for _ in range(20):
        buf = Buffers(torch_cuda, caller, (len(rows_a) + len(rows_b),) * 2 + (8 * (len(rows_a) + len(rows_b)),), len(rows_a), len(rows_b))
        caller.synchronize()
        caller.venn_consensus_device(pa, pb, buf.out(), V.options_struct(o))
        caller.synchronize()
        raw = buf.raw()
        blob = b"".join(raw[k].tobytes() for k in sorted(raw))
        first = first or blob
        assert blob == first


def test_device_refusals(torch_cuda, caller):
    from pisces_amd import engine
    lib, h = engine.lib, caller._h
    err = lambda: lib.pisces_hip_last_error(h).decode()
    recs = V.records_of([_single(p) for p in range(1, 20)])[0]
    pool, keep = device_pool(torch_cuda, caller, recs, None)
    buf = Buffers(torch_cuda, caller, (64, 4, 4), 19, 19)
    out = buf.out()
    call = lambda o, a, b, out_: lib.pisces_hip_venn_consensus_device(h, None if o is None else C.byref(o), None if a is None else C.byref(a),
                                                                      None if b is None else C.byref(b), None if out_ is None else C.byref(out_), None)
    opts = engine.venn_options()
    misaligned = engine.venn_rows(keep[0].data_ptr() + 8, 10)
    no_table = engine.venn_rows(keep[0], 19, cand_index=keep[0])
    for args, word in (((None, pool, pool, out), "options"), ((opts, None, pool, out), "pool A"), ((opts, pool, None, out), "pool B"), ((opts, pool, pool, None), "out"),
                       ((opts, engine.venn_rows(keep[0], -1), pool, out), "negative"), ((opts, engine.venn_rows(None, 3), pool, out), "null recs"),
                       ((opts, no_table, pool, out), "cand_index"), ((opts, misaligned, pool, out), "aligned"),
                       ((engine.venn_options(pool_bias_threshold=1.5), pool, pool, out), "pool_bias_threshold"),
                       ((engine.venn_options(min_frequency=-0.1), pool, pool, out), "min_frequency"),
                       ((engine.venn_options(combine_qscore_method=7), pool, pool, out), "combine_qscore_method")):
        assert call(*args) == _abi.E_INVALID_ARG, word
        assert word in err(), (word, err())
    caller.synchronize()
    raw = buf.raw()
    assert untouched(raw) and (raw["n_out"] == SENTINEL).all()   # a refused call launches nothing


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def test_chain_from_two_handles_tuples_to_text(torch_cuda):
    """two pools' synthetic reads over the same 2000 loci, a handle each -> call_tiles -> compact_records -> consensus -> vqr_count_device ->
    format_vcf_device, one stream, no host wait between the kernels.  The text equals the host formatter's over the host entry's consensus
    of the compacted rows copied back."""
    torch = torch_cuda
    from pisces_amd import engine, synth
    pa = synth.make_pileup(n_loci=2000, depth=100, seed=5, device="cpu", snv_every=40)   # one seed: one reference; the depth changes every later draw,
    pb = synth.make_pileup(n_loci=2000, depth=60, seed=5, device="cpu", snv_every=40)    # so the planted alternates agree at a third of the sites
    vcf = dict(output_strand_bias_and_noise_level=1, noise_level_from_records=1)
    o = engine.venn_options(min_frequency_filter=0.03)
    with engine.HipVariantCaller(_abi.default_config()) as ca, engine.HipVariantCaller(_abi.default_config()) as cb:
        ts, dev = ca.torch_stream(), torch.device("cuda", ca.device)
        side = []
        with torch.cuda.stream(ts):
            for p in (pa, pb):
                cap = p.n_tiles * _abi.SLOTS_PER_TILE
                side.append(dict(p=p, cap=cap, tup=p.tuples.to(dev), tiles=p.tiles.to(dev), ref=p.ref.to(dev), recs=torch.zeros(cap * 64, dtype=torch.uint8, device=dev),
                                 tres=torch.zeros(p.n_tiles * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                                 out=torch.zeros(cap * 64, dtype=torch.uint8, device=dev), offs=torch.zeros(p.n_tiles, dtype=torch.int32, device=dev),
                                 count=torch.zeros(1, dtype=torch.int32, device=dev)))
            cap = side[0]["cap"] + side[1]["cap"]
            d_rows = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
            d_idx = torch.zeros(cap, dtype=torch.int32, device=dev)
            d_cands = torch.zeros(56, dtype=torch.uint8, device=dev)
            d_bytes = torch.zeros(16, dtype=torch.uint8, device=dev)
            d_info = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
            d_n_out = torch.zeros(3, dtype=torch.int64, device=dev)
            d_counts = torch.zeros(34, dtype=torch.int64, device=dev)
        ca.synchronize()
        for c, s in zip((ca, cb), side):
            p = s["p"]
            c.call_tiles(s["tup"].data_ptr(), s["tiles"].data_ptr(), p.n_tiles, s["ref"].data_ptr(), p.ref_start, p.ref_len, s["recs"].data_ptr(), s["cap"], s["tres"].data_ptr(), ts)
            c.compact_records(s["recs"].data_ptr(), s["tres"].data_ptr(), p.n_tiles, s["offs"].data_ptr(), s["out"].data_ptr(), s["cap"], s["count"].data_ptr(), ts)
        rows_a = engine.venn_rows(side[0]["out"], side[0]["cap"], side[0]["count"])
        rows_b = engine.venn_rows(side[1]["out"], side[1]["cap"], side[1]["count"])
        ca.venn_consensus_device(rows_a, rows_b, engine.venn_out(d_rows, d_idx, d_cands, d_bytes, d_n_out, cap, 0, 0, info=d_info), o, stream=ts)
        # the consensus' row count is a count word for what follows: n_out[0]'s low half
        ca.vqr_count_device(d_rows, cap, d_counts, engine.vqr_options(), d_count=d_n_out, stream=ts)
        text = ca.format_vcf_device("chr7", d_rows, cap, d_count=d_n_out, d_cand_index=d_idx, d_cands=d_cands, d_alleles=d_bytes, stream=ts, **vcf)
        ca.synchronize()
        n_a, n_b = int(side[0]["count"].cpu()[0]), int(side[1]["count"].cpu()[0])
        host_a = side[0]["out"].cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n_a].copy()
        host_b = side[1]["out"].cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n_b].copy()
        n = int(d_n_out.cpu()[0])
        got_rows = d_rows.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy()
        counted = int(d_counts.cpu()[16])
    host = engine.venn_consensus(host_a, host_b, o)
    assert n == host["n_out"][0] >= 2000 and got_rows.tobytes() == host["records"].tobytes() and counted == n
    cases = host["info"]["comparison_case"].tolist()
    assert cases.count(0) > 1500 and cases.count(1) > 3 and cases.count(3) > 3 and (host["records"]["filter_bits"] & 2).any()
    assert text == engine.format_vcf("chr7", host["records"], **vcf).encode()
