"""PloidyModel.DiploidByAdaptiveGT on the device.  Expected rows everywhere: the oracle's rows of the same reads with ploidy = SOMATIC and no
LowGQ filter (everything upstream of the genotyper is ploidy-independent), genotyped locus by locus by tests/adaptive_ref.py exactly as
the host pass of a flush does it (tests/test_adaptive_cpu.py::genotype_oracle_rows, which that file checks against the oracle's own
diploid rows for the thresholding genotyper)."""
import ctypes as C

import numpy as np
import pytest

from pisces_amd import _abi
from tests import adaptive_ref as R
from tests import orc
from tests.test_adaptive_cpu import adaptive_expected, gp_close
from tests.test_gpu_parity import _forced_case, _germline_reads, assert_records_match, torch_cuda  # noqa: F401
from tests.test_read_store import env

pytestmark = pytest.mark.gpu
ADAPTIVE = _abi.PLOIDY_DIPLOID_ADAPTIVE


def somatic_of(cfg):
    """the configuration of the oracle run under an adaptive handle's expected rows"""
    s = _abi.PiscesHipConfig()
    C.memmove(C.byref(s), C.byref(cfg), C.sizeof(cfg))
    s.ploidy = _abi.PLOIDY_SOMATIC
    s.low_gq_filter = -1
    return s


def assert_posteriors_match(got, want_gp, what=""):
    assert len(got) == len(want_gp), (what, len(got), len(want_gp))
    for i, (g, w) in enumerate(zip(got, want_gp)):
        if w is None:
            assert g["n"] == 0, (what, i, g)
        else:
            assert g["n"] == len(w) and gp_close(g["gp"][: g["n"]], w), (what, i, g, w)


def flush_all(c, form, schedule):
    """The rows, allele strings (None when the form returns none) and posteriors of every flush of the schedule through one form"""
    rows, alleles, post = [], [], []
    for up_to in schedule:
        a = None
        if form == "flush":
            r = c.Call(up_to, capacity=64)   # (too small on purpose: the repeated call returns the batch)
        elif form == "flush_ex":
            r, a = c.CallWithAlleles(up_to)
        elif form == "view":
            r = c.CallView(up_to)
        else:
            c.CallBegin(up_to)
            if form == "pair":
                r = c.CallEnd()
            elif form == "pair_ex":
                r, a = c.CallEndWithAlleles()
            else:
                r = c.CallEndView()
        p = c.PosteriorsView() if form in ("view", "pair_view") else c.Posteriors(capacity=16)
        assert len(p) == len(r)
        rows.append(np.array(r, copy=True))
        post.append(np.array(p, copy=True))
        alleles = None if a is None or alleles is None else alleles + a
    return np.concatenate(rows), alleles, np.concatenate(post)


FLUSH_CASES = {
    # reads without insertions / deletions, SNVs from the allele counts: the device pass alone makes the rows
    "device pass": dict(with_deletion=False, cfg=dict(collapse=1, call_mnvs=0, strand_bias_model=_abi.SB_EXTENDED, min_frequency=0.0), intervals=[(10, 1600)]),
    # a deletion joins the tile kernels' rows: the host pass
    "host pass": dict(with_deletion=True, cfg=dict(collapse=1, call_mnvs=0, strand_bias_model=_abi.SB_DIPLOID, min_frequency=0.0), intervals=[(20, 700), (720, 1595)]),
    "host pass, mnvs": dict(with_deletion=True, cfg=dict(collapse=0, call_mnvs=1, strand_bias_model=_abi.SB_EXTENDED, min_frequency=0.0), intervals=None),
    "snvs as candidates": dict(with_deletion=False, cfg=dict(collapse=0, call_mnvs=1, strand_bias_model=_abi.SB_DIPLOID, min_frequency=0.2, variant_freq_filter=0.2),
                               intervals=[(10, 1600)]),
}


@pytest.mark.parametrize("case", list(FLUSH_CASES), ids=lambda s: s.replace(" ", "_"))
def test_adaptive_flush_matches_oracle_and_transcription(torch_cuda, case):
    from pisces_amd import engine
    k = FLUSH_CASES[case]
    ref, reads = _germline_reads(900 + len(case), with_deletion=k["with_deletion"])
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    cfg = _abi.default_config(ploidy=ADAPTIVE, low_gq_filter=30, block_size=500, emit_zero_coverage_refs=1 if k["intervals"] else 0, **k["cfg"])
    schedule = [500, 1000]
    rows, alleles, _ = orc.run_reads_schedule(batch, refa, 1, len(ref), somatic_of(cfg), schedule, intervals=k["intervals"])
    exp, exp_alleles, exp_gp = adaptive_expected(rows, alleles, cfg)
    gts = set((exp["info"] & 15).tolist())
    assert {_abi.GT_HET_ALT1_ALT2, _abi.GT_HET_ALT_REF, _abi.GT_HOM_ALT, _abi.GT_HOM_REF, _abi.GT_REF_LIKE_NOCALL} <= gts, gts
    assert ((exp["filter_bits"] >> _abi.FILTER_MULTI_ALLELIC_SITE) & 1).any() and ((exp["filter_bits"] >> _abi.FILTER_LOW_GENOTYPE_QUALITY) & 1).any()
    assert any(g is not None and len(g) == 6 for g in exp_gp) and len(exp) < len(rows)   # a multinomial locus; pruned alleles
    if k["intervals"]:
        assert (exp["total_coverage"] == 0).any()   # the uncovered stretch: the threshold divides by zero there
    if k["with_deletion"]:
        assert (((exp["info"] >> 4) & 7) == _abi.CAT_DELETION).any()
    for form in ("flush", "flush_ex", "view", "pair", "pair_ex", "pair_view"):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(refa)
            if k["intervals"]:
                c.SetIntervals(k["intervals"])
            c.AddAlleleCounts(batch)
            got, got_alleles, post = flush_all(c, form, schedule + [None])
        assert_records_match(got, exp)
        assert got_alleles is None or got_alleles == exp_alleles
        assert_posteriors_match(post, exp_gp, form)
        if form == "flush_ex":
            fmt = lambda recs, al, gp: engine.format_vcf("chrG", recs, alleles=al, posteriors=gp, noise_level_from_records=1, crush=1)
            want_post = np.zeros(len(exp), dtype=_abi.POSTERIORS_DTYPE)
            for i, g in enumerate(exp_gp):
                want_post["n"][i] = len(g)
                want_post["gp"][i][: len(g)] = np.where(g == 0, 0, g)
            text = fmt(got, got_alleles, post)
            assert ":GP\t" in text
            # two decimals of a float32 one step apart may print differently once in many rows: compare all but the GP values, and those as numbers
            strip = lambda t: [ln.rsplit(":", 1) for ln in t.rstrip("\n").split("\n")]
            a, b = strip(text), strip(fmt(exp, exp_alleles, want_post))
            assert [x[0] for x in a] == [x[0] for x in b]
            assert all(np.allclose([float(v) for v in x[1].split(",")], [float(v) for v in y[1].split(",")], atol=0.011) for x, y in zip(a, b))


def test_adaptive_device_pass_equals_host_pass(torch_cuda):
    """The A / B of the diploid mode: the same SNV-only reads with the device genotyper on and off (PISCES_HIP_DEVICE_GENOTYPER)"""
    from pisces_amd import engine
    ref, reads = _germline_reads(77, with_deletion=False)
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    cfg = _abi.default_config(ploidy=ADAPTIVE, low_gq_filter=30, min_frequency=0.0)
    rows, alleles, _, _ = orc.run_reads_full(batch, refa, 1, len(ref), somatic_of(cfg))
    exp, _, exp_gp = adaptive_expected(rows, alleles, cfg)
    out = {}
    for on_device in (1, 0):
        with env(PISCES_HIP_DEVICE_GENOTYPER=on_device):
            with engine.HipVariantCaller(cfg) as c:
                c.SetReference(refa)
                c.AddAlleleCounts(batch)
                got = [(c.Call(up, capacity=1 << 14), c.Posteriors()) for up in (1000, None)]   # (16 tiles: the small compaction; then the rest)
                out[on_device] = (np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]))
    assert out[1][0].tobytes() == out[0][0].tobytes()
    assert (out[1][1]["n"] == out[0][1]["n"]).all()
    for k in (0, 1):
        assert_records_match(out[k][0], exp)
        assert_posteriors_match(out[k][1], exp_gp, "device" if k else "host")
    # the same reads three times side by side in one flush: 75 tiles, so the posteriors follow the rows through the large launch's
    # compaction (its offsets, the speculative copy) instead of the small launch's
    ref3 = bytes(ref) * 3
    reads3 = [dict(r, pos=r["pos"] + 1600 * k) for k in range(3) for r in reads]
    reads3.sort(key=lambda r: r["pos"])
    batch3 = _abi.ReadBatch(reads3)
    refa3 = np.frombuffer(ref3, dtype=np.uint8)
    cfg3 = _abi.default_config(ploidy=ADAPTIVE, low_gq_filter=30, min_frequency=0.0, block_size=5000)
    rows, alleles, _, _ = orc.run_reads_full(batch3, refa3, 1, len(ref3), somatic_of(cfg3))
    exp3, _, exp_gp3 = adaptive_expected(rows, alleles, cfg3)
    with engine.HipVariantCaller(cfg3) as c:
        c.SetReference(refa3)
        c.AddAlleleCounts(batch3)
        got3 = c.Call(capacity=1 << 15)
        post3 = c.Posteriors()
    assert len(exp3) > 4500
    assert_records_match(got3, exp3)
    assert_posteriors_match(post3, exp_gp3, "75 tiles")


def run_tiles(torch, caller, p):
    """pisces_hip_call_tiles with a posteriors buffer + both compactions: (rows, posteriors, tile results)"""
    dev = p.tuples.device
    cap = p.n_tiles * _abi.SLOTS_PER_TILE
    ts = caller.torch_stream()
    with torch.cuda.stream(ts):
        recs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
        post = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        tres = torch.zeros(p.n_tiles * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        out_d = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
        post_d = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        offs = torch.zeros(max(p.n_tiles, 1), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    caller.call_tiles(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, recs.data_ptr(), cap, tres.data_ptr(), ts, posteriors=post)
    caller.compact_records(recs.data_ptr(), tres.data_ptr(), p.n_tiles, offs.data_ptr(), out_d.data_ptr(), cap, count.data_ptr(), ts)
    caller.compact_posteriors(post.data_ptr(), tres.data_ptr(), p.n_tiles, offs.data_ptr(), post_d.data_ptr(), cap, ts)
    caller.synchronize()
    torch.cuda.synchronize()
    n = int(count.item())
    tr = tres.cpu().numpy().view(_abi.TILE_RESULT_DTYPE)
    assert n == int(tr["n_records"].sum())
    return (out_d.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy(), post_d.cpu().numpy().view(_abi.POSTERIORS_DTYPE)[:n].copy(), tr)


def assert_windows_match(p, got, post, cfg, n_windows=16, window_loci=1000, seed=7):
    """assert_random_windows_match_oracle of tests/test_gpu_parity.py for an adaptive handle: seeded 1000-locus windows, the first and the
    last block always among them"""
    from pisces_amd import synth
    tiles = p.tiles.cpu().numpy().view(_abi.TILE_DTYPE)
    per = max(1, min(p.n_tiles, -(-window_loci // max(int(tiles[0]["n_loci"]), 1))))
    rng = np.random.default_rng(seed)
    firsts = {0, p.n_tiles - per}
    while len(firsts) < min(n_windows, p.n_tiles - per + 1):
        firsts.add(int(rng.integers(0, p.n_tiles - per + 1)))
    ref = p.ref.cpu().numpy()
    letters = _abi.BASE_OF_ALLELE
    seen = set()
    for t0 in sorted(firsts):
        start = int(tiles[t0]["start_position"])
        n = int(tiles[t0 + per - 1]["start_position"] + tiles[t0 + per - 1]["n_loci"]) - start
        pos, tup = synth.observations_of(p, per, first_tile=t0)
        rows, _ = orc.run_observations(pos, tup, ref, start, n, somatic_of(cfg))
        alleles = [(letters[(int(i) >> 7) & 7], letters[(int(i) >> 10) & 7]) for i in rows["info"]]
        exp, _, exp_gp = adaptive_expected(rows, alleles, cfg)
        lo, hi = np.searchsorted(got["position"], [start, start + n])
        assert_records_match(got[lo:hi], exp)
        assert_posteriors_match(post[lo:hi], exp_gp, "window at %d" % start)
        seen |= set((exp["info"] & 15).tolist())
    return seen


@pytest.mark.parametrize("depth", [500, 300, 1500])
def test_adaptive_tile_surface_at_size(torch_cuda, depth):
    """BASELINE config 2's tuples (100 000 loci x 500x: the multinomial's dp > 500 edge) and a 300x and a 1500x variant through
    pisces_hip_call_tiles on an adaptive handle: compacted records and compacted posteriors against sixteen windows of the oracle"""
    from pisces_amd import engine, synth
    torch = torch_cuda
    p = synth.make_pileup(n_loci=100_000, depth=depth, device="cuda")
    cfg = _abi.default_config(ploidy=ADAPTIVE, min_frequency=0.0, low_gq_filter=30)
    with engine.HipVariantCaller(cfg) as c:
        got, post, tr = run_tiles(torch, c, p)
    # (fewer rows than loci: where the only variant of a locus is pruned nothing is left of the locus, AlleleCaller.cs:146-162)
    assert (np.diff(got["position"]) >= 0).all() and len(got) > 90_000
    seen = assert_windows_match(p, got, post, cfg)
    assert {_abi.GT_HOM_REF, _abi.GT_HET_ALT_REF} <= seen, seen


def test_adaptive_tile_surface_with_every_kind_of_locus(torch_cuda):
    """A pileup with a planted SNV at every fourth locus over the whole frequency range, and the refusals of the batched / graph forms"""
    from pisces_amd import engine, synth
    torch = torch_cuda
    p = synth.make_pileup(n_loci=3000, depth=120, seed=80, device="cuda", snv_every=4, snv_offset=1, vaf_range=(0.05, 0.99))
    cfg = _abi.default_config(ploidy=ADAPTIVE, min_frequency=0.0, low_gq_filter=30)
    with engine.HipVariantCaller(cfg) as c:
        got, post, tr = run_tiles(torch, c, p)
        totals = c.device_totals()
        with pytest.raises(engine.PiscesHipError) as e:
            c.call_tiles_batched([(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, 0, 0, 0)])
        assert e.value.code == _abi.E_UNSUPPORTED
        with pytest.raises(engine.PiscesHipError) as e:
            c.call_tiles_graph_build([(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, 0, 0, 0)])
        assert e.value.code == _abi.E_UNSUPPORTED
        with pytest.raises(engine.PiscesHipError) as e:   # a posteriors buffer that is too short for the launch
            small = torch.zeros(32 * 16, dtype=torch.uint8, device="cuda")
            c.call_tiles(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, 1, p.n_tiles * _abi.SLOTS_PER_TILE, 1, None, posteriors=small)
        assert e.value.code == _abi.E_BUFFER_TOO_SMALL
        with pytest.raises(engine.PiscesHipError) as e:
            c.SetAdaptiveGenotypingParameters(snv_model=(0.5, 0.4, 0.9))
        assert e.value.code == _abi.E_INVALID_ARG
    seen = assert_windows_match(p, got, post, cfg, n_windows=3)
    assert {_abi.GT_HOM_REF, _abi.GT_HET_ALT_REF, _abi.GT_HOM_ALT} <= seen, seen
    assert totals["records"] == len(got) == int(tr["n_records"].sum())


def test_adaptive_parameters_reach_both_passes(torch_cuda):
    """pisces_hip_set_adaptive_params: the models of example.model instead of the defaults, through the device pass and the host pass"""
    from pisces_amd import engine
    from tests.test_adaptive_cpu import CASES
    mod = CASES["model"]
    rp = dict(R.DEFAULT_PARAMS, **{k: tuple(v) for k, v in mod.items()})
    for with_deletion in (False, True):
        ref, reads = _germline_reads(31, with_deletion=with_deletion)
        batch = _abi.ReadBatch(reads)
        refa = np.frombuffer(bytes(ref), dtype=np.uint8)
        cfg = _abi.default_config(ploidy=ADAPTIVE, min_frequency=0.0, block_size=2000)
        rows, alleles, _, _ = orc.run_reads_full(batch, refa, 1, len(ref), somatic_of(cfg))
        exp, exp_alleles, exp_gp = adaptive_expected(rows, alleles, cfg, rp)
        with engine.HipVariantCaller(cfg) as c:
            c.SetAdaptiveGenotypingParameters(mod["snv_model"], mod["indel_model"], mod["snv_prior"], mod["indel_prior"])
            c.SetReference(refa)
            c.AddAlleleCounts(batch)
            got, got_alleles = c.CallWithAlleles()
            post = c.Posteriors()
        assert got_alleles == exp_alleles
        assert_records_match(got, exp)
        assert_posteriors_match(post, exp_gp)


@pytest.mark.parametrize("gvcf", [1, 0], ids=["gvcf", "variants only"])
def test_adaptive_forced_alleles(torch_cuda, gvcf):
    """Forced alleles with an adaptive handle: a forced allele the genotyper prunes stays (AlleleCaller.cs:155-163), forced-report rows are
    not shown to the genotyper and have no posteriors, and there is no DiploidLocusProcessor rewrite (no PISCES_GT_OTHERS, no shared q-score)"""
    from pisces_amd import engine
    ref, reads, forced = _forced_case()
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    cfg = _abi.default_config(ploidy=ADAPTIVE, block_size=250, min_frequency=0.0, include_reference_calls=gvcf)
    schedule = [260, 520]
    rows, alleles, _ = orc.run_reads_schedule(batch, refa, 1, len(ref), somatic_of(cfg), schedule, forced=forced)
    keys = {(p, r, a) for (p, r, a) in forced}
    exp, exp_alleles, exp_gp = adaptive_expected(rows, alleles, cfg, forced_keys=keys)
    unforced, _, _ = adaptive_expected(rows, alleles, cfg)
    assert len(unforced) < len(exp)                                   # a forced allele that the genotyper prunes, and that stays
    assert sum(g is None for g in exp_gp) >= 4                        # forced-report rows
    assert _abi.GT_OTHERS not in set((exp["info"] & 15).tolist())
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(refa)
        c.SetForcedAlleles(forced)
        c.AddAlleleCounts(batch)
        got, got_alleles, post = [], [], []
        for up_to in schedule + [None]:
            rr, a = c.CallWithAlleles(upToPosition=up_to)
            got.append(rr)
            got_alleles += a
            post.append(c.Posteriors())
    assert got_alleles == exp_alleles
    assert_records_match(np.concatenate(got), exp)
    assert_posteriors_match(np.concatenate(post), exp_gp)


@pytest.mark.parametrize("ploidy", [_abi.PLOIDY_SOMATIC, _abi.PLOIDY_DIPLOID, _abi.PLOIDY_HAPLOID], ids=["somatic", "diploid", "haploid"])
def test_other_ploidies_have_no_posteriors(torch_cuda, ploidy):
    from pisces_amd import engine
    ref, reads = _germline_reads(12, with_deletion=ploidy != _abi.PLOIDY_HAPLOID)
    batch = _abi.ReadBatch(reads)
    refa = np.frombuffer(bytes(ref), dtype=np.uint8)
    cfg = _abi.default_config(ploidy=ploidy, min_frequency=0.2, variant_freq_filter=0.2)
    exp, _, _, _ = orc.run_reads_full(batch, refa, 1, len(ref), cfg)
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(refa)
        c.AddAlleleCounts(batch)
        assert len(c.Posteriors()) == 0   # nothing flushed yet
        got = c.Call()
        post = c.Posteriors()
        assert len(c.PosteriorsView()) == len(got)
        for call in (lambda: c.SetAdaptiveGenotypingParameters(), lambda: engine._check(c.handle, engine.lib.pisces_hip_set_posteriors_buffer(c.handle, 1, 1))):
            with pytest.raises(engine.PiscesHipError) as e:
                call()
            assert e.value.code == _abi.E_STATE
    assert_records_match(got, exp)
    assert len(post) == len(got) > 1000 and (post["n"] == 0).all() and not post["gp"].any()
