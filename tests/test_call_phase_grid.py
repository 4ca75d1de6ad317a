"""The call phase at the edges of its memo tables, in its proved early-outs and on its cold path, against the oracle.

tests/call_phase_grid.py places loci on purpose where random pileups never land: coverage 8191 / 8192 / 8193 and beyond (the coverage
edge of vq_tab, sb_tab, sb0_tab, gq_tail and gq_cap), support 254 .. 257, the last support below MaximumVariantQScore and the first at
it, the last support of the cold path and the first of the early-out, non-allele observations across 31 / 32 / 33, a per-strand
coverage of exactly 8191 and 8192, odd stitched halves.  The CPU tests prove from the oracle alone that every regime is reached and
that no row sits on a rounding tie; the GPU tests hold every kernel form, the table switches, the table-less kernels and the
counts-fed and candidate call phases to the oracle on those loci, every field exact.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from pisces_amd import _abi, _native
from tests import call_phase_grid as cpg
from tests import orc
from tests.test_gpu_parity import assert_records_match, run_fused, torch_cuda  # noqa: F401
from tests.test_read_store import env

gpu = pytest.mark.gpu

# q-scores below the cap must show up in rows: nothing is dropped for a low q-score or a low frequency, and LowGQ is on
BASE = dict(min_variant_qscore=0, min_frequency=0.0001, variant_freq_filter=0.0001, low_gq_filter=30)
CONFIGS = {
    "nl20_cap100": dict(BASE, noise_level=20, max_variant_qscore=100),
    "nl30_cap100": dict(BASE, noise_level=30, max_variant_qscore=100),
    "nl37_cap100": dict(BASE, noise_level=37, max_variant_qscore=100),
    "nl20_cap60": dict(BASE, noise_level=20, max_variant_qscore=60),
    "nl20_cap110": dict(BASE, noise_level=20, max_variant_qscore=110),
    "nl20_cap111": dict(BASE, noise_level=20, max_variant_qscore=111),          # the q-score early-out is guarded by max_vq <= 110
    "nl20_cap3000": dict(BASE, noise_level=20, max_variant_qscore=3000, max_genotype_qscore=3000),
    "defaults": dict(),
    "poisson_sb": dict(strand_bias_model=_abi.SB_POISSON, filter_single_strand=1),
    "lod05_gq10_40": dict(target_lod_frequency=0.05, genotype_min_freq_filter=0.05, min_genotype_qscore=10, max_genotype_qscore=40),
    # target_lod below the genotyper's frequency: hom-ref / hom-alt calls whose non-allele observations reach target_lod * coverage
    # (the genotype q-score's floor; with the two equal, as in every configuration above, no hom call gets there)
    "lod002_floor": dict(BASE, target_lod_frequency=0.002),
}
MIN_PER_REGIME = 20


def _cfg(name):
    return _abi.default_config(**CONFIGS[name])


_EXPECTED = {}


def _expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = cpg.oracle_rows(cpg.grid(), _cfg(name))
    return _EXPECTED[name]


def _assert_the_rows_show_the_edges(rows, cap, hom_ref=True):
    """A variant below the cap and one at it, both at a coverage beyond the tables, and (hom_ref; a called variant takes its locus'
    Reference row away, so only where something is left uncalled) a LowGQ-filtered hom-ref there too."""
    cat, gt = _abi.info_category(rows["info"]), _abi.info_genotype(rows["info"])
    deep = rows["total_coverage"] >= cpg.TAB_COV - 1
    var = (cat == _abi.CAT_SNV) & deep
    assert (var & (rows["variant_qscore"] < cap) & (rows["variant_qscore"] > 0)).any() and (var & (rows["variant_qscore"] == cap)).any()
    low_gq = (rows["filter_bits"] & (1 << _abi.FILTER_LOW_GENOTYPE_QUALITY)) != 0
    assert not hom_ref or ((cat == _abi.CAT_REFERENCE) & (gt == _abi.GT_HOM_REF) & low_gq & deep).any()


# The configurations of the counts-fed call phase: (configuration, does a hom-ref row show).  With the frequency threshold at its default
# the alternates under 1 % stay uncalled and leave their Reference rows.
COUNTS_FED = {"nl20_cap100": (CONFIGS["nl20_cap100"], False), "nl20_cap3000": (CONFIGS["nl20_cap3000"], False), "defaults_low_gq": (dict(low_gq_filter=30), True)}
# ... and of the read-fed ones: an alternate under 0.95 % stays uncalled
READ_FED = dict(CONFIGS["nl20_cap100"], min_frequency=0.0095)
READ_FORMS = {"store_1_wave": dict(PISCES_HIP_STORE_WAVES=1), "store_2_waves": dict(PISCES_HIP_STORE_WAVES=2), "call_mnvs": dict(),
              "log_chain": dict(PISCES_HIP_READ_PATH="log")}
_CASES = {}


def _counts_fed_case(name):
    if ("counts", name) not in _CASES:
        g, cfg = cpg.grid("reduced"), _abi.default_config(**COUNTS_FED[name][0])
        _, _, pos, tup = cpg.tuples_of(g)
        exp, _ = orc.run_observations(pos, tup, g.ref, g.start, g.n_loci, cfg)
        _CASES["counts", name] = (g, cfg, pos, tup, exp)
    return _CASES["counts", name]


def _read_fed_case(how):
    """how: a key of READ_FORMS, or "window" (NoiseModel.Window: mixed qualities, the exhaustive corner as three-base reads too)."""
    key = "window" if how == "window" else "mnv" if how == "call_mnvs" else "plain"
    if ("reads", key) not in _CASES:
        batch, ref, layout = cpg.reads_of(corner=key == "window", mixed_quality=key == "window")
        cfg = _abi.default_config(noise_model=1, **BASE) if key == "window" else _abi.default_config(**dict(READ_FED, call_mnvs=1 if key == "mnv" else 0))
        exp, exp_alleles, _, exp_called = orc.run_reads_full(batch, ref, 1, len(ref), cfg)
        _CASES["reads", key] = (batch, ref, layout, cfg, exp, exp_alleles, exp_called)
    return _CASES["reads", key]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: what the grid exercises, from the oracle alone
# ------------------------------------------------------------------------------------------------------------------------------------
def _wanted(name, r):
    """[(regime, rows in it, at least, at most)] for a configuration."""
    cfg = _cfg(name)
    early_possible = cfg.max_variant_qscore <= 110
    none = 10 ** 9
    want = [("vq table", r["vq"].get("table", 0), MIN_PER_REGIME, none),
            ("vq early-out", r["vq"].get("early", 0), MIN_PER_REGIME if early_possible else 0, none if early_possible else 0),
            ("vq cold", r["vq"].get("cold", 0), MIN_PER_REGIME if early_possible else 500, none),
            ("vq cold below the cap", r["vq_cold_below_cap"], MIN_PER_REGIME, none),
            ("vq cold at the cap", r["vq_cold_at_cap"], MIN_PER_REGIME, none)]
    for which in ("sb_overall", "sb_forward", "sb_reverse"):
        want += [("%s %s" % (which, k), r[which].get(k, 0), MIN_PER_REGIME, none) for k in ("table", "early", "cold")]
    if cfg.strand_bias_model == _abi.SB_POISSON:   # support 0 on a strand: the constant, not sb0_tab
        want.append(("sb support 0, Poisson model", sum(r[w].get("const", 0) for w in ("sb_overall", "sb_forward", "sb_reverse")), MIN_PER_REGIME, none))
    want += [("gq gq_cap", r["gq"].get("gq_cap", 0), MIN_PER_REGIME, none), ("gq cold", r["gq"].get("cold", 0), MIN_PER_REGIME, none)]
    if cfg.max_variant_qscore == 3000:   # a hom call with a q-score below the cap: only where the cap is out of reach
        want.append(("gq gq_tail", r["gq"].get("gq_tail", 0), MIN_PER_REGIME, none))
    if name == "lod002_floor":
        want.append(("gq floor", r["gq"].get("floor", 0), MIN_PER_REGIME, none))
    return want


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_grid_reaches_every_regime(name):
    g = cpg.grid()
    r = cpg.regimes(g, _cfg(name))
    report = "%s: %d rows, regimes %r, %d loci dropped as tie-prone" % (name, r["rows"], r, len(cpg.DROPPED))
    for regime, n, lo, hi in _wanted(name, r):
        assert lo <= n <= hi, "%s: %d rows (wanted %d .. %d)\n%s" % (regime, n, lo, hi, report)
    # with the call tables off every table hit is an early-out or the cold path; with the gq table off every hom call is
    off = cpg.regimes(g, _cfg(name), tables=False, gq_table=False)
    assert "table" not in off["vq"] and "gq_cap" not in off["gq"] and "gq_tail" not in off["gq"], off
    assert off["vq"].get("cold", 0) >= r["vq"].get("cold", 0) + MIN_PER_REGIME, (off, report)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_no_row_of_the_grid_sits_on_a_rounding_tie(name):
    g = cpg.grid()
    ties = cpg.tie_prone(g, _cfg(name))
    n_rows = len(_expected(name))
    assert ties == [], "%s: %d tie-prone rows left in the grid (drop their loci by name in call_phase_grid.DROPPED): %r" % (name, len(ties), ties[:20])
    assert len(cpg.DROPPED) <= n_rows // 1000, "%d loci dropped as tie-prone, %d rows: more than 0.1 %%: %r" % (len(cpg.DROPPED), n_rows, cpg.DROPPED)


def test_every_deep_column_holds_the_edges_it_was_made_for():
    g = cpg.grid()
    assert g.n_obs < cpg.MAX_OBSERVATIONS
    for cov in cpg.DEEP_COLUMNS:
        m = (g.column == cov) & (g.part == "column")
        assert 0 < m.sum() <= (2 * cpg.TILE if cov in cpg.TWO_TILE_COLUMNS else cpg.TILE)
        assert (g.counts[m].sum(axis=(1, 2)) == cov).all()
        have = {int(n.split("/k")[1]) for n, keep in zip(g.names, m) if keep}
        cap_k, early_k = cpg.first_support_at_cap(cov), cpg.first_early_out_support(cov)
        assert orc.lib.orc_poisson_qscore(cap_k - 1, cov, cpg.PICK_NOISE, cpg.PICK_CAP) < cpg.PICK_CAP == orc.lib.orc_poisson_qscore(cap_k, cov, cpg.PICK_NOISE, cpg.PICK_CAP)
        assert cap_k < early_k and not cpg.vq_early_out(early_k - 1, cov, cpg.PICK_NOISE, cpg.PICK_CAP)
        want = {cap_k - 1, cap_k, early_k - 1, early_k, 254, 255, 256, 257, cov // 2} | {cov - n for n in range(36)}
        assert want <= have, (cov, sorted(want - have))
    # the strand layouts: per-strand table indices on both sides of the coverage edge, odd stitched halves, one strand without support
    lay = g.counts[g.part == "layout"]
    cov_d, fwd = lay.sum(axis=1), lay.sum(axis=1)[:, 0] + lay.sum(axis=1)[:, 2] // 2
    assert {8191, 8192} <= set(fwd.tolist()) and (cov_d[:, 2] % 2 == 1).any() and (cov_d[:, 1] == 0).any()
    assert (g.n_alts == 3).sum() >= 4 and (g.counts[:, _abi.ALLELE_N].sum(axis=1) > 0).sum() >= 4 and (g.counts[:, _abi.ALLELE_DEL].sum(axis=1) > 0).sum() >= 4


def test_the_tuple_stream_and_the_counts_are_the_same_pileup():
    """oracle_rows (counts set into the state) equals the oracle fed with the tuples of tuples_of one by one; the tiles cover the stream."""
    g = cpg.grid()
    stream, tiles, pos, tup = cpg.tuples_of(g)
    assert len(tup) == g.n_obs and tiles["tuple_begin"][0] == 1 and tiles["tuple_end"][-1] == 1 + g.n_obs == len(stream) - 3
    assert (tiles["tuple_begin"][1:] == tiles["tuple_end"][:-1]).all() and (tiles["n_loci"] <= cpg.TILE).all() and tiles["n_loci"].sum() == g.n_loci
    locus = _abi.tuple_fields(stream[1:1 + g.n_obs])[0] + np.repeat(tiles["start_position"], tiles["tuple_end"] - tiles["tuple_begin"])
    assert (locus == pos).all()
    for name in ("nl20_cap100", "defaults"):
        fed, _ = orc.run_observations(pos, tup, g.ref, g.start, g.n_loci, _cfg(name))
        assert fed.tobytes() == _expected(name).tobytes()


def test_the_read_columns_carry_the_supports_they_name():
    batch, ref, layout = cpg.reads_of()
    rows, alleles, _, _ = orc.run_reads_full(batch, ref, 1, len(ref), _cfg("nl20_cap100"))
    snv = {int(r["position"]): (int(r["allele_support"]), int(r["total_coverage"])) for r, a in zip(rows, alleles) if a[0] != a[1]}
    for cov, first, sup in layout:
        assert {first + l: (k, cov) for l, k in enumerate(sup) if k} == {p: v for p, v in snv.items() if first <= p < first + cpg.TILE}
    assert all(len(a[0]) == 1 and len(a[1]) == 1 for a in alleles)


def test_the_expected_rows_show_the_edges():
    """What the GPU tests assert of the rows they get, asserted here of the oracle's rows."""
    for name in CONFIGS:
        if _cfg(name).low_gq_filter >= 0:
            _assert_the_rows_show_the_edges(_expected(name), _cfg(name).max_variant_qscore)
    _assert_the_rows_show_the_edges(cpg.oracle_rows(cpg.grid("reduced"), _abi.default_config(strand_bias_model=_abi.SB_DIPLOID, **BASE)), 100, hom_ref=False)
    for name, (_, hom_ref) in COUNTS_FED.items():
        g, cfg, _, _, exp = _counts_fed_case(name)
        assert exp.tobytes() == cpg.oracle_rows(g, cfg).tobytes()
        _assert_the_rows_show_the_edges(exp, cfg.max_variant_qscore, hom_ref)
    for how in ("store_1_wave", "call_mnvs", "window"):
        batch, _, layout, cfg, exp, exp_alleles, _ = _read_fed_case(how)
        _assert_the_rows_show_the_edges(exp, cfg.max_variant_qscore, hom_ref=how != "window")
        assert all(len(a[0]) == 1 and len(a[1]) == 1 for a in exp_alleles)
    batch, _, layout, _, exp, _, _ = _read_fed_case("window")
    assert len(layout) == len(cpg.READ_COLUMNS) + 48 * 49 // 2 - 1 and cpg.window_level_margin_of_reads(batch).min() >= 1e-6
    assert len(np.unique(exp["noise_level"])) >= 4 and exp["noise_level"].min() >= 30


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _upload(torch, g):
    stream, tiles, pos, tup = cpg.tuples_of(g)
    return SimpleNamespace(tuples=torch.from_numpy(stream.view(np.int32)).cuda(), tiles=torch.from_numpy(tiles.view(np.uint8)).cuda(), n_tiles=len(tiles),
                           ref=torch.from_numpy(g.ref).cuda(), ref_len=len(g.ref), positions=pos, observations=tup)


@pytest.fixture(scope="module")
def full_stream(torch_cuda):
    """The tuple stream of the whole grid, uploaded once for the module."""
    return _upload(torch_cuda, cpg.grid())


@gpu
@pytest.mark.parametrize("form", ["block", "wave", "wave2", "auto"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_tile_surface_in_every_kernel_form_matches_oracle_at_the_table_edges(torch_cuda, full_stream, monkeypatch, form, name):
    from pisces_amd import engine
    monkeypatch.setenv("PISCES_HIP_KERNEL", form)
    cfg = _cfg(name)
    with engine.HipVariantCaller(cfg) as caller:
        got, tr = run_fused(torch_cuda, caller, full_stream)
        got_c, _ = run_fused(torch_cuda, caller, full_stream, compact=True)
    exp = _expected(name)
    assert_records_match(got, exp)
    assert got.tobytes() == got_c.tobytes()
    assert int(tr["n_candidate_loci"].sum()) == len(np.unique(exp["position"]))
    if cfg.low_gq_filter >= 0:
        _assert_the_rows_show_the_edges(got, cfg.max_variant_qscore)


@gpu
@pytest.mark.parametrize("name", ["nl20_cap100", "nl20_cap3000"])
def test_tables_off_gives_the_rows_of_tables_on(torch_cuda, full_stream, monkeypatch, name):
    """PISCES_HIP_NO_CALL_TABLES / PISCES_HIP_NO_GQ_TABLE (read at create): every memo hit of the default handle evaluated the long way
    instead — byte for byte the same rows, and the oracle's."""
    from pisces_amd import engine
    monkeypatch.delenv("PISCES_HIP_KERNEL", raising=False)
    cfg = _cfg(name)
    with env(PISCES_HIP_NO_CALL_TABLES=None, PISCES_HIP_NO_GQ_TABLE=None):
        with engine.HipVariantCaller(cfg) as caller:
            want, _ = run_fused(torch_cuda, caller, full_stream)
    assert_records_match(want, _expected(name))
    for switches in (dict(PISCES_HIP_NO_CALL_TABLES=1, PISCES_HIP_NO_GQ_TABLE=None), dict(PISCES_HIP_NO_CALL_TABLES=None, PISCES_HIP_NO_GQ_TABLE=1),
                     dict(PISCES_HIP_NO_CALL_TABLES=1, PISCES_HIP_NO_GQ_TABLE=1)):
        _native.lib.pisces_hip_trim_memory()   # no table set of an earlier handle is there to be taken over
        with env(**switches):
            with engine.HipVariantCaller(cfg) as caller:
                got, _ = run_fused(torch_cuda, caller, full_stream)
                got_c, _ = run_fused(torch_cuda, caller, full_stream, compact=True)
        assert got.tobytes() == want.tobytes() == got_c.tobytes(), switches
        assert_records_match(got, _expected(name))


@gpu
def test_diploid_strand_bias_kernel_at_depth(torch_cuda):
    """The Diploid strand-bias model has no memo tables and routes to call_tiles_kernel (MathNet's BetaRegularized): the exhaustive
    corner and the columns 8191, 8192 and 20000."""
    from pisces_amd import engine
    g, cfg = cpg.grid("reduced"), _abi.default_config(strand_bias_model=_abi.SB_DIPLOID, **BASE)
    view = _upload(torch_cuda, g)
    exp = cpg.oracle_rows(g, cfg)
    with engine.HipVariantCaller(cfg) as caller:
        got, tr = run_fused(torch_cuda, caller, view)
        got_c, _ = run_fused(torch_cuda, caller, view, compact=True)
    assert_records_match(got, exp)
    assert got.tobytes() == got_c.tobytes() and int(tr["n_candidate_loci"].sum()) == len(np.unique(exp["position"]))
    _assert_the_rows_show_the_edges(got, cfg.max_variant_qscore, hom_ref=False)


@gpu
def test_window_noise_model_at_depth(torch_cuda):
    """NoiseModel.Window has no memo tables either (every allele has its own noise level).  The oracle knows base-quality sums from
    reads only, so this goes through AddAlleleCounts: the read columns 48, 8191, 8192 and 20000 and the exhaustive corner as three-base
    reads, base qualities mixed so that no locus' noise level sits on an integer edge of PtoQ (1e-6 away at the least:
    test_the_expected_rows_show_the_edges)."""
    from pisces_amd import engine
    batch, ref, _, cfg, exp, exp_alleles, exp_called = _read_fed_case("window")
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(ref)
        c.AddAlleleCounts(batch)
        got, got_alleles = c.CallWithAlleles()
        stats = c.Stats()
    assert got_alleles == exp_alleles
    assert_records_match(got, exp)
    assert stats["TotalNumCalled"] == exp_called
    _assert_the_rows_show_the_edges(got, cfg.max_variant_qscore, hom_ref=False)


@gpu
@pytest.mark.parametrize("name", list(COUNTS_FED))
def test_counts_fed_call_phase_at_the_table_edges(torch_cuda, name):
    """AddObservations + Call (call_counts_kernel) on the exhaustive corner and the columns 8191, 8192 and 20000."""
    from pisces_amd import engine
    g, cfg, pos, tup, exp = _counts_fed_case(name)
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(g.ref)
        c.AddObservations(pos, tup)
        got = c.Call()
    assert_records_match(got, exp)
    _assert_the_rows_show_the_edges(got, cfg.max_variant_qscore, COUNTS_FED[name][1])


@gpu
@pytest.mark.parametrize("how", list(READ_FORMS))
def test_read_fed_call_phases_at_the_table_edges(torch_cuda, how):
    """AddAlleleCounts + CallWithAlleles on one tile of reads per coverage column (48, 8191, 8192, 20000): call_store_tiles_kernel with one
    and two waves a tile, the candidate kernel's table-first path (MNV calling on: the SNVs come from the read walk), the
    observation-log chain."""
    from pisces_amd import engine
    batch, ref, _, cfg, exp, exp_alleles, exp_called = _read_fed_case(how)
    with env(**dict(dict(PISCES_HIP_STORE_WAVES=None, PISCES_HIP_READ_PATH=None), **READ_FORMS[how])):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(ref)
            c.AddAlleleCounts(batch)
            got, got_alleles = c.CallWithAlleles()
            stats = c.Stats()
    assert got_alleles == exp_alleles
    assert_records_match(got, exp)
    assert stats["TotalNumCalled"] == exp_called
    _assert_the_rows_show_the_edges(got, cfg.max_variant_qscore)
