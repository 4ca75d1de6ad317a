"""call_tiles_wave_kernel's argument block: eight launch values, the per-launch parameters (TileLaunchParams) and a pointer to the handle's
device copy of its constant parameters.  What can go wrong with that split shows in the rows: a field read from the wrong place, a device
copy shared between handles or left stale, a per-flush field (the dirty-locus bitmap, refs_only) taken from the create-time copy, a tile
descriptor read for the wrong tile at the launch head.  Every case is compared with the oracle as tests/test_tuple_geometry_gpu.py does it:
integer fields and q-scores at tolerance 0, the tile directory against the oracle's rows per tile.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc
from tests import tuple_geometry as tg
from tests.test_read_store import env, torch_cuda  # noqa: F401
from tests.test_tuple_geometry_gpu import NO_SWITCH, assert_rows

pytestmark = pytest.mark.gpu
WAVE_FORMS = ["wave", "wave2"]    # call_tiles_wave_kernel<1> and <2>, selected as tests/test_tuple_geometry_gpu.py selects them
DEPTH = 40
B = tg.K.B                        # tuples in one batch of the stream loop
_CACHE = {}

# (start alignment modulo 4, tuples, loci) of each tile: an empty segment; one, 56 and 64 loci at depth ~40; exactly one batch and one
# batch plus one tuple; a head and a tail of one to three words around a body (the scalar loops in front of and behind the 16-byte loads)
CELLS = [(0, 0, 64), (1, DEPTH * 1, 1), (2, DEPTH * 56, 56), (3, DEPTH * 64, 64), (0, B, 64), (0, B + 1, 64), (1, B + 2, 64), (3, 2 * B + 3, 56), (2, 7, 64)]
# the same shapes on whole tiles, for the configurations that emit a Reference row on every locus of the region, covered or not
FULL = [(a, n, 64) for a, n, _ in CELLS]
NON_DEFAULT = dict(min_base_call_quality=30, min_variant_qscore=35, strand_bias_threshold=0.2, emit_zero_coverage_refs=1, min_frequency=0.02)


def grid_of(cells, seed=tg.SEED + 11):
    key = (tuple(cells), seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        segments, loci = [], []
        for _, length, n_loci in cells:
            l, t = tg.draw_tuples(rng, length, n_loci)
            loci.append(l)
            segments.append(t)
        _CACHE[key] = tg._finish([(a, length) for a, length, _ in cells], segments, loci, [n for _, _, n in cells], tg.make_reference(rng, tg.TILE * len(cells) + 40))
    return _CACHE[key]


def view_of(torch, g, layout="guarded"):
    key = ("view", id(g), layout)
    if key not in _CACHE:
        buf, tiles = g.layouts[layout]
        _CACHE[key] = SimpleNamespace(tuples=torch.from_numpy(buf.view(np.int32)).cuda(), tiles=torch.from_numpy(tiles.view(np.uint8)).cuda(), n_tiles=g.n_tiles,
                                      ref=torch.from_numpy(g.ref).cuda(), ref_len=len(g.ref))
    return _CACHE[key]


def cfg_of(**kw):
    return _abi.default_config(**kw)


def check(torch, g, cfg, form, caller=None, layout="guarded", where=""):
    from pisces_amd import engine
    from tests.test_gpu_parity import run_fused
    exp, nloci = tg.oracle_rows(g, cfg)
    if caller is not None:
        got, tr = run_fused(torch, caller, view_of(torch, g, layout))
    else:
        with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form)):
            with engine.HipVariantCaller(cfg) as c:
                got, tr = run_fused(torch, c, view_of(torch, g, layout))
    assert_rows(got, tr, exp, nloci, g, layout, "%s %s" % (form, where))
    return got, tr


@pytest.mark.parametrize("layout", ["guarded", "padded"])
@pytest.mark.parametrize("form", WAVE_FORMS)
def test_every_segment_shape_against_the_oracle(torch_cuda, form, layout):
    g = grid_of(CELLS)
    assert [int(e - b) for _, _, b, e in g.layouts[layout][1].tolist()] == [n for _, n, _ in CELLS]
    if layout == "guarded":
        assert {int(b) % 4 for _, _, b, _ in g.layouts[layout][1].tolist()} == {0, 1, 2, 3}
    got, _ = check(torch_cuda, g, cfg_of(), form, layout=layout, where=layout)
    assert len(got) >= sum(n for _, length, n in CELLS if length >= DEPTH) > 0


@pytest.mark.parametrize("n_tiles", [1, 2, 3])
@pytest.mark.parametrize("form", WAVE_FORMS)
def test_launches_of_one_two_and_three_tiles(torch_cuda, form, n_tiles):
    g = grid_of([(1, DEPTH * 64 + 5, 64), (2, DEPTH * 56 + 1, 56), (3, B + 1, 64)][:n_tiles], seed=tg.SEED + 12)
    assert g.n_tiles == n_tiles
    check(torch_cuda, g, cfg_of(), form, where="%d tiles" % n_tiles)


@pytest.mark.parametrize("form", WAVE_FORMS)
def test_a_configuration_that_is_not_the_default(torch_cuda, form):
    g = grid_of(FULL)
    plain, _ = tg.oracle_rows(g, cfg_of())
    other, _ = tg.oracle_rows(g, cfg_of(**NON_DEFAULT))
    assert len(other) != len(plain)                                                                         # (the configuration matters on this input)
    assert tg.rows_by_tile(plain, g.n_tiles)[0] == 0 and tg.rows_by_tile(other, g.n_tiles)[0] == tg.TILE     # (zero-coverage Reference rows of the empty tile)
    check(torch_cuda, g, cfg_of(**NON_DEFAULT), form, where="non-default configuration")


@pytest.mark.parametrize("form", WAVE_FORMS)
def test_two_handles_alive_at_once_keep_their_own_parameters(torch_cuda, form):
    """Launches alternate between two handles of different configurations: each gives its own oracle rows, every time."""
    from pisces_amd import engine
    g = grid_of(FULL)
    cfgs = [cfg_of(), cfg_of(**NON_DEFAULT)]
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form)):
        with engine.HipVariantCaller(cfgs[0]) as a, engine.HipVariantCaller(cfgs[1]) as b:
            for turn in range(2):
                for which, caller in enumerate((a, b)):
                    check(torch_cuda, g, cfgs[which], form, caller=caller, where="handle %d, turn %d" % (which, turn))


def _plain_and_batches(torch, g, c, cuts):
    from tests.test_gpu_parity import run_fused
    p = view_of(torch, g)
    want, _ = run_fused(torch, c, p)
    tile_bytes = _abi.TILE_DTYPE.itemsize
    outs, batches = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        n = hi - lo
        cap = n * _abi.SLOTS_PER_TILE
        rec = torch.zeros(cap * 64, dtype=torch.uint8, device=p.tuples.device)
        tr = torch.zeros(n * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=p.tuples.device)
        outs.append((rec, tr))
        batches.append((p.tuples.data_ptr(), p.tiles.data_ptr() + lo * tile_bytes, n, p.ref.data_ptr(), 1, p.ref_len, rec.data_ptr(), cap, tr.data_ptr()))
    torch.cuda.synchronize()
    return want, outs, batches


def _rows(outs):
    return np.concatenate([_abi.records_in_order(rec.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE), tr.cpu().numpy().view(_abi.TILE_RESULT_DTYPE)) for rec, tr in outs])


@pytest.mark.parametrize("form", WAVE_FORMS)
def test_batched_launches_equal_the_plain_launch(torch_cuda, form):
    from pisces_amd import engine
    g = grid_of(FULL)
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form)):
        with engine.HipVariantCaller(cfg_of(**NON_DEFAULT)) as c:
            want, outs, batches = _plain_and_batches(torch_cuda, g, c, [0, 2, 3, g.n_tiles])
            c.call_tiles_batched(batches)
            c.synchronize()
            torch_cuda.cuda.synchronize()
            assert _rows(outs).tobytes() == want.tobytes() and len(want) > 0


@pytest.mark.parametrize("form", WAVE_FORMS)
def test_a_graph_of_two_launches_equals_the_plain_launch(torch_cuda, form):
    """pisces_hip_call_tiles_graph_build with K = 2, launched twice: the captured argument blocks keep giving the plain launch's bytes."""
    from pisces_amd import engine
    g = grid_of(FULL)
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form)):
        with engine.HipVariantCaller(cfg_of(**NON_DEFAULT)) as c:
            want, outs, batches = _plain_and_batches(torch_cuda, g, c, [0, 4, g.n_tiles])
            assert len(batches) == 2
            gid = c.call_tiles_graph_build(batches)
            for _ in range(2):
                for rec, tr in outs:
                    rec.zero_()
                    tr.zero_()
                torch_cuda.cuda.synchronize()
                c.call_tiles_graph_launch(gid)
                c.synchronize()
                torch_cuda.cuda.synchronize()
                assert _rows(outs).tobytes() == want.tobytes() and len(want) > 0


@pytest.mark.parametrize("form", WAVE_FORMS)
def test_fields_that_change_between_the_flushes_of_a_streaming_run(torch_cuda, form):
    """Two 1000-locus blocks, a few hundred reads each, MNV calling on, through the observation log (the path on which a flush calls
    call_tiles_wave_kernel): refs_only and the dirty-locus bitmap of the second flush are not those of the first, and neither is what the
    handle was created with.  Each flush carries its own in a FlushScope and hands them to the launch as TileLaunchParams; the handle's
    parameters stay what pisces_hip_create made them.  (The folded-count window, the other part of a flush's scope, never reaches this
    kernel: it goes to call_store_tiles_kernel's DeviceParams only, and TileLaunchParams cannot carry it.)  Rows, allele strings and
    TotalNumCalled against the oracle's schedule."""
    from pisces_amd import engine
    from tests.test_gpu_parity import _mnv_reads, assert_records_match
    rng = np.random.default_rng(4711)
    ref = bytes(rng.choice(list(b"ACGT"), 2000).astype(np.uint8))
    reads = []
    for lo in (1, 1001):   # reads stay inside their block
        reads += _mnv_reads(rng, ref, 300, read_len=90, region=(lo + 6, lo + 993))
    reads.sort(key=lambda r: r["pos"])
    refa = np.frombuffer(ref, dtype=np.uint8)
    cfg = _abi.default_config(call_mnvs=1)
    ups = [1000]
    exp, exp_alleles, exp_called = orc.run_reads_schedule(_abi.ReadBatch(reads), refa, 1, len(ref), cfg, ups)
    cats = (exp["info"] >> 4) & 7
    assert (cats == _abi.CAT_MNV).sum() >= 2 and (cats == _abi.CAT_SNV).sum() >= 4
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form, PISCES_HIP_READ_PATH="log")):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(refa)
            c.AddAlleleCounts(_abi.ReadBatch(reads))
            r1, a1 = c.CallWithAlleles(upToPosition=ups[0])
            r2, a2 = c.CallWithAlleles()
            stats = c.Stats()
    assert len(r1) and len(r2) and r1["position"].max() <= 1000 < r2["position"].min()
    assert a1 + a2 == exp_alleles
    assert_records_match(np.concatenate([r1, r2]), exp)
    assert stats["TotalNumCalled"] == exp_called
