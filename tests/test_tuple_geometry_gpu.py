"""The tuple path on the device at every segment geometry (tests/tuple_geometry.py; the grid's coverage is shown on the CPU by
tests/test_tuple_geometry_cpu.py): pisces_hip_call_tiles in its four forms, pisces_hip_accumulate_tiles, the NoiseModel.Window pair,
batched launches, the ordered compaction over sparse tiles, tuples that must count for nothing, and pisces_hip_add_observations through
the bucketing chain (chunk edges, tiles further apart than the privatised range, drop and keep).

The reference is exact: a numpy.bincount over the tuple fields for the count tensors, the oracle's rows (tolerance 0) for the records.  A
failing assertion names the tile's (start alignment, length) and the regime the loop models put it in.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc
from tests import tuple_geometry as tg
from tests.test_read_store import env, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
FORMS = ["block", "wave", "wave2", "auto"]
LAYOUTS = ["guarded", "padded"]
NO_SWITCH = dict(PISCES_HIP_KERNEL=None, PISCES_HIP_STORE_WAVES=None, PISCES_HIP_TILE_LOCI=None, PISCES_HIP_READ_PATH=None, PISCES_HIP_COMPACT=None)
ROW_FIELDS = ["position", "total_coverage", "allele_support", "reference_support", "num_no_calls", "coverage_by_dir", "support_by_dir",
              "variant_qscore", "genotype_qscore", "info", "noise_level", "filter_bits"]
_VIEWS, _RUNS = {}, {}


def _cfg(**kw):
    return _abi.default_config(emit_zero_coverage_refs=1, **kw)


def view_of(torch, g, layout):
    key = (id(g), layout)
    if key not in _VIEWS:
        buf, tiles = g.layouts[layout]
        _VIEWS[key] = SimpleNamespace(tuples=torch.from_numpy(buf.view(np.int32)).cuda(), tiles=torch.from_numpy(tiles.view(np.uint8)).cuda(),
                                      n_tiles=g.n_tiles, ref=torch.from_numpy(g.ref).cuda(), ref_len=len(g.ref))
    return _VIEWS[key]


def launch(torch, g, layout, form, cfg, compact=False, **switches):
    from pisces_amd import engine
    from tests.test_gpu_parity import run_fused
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form, **switches)):
        with engine.HipVariantCaller(cfg) as caller:
            return run_fused(torch, caller, view_of(torch, g, layout), compact=compact)


def bad_tiles(got, exp, n_tiles):
    """Tiles whose rows differ (in number or in any integer field)."""
    ng, ne = tg.rows_by_tile(got, n_tiles), tg.rows_by_tile(exp, n_tiles)
    bad = set(np.flatnonzero(ng != ne).tolist())
    if not bad and len(got) == len(exp):
        differ = np.zeros(len(got), bool)
        for f in ROW_FIELDS:
            d = got[f] != exp[f]
            differ |= d.reshape(len(got), -1).any(axis=1)
        bad = set(((exp["position"][differ].astype(np.int64) - 1) // tg.TILE).tolist())
    return sorted(bad)


def assert_rows(got, tr, exp, nloci, g, layout, where):
    """Rows against the oracle's at tolerance 0, n_candidate_loci, n_records per tile; names the first tiles that differ."""
    from tests.test_gpu_parity import assert_records_match
    try:
        assert_records_match(got, exp)
        np.testing.assert_array_equal(tr["n_records"], tg.rows_by_tile(exp, g.n_tiles))
        assert int(tr["n_candidate_loci"].sum()) == nloci
    except AssertionError as e:
        bad = bad_tiles(got, exp, g.n_tiles) or np.flatnonzero(tr["n_records"] != tg.rows_by_tile(exp, g.n_tiles)).tolist()
        raise AssertionError("%s: %d tiles differ from the oracle; first: %s\n%s" % (where, len(bad), " | ".join(tg.cell_name(g, t, layout) for t in bad[:4]),
                                                                                       str(e)[:600])) from e


def run_of(torch, form, layout):
    key = (form, layout)
    if key not in _RUNS:
        _RUNS[key] = launch(torch, tg.build_grid(), layout, form, _cfg())
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# the device-resident surface
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", FORMS)
def test_call_tiles_against_the_oracle(torch_cuda, form, layout):
    g = tg.build_grid()
    exp, nloci = tg.oracle_rows(g, _cfg())
    got, tr = run_of(torch_cuda, form, layout)
    assert_rows(got, tr, exp, nloci, g, layout, "%s, %s" % (form, layout))


def test_the_forms_and_the_layouts_give_the_same_bytes(torch_cuda):
    g = tg.build_grid()
    want, want_tr = run_of(torch_cuda, "block", "guarded")
    assert len(want) >= g.region_loci
    for form in FORMS:
        for layout in LAYOUTS:
            got, tr = run_of(torch_cuda, form, layout)
            if got.tobytes() != want.tobytes() or tr.tobytes() != want_tr.tobytes():
                bad = bad_tiles(got, want, g.n_tiles) or np.flatnonzero((tr != want_tr)).tolist()
                raise AssertionError("%s, %s differs from block, guarded in %d tiles; first: %s" % (form, layout, len(bad), " | ".join(tg.cell_name(g, t, layout) for t in bad[:4])))


def accumulate(torch, g, layout, launches=1):
    from pisces_amd import engine
    p = view_of(torch, g, layout)
    with env(**NO_SWITCH):
        with engine.HipVariantCaller(_cfg()) as caller:
            ts = caller.torch_stream()
            with torch.cuda.stream(ts):
                counts = torch.zeros(g.n_tiles * tg.TILE * _abi.COUNTS_PER_LOCUS, dtype=torch.int32, device=p.tuples.device)
            torch.cuda.synchronize()
            for _ in range(launches):
                caller.accumulate_tiles(p.tuples.data_ptr(), p.tiles.data_ptr(), g.n_tiles, counts.data_ptr(), ts)
            caller.synchronize()
            torch.cuda.synchronize()
            return counts.cpu().numpy().reshape(g.n_tiles * tg.TILE, 6, 3, _abi.NUM_ANCHORS)


def assert_tensor(got, want, g, layout, where):
    if not (got == want).all():
        bad = sorted(set((np.argwhere(got != want)[:, 0] // tg.TILE).tolist()))
        first = np.argwhere(got != want)[0]
        raise AssertionError("%s: %d cells in %d tiles differ; first cell %s: %d, not %d; first tiles: %s" % (
            where, int((got != want).sum()), len(bad), first.tolist(), got[tuple(first)], want[tuple(first)], " | ".join(tg.cell_name(g, t, layout) for t in bad[:4])))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_accumulate_tiles_equals_the_bincount_and_adds(torch_cuda, layout):
    g = tg.build_grid()
    want = tg.count_tensor(g.positions, g.tuples, g.region_loci)
    assert_tensor(accumulate(torch_cuda, g, layout), want, g, layout, "accumulate_tiles, " + layout)
    assert_tensor(accumulate(torch_cuda, g, layout, launches=2), 2 * want, g, layout, "accumulate_tiles twice, " + layout)


def test_window_noise_model_on_the_guarded_layout(torch_cuda):
    """NoiseModel.Window: accumulate_tiles_kernel with the quality sums, then call_counts_kernel."""
    g = tg.build_grid()
    cfg = _cfg(noise_model=1)
    exp, nloci = tg.oracle_rows(g, cfg)
    flat, _ = tg.oracle_rows(g, _cfg())
    assert len(exp) != len(flat) or (exp["noise_level"] != flat["noise_level"]).any()      # the model matters on this input
    got, tr = launch(torch_cuda, g, "guarded", None, cfg)
    assert_rows(got, tr, exp, nloci, g, "guarded", "NoiseModel.Window")


INERT_SALTS = [(k,) for k in tg.INERT_KINDS] + [tg.INERT_KINDS]


@pytest.mark.parametrize("form", FORMS)
def test_inert_tuples_count_for_nothing_in_call_tiles(torch_cuda, form):
    """A locus at or beyond the tile's n_loci, allele codes 6 and 7, direction 3, anchors 11..15, a pad word mid-segment -- one kind at a
    time, then all together: the launch over the salted segments writes the bytes of the launch without the salt, and the oracle's rows."""
    cfg = _abi.default_config()
    counted = []
    for layout in LAYOUTS:
        want = None
        for salt in INERT_SALTS:
            plain, salted, kinds = tg.build_inert_grid(kinds=salt)
            if want is None:
                exp, nloci = tg.oracle_rows(plain, cfg)
                want, want_tr = launch(torch_cuda, plain, layout, form, cfg)
                assert_rows(want, want_tr, exp, nloci, plain, layout, "%s, %s, no salt" % (form, layout))
            got, tr = launch(torch_cuda, salted, layout, form, cfg)
            if got.tobytes() != want.tobytes() or tr.tobytes() != want_tr.tobytes():
                bad = bad_tiles(got, want, plain.n_tiles) or np.flatnonzero(tr != want_tr).tolist()
                counted.append("%s, %s: %s counted in %d tiles; first: %s of %d loci" % (form, layout, " + ".join(salt), len(bad), tg.cell_name(salted, bad[0], layout),
                                                                                         plain.n_loci[bad[0]]))
    assert not counted, "\n".join(counted)


def test_inert_tuples_count_for_nothing_in_accumulate_tiles(torch_cuda):
    for layout in LAYOUTS:
        for salt in INERT_SALTS:
            plain, salted, _ = tg.build_inert_grid(kinds=salt)
            want = tg.count_tensor(plain.positions, plain.tuples, plain.region_loci)
            if salt == INERT_SALTS[0]:
                assert_tensor(accumulate(torch_cuda, plain, layout), want, plain, layout, "no salt, " + layout)
            assert_tensor(accumulate(torch_cuda, salted, layout), want, salted, layout, "salted with %s, %s" % (" + ".join(salt), layout))


def test_three_unequal_batches_equal_the_single_launch(torch_cuda):
    from pisces_amd import engine
    torch = torch_cuda
    g = tg.build_grid()
    want, _ = run_of(torch, "auto", "guarded")
    p = view_of(torch, g, "guarded")
    cuts = [0, 57, 57 + 143, g.n_tiles]
    tile_bytes = _abi.TILE_DTYPE.itemsize
    with env(**NO_SWITCH):
        with engine.HipVariantCaller(_cfg()) as c:
            outs, batches = [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                n = hi - lo
                cap = n * _abi.SLOTS_PER_TILE
                rec = torch.zeros(cap * 64, dtype=torch.uint8, device=p.tuples.device)
                tr = torch.zeros(n * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=p.tuples.device)
                outs.append((rec, tr))
                batches.append((p.tuples.data_ptr(), p.tiles.data_ptr() + lo * tile_bytes, n, p.ref.data_ptr(), 1, p.ref_len, rec.data_ptr(), cap, tr.data_ptr()))
            torch.cuda.synchronize()
            c.call_tiles_batched(batches)
            c.synchronize()
            torch.cuda.synchronize()
    rows = [_abi.records_in_order(rec.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE), tr.cpu().numpy().view(_abi.TILE_RESULT_DTYPE)) for rec, tr in outs]
    got = np.concatenate(rows)
    assert len({n for n in np.diff(cuts)}) == 3
    if got.tobytes() != want.tobytes():
        bad = bad_tiles(got, want, g.n_tiles)
        raise AssertionError("batched launches differ in %d tiles; first: %s" % (len(bad), " | ".join(tg.cell_name(g, t) for t in bad[:4])))


@pytest.mark.parametrize("mode", ["one launch", "two", "lookback"])
def test_compaction_over_sparse_tiles(torch_cuda, mode):
    """include_reference_calls = 0 on the guarded grid: the empty tiles and the twelve-tuple ones have no record; rows, offsets and count
    of pisces_hip_compact_records (run_fused checks the last two against the validity masks' counts) in its three forms."""
    from pisces_amd import engine
    from tests.test_gpu_parity import run_fused
    g = tg.build_grid()
    cfg = _abi.default_config(include_reference_calls=0)
    exp, nloci = tg.oracle_rows(g, cfg)
    p = view_of(torch_cuda, g, "guarded")
    with env(**dict(NO_SWITCH, PISCES_HIP_COMPACT=None if mode == "one launch" else mode)):
        with engine.HipVariantCaller(cfg) as caller:
            plain, tr0 = run_fused(torch_cuda, caller, p)
            for launch_no in range(2):
                got, tr = run_fused(torch_cuda, caller, p, compact=True)
                assert got.tobytes() == plain.tobytes() and tr.tobytes() == tr0.tobytes(), (mode, launch_no)
    assert_rows(plain, tr0, exp, nloci, g, "guarded", "variants only")
    empty = tr0["n_records"] == 0
    assert empty.sum() >= 40 and all(empty[t] for t, (_, length) in enumerate(g.cells) if length == 0)
    assert 0 < empty.sum() < g.n_tiles - 200 and not empty[-1] and empty[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# pisces_hip_add_observations and the log chain
# ------------------------------------------------------------------------------------------------------------------------------------
PATHS = {"default": None, "log": "log"}


def flush_schedule(case, path, up_to=(), counts_of=None):
    """AddObservations in the case's three calls, then Call(upTo) for every upTo and Call(): the rows of each flush, and GetCounts of
    counts_of = (first position, loci) before the first flush and after each but the last."""
    from pisces_amd import engine
    with env(**dict(NO_SWITCH, PISCES_HIP_READ_PATH=PATHS[path])):
        with engine.HipVariantCaller(_abi.default_config()) as c:
            c.SetReference(case.ref)
            for part in case.parts:
                c.AddObservations(case.positions[part], case.tuples[part])
            counts = [c.GetCounts(*counts_of)] if counts_of else []
            flushes = []
            for u in list(up_to) + [None]:
                flushes.append(c.Call(u, capacity=1 << 18))
                if counts_of and u is not None:
                    counts.append(c.GetCounts(*counts_of))
            assert len(c.Call(None)) == 0
    return flushes, counts


def case_rows(case):
    if not hasattr(case, "rows"):
        case.rows, _ = orc.run_observations(case.positions, case.tuples, case.ref, 1, case.region_loci, _abi.default_config())
    return case.rows


def assert_log_rows(got, case, where):
    from tests.test_gpu_parity import assert_records_match
    exp = case_rows(case)
    try:
        assert_records_match(got, exp)
    except AssertionError as e:
        tiles = sorted(set(tg.log_tile_of(np.setxor1d(got["position"], exp["position"])).tolist())) if len(got) != len(exp) else \
            sorted(set(tg.log_tile_of(exp["position"][(got["total_coverage"] != exp["total_coverage"]) | (got["allele_support"] != exp["allele_support"])]).tolist()))
        raise AssertionError("%s: rows differ from the oracle (%d against %d rows); tiles %s\n%s" % (where, len(got), len(exp), tiles[:12], str(e)[:500])) from e


@pytest.mark.parametrize("n", tg.chunk_edge_sizes(), ids=lambda n: "C%+d" % (n - tg.K.log_chunk) if n < 2 * tg.K.log_chunk - 1 else "2C%+d" % (n - 2 * tg.K.log_chunk))
def test_log_chunk_edges(torch_cuda, n):
    case = tg.chunk_edge_case(n)
    rows = {}
    for path in PATHS:
        (rows[path],), _ = flush_schedule(case, path)
        assert_log_rows(rows[path], case, "%d entries, %s path" % (n, path))
    assert rows["default"].tobytes() == rows["log"].tobytes()


def test_log_tiles_further_apart_than_the_privatised_range(torch_cuda):
    case = tg.far_tile_case()
    rows = {}
    for path in PATHS:
        (rows[path],), _ = flush_schedule(case, path)
        assert_log_rows(rows[path], case, "far tiles, %s path" % path)
    assert rows["default"].tobytes() == rows["log"].tobytes()
    assert len(np.unique(rows["log"]["position"])) == tg.FAR_LOCI


@pytest.mark.parametrize("path", list(PATHS))
def test_log_drop_and_keep(torch_cuda, path):
    """Call(upTo) in the middle, then Call(): the first flush takes whole blocks, log_drop_kernel keeps the rest; the two flushes together
    are the one-shot rows, and the counts of the kept last block do not move."""
    case = tg.chunk_edge_case(2 * tg.K.log_chunk + 1)
    kept = (2 * tg.BLOCK + 1, tg.BLOCK)
    (first, second), counts = flush_schedule(case, path, up_to=[tg.BLOCK + tg.BLOCK // 2], counts_of=kept)
    assert len(first) and len(second) and first["position"].max() <= tg.BLOCK + tg.BLOCK // 2 < second["position"].max()
    assert first["position"].max() < second["position"].min()
    assert_log_rows(np.concatenate([first, second]), case, "drop and keep, %s path" % path)
    m = case.positions > 2 * tg.BLOCK
    want = tg.count_tensor(case.positions[m], case.tuples[m], tg.BLOCK, region_start=kept[0])
    assert want.sum() > 1000 and (counts[0] == want).all() and (counts[1] == want).all()


@pytest.mark.parametrize("path", list(PATHS))
def test_log_flush_below_the_first_block_end_returns_nothing(torch_cuda, path):
    case = tg.chunk_edge_case(tg.K.log_chunk + 1)
    (first, second), _ = flush_schedule(case, path, up_to=[tg.BLOCK // 2])
    assert len(first) == 0
    assert_log_rows(second, case, "after an empty flush, %s path" % path)


@pytest.mark.parametrize("path", list(PATHS))
def test_log_inert_tuples_count_for_nothing(torch_cuda, path):
    """Allele codes 6 and 7, direction 3, anchors 11..15 and pad words among the observations handed to AddObservations: the rows and the
    counts are those of the entries that count."""
    case = tg.chunk_edge_case(tg.K.log_chunk + 1)
    pos, tup = tg.salted_observations(case)
    assert len(pos) == len(case.positions) + 400
    salted = SimpleNamespace(positions=pos, tuples=tup, parts=[slice(0, 1000), slice(1000, 1001), slice(1001, len(pos))], ref=case.ref, region_loci=case.region_loci)
    (rows,), (counts,) = flush_schedule(salted, path, counts_of=(1, case.region_loci))
    assert_log_rows(rows, case, "salted observations, %s path" % path)
    assert (counts == tg.count_tensor(case.positions, case.tuples, case.region_loci)).all()
