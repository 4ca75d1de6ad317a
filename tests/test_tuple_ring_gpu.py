"""The register ring of stream_tuples_wave on the device (tests/tuple_ring.py; the grid's coverage and the loop's index arithmetic are shown
on the CPU by tests/test_tuple_ring_cpu.py): pisces_hip_call_tiles in the forms that stream through the ring (wave, wave2, auto), one tile
per (rows of the body, n4 % 64, start alignment) in the guarded and the padded layout -- bodies of 0 .. 49 rows at every edge of a ring of
16 slots dealt in batches of 8 rows to one and to two waves, and seven longer ones for what only more revolutions reach.

The reference is exact: the oracle's rows at tolerance 0 (which tests/test_tuple_ring_cpu.py holds to a numpy.bincount over the tuple
fields): every tuple counts once, the guard words in front of and behind every segment count for nothing, and the three forms write the
same bytes.  A failing assertion names the tile's (alignment, length, rows, n4 % 64) and the regime the ring model puts it in.
"""
import numpy as np
import pytest

from tests import tuple_geometry as tg
from tests import tuple_ring as tr
from tests.test_read_store import torch_cuda  # noqa: F401
from tests.test_tuple_geometry_gpu import _cfg, bad_tiles, launch

pytestmark = pytest.mark.gpu
FORMS = ["wave", "wave2", "auto"]
LAYOUTS = ["guarded", "padded"]
_RUNS = {}


def run_of(torch, form, layout):
    key = (form, layout)
    if key not in _RUNS:
        _RUNS[key] = launch(torch, tr.build_grid(), layout, form, _cfg())
    return _RUNS[key]


def names(g, tiles, layout):
    return " | ".join(tr.cell_name(g, t, layout) for t in tiles[:4])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", FORMS)
def test_ring_against_the_oracle(torch_cuda, form, layout):
    from tests.test_gpu_parity import assert_records_match
    g = tr.build_grid()
    exp, nloci = tg.oracle_rows(g, _cfg())
    got, res = run_of(torch_cuda, form, layout)
    try:
        assert_records_match(got, exp)
        np.testing.assert_array_equal(res["n_records"], tg.rows_by_tile(exp, g.n_tiles))
        assert int(res["n_candidate_loci"].sum()) == nloci
    except AssertionError as e:
        bad = bad_tiles(got, exp, g.n_tiles) or np.flatnonzero(res["n_records"] != tg.rows_by_tile(exp, g.n_tiles)).tolist()
        raise AssertionError("%s, %s: %d tiles differ from the oracle; first: %s\n%s" % (form, layout, len(bad), names(g, bad, layout), str(e)[:600])) from e


def test_the_ring_forms_and_the_layouts_give_the_same_bytes(torch_cuda):
    g = tr.build_grid()
    want, want_res = run_of(torch_cuda, "wave", "guarded")
    assert len(want) >= g.region_loci
    for form in FORMS:
        for layout in LAYOUTS:
            got, res = run_of(torch_cuda, form, layout)
            if got.tobytes() != want.tobytes() or res.tobytes() != want_res.tobytes():
                bad = bad_tiles(got, want, g.n_tiles) or np.flatnonzero(res != want_res).tolist()
                raise AssertionError("%s, %s differs from wave, guarded in %d tiles; first: %s" % (form, layout, len(bad), names(g, bad, layout)))
