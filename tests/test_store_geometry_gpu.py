"""The read store's flush on the device at every fragment geometry (tests/store_geometry.py; the grid's coverage and the agreement of
the two references are shown on the CPU by tests/test_store_geometry_cpu.py).

The flush (call_store_tiles_kernel -> walk_segment_fast) runs every scene of the grid through the C ABI, in one flush or under the
scene's floor schedule, and its records must equal the oracle's rows at tolerance 0 — with 1, 2, 4, 8 and 16 waves a tile, tiles of
64, 59, 48 and 33 loci, tiles dealt by price and in position order, the position grid deferred and not, every way a batch joins the
store, reads handed over in host and in device memory, and the observation-log chain as one more form — under both configurations
of store_geometry.config.  All forms of one configuration must give the same bytes.  GetCounts (accumulate_store_tiles_kernel ->
walk_segment) must equal the numpy count tensor, anchors included, before a flush and, after one, on the blocks that are kept; flushed
blocks read 0.  A failing assertion names the case, the tile, the locus and the regimes the model gives that tile.

That every unit load of walk_segment_fast stays inside an allocation (the scenes "ends of the arrays": the first read of a segment's
arrays begins on locus 31 / 63 of its tile, the last ends on locus 0 of its tile).  A pair exists on a half only if the fragment has a
base on that half, and a unit's four lanes load the half's 32 loci, eight bytes each: so a load begins at most 31 bytes before the
fragment's first base still to count and ends at most 31 bytes behind its last (the model asserts both for every pair of the grid:
("load", "bytes before / behind the fragment", n), n <= 31 < kSegmentPad = 64).  The row codes, which every flush loads, are always the
store's own array: store_shape_begin reserves n_seq + 2 * kSegmentPad (a batch that is a segment of its own) or grows to n_bases + n_seq
+ 2 * kSegmentPad (the open segment) and hands the kernel codes.p + kSegmentPad.  The per-base directions are loaded at the same indices.
Appended to the open segment they lie in g.dirs, grown like the codes with kSegmentPad in front.  A decoded batch (surface_bam.inc.h)
reserves nb + 16 + 2 * kSegmentPad for bases, qualities and directions and decodes to .p + kSegmentPad.  A host-fed or device-fed batch
that becomes a segment of its own lies in the segment's blob in stage_layout's order: the directions at off_dirs, behind positions,
flags, offsets, CIGARs, bases and qualities (at least 96 bytes even for one read) and in front of the candidate-slot table ((n_reads + 1)
* 8 bytes, rounded up to 16) and the found-slot table ((n_reads + 1) * 4, rounded up to 16): 32 bytes at the least behind the last
direction, one more than the 31 a load can reach.  So the argument holds for all three; nothing had to be fixed before these scenes ran.
"""
import numpy as np
import pytest

from pisces_amd import _abi
from tests import store_geometry as sg
from tests.test_read_store import STORE_MODES, env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


NO_SWITCH = dict(PISCES_HIP_KERNEL=None, PISCES_HIP_STORE_WAVES=None, PISCES_HIP_TILE_LOCI=None, PISCES_HIP_TILE_ORDER=None, PISCES_HIP_DEFER_GRID=None,
                 PISCES_HIP_READ_PATH=None, PISCES_HIP_STORE_DIRECT_BYTES=None, PISCES_HIP_STORE_SEAL_BYTES=None, PISCES_HIP_COMPACT=None)
FORMS = {"default": ({}, "host")}
FORMS.update({"%d waves a tile" % nw: (dict(PISCES_HIP_STORE_WAVES=nw), "host") for nw in sg.WAVES})
FORMS.update({"tiles of %d loci" % n: (dict(PISCES_HIP_TILE_LOCI=n), "host") for n in (64, 59, 48, 33)})
FORMS.update({"tiles in position order": (dict(PISCES_HIP_TILE_ORDER=0), "host"), "grid enqueued by the add": (dict(PISCES_HIP_DEFER_GRID=0), "host")})
FORMS.update({mode: (dict(switches), "host") for mode, switches in STORE_MODES.items() if mode != "default"})
FORMS.update({"reads handed over in device memory": ({}, "device"),
              "device memory, every batch its own segment": (dict(STORE_MODES["every batch its own segment"]), "device"),
              "the observation-log chain": (dict(PISCES_HIP_READ_PATH="log"), "host")})
INT_FIELDS = ["position", "total_coverage", "allele_support", "reference_support", "num_no_calls", "coverage_by_dir", "support_by_dir", "info",
              "filter_bits", "variant_qscore", "genotype_qscore"]
_BATCHES, _RUNS = {}, {}


def batches_of(scene):
    if scene.name not in _BATCHES:
        _BATCHES[scene.name] = [sg.read_batch(b) for b in scene.batches]
    return _BATCHES[scene.name]


def run_scene(scene, which, switches, feed):
    """The scene's schedule on a fresh handle: add batch k, flush up to ups[k] where the schedule says so, a final flush.  Returns the
    records and the allele strings."""
    from pisces_amd import engine
    recs, alleles = [], []
    cap = 2 * scene.n_loci
    with env(**dict(NO_SWITCH, **switches)):
        with engine.HipVariantCaller(sg.config(which)) as c:
            c.SetReference(scene.ref)
            for batch, up in zip(batches_of(scene), scene.ups):
                (c.AddDeviceReads if feed == "device" else c.AddAlleleCounts)(batch)
                if up is not None:
                    r, a = c.CallWithAlleles(up, capacity=cap)
                    recs.append(r)
                    alleles += a
            r, a = c.CallWithAlleles(None, capacity=cap)
            recs.append(r)
            alleles += a
            assert c.Stats()["reads"] == len(scene.reads)
    return np.concatenate(recs), alleles


def run_form(form, which):
    key = (form, which)
    if key not in _RUNS:
        switches, feed = FORMS[form]
        _RUNS[key] = {scene.name: run_scene(scene, which, switches, feed) for scene in sg.build_scenes()}
    return _RUNS[key]


def first_difference(got, exp):
    """Position of the first locus whose rows differ, and what differs."""
    n = int(max(got["position"].max(initial=0), exp["position"].max(initial=0))) + 1
    ng, ne = np.bincount(got["position"], minlength=n), np.bincount(exp["position"], minlength=n)
    if (ng != ne).any():
        p = int(np.flatnonzero(ng != ne)[0])
        return p, "%d rows, not %d" % (ng[p], ne[p])
    for i in range(len(got)):
        for f in INT_FIELDS:
            if not np.array_equal(got[f][i], exp[f][i]):
                return int(exp["position"][i]), "%s %s, not %s" % (f, got[f][i], exp[f][i])
    return None, "no integer field differs"


def assert_rows(got, exp, scene, where):
    from tests.test_gpu_parity import assert_records_match
    try:
        assert_records_match(got, exp)
    except AssertionError as e:
        p, what = first_difference(got, exp)
        raise AssertionError("%s, scene '%s': %s; %s\n%s" % (where, scene.name, what, sg.describe_locus(scene, p) if p else "", str(e)[:500])) from e


def point_rows(rows):
    cat = _abi.info_category(rows["info"].astype(np.int64))
    return rows[(cat == _abi.CAT_SNV) | (cat == _abi.CAT_REFERENCE)]


def assert_rows_show_the_tensor(got, scene, where):
    """The scene the oracle has no rows for (deletions of 65 000 bases): the Reference and SNV rows against the numpy count tensor folded
    over anchors, a row on every locus with a count but those an insertion / deletion row stands on."""
    tensor = sg.count_tensor(scene.reads, 1, scene.n_loci, scene.min_bq)
    pr = point_rows(got)
    try:
        assert sg.rows_agree_with_tensor(pr, tensor, scene.ref) > 9 * len(pr) > 9 * 60_000
    except AssertionError as e:
        folded = tensor.sum(axis=3, dtype=np.int64)
        cov = folded[:, [0, 1, 2, 3, 5], :].sum(axis=1)
        li = pr["position"].astype(np.int64) - 1
        bad = np.flatnonzero((pr["coverage_by_dir"] != cov[li]).any(axis=1) | (pr["num_no_calls"] != folded[li, 4, :].sum(axis=1)))
        p = int(pr["position"][bad[0]]) if len(bad) else None
        raise AssertionError("%s, scene '%s': %s\n%s" % (where, scene.name, sg.describe_locus(scene, p) if p else "", str(e)[:500])) from e
    counted = set(np.flatnonzero(tensor.sum(axis=(1, 2, 3)) > 0).tolist())
    cat = _abi.info_category(got["info"].astype(np.int64))
    indel_loci = set((got["position"][(cat != _abi.CAT_SNV) & (cat != _abi.CAT_REFERENCE)].astype(np.int64) - 1).tolist())
    shown = set((pr["position"].astype(np.int64) - 1).tolist())
    assert shown <= counted and counted - shown <= indel_loci, (where, scene.name, sorted(counted - shown - indel_loci)[:5], sorted(shown - counted)[:5])


# ------------------------------------------------------------------------------------------------------------------------------------
# the flush
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sg.CONFIGS)
@pytest.mark.parametrize("form", list(FORMS))
def test_the_flush_equals_the_oracle(torch_cuda, form, which):
    runs = run_form(form, which)
    for scene in sg.build_scenes():
        got, alleles = runs[scene.name]
        where = "%s, %s" % (form, which)
        if scene.name in sg.NO_ORACLE_ROWS:
            assert_rows_show_the_tensor(got, scene, where)
            continue
        exp, exp_alleles = sg.oracle_rows(scene, which)
        assert_rows(got, exp, scene, where)
        if exp_alleles is not None:
            assert alleles == exp_alleles, (where, scene.name)


@pytest.mark.parametrize("which", sg.CONFIGS)
def test_all_forms_give_the_same_bytes(torch_cuda, which):
    want = run_form("default", which)
    for form in FORMS:
        runs = run_form(form, which)
        for scene in sg.build_scenes():
            (got, alleles), (exp, exp_alleles) = runs[scene.name], want[scene.name]
            if got.tobytes() != exp.tobytes() or alleles != exp_alleles:
                p, what = first_difference(got, exp)
                raise AssertionError("%s differs from the default form, %s, scene '%s': %s; %s" % (form, which, scene.name, what, sg.describe_locus(scene, p) if p else ""))


# ------------------------------------------------------------------------------------------------------------------------------------
# GetCounts
# ------------------------------------------------------------------------------------------------------------------------------------
def assert_tensor(got, want, start, scene, where):
    if not (got == want).all():
        first = np.argwhere(got != want)[0]
        raise AssertionError("%s, scene '%s': %d cells differ; first [allele %d][direction %d][anchor %d]: %d, not %d; %s" % (
            where, scene.name, int((got != want).sum()), first[1], first[2], first[3], got[tuple(first)], want[tuple(first)],
            sg.describe_locus(scene, int(start + first[0]))))


@pytest.mark.parametrize("mode", list(STORE_MODES))
def test_counts_before_a_flush_equal_the_tensor(torch_cuda, mode):
    """Every block any read of a scene touches, anchors included, however the batches joined the store."""
    from pisces_amd import engine
    for scene in sg.build_scenes():
        with env(**dict(NO_SWITCH, **STORE_MODES[mode])):
            with engine.HipVariantCaller(sg.config("default")) as c:
                for batch in batches_of(scene):
                    c.AddAlleleCounts(batch)
                for start, n in sg.runs_of_keys(scene.keys):
                    want = sg.count_tensor(scene.reads, start, n, scene.min_bq)
                    assert want.sum() > 0
                    assert_tensor(c.GetCounts(start, n), want, start, scene, "GetCounts before a flush, " + mode)


@pytest.mark.parametrize("mode", list(STORE_MODES))
@pytest.mark.parametrize("n_flushes", [2, 3])
def test_counts_after_a_flush_kept_blocks_hold_and_flushed_blocks_read_zero(torch_cuda, n_flushes, mode):
    from pisces_amd import engine
    scene = sg.scene_named("floor, %d flushes in a row" % n_flushes)
    with env(**dict(NO_SWITCH, **STORE_MODES[mode])):
        with engine.HipVariantCaller(sg.config("default")) as c:
            c.SetReference(scene.ref)
            held = []
            for k, (batch, up) in enumerate(zip(batches_of(scene), scene.ups)):
                c.AddAlleleCounts(batch)
                held += scene.batches[k]
                if up is None:
                    continue
                c.CallWithAlleles(up, capacity=1 << 14)
                assert up % sg.BLOCK == 0
                flushed = c.GetCounts(1, up)
                assert not flushed.any(), (mode, "flush %d: %d counts left in the flushed blocks" % (k + 1, int(flushed.sum())))
                want = sg.count_tensor(held, up + 1, 2 * sg.BLOCK, scene.min_bq)
                assert want.sum() > 0
                assert_tensor(c.GetCounts(up + 1, 2 * sg.BLOCK), want, up + 1, scene, "GetCounts after flush %d, %s" % (k + 1, mode))


@pytest.mark.parametrize("feed", ["host", "device"])
@pytest.mark.parametrize("mode", list(STORE_MODES))
def test_reads_added_behind_a_flush_into_the_flushed_block(torch_cuda, mode, feed):
    """store_geometry.late_scene: the flushed block's last tiles are walked a second time with floored and late fragments side by side.
    GetCounts and the final flush's rows against the tensor DoneProcessing leaves (late_tensor); single-M reads only, so every locus
    with a count has its Reference / SNV rows."""
    from pisces_amd import engine
    scene = sg.late_scene()
    n = 3 * sg.BLOCK
    want = sg.late_tensor(scene, n)
    with env(**dict(NO_SWITCH, **STORE_MODES[mode])):
        with engine.HipVariantCaller(sg.config("every allele a row")) as c:
            c.SetReference(scene.ref)
            add = c.AddDeviceReads if feed == "device" else c.AddAlleleCounts
            add(sg.read_batch(scene.batches[0]))
            first, _ = c.CallWithAlleles(scene.ups[0], capacity=1 << 14)
            assert len(first) and first["position"].max() <= scene.ups[0] and not c.GetCounts(1, scene.ups[0]).any()
            add(sg.read_batch(scene.batches[1]))
            assert_tensor(c.GetCounts(1, n), want, 1, scene, "GetCounts behind the late batch, %s, %s" % (mode, feed))
            got, _ = c.CallWithAlleles(None, capacity=1 << 14)
    pr = point_rows(got)
    assert len(pr) == len(got)
    try:
        assert sg.rows_agree_with_tensor(pr, want, scene.ref) > 9 * len(pr)
    except AssertionError as e:
        folded = want.sum(axis=3, dtype=np.int64)
        li = pr["position"].astype(np.int64) - 1
        bad = np.flatnonzero((pr["coverage_by_dir"] != folded[:, [0, 1, 2, 3, 5], :].sum(axis=1)[li]).any(axis=1) | (pr["num_no_calls"] != folded[li, 4, :].sum(axis=1)))
        raise AssertionError("the final flush, %s, %s: first locus that differs %s (floor %d)\n%s" % (
            mode, feed, int(pr["position"][bad[0]]) if len(bad) else "?", scene.ups[0] + 1, str(e)[:500])) from e
    assert set((pr["position"].astype(np.int64) - 1).tolist()) == set(np.flatnonzero(want.sum(axis=(1, 2, 3)) > 0).tolist())
    assert (pr["position"] <= scene.ups[0]).any() and (pr["position"] > scene.ups[0]).any()
